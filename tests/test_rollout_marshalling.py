"""CPU tests of what every rollout entry point of hjbdp/core.py does to its arguments before the library call and to its path
buffers after it (_starts, _int32_vector, _path_buffers, _f64_vec, _f64_colmajor): pure numpy, no library, no device."""
import numpy as np
import pytest

from hjbdp import core


def test_starts_one_dimensional_is_one_start():
    x = np.arange(13.0)
    one, col = core._starts(x, 13), core._starts(x.reshape(13, 1), 13)
    assert one.shape == col.shape == (1, 13) and np.array_equal(one, col) and np.array_equal(one[0], x)


@pytest.mark.parametrize("rows,n", [(7, 5), (13, 3), (2, 1)])
def test_starts_come_back_as_n_by_rows_contiguous_float64(rows, n):
    X0 = np.arange(rows * n, dtype=np.int64).reshape(rows, n)
    X = core._starts(X0, rows)
    assert X.shape == (n, rows) and X.dtype == np.float64 and X.flags.c_contiguous
    assert np.array_equal(X, X0.T)
    assert np.array_equal(core._starts(np.asfortranarray(X0.astype(np.float64)), rows), X0.T)
    assert np.array_equal(core._starts(X0.tolist(), rows), X0.T)


def test_starts_refuse_a_wrong_element_count():
    with pytest.raises(ValueError):
        core._starts(np.zeros(12), 13)
    with pytest.raises(ValueError):
        core._starts(np.zeros((7, 3)), 13)


def test_planes_are_flattened_checked_and_cast():
    ps = core._int32_vector(np.arange(6, dtype=np.int64).reshape(2, 3), "plane_of_step")
    assert ps.dtype == np.int32 and ps.flags.c_contiguous and ps.tolist() == [0, 1, 2, 3, 4, 5]
    assert core._int32_vector([], "plane_of_step").shape == (0,)
    assert core._int32_vector(np.zeros(4, np.int32), "plane_of_step").tolist() == [0, 0, 0, 0]
    # plane_of_step has never been held to an integer type: whole-valued doubles are taken as they always were
    assert core._int32_vector(np.array([0.0, 2.0]), "plane_of_step").tolist() == [0, 2]


@pytest.mark.parametrize("name,n_traj", [("plane_of_step", None), ("fault_mask", 3), ("fault_stage", 3), ("switch_stage", 3)])
@pytest.mark.parametrize("bad", [2 ** 31, -2 ** 31 - 1])
def test_a_value_outside_int32_is_refused_by_name(name, n_traj, bad):
    with pytest.raises(ValueError, match="%s does not fit int32" % name):
        core._int32_vector([0, bad, 1], name, n_traj)
    good = core._int32_vector([0, 2 ** 31 - 1, -2 ** 31], name, n_traj)
    assert good.dtype == np.int32 and good.tolist() == [0, 2 ** 31 - 1, -2 ** 31]


def test_per_trajectory_values_must_be_integers():
    with pytest.raises(TypeError, match="fault_mask must be integers"):
        core._int32_vector(np.array([1.0, 0.0]), "fault_mask", 2)
    with pytest.raises(TypeError, match="fault_stage must be integers"):
        core._int32_vector(1.0, "fault_stage", 2)


def test_per_trajectory_scalar_broadcasts_and_none_stays_none():
    assert core._int32_vector(None, "fault_mask", 4) is None
    for v in (5, np.int64(5), [5], np.array([5], np.uint8)):
        a = core._int32_vector(v, "switch_stage", 4)
        assert a.dtype == np.int32 and a.flags.c_contiguous and a.flags.writeable and a.tolist() == [5, 5, 5, 5]
    assert core._int32_vector([1, 2, 3, 4], "fault_mask", 4).tolist() == [1, 2, 3, 4]
    with pytest.raises(ValueError):
        core._int32_vector([1, 2, 3], "fault_mask", 4)


SPECS = (("X_path", 13, 6), ("F_path", 12, 5), ("FM_path", 6, 5))


def test_without_keep_path_every_path_is_none():
    flat, views = core._path_buffers(3, False, *SPECS)
    assert flat == [None, None, None]
    assert list(views) == ["X_path", "F_path", "FM_path"] and all(v is None for v in views.values())
    assert [core._f64p(a) for a in flat] == [None, None, None]


def test_with_keep_path_the_views_are_the_flat_buffers_in_fortran_order():
    nt = 3
    flat, views = core._path_buffers(nt, True, *SPECS)
    assert list(views) == [s[0] for s in SPECS]
    for a, (name, rows, cols) in zip(flat, SPECS):
        v = views[name]
        assert a.shape == (nt * rows * cols,) and a.dtype == np.float64 and a.flags.c_contiguous
        assert v.shape == (nt, rows, cols) and v.flags.f_contiguous and np.shares_memory(v, a)
        a[:] = np.arange(a.size)                                 # what the library writes: trajectory fastest, then row, then step
        assert v[2, 1, 4] == 2 + nt * (1 + rows * 4)
    flat, views = core._path_buffers(2, True, ("X_path", 7, 1), ("U_path", 3, 0))
    assert views["X_path"].shape == (2, 7, 1) and views["U_path"].shape == (2, 3, 0) and flat[1].size == 0


def test_vectors_and_column_major_matrices():
    assert core._f64_vec(None, 3) is None and core._f64_colmajor(None, 3, 3) is None
    v = core._f64_vec([1, 2, 3], 3)
    assert v.dtype == np.float64 and v.flags.c_contiguous and v.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        core._f64_vec([1, 2], 3)
    m = core._f64_colmajor([[1, 2, 3], [4, 5, 6]], 2, 3)
    assert m.dtype == np.float64 and m.flags.c_contiguous and m.tolist() == [1.0, 4.0, 2.0, 5.0, 3.0, 6.0]
    with pytest.raises(ValueError):
        core._f64_colmajor(np.zeros(8), 3, 3)
