"""The lattice problems of tests/tie_problems.py meet their own conditions, and the C twin computes them EXACTLY (no GPU).

tie_reference is int64 fixed-point arithmetic that shares nothing with the twin and asserts that no operation of the canonical
arithmetic rounds on these inputs; the twin (oracle/hjb_oracle.c: sequential `<` over the visiting order) must then give the same
stored J bit for bit and the first minimiser's label at every state of every stage - exact ties between controls of DIFFERENT
stage cost included, which is what assert_ties asserts the problems hold.  tests/test_gpu_ties.py runs the stage kernels on the
same cases."""
import numpy as np
import pytest

import tie_problems as TP


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("name", sorted(TP.TIE_CASES))
def test_every_registered_case_meets_its_conditions_and_the_twin_is_exact(name, built):
    from hjbdp import _abi
    from oracle import c_oracle
    counts = TP.assert_ties(name)
    print(name, counts)
    dist = TP.TIE_CASES[name].dist
    for spec, term, ref in TP.tie_case(name):
        stages = ref["J_stages"].shape[1]
        if dist is not None:
            # the twin has no disturbance-aware stage: the float restatement of the contract (tests/disturbance_refs.py), stage by
            # stage from the exact reference's own J
            from disturbance_refs import DisturbedRef
            dref = DisturbedRef(spec, *dist)
            for k in range(stages - 1, -1, -1):
                J, idx = dref.backup(term if k == stages - 1 else ref["J_stages"][:, k + 1])
                assert np.array_equal(_bits(J), _bits(ref["J_stages"][:, k])) and np.array_equal(idx, ref["idx_stages"][:, k]), (name, k)
            continue
        twin = c_oracle.sweep(_abi, spec, stages, terminal=term, keep_J=True, keep_idx=True)
        assert twin["J_stages"].dtype == ref["J_stages"].dtype
        for k in range(stages - 1, -1, -1):
            bad = np.flatnonzero(_bits(twin["J_stages"][:, k]) != _bits(ref["J_stages"][:, k]))
            assert bad.size == 0, (name, "J", k, bad.size, bad[:6])
            bad = np.flatnonzero(twin["idx_stages"][:, k] != ref["idx_stages"][:, k])
            assert bad.size == 0, (name, "labels", k, bad.size, bad[:6])


def test_fits_knows_the_formats():
    """The representability test itself, on values whose answer is known."""
    one = 1 << TP.F
    assert TP.fits(np.array([0, one, -3 * one, (1 << 24) * one - one]), TP.F, np.float32)
    assert not TP.fits(np.array([(1 << 24) * one + one]), TP.F, np.float32)            # 2^24 + 1: 25 bits
    assert TP.fits(np.array([2047 * one, one >> 4, 65504 * one]), TP.F, np.float16)
    assert not TP.fits(np.array([2049]), 0, np.float16)
    assert not TP.fits(np.array([65536 * one]), TP.F, np.float16)                      # beyond the largest finite binary16
    assert TP.fits(np.array([1]), 24, np.float16) and not TP.fits(np.array([1]), 25, np.float16)   # its smallest subnormal, 2^-24
    assert TP.fits(np.array([(1 << 52) + 1]), TP.F, np.float64)


def test_the_visiting_order_and_the_label():
    """Control dim 0 slowest in the visiting order, fastest in the label."""
    assert TP.visiting_labels((2, 3), 1).tolist() == [1, 3, 5, 2, 4, 6]
    assert TP.visiting_labels((4,), 0).tolist() == [0, 1, 2, 3]


def test_the_reference_rejects_an_inexact_problem():
    """A third of a cell is on no dyadic lattice; a weight of 1 / 2048 is finer than the reference carries; and the float32 form
    of the half-cell local 2-D problem, exact in float64, leaves float32's 24 bits within the sixteen stages K9 needs - which is
    why the float32 K9 cases move whole cells only."""
    spec = TP.tie_free_problem(3, (5,), (3,))
    spec.next_terms[0][1].data[0] = 1.0 / 3.0
    with pytest.raises(AssertionError):
        TP.tie_reference(spec, TP.lattice_terminal(spec), 1)
    spec = TP.tie_free_problem(3, (5,), (3,))
    spec.next_terms[0][1].data[0] = 1.0 / 2048.0
    with pytest.raises(AssertionError):
        TP.tie_reference(spec, TP.lattice_terminal(spec), 1)
    spec = TP.tie_local2d_problem(90, m=(4,), dtype=np.float32, half=True)
    with pytest.raises(AssertionError):
        TP.tie_reference(spec, TP.lattice_terminal(spec, 90), 16)
    spec = TP.tie_local2d_problem(90, m=(4,), dtype=np.float64, half=True)
    TP.tie_reference(spec, TP.lattice_terminal(spec, 90), 16)
