"""bench.py --dump-outputs without a GPU: sample_outputs on host tensors standing in for one rank's slab of a sweep
(J [owned planes, inner] and the argmin labels), whole grids and seeded samples, one rank and two."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import bench  # noqa: E402


def _slab(n_planes, inner, begin, end, idx_dtype, seed=3):
    rng = np.random.default_rng(seed)
    J = rng.random((n_planes, inner)).astype(np.float32)
    lab = rng.integers(1, 1332, (n_planes, inner)).astype(idx_dtype)
    Jt = torch.from_numpy(J[begin:end].copy())
    sw = SimpleNamespace(begin=begin, end=end, inner=inner, device=torch.device("cpu"), owned_J=lambda: Jt,
                         idx=torch.from_numpy(lab[begin:end].copy()))
    spec = SimpleNamespace(nS=n_planes * inner, j_dtype=np.dtype(np.float32), idx_np_dtype=np.dtype(idx_dtype))
    return sw, spec, J.reshape(-1), lab.reshape(-1)


def test_dump_budget():
    # a sampled dump: float32 J + float32 labels + float64 indices; a whole one: at most float64 J + float64 labels
    assert bench.DUMP_SAMPLE * (4 + 4 + 8) <= 64 << 20 and bench.DUMP_SAMPLE * (8 + 8) <= 64 << 20


@pytest.mark.parametrize("idx_dtype", [np.uint8, np.uint16, np.int32])
def test_whole_grid_is_written_in_state_order(idx_dtype):
    sw, spec, J, lab = _slab(7, 50, 0, 7, idx_dtype)
    out = bench.sample_outputs(sw, spec, None, "nccl")
    assert sorted(out) == ["J", "argmin"]
    assert out["J"].dtype == np.float32 and np.array_equal(out["J"], J)
    assert out["argmin"].dtype == (np.float64 if idx_dtype == np.int32 else np.float32)
    assert np.array_equal(out["argmin"], lab.astype(out["argmin"].dtype))


def test_large_grid_is_a_fixed_seeded_sample(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    sw, spec, J, lab = _slab(40, 250, 0, 40, np.uint16)
    a = bench.sample_outputs(sw, spec, None, "nccl")
    b = bench.sample_outputs(sw, spec, None, "nccl")
    pos = a["state_index"]
    assert pos.dtype == np.float64 and 900 < pos.size <= 1000
    assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < spec.nS
    k = pos.astype(np.int64)
    assert np.array_equal(a["J"], J[k]) and np.array_equal(a["argmin"], lab[k].astype(np.float32))
    for name in a:
        assert np.array_equal(a[name], b[name]), name


def test_two_ranks_contribute_disjoint_parts(monkeypatch):
    """N > 1 all-reduces the ranks' parts: each holds its owned planes' states and zeros elsewhere, so the sum is the whole."""
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    parts = []
    for begin, end in ((0, 17), (17, 40)):
        sw, spec, J, lab = _slab(40, 250, begin, end, np.uint8)
        parts.append(bench.sample_outputs(sw, spec, None, "gloo"))
    k = parts[0]["state_index"].astype(np.int64)
    assert np.array_equal(parts[0]["state_index"], parts[1]["state_index"])
    assert np.array_equal(parts[0]["J"] + parts[1]["J"], J[k])
    assert np.array_equal(parts[0]["argmin"] + parts[1]["argmin"], lab[k].astype(np.float32))
