"""GPU tests of K16's two placements and of the lookup's edges (k_rollout, HJB_ROLLOUT_LOOKUP in csrc/kernels_rollout.h): the
global-memory form where hjb_rollout_run chooses it itself (2,100 knots on one axis; a control table beyond 4,096 doubles) and
where option "lds" = 0 forces it, the 32 KiB boundary between the two forms, partly filled workgroups, labels at the top of
uint8 / uint16 and beyond 16 bits in int32, starts exactly on knots, on cell midpoints and one ulp either side of both at every D
(non-uniform and uniform grids), and label offsets beyond 2^32.  The checker is tests/rollout_refs.py (bit equality,
test_gpu_rollout._check_bits); the exact placements are also checked against labels and u_table directly."""
import time

import numpy as np
import pytest

import rollout_refs
from test_gpu_rollout import _check_bits, _random_problem

pytestmark = pytest.mark.gpu

LDS_DOUBLES = 4096          # DESIGN.md, "LDS staging": 2 * sum(n) + n_labels * n_u doubles <= 32 KiB are staged
DTYPES = (np.uint8, np.uint16, np.int32)


def _staged_doubles(knots, n_labels, nu):
    return 2 * sum(len(k) for k in knots) + n_labels * nu


def _all_finite(out):
    return all(np.isfinite(out[key]).all() for key in ("X_final", "cost", "X_path", "U_path"))


def _model(rng, D, nu):
    """_random_problem's model: A with spectral norm 0.5, small B and c"""
    A = rng.uniform(-1.0, 1.0, size=(D, D))
    A *= 0.5 / np.linalg.norm(A, 2)
    return A, rng.uniform(-0.02, 0.02, size=(D, nu)), rng.uniform(-0.02, 0.02, size=D)


# ---- (b) the global form by knots ------------------------------------------------------------------------------------------
def _long_axis_problem(rng, D, la, nu, dtype, n_long=2100, n_labels=7, n_planes=3):
    """_random_problem with n_long knots on axis la.  Every axis is rescaled to a span drawn from [1.5, 3] about 0 +- 0.1: a long
    axis of unit-sized cells would span about 1,500 units, A would carry that into the short axes and 'linear' would overflow."""
    n = [int(v) for v in rng.integers(2, 6 if D <= 4 else 4, size=D)]
    n[la] = n_long
    knots = []
    for m in n:
        k = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.0, size=m - 1))])
        knots.append((k - k[-1] / 2) * (rng.uniform(1.5, 3.0) / k[-1]) + rng.uniform(-0.1, 0.1))
    nS = int(np.prod(n))
    base = int(rng.integers(0, 2))
    labels = rng.integers(base, base + n_labels, size=(nS, n_planes)).astype(dtype)
    ut = rng.uniform(-1.0, 1.0, size=(n_labels, nu))
    A, B, c = _model(rng, D, nu)
    return knots, labels, ut, base, A, B, c


def _long_axis_starts(rng, knots, la, method, n=300):
    """up to 0.1 outside on every axis; for 'linear' inside on the long axis (random labels on knots 1e-3 apart give slopes of
    thousands per unit: 0.1 outside leaves the grid for good), but for 8 starts outside by <= 1 % of the end cell's width"""
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X0 = rng.uniform(lo[:, None], hi[:, None], size=(len(knots), n))
    if method == "linear":
        k = knots[la]
        X0[la] = rng.uniform(k[0], k[-1], size=n)
        X0[la, :4] = k[0] - rng.uniform(0.0, 0.01, size=4) * (k[1] - k[0])
        X0[la, 4:8] = k[-1] + rng.uniform(0.0, 0.01, size=4) * (k[-1] - k[-2])
    return X0


def _long_axis_cases(D, la):
    """(n_u, label type) pairs of one (D, la): all three types at D = 1, else two by rotation, which at every D > 1 meets each type"""
    if D == 1:
        return [(1, np.uint8), (4, np.uint16), (1, np.int32), (4, np.uint8), (1, np.uint16), (4, np.int32)]
    return [(1, DTYPES[(D + la) % 3]), (4, DTYPES[(D + la + 1) % 3])]


LONG_AXIS = sorted({(D, la) for D in range(1, 7) for la in (0, D // 2, D - 1)})


@pytest.mark.parametrize("D,la", LONG_AXIS)
def test_global_form_chosen_by_a_2100_knot_axis(built, D, la):
    import hjbdp
    for nu, dtype in _long_axis_cases(D, la):
        rng = np.random.default_rng(100 * D + la + nu)
        knots, labels, ut, base, A, B, c = _long_axis_problem(rng, D, la, nu, dtype)
        assert 2 * sum(len(k) for k in knots) > LDS_DOUBLES             # the library itself takes LDS = false
        planes = rng.integers(0, 3, size=8)
        q = rng.uniform(0, 1, size=D)
        r = rng.uniform(0, 1, size=nu)
        with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
            ro.set_model(A, B, c=c if nu == 4 else None, q=q, r=r)
            for method in ("nearest", "linear"):
                X0 = _long_axis_starts(rng, knots, la, method)
                out = ro.run(X0, planes, method=method, keep_path=True)
                ref = rollout_refs.rollout(knots, labels, ut, base, A, B, X0, planes, method, c=c if nu == 4 else None, q=q, r=r)
                _check_bits(out, ref)
                assert _all_finite(out), (D, la, nu, dtype, method)


# ---- (c) the global form by table size, and the top of each label type ------------------------------------------------------
#            type       base  n_labels  labels that must be read (every one < base + n_labels)
TOP_CASES = [(np.uint16, 0, 65536, (0xFFFF, 0x8000)),
             (np.uint16, 1, 65535, (0xFFFF, 0x8000)),
             (np.int32, 0, 70000, (69999, 0x8000, 0xFFFF, 0x10000)),
             (np.int32, 1, 70000, (70000, 0x8000, 0xFFFF, 0x10000)),
             (np.uint8, 0, 256, (0xFF, 0x80)),
             (np.uint8, 1, 255, (0xFF, 0x80))]


def _plant(knots, labels, plane, wanted, X0):
    """write each wanted label into a node of `plane` that is the last knot on no axis (distinct nodes) and move one start per label
    onto that node: 'nearest' and 'linear' (every weight 0, fma(0, d, v) = v) both return that label's row of u_table exactly.
    Returns the trajectory index of each label."""
    n = [len(k) for k in knots]
    room = int(np.prod([m - 1 for m in n]))
    assert room >= len(wanted)
    where = []
    for t, lab in enumerate(wanted):
        idx = np.unravel_index(t * (room // len(wanted)), [m - 1 for m in n], order="F")
        off = int(np.ravel_multi_index(idx, n, order="F"))
        labels[off, plane] = lab
        X0[:, t] = [knots[a][idx[a]] for a in range(len(n))]
        where.append(t)
    return where


@pytest.mark.parametrize("D", [1, 3, 6])
@pytest.mark.parametrize("case", range(len(TOP_CASES)))
def test_global_form_chosen_by_the_table_and_the_top_of_each_label_type(built, D, case):
    import hjbdp
    dtype, base, n_labels, wanted = TOP_CASES[case]
    rng = np.random.default_rng(1000 * D + case)
    for nu in (1, 4):
        n = [5] + [int(v) for v in rng.integers(2, 4, size=D - 1)]
        knots = []
        for m in n:
            k = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.0, size=m - 1))])
            knots.append(k - k[-1] / 2 + rng.uniform(-0.1, 0.1))
        nS = int(np.prod(n))
        labels = rng.integers(base, base + n_labels, size=(nS, 3)).astype(dtype)
        ut = rng.uniform(-1.0, 1.0, size=(n_labels, nu))
        A, B, c = _model(rng, D, nu)
        fits = _staged_doubles(knots, n_labels, nu) <= LDS_DOUBLES
        assert fits == (dtype == np.uint8)                              # the uint8 tables fit LDS, the others cannot
        lo = np.array([k[0] for k in knots]) - 0.1
        hi = np.array([k[-1] for k in knots]) + 0.1
        X0 = rng.uniform(lo[:, None], hi[:, None], size=(D, 300))
        planes = rng.integers(0, 3, size=8)
        where = _plant(knots, labels, int(planes[0]), wanted, X0)
        assert int(labels.max()) == base + n_labels - 1
        q = rng.uniform(0, 1, size=D)
        r = rng.uniform(0, 1, size=nu)
        with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
            ro.set_model(A, B, c=c if nu == 4 else None, q=q, r=r)
            for method in ("nearest", "linear"):
                ref = rollout_refs.rollout(knots, labels, ut, base, A, B, X0, planes, method, c=c if nu == 4 else None, q=q, r=r)
                for lds in ((1, 0) if fits else (1,)):
                    ro.set_option("lds", lds)
                    out = ro.run(X0, planes, method=method, keep_path=True)
                    _check_bits(out, ref)
                    assert _all_finite(out)
                    for t, lab in zip(where, wanted):                   # the rows of the top labels were read, not only permitted
                        assert np.array_equal(out["U_path"][t, :, 0], ut[lab - base]), (method, lds, lab)


# ---- (d) the 32 KiB boundary and launch sizes -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("n_labels", [4080, 4081])
def test_the_32_kib_boundary_at_partly_filled_workgroups(built, dtype, n_labels):
    """n = (3, 5), n_u = 1: 2 * 8 + 4080 = 4,096 doubles is the last size staged in LDS, 4,081 labels the first read from global
    memory.  1, 255, 256 and 257 trajectories: with one trajectory in the LDS form 255 threads stage the tables and then return."""
    import hjbdp
    rng = np.random.default_rng(4080 + np.dtype(dtype).itemsize)
    n = (3, 5)
    knots = []
    for m in n:
        k = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.0, size=m - 1))])
        knots.append(k - k[-1] / 2 + rng.uniform(-0.1, 0.1))
    base = 1
    assert _staged_doubles(knots, 4080, 1) == LDS_DOUBLES
    labels = rng.integers(base, base + n_labels, size=(15, 3)).astype(dtype)
    ut = rng.uniform(-1.0, 1.0, size=(n_labels, 1))
    A, B, c = _model(rng, 2, 1)
    planes = rng.integers(0, 3, size=8)
    lo = np.array([k[0] for k in knots]) - 0.1
    hi = np.array([k[-1] for k in knots]) + 0.1
    X_all = rng.uniform(lo[:, None], hi[:, None], size=(2, 257))
    top = base + n_labels - 1                                           # the last element staged / the first past 32 KiB
    where = _plant(knots, labels, int(planes[0]), (top, base), X_all)
    q, r = [1.0, 0.5], [0.25]
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c, q=q, r=r)
        for method in ("nearest", "linear"):
            full = rollout_refs.rollout(knots, labels, ut, base, A, B, X_all, planes, method, c=c, q=q, r=r)
            for nt, chunk in ((1, 1 << 20), (255, 1 << 20), (256, 1 << 20), (257, 1 << 20), (257, 64)):
                ref = (full[0][:, :nt], full[1][:nt], full[2][:nt], full[3][:nt])       # trajectories are independent
                ro.set_option("chunk", chunk)
                for lds in ((1, 0) if n_labels == 4080 else (1,)):      # 4,080: LDS by the documented rule, and forced out of it
                    ro.set_option("lds", lds)
                    out = ro.run(X_all[:, :nt], planes, method=method, keep_path=True)
                    _check_bits(out, ref)
                    assert _all_finite(out)
                    for t, lab in zip(where, (top, base)):
                        if t < nt:
                            assert out["U_path"][t, 0, 0] == ut[lab - base, 0], (method, nt, chunk, lds, lab)
                    lean = ro.run(X_all[:, :nt], planes, method=method, keep_path=False)
                    assert lean["X_path"] is None
                    _check_bits(lean, ref)


def test_option_lds_takes_0_and_1_only(built):
    import hjbdp
    from hjbdp import _abi
    rng = np.random.default_rng(5)
    knots, labels, ut, base, A, B, c = _random_problem(rng, 2, 1, np.uint8, 7, 2)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        for bad in (-1, 2, 1 << 40):
            with pytest.raises(hjbdp.HjbError) as ei:
                ro.set_option("lds", bad)
            assert ei.value.status == _abi.HJB_E_INVALID and "lds" in str(ei.value)
        ro.set_option("lds", 0)
        ro.set_option("lds", 1)


# ---- (e) exact placements at every D ----------------------------------------------------------------------------------------
def _placements(rng, knots, n_on_nodes=64):
    """Starts with one coordinate on every knot of its axis (first and last included), on every cell midpoint k[i] + (k[i+1] - k[i]) / 2
    and on np.nextafter of each of these in both directions, the other coordinates drawn inside the grid; then n_on_nodes starts
    that lie on a knot on EVERY axis, none of them the last.  Returns X0 [D, n] and the number of the latter (they come last)."""
    D = len(knots)
    cols = []
    for a, k in enumerate(knots):
        v = np.concatenate([k, k[:-1] + np.diff(k) / 2])
        v = np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])
        X = np.stack([rng.uniform(kk[0], kk[-1], size=v.size) for kk in knots])
        X[a] = v
        cols.append(X)
    cols.append(np.stack([k[rng.integers(0, len(k) - 1, size=n_on_nodes)] for k in knots]))
    return np.concatenate(cols, axis=1).reshape(D, -1), n_on_nodes


def _nearest_rows(knots, plane, ut, base, X0):
    """include/hjbdp.h's 'nearest' from labels and u_table directly: the cell with k[c] <= x < k[c+1], clamped to the grid; its
    upper knot when (x - k[c]) >= (k[c+1] - x) in float64; the row of the label at that node"""
    off = np.zeros(X0.shape[1], dtype=np.int64)
    stride = 1
    for a, k in enumerate(knots):
        x = X0[a]
        c = np.clip(np.searchsorted(k, x, side="right") - 1, 0, len(k) - 2)
        up = (x - k[c]) >= (k[c + 1] - x)
        off += stride * (c + up)
        stride *= len(k)
    return ut[plane[off].astype(np.int64) - base]


def _check_placements(hjbdp, rng, knots, dtype, n_labels, nu):
    D = len(knots)
    nS = int(np.prod([len(k) for k in knots]))
    base = D % 2
    labels = rng.integers(base, base + n_labels, size=(nS, 2)).astype(dtype)
    ut = rng.uniform(-1.0, 1.0, size=(n_labels, nu))
    A, B, c = _model(rng, D, nu)
    assert _staged_doubles(knots, n_labels, nu) <= LDS_DOUBLES          # "lds" = 1 is the LDS form here
    X0, n_nodes = _placements(rng, knots)
    planes = [1]
    want_nearest = _nearest_rows(knots, labels[:, 1], ut, base, X0)
    with hjbdp.Rollout(knots, labels, ut, index_base=base) as ro:
        ro.set_model(A, B, c=c)
        for method in ("nearest", "linear"):
            ref = rollout_refs.rollout(knots, labels, ut, base, A, B, X0, planes, method, c=c)
            for lds in (1, 0):
                ro.set_option("lds", lds)
                out = ro.run(X0, planes, method=method, keep_path=True)
                U = out["U_path"][:, :, 0]
                if method == "nearest":
                    bad = np.flatnonzero((U != want_nearest).any(axis=1))
                    assert bad.size == 0, "nearest, lds=%d: %d starts differ, first %d at %r" % (lds, bad.size, bad[0], X0[:, bad[0]])
                else:       # on a node, no axis at its last knot: every weight is 0 and fma(0, d, v) = v, so 'linear' = 'nearest' there
                    assert np.array_equal(U[-n_nodes:], want_nearest[-n_nodes:]), "linear on nodes, lds=%d" % lds
                _check_bits(out, ref)
                assert _all_finite(out)


def _short_knots(rng, D, uniform):
    knots = []
    for m in rng.integers(3, 6 if D <= 4 else 4, size=D):
        if uniform:
            lo = rng.uniform(-1.5, -0.5)
            knots.append(np.linspace(lo, lo + rng.uniform(1.0, 3.0), int(m)))
        else:
            k = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.0, size=int(m) - 1))])
            knots.append(k - k[-1] / 2 + rng.uniform(-0.1, 0.1))
    return knots


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("grid", ["nonuniform", "uniform"])
def test_exact_placements_at_every_d(built, D, grid):
    """Knots, midpoints and their float64 neighbours on every axis, one step, both placements: 'nearest' against labels and u_table
    directly (the tie rule: the upper knot at the midpoint), 'linear' on nodes likewise, everything against the twin.  The np.linspace
    grids take find_cell's arithmetic first guess (uniform, x0, inv_h); that hjb_rollout_create saw them as uniform shows from
    outside only in that the result still equals the twin's, whose find_cell is exact either way.  At D = 1 and D = 2 one uniform
    axis is np.linspace(-0.7, 0.9, 1001).  numpy forms it as x0 + i * h, so knots[i] equals that sum but for one i; what rounds
    apart is the guess (x - x0) * (1 / h): it falls one cell short on 54 of the knots and one cell far on 652 of the values just
    below a knot, and find_cell's correction steps have to mend it."""
    import hjbdp
    rng = np.random.default_rng(700 + 10 * D + (grid == "uniform"))
    knots = _short_knots(rng, D, grid == "uniform")
    if grid == "uniform" and D <= 2:
        knots[D - 1] = np.linspace(-0.7, 0.9, 1001)
        k = knots[D - 1]
        guess = lambda x: np.clip((x - k[0]) * (1.0 / ((k[-1] - k[0]) / 1000)), 0, 999).astype(np.int64)
        assert (guess(k) != np.minimum(np.arange(1001), 999)).sum() == 54
        assert (guess(np.nextafter(k, -np.inf)) != np.clip(np.arange(1001) - 1, 0, 999)).sum() == 652
    _check_placements(hjbdp, rng, knots, DTYPES[D % 3], 251, 1 + D % 2)


# ---- (f) label offsets beyond 2^32 ------------------------------------------------------------------------------------------
def _check_far_planes(hjbdp, side, n_planes, used):
    """uint8 labels on side^3 states x n_planes planes, passed 1-D (Rollout does not copy a contiguous 1-D array of a supported type).
    The three planes `used` hold random labels; every other plane holds a filler label whose u_table row, 1e6, is found nowhere else.
    The twin gets the used planes as a compact 3-plane array (it converts its labels to int64) and the remapped plane_of_step."""
    rng = np.random.default_rng(n_planes)
    nS = side ** 3
    n_labels, nu, base, filler = 200, 2, 1, 200                         # labels 1 .. 200, the filler is the last
    t0 = time.time()
    try:
        lab = np.full(n_planes * nS, filler, dtype=np.uint8)
    except MemoryError:
        pytest.skip("the host cannot allocate the %.1f GB label array" % (n_planes * nS / 1e9))
    compact = rng.integers(base, filler, size=(nS, 3)).astype(np.uint8)          # excludes the filler
    for j, p in enumerate(used):
        lab[p * nS:(p + 1) * nS] = compact[:, j]
    knots = []
    for m in (side,) * 3:
        k = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.0, size=m - 1))])
        knots.append((k - k[-1] / 2) * (2.0 / k[-1]))
    ut = rng.uniform(-1.0, 1.0, size=(n_labels, nu))
    ut[filler - base] = 1.0e6
    A, B, c = _model(rng, 3, nu)
    X0 = rng.uniform(-1.0, 1.0, size=(3, 300))      # inside [-1, 1]^3, and |A| = 0.5 with |B u| + |c| <= 0.06 keeps every step inside
    X0[:, 0] = [k[-1] for k in knots]               # the last node, looked up first on the last plane: the array's last byte
    X0[:, 1] = [k[0] for k in knots]
    steps = (np.arange(9) + 2) % 3                  # the compact array's planes 2, 0, 1 in turn
    q, r = [1.0, 0.5, 0.25], [0.1, 0.2]
    t1 = time.time()
    with hjbdp.Rollout(knots, lab, ut, index_base=base) as ro:
        t2 = time.time()
        ro.set_model(A, B, c=c, q=q, r=r)
        for method in ("nearest", "linear"):
            out = ro.run(X0, np.asarray(used)[steps], method=method, keep_path=True)
            ref = rollout_refs.rollout(knots, compact, ut, base, A, B, X0, steps, method, c=c, q=q, r=r)
            _check_bits(out, ref)
            assert _all_finite(out) and not (out["U_path"] == 1.0e6).any()
            assert np.abs(out["U_path"]).max() <= 1.0 + 1e-12           # inside the grid a blend of rows in (-1, 1): no filler corner
            if method == "nearest":
                assert np.array_equal(out["U_path"][0, :, 0], ut[int(compact[-1, 2]) - base])
    print("label array %.1f s, create %.1f s, runs and twin %.1f s" % (t1 - t0, t2 - t1, time.time() - t2))


def test_label_offsets_beyond_two_to_the_32(built):
    """128^3 states x 2,049 planes of uint8 labels (4.3e9 bytes): plane 1025 starts at offset 2^31 + 2^21, plane 2048 at 2^32, and
    plane_of_step cycles through planes 0, 1025 and 2048.  An offset formed in 32 bits (base = plane * nS and stride[a] * cell in
    HJB_ROLLOUT_LOOKUP, which K17 to K20 share) reads the filler or another plane's labels."""
    import hjbdp
    free, _ = hjbdp.device_mem_info(0)
    if free < 16 << 30:
        pytest.skip("device 0 has %.1f GB free: the 4.3 GB label array and its run want 16 GB" % (free / 1e9))
    nS = 128 ** 3
    assert 1025 * nS == (1 << 31) + (1 << 21) and 2048 * nS == 1 << 32
    _check_far_planes(hjbdp, 128, 2049, (0, 1025, 2048))
