"""GPU tests (-m gpu) of the three small kernel families beside the stage kernels, at every instantiation the library
builds:

* k_policy_lookup<T, D> (kernels_lookup.h, hjb_policy_lookup): T = float, double x D = 1..6 x nearest, linear,
* k_probe<T, TJ, D> (kernels_probe.h, hjb_probe_stage / hjb_solve_opts.probe): (float, _Float16), (float, float),
  (double, double) x D = 1..6, C = 1..3,
* k_fill_separable<T, TJ> (kernels_devmem.h, hjb_device_fill_separable / hjb_rank_fill_separable) x 3, and
  k_gather_bytes (hjb_device_gather) at element sizes 1, 2, 4, 8.

Every result is held two ways: to the C twin (oracle/hjb_oracle.c) or the ordered numpy sum of the same arithmetic,
bit for bit, and to a plain float64 restatement (tests/float64_refs.py) within a tolerance derived from the arithmetic
type (stated where it is used)."""
import numpy as np
import pytest

from float64_refs import linear_ref, linear_tol, nearest_ref, ordered_sum, separable_ref, term_block

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f64": np.float64}
STORAGE = ["f32", "f16s", "f64"]          # HJB_F32, HJB_F16S (float32 arithmetic, binary16 J), HJB_F64


@pytest.fixture(scope="module")
def env(built):
    import hjbdp
    from hjbdp import _abi
    from oracle import c_oracle
    if hjbdp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run the HIP path (no fallback)")
    return hjbdp, _abi, c_oracle


# ---- k_policy_lookup ------------------------------------------------------------------------------------------------------
def _lookup_grid(rng, D, dtype):
    """Non-uniform knots rounded to dtype, an axis of exactly 2 knots in every D, random values."""
    sizes = [2, 5, 3, 7, 4, 6][:D]
    knots = [(np.cumsum(rng.uniform(0.3, 1.7, n)) - 1.0).astype(dtype).astype(np.float64) for n in sizes]
    V = rng.standard_normal(tuple(sizes)).astype(dtype)
    return knots, V


def _lookup_points(rng, knots, dtype, n_random=3000):
    """Random points in and around the grid, every knot of every axis (first and last included), midpoints of
    every cell, and points 10 and 25 cell widths outside either end of every axis."""
    D = len(knots)
    lo = np.array([k[0] for k in knots])
    hi = np.array([k[-1] for k in knots])
    span = hi - lo
    pts = [lo + (hi - lo) * rng.uniform(-0.3, 1.3, size=(n_random, D))]
    for a, k in enumerate(knots):
        inner = np.stack([rng.choice(kk, len(k)) for kk in knots], axis=1)
        inner[:, a] = k                                              # every knot on axis a, knots elsewhere
        mids = np.stack([rng.uniform(kk[0], kk[-1], len(k) - 1) for kk in knots], axis=1)
        mids[:, a] = 0.5 * (k[:-1] + k[1:])
        far = np.tile(lo + 0.5 * span, (4, 1))
        h0, h1 = k[1] - k[0], k[-1] - k[-2]
        far[:, a] = [k[0] - 10 * h0, k[0] - 25 * h0, k[-1] + 10 * h1, k[-1] + 25 * h1]
        pts += [inner, mids, far]
    return np.concatenate(pts).astype(dtype)


@pytest.mark.parametrize("method", ["nearest", "linear"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_policy_lookup_every_instantiation(env, D, dt, method):
    """k_policy_lookup<T, D> for every T and D: bit-exact against the C twin's lookup; 'linear' against scipy's
    RegularGridInterpolator (linear extrapolation) to linear_tol (1e-12 of max|V| x the weight sum in float64,
    8 (D + 1) float32 units there); 'nearest' against the float64 nearest-knot rule at every point that is not within
    a few units in the last place of a cell midpoint."""
    hjbdp, _abi, c_oracle = env
    dtype = DTYPES[dt]
    rng = np.random.default_rng(100 * D + len(dt) + len(method))
    knots, V = _lookup_grid(rng, D, dtype)
    pts = _lookup_points(rng, knots, dtype)
    got = hjbdp.policy_lookup(knots, V, pts, method)
    assert got.dtype == dtype and got.shape == (len(pts),)
    assert np.array_equal(got, c_oracle.lookup(_abi, knots, V, pts, method))
    if method == "linear":
        ref, w = linear_ref(knots, V, pts)
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err <= linear_tol(dtype, D, np.max(np.abs(V)), w)), np.max(err / w)
    else:
        ref, near_mid = nearest_ref(knots, V, pts)
        assert near_mid.mean() < 0.2
        assert np.array_equal(got[~near_mid], ref[~near_mid])
        on_knots = np.all([np.isin(pts[:, a].astype(np.float64), knots[a]) for a in range(D)], axis=0)
        assert on_knots.sum() > 0 and np.array_equal(got[on_knots], ref[on_knots])


def _dyadic_grid():
    """Three axes whose knots, cell widths, midpoints and reciprocal widths are all exact in float32: a 2-knot axis,
    cells of 2^-10 beside cells of 1 (ratio 1:1024), and a uniform axis of width 1/4."""
    return [np.array([-0.5, 0.5]),
            np.array([-1.0, -1.0 + 2 ** -10, -1.0 + 2 ** -9, 2 ** -9, 1.0 + 2 ** -9, 1.0 + 2 ** -9 + 2 ** -10]),
            np.array([0.0, 0.25, 0.5, 0.75])]


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_policy_lookup_edges(env, dt):
    """On every knot the value of that knot; at an exact midpoint (dyadic knots: the midpoint is exact in either type)
    the UPPER knot; 10 and 25 cell widths outside an end the edge knot ('nearest') or the linear extension of the end
    cell ('linear'), which reproduces an affine V exactly in float64.  Both methods bit-exact against the twin."""
    hjbdp, _abi, c_oracle = env
    dtype = DTYPES[dt]
    knots = _dyadic_grid()
    n = tuple(len(k) for k in knots)
    grids = np.meshgrid(*knots, indexing="ij")
    c = (0.75, -2.0, 0.5, 4.0)                                  # affine V = c0 + c1 x0 + c2 x1 + c3 x2: exact in both types
    V_aff = (c[0] + c[1] * grids[0] + c[2] * grids[1] + c[3] * grids[2]).astype(dtype)
    rng = np.random.default_rng(7)
    V_rnd = rng.standard_normal(n).astype(dtype)
    on = np.stack([g.reshape(-1) for g in grids], axis=1)       # all 2 x 6 x 4 knot combinations
    mids, upper = [], []
    for a, k in enumerate(knots):
        for i in range(len(k) - 1):
            p = on[::7].copy()
            p[:, a] = 0.5 * (k[i] + k[i + 1])
            mids.append(p)
            u = p.copy()
            u[:, a] = k[i + 1]
            upper.append(u)
    mids, upper = np.concatenate(mids), np.concatenate(upper)
    far = []
    for a, k in enumerate(knots):
        for d in (10, 25):
            for end in (0, 1):
                p = on[::5].copy()
                p[:, a] = k[0] - d * (k[1] - k[0]) if end == 0 else k[-1] + d * (k[-1] - k[-2])
                far.append(p)
    far = np.concatenate(far)
    for V in (V_aff, V_rnd):
        for pts in (on, mids, far):
            q = pts.astype(dtype)
            for method in ("nearest", "linear"):
                got = hjbdp.policy_lookup(knots, V, q, method)
                assert np.array_equal(got, c_oracle.lookup(_abi, knots, V, q, method)), method
        # on every knot: that knot's value ('linear' at the last knot of an axis is a lerp with t = 1: to rounding)
        at = V[tuple(np.searchsorted(knots[a], on[:, a]) for a in range(3))]
        assert np.array_equal(hjbdp.policy_lookup(knots, V, on.astype(dtype), "nearest"), at)
        lin = hjbdp.policy_lookup(knots, V, on.astype(dtype), "linear")
        assert np.all(np.abs(lin - at) <= linear_tol(dtype, 3, np.max(np.abs(V)), 1.0))
        # exact midpoints: the upper knot
        up = V[tuple(np.searchsorted(knots[a], upper[:, a]) for a in range(3))]
        assert np.array_equal(hjbdp.policy_lookup(knots, V, mids.astype(dtype), "nearest"), up)
        # far outside: nearest = the edge knot
        edge = V[tuple(np.clip(np.searchsorted(knots[a], far[:, a]), 0, len(knots[a]) - 1) for a in range(3))]
        assert np.array_equal(hjbdp.policy_lookup(knots, V, far.astype(dtype), "nearest"), edge)
        lin = hjbdp.policy_lookup(knots, V, far.astype(dtype), "linear")
        ref, w = linear_ref(knots, V, far)
        assert np.all(np.abs(lin - ref) <= linear_tol(dtype, 3, np.max(np.abs(V)), w))
    aff = c[0] + c[1] * far[:, 0] + c[2] * far[:, 1] + c[3] * far[:, 2]
    lin = hjbdp.policy_lookup(knots, V_aff, far.astype(dtype), "linear")
    if dtype == np.float64:
        assert np.array_equal(lin, aff)                         # linear extrapolation of an affine function: exact
    else:
        assert np.all(np.abs(lin - aff) <= linear_tol(dtype, 3, np.max(np.abs(V_aff)), linear_ref(knots, V_aff, far)[1]))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_policy_lookup_batch_sizes(env, dt):
    """nq = 0, 1, 255 and 257 (one workgroup, one short of it, one past it): bit-exact against the twin."""
    hjbdp, _abi, c_oracle = env
    dtype = DTYPES[dt]
    rng = np.random.default_rng(11)
    knots, V = _lookup_grid(rng, 3, dtype)
    for nq in (0, 1, 255, 257):
        pts = _lookup_points(rng, knots, dtype, 300)[:nq]
        for method in ("nearest", "linear"):
            got = hjbdp.policy_lookup(knots, V, pts, method)
            assert got.shape == (nq,) and np.array_equal(got, c_oracle.lookup(_abi, knots, V, pts, method)), (nq, method)


def test_policy_lookup_grid_stride(env):
    """More queries than one launch's 65,536 workgroups x 256 threads: the threads walk the queries in grid strides,
    and every output - the last pass's included - equals the twin's, and the float64 restatement to linear_tol."""
    hjbdp, _abi, c_oracle = env
    rng = np.random.default_rng(12)
    k = np.cumsum(rng.uniform(0.5, 1.5, 300)).astype(np.float32).astype(np.float64)
    V = rng.standard_normal(300).astype(np.float32)
    nq = 65536 * 256 + 4099
    q = (k[0] + (k[-1] - k[0]) * np.linspace(-0.05, 1.05, nq)).astype(np.float32).reshape(-1, 1)
    for method in ("nearest", "linear"):
        got = hjbdp.policy_lookup([k], V, q, method)
        twin = c_oracle.lookup(_abi, [k], V, q, method)
        bad = np.flatnonzero(got != twin)
        assert bad.size == 0, (method, bad[:5])
        tail = slice(65536 * 256 - 10, nq)
        if method == "linear":
            ref, w = linear_ref([k], V, q[tail])
            assert np.all(np.abs(got[tail] - ref) <= linear_tol(np.float32, 1, np.max(np.abs(V)), w))
        else:
            ref, near_mid = nearest_ref([k], V, q[tail])
            assert np.array_equal(got[tail][~near_mid], ref[~near_mid])


def test_policy_lookup_refusals_with_a_device(env):
    """With a device the argument checks still come first: each returns its status (tests/test_abi.py has the same
    without a device), and knots that merge only in float32 are fine in float64."""
    hjbdp, _abi, c_oracle = env
    k = [np.array([0.0, 1.0, 1.0 + 1e-9])]
    with pytest.raises(hjbdp.HjbError) as ei:
        hjbdp.policy_lookup(k, np.zeros(3, np.float32), np.zeros((1, 1), np.float32))
    assert ei.value.status == _abi.HJB_E_INVALID
    got = hjbdp.policy_lookup(k, np.array([1.0, 2.0, 3.0]), np.array([[1.0 + 0.6e-9], [0.4]]))
    assert np.array_equal(got, [3.0, 1.0])
    with pytest.raises(hjbdp.HjbError) as ei:
        hjbdp.policy_lookup([np.array([0.0])], np.zeros(1), np.zeros((1, 1)))
    assert ei.value.status == _abi.HJB_E_INVALID
    with pytest.raises(hjbdp.HjbError) as ei:
        hjbdp.policy_lookup([np.array([0.0, 1.0])] * 7, np.zeros((2,) * 7), np.zeros((1, 7)))
    assert ei.value.status == _abi.HJB_E_UNSUPPORTED


# ---- GPU lookups vs the host's rollout lookups ---------------------------------------------------------------------------
def _probe_points(rng, knots):
    """Midpoints of every cell, the midpoints nudged by about one float32 unit either way (where a float32 decision
    differs from the float64 one), every knot, and points 10 cell widths outside either end - on one axis at a time."""
    base = np.array([k[len(k) // 2] for k in knots])
    out = []
    for a, k in enumerate(knots):
        m = 0.5 * (k[:-1] + k[1:])
        du = np.spacing(np.abs(m).astype(np.float32)).astype(np.float64)
        vals = np.concatenate([m, m - 0.3 * du, m + 0.3 * du, m - du, m + du, k,
                               [k[0] - 10 * (k[1] - k[0]), k[-1] + 10 * (k[-1] - k[-2])]])
        p = np.tile(base, (len(vals), 1))
        p[:, a] = vals
        out.append(p)
    return np.concatenate(out)


def _host_vs_gpu(hjbdp, knots, table, pts, linear_values=None):
    """NearestPolicy.lookup_many == NearestPolicy.__call__ (the host rule the rollouts follow) at every point, with the
    table in float64 and in float32; policy_lookup 'linear' vs matlab_compat.interp_linear_point (float64 host
    arithmetic) to linear_tol - in float32 at the float32-rounded query, the point the float32 lookup evaluates."""
    from hjbdp.matlab_compat import interp_linear_point
    from hjbdp.solver_position import NearestPolicy
    D = len(knots)
    for tab in (np.asarray(table, dtype=np.float64), np.asarray(table, dtype=np.float32)):
        pol = NearestPolicy(knots, tab)
        many = pol.lookup_many(pts)
        one = np.array([pol(*p) for p in pts])
        bad = np.flatnonzero(many != one)
        assert bad.size == 0, (tab.dtype, pts[bad[:3]], many[bad[:3]], one[bad[:3]])
        assert many.dtype == tab.dtype
    if linear_values is None:
        return
    for V in (np.asarray(linear_values, dtype=np.float64), np.asarray(linear_values, dtype=np.float32)):
        dt = V.dtype.type
        kq = [k.astype(dt).astype(np.float64) for k in knots]
        q = pts.astype(dt)
        got = hjbdp.policy_lookup(knots, V, q, "linear")
        host = np.array([interp_linear_point(kq, V, p) for p in q.astype(np.float64)])
        _, w = linear_ref(kq, V, q)
        assert np.all(np.abs(got - host) <= linear_tol(dt, D, np.max(np.abs(V)), w)), V.dtype


class _Recorder:
    def __init__(self, pol):
        self.pol, self.q = pol, []

    def __call__(self, *x):
        self.q.append(tuple(float(v) for v in x))
        return self.pol(*x)


def test_nearest_policy_float32_decides_like_the_host(env):
    """A float32 policy table queried just below a cell midpoint: the host's float64 rule takes the lower knot; a
    float32 lookup rounds the query onto the midpoint and would take the upper one.  lookup_many follows the host."""
    hjbdp, _abi, c_oracle = env
    from hjbdp.solver_position import NearestPolicy
    pol = NearestPolicy([np.array([0.0, 1.0]), np.array([0.0, 1.0])], np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32))
    q = np.array([[0.5 - 2.0 ** -30, 0.25], [0.5 + 2.0 ** -30, 0.75], [0.5, 0.5 - 2.0 ** -40]])
    assert [pol(*p) for p in q] == [1.0, 4.0, 3.0]
    assert np.array_equal(pol.lookup_many(q), np.array([1.0, 4.0, 3.0], dtype=np.float32))
    # the float32 lookup itself (documented: knots, query and distances in float32) rounds onto the midpoint
    assert np.array_equal(hjbdp.policy_lookup(pol.GridVectors, pol.Values, q, "nearest"), np.array([3.0, 4.0, 4.0], np.float32))


def test_position_policy_lookups_equal_the_host(env):
    """Solver_position after a reduced sweep: the 2-D 'nearest' policies at every point the closed-loop rollout
    queries plus midpoints, knots and outside points; the value tables F_i with 'linear'."""
    hjbdp, _abi, c_oracle = env
    sp = hjbdp.Solver_position()
    sp.n_mesh_x = sp.n_mesh_v = 60
    sp.simplified_run(n_stages=120)
    recs = [_Recorder(sp.U1_Opt), _Recorder(sp.U2_Opt), _Recorder(sp.U3_Opt)]
    sp.U1_Opt, sp.U2_Opt, sp.U3_Opt = recs
    sp.get_optimal_path(n_steps=200)
    rng = np.random.default_rng(3)
    for ch, r in enumerate(recs):
        knots = r.pol.GridVectors
        pts = np.concatenate([np.array(r.q), _probe_points(rng, knots)])
        assert len(r.q) == 200
        _host_vs_gpu(hjbdp, knots, r.pol.Values, pts, linear_values=sp.F_values[ch])


def test_pos_att_controller_lookups_equal_the_host(env, monkeypatch):
    """Solver_pos_att's 4-D controller tables (_store_controller -> thruster_policies, as set_controller builds them):
    the twelve thruster policies at every point the 13-state rollout queries, plus midpoints, knots and outside
    points; F_gI_Values (float32) with 'linear'."""
    hjbdp, _abi, c_oracle = env
    from hjbdp import rollout
    from hjbdp.solver_position import NearestPolicy
    pa = hjbdp.Solver_pos_att()
    pa.n_mesh_x, pa.n_mesh_v, pa.n_mesh_t, pa.n_mesh_w = 8, 8, 6, 5
    pa.simplified_run(n_stages=40)
    seen = []
    call = NearestPolicy.__call__

    def record(self, *x):
        seen.append(tuple(float(v) for v in x))
        return call(self, *x)
    monkeypatch.setattr(NearestPolicy, "__call__", record)
    pa.get_optimal_path(n_steps=60)
    monkeypatch.setattr(NearestPolicy, "__call__", call)
    assert len(seen) == 60 * 12
    pols = rollout.thruster_policies(pa)
    rng = np.random.default_rng(4)
    for name, c in pa.controllers.items():
        if name.endswith("failure"):
            continue
        knots = [np.asarray(g, dtype=np.float64) for g in c["GridVectors"]]
        pts = np.concatenate([np.array(seen), _probe_points(rng, knots)])
        for key in ("f0_allcomb", "f1_allcomb", "f6_allcomb", "f7_allcomb"):
            table = np.asarray(c[key])[np.asarray(c["U_Optimal_id"], dtype=np.int64) - 1]
            _host_vs_gpu(hjbdp, knots, table, pts, linear_values=c["F_gI_Values"] if key == "f0_allcomb" else None)
    assert all(isinstance(p, NearestPolicy) for p in pols)


def test_attitude_6d_policy_lookups_equal_the_host(env, monkeypatch):
    """Solver_attitude.run's 6-D U1_Opt .. U3_Opt (float32, as :296-298 stores them) at every point the rollout
    queries ('nearest' and 'linear' rollouts), plus midpoints, knots and outside points."""
    hjbdp, _abi, c_oracle = env
    from hjbdp import matlab_compat
    sa = hjbdp.Solver_attitude(n_mesh_w=5, n_mesh_q=4)
    sa.run(n_stages=6)
    assert sa.U1_Opt.dtype == np.float32 and sa.U1_Opt.ndim == 6
    seen = []
    near, lin = matlab_compat.interp_nearest_point, matlab_compat.interp_linear_point
    monkeypatch.setattr(matlab_compat, "interp_nearest_point", lambda k, V, x: (seen.append(tuple(map(float, x))), near(k, V, x))[1])
    monkeypatch.setattr(matlab_compat, "interp_linear_point", lambda k, V, x: (seen.append(tuple(map(float, x))), lin(k, V, x))[1])
    sa.get_optimal_path(n_steps=30)
    sa.get_optimal_path(method="linear", n_steps=30)
    monkeypatch.setattr(matlab_compat, "interp_nearest_point", near)
    monkeypatch.setattr(matlab_compat, "interp_linear_point", lin)
    assert len(seen) == 2 * 30 * 3
    knots = sa.grid_vectors_full()
    pts = np.concatenate([np.array(seen), _probe_points(np.random.default_rng(5), knots)])
    for T in (sa.U1_Opt, sa.U2_Opt, sa.U3_Opt):
        _host_vs_gpu(hjbdp, knots, T, pts, linear_values=T)


# ---- k_probe ------------------------------------------------------------------------------------------------------------
PROBE_SHAPES = {   # D: (generator, n, m)
    1: ("random", (7,), (5,)),
    2: ("nested", (6, 5), (3, 4)),
    3: ("random", (5, 4, 6), (3, 2, 4)),
    4: ("nested", (4, 5, 3, 4), (6,)),
    5: ("random", (3, 4, 3, 3, 4), (3, 2)),
    6: ("nested", (3, 3, 4, 3, 3, 3), (2, 3, 2)),
}


def _probe_spec(hjbdp, D, storage, seed=0):
    from problems import nested_problem, random_problem
    kind, n, m = PROBE_SHAPES[D]
    dtype = np.float64 if storage == "f64" else np.float32
    gen = random_problem if kind == "random" else nested_problem
    spec = gen(1000 + 10 * D + seed, n, m, dtype=dtype, nonuniform=(D % 2 == 1))
    if storage == "f16s":
        spec = hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, dtype=np.float32,
                                 index_base=spec.index_base, j_storage=np.float16)
    return spec


def _probe_blocks(spec, rng):
    """The whole grid (first and last index of every axis) at the last level of every control dim, one state at a
    random control, and a block against the upper ends at the first levels."""
    n, m = spec.n, spec.m
    whole = ((0,) * spec.D, n, tuple(x - 1 for x in m))
    s = tuple(int(rng.integers(0, x)) for x in n)
    one = (s, tuple(x + 1 for x in s), tuple(int(rng.integers(0, x)) for x in m))
    top = (tuple(max(0, x - 2) for x in n), n, (0,) * spec.C)
    return [whole, one, top]


def _j_of(J, spec):
    """J_next as the kernels read it: binary16 decoded to float32."""
    return np.asarray(J).astype(spec.dtype).reshape(spec.n, order="F")


def _check_probe(c_oracle, _abi, spec, block, got, J):
    """g and x_next = the terms' ordered sums in the spec's dtype, bit for bit; j_interp = the twin's lookup of J at
    those next states, bit for bit, and hjb_oracle.interp_linear (unfused lerps) / scipy in float64 to linear_tol; g
    and x_next against float64 sums to (terms) float units of the sum of |terms|."""
    from oracle import hjb_oracle
    lo, hi, ctrl = block
    D, dt = spec.D, spec.dtype
    ext = tuple(h - l for l, h in zip(lo, hi))
    eps = np.finfo(dt).eps
    g_parts = [term_block(t, D, lo, hi, ctrl, dt) for t in spec.cost_terms]
    assert np.array_equal(got["g"], ordered_sum(g_parts, dt))
    g64 = sum(p.astype(np.float64) for p in g_parts)
    assert np.all(np.abs(got["g"] - g64) <= len(g_parts) * eps * sum(np.abs(p.astype(np.float64)) for p in g_parts))
    for a in range(D):
        parts = [term_block(t, D, lo, hi, ctrl, dt) for t in spec.next_terms[a]]
        assert np.array_equal(got["x_next"][..., a], ordered_sum(parts, dt)), a
        x64 = sum(p.astype(np.float64) for p in parts)
        assert np.all(np.abs(got["x_next"][..., a] - x64) <= len(parts) * eps * sum(np.abs(p.astype(np.float64)) for p in parts))
    Jd = _j_of(J, spec)
    q = got["x_next"].reshape(-1, D, order="F")
    twin = c_oracle.lookup(_abi, spec.knots, Jd, q, "linear").reshape(ext, order="F")
    assert np.array_equal(got["j_interp"], twin)
    kn = [k.astype(dt).astype(np.float64) for k in spec.knots]
    py = hjb_oracle.interp_linear([k.astype(dt) for k in spec.knots], Jd, [q[:, a] for a in range(D)]).reshape(ext, order="F")
    ref, w = linear_ref(kn, Jd, q)
    tol = linear_tol(dt, D, np.max(np.abs(Jd)), w).reshape(ext, order="F")
    assert np.all(np.abs(got["j_interp"] - py) <= 2 * tol)
    assert np.all(np.abs(got["j_interp"] - ref.reshape(ext, order="F")) <= tol)


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_probe_block_every_instantiation(env, D, storage):
    """k_probe<T, TJ, D> through hjb_probe_stage on three blocks of a small random / nested problem with C = 1..3."""
    hjbdp, _abi, c_oracle = env
    spec = _probe_spec(hjbdp, D, storage)
    rng = np.random.default_rng(D)
    J = (5.0 * rng.standard_normal(spec.nS)).astype(spec.j_dtype)
    with hjbdp.Backup(spec) as bk:
        for block in _probe_blocks(spec, rng):
            lo, hi, ctrl = block
            got = bk.probe_stage({"lo": lo, "hi": hi, "control": ctrl}, J_next=J)
            _check_probe(c_oracle, _abi, spec, block, got, J)


@pytest.mark.parametrize("D,storage", [(3, "f32"), (5, "f64"), (6, "f16s"), (1, "f16s")])
def test_probe_per_stage_in_solve(env, D, storage):
    """solve(3, probe=...): plane k of the taps is loop counter k_s = k + 1; its j_interp interpolates the J of the
    stage computed before it (k_s = 3: the terminal cost, then J_stages[:, k_s]), g and x_next are the same every
    stage and equal hjb_probe_stage's."""
    hjbdp, _abi, c_oracle = env
    spec = _probe_spec(hjbdp, D, storage, seed=1)
    rng = np.random.default_rng(20 + D)
    term = (3.0 * rng.random(spec.nS)).astype(spec.j_dtype)
    lo, hi, ctrl = _probe_blocks(spec, rng)[0]
    with hjbdp.Backup(spec) as bk:
        out = bk.solve(3, terminal=term, keep_J=True, probe={"lo": lo, "hi": hi, "control": ctrl})
        pr = out["probe"]
        for k in range(3):
            Jn = term if k == 2 else out["J_stages"][:, k + 1]
            plane = {"g": pr["g"][..., k], "x_next": pr["x_next"][..., k], "j_interp": pr["j_interp"][..., k]}
            _check_probe(c_oracle, _abi, spec, (lo, hi, ctrl), plane, Jn)
            one = bk.probe_stage({"lo": lo, "hi": hi, "control": ctrl}, J_next=Jn)
            for key in plane:
                assert np.array_equal(one[key], plane[key]), (k, key)
    assert not np.array_equal(pr["j_interp"][..., 0], pr["j_interp"][..., 2])


def test_probe_refusals(env):
    """make_probe's refusals: a state model, table_dtype HJB_TAB_F64 and cost_dtype HJB_COST_F64 are HJB_E_UNSUPPORTED,
    through hjb_probe_stage and through hjb_solve."""
    hjbdp, _abi, c_oracle = env
    from problems import pos_att_channel_spec, random_problem
    base = random_problem(5, (5, 4, 6), (3,), dtype=np.float32)
    cost64 = hjbdp.ProblemSpec(base.knots, base.m, base.next_terms, base.cost_terms, dtype=np.float32, cost_dtype=np.float64)
    tab64 = pos_att_channel_spec(cost_mode="terms", n=6)
    model = hjbdp.Solver_attitude(n_mesh_w=4, n_mesh_q=3).build_spec_model()
    for spec, word in ((model, "state model"), (tab64, "HJB_TAB_F64"), (cost64, "HJB_COST_F64")):
        block = {"lo": (0,) * spec.D, "hi": (1,) * spec.D, "control": (0,) * spec.C}
        with hjbdp.Backup(spec) as bk:
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.probe_stage(block, J_next=np.zeros(spec.nS, spec.j_dtype))
            assert ei.value.status == _abi.HJB_E_UNSUPPORTED and word in str(ei.value), str(ei.value)
            with pytest.raises(hjbdp.HjbError) as ei:
                bk.solve(2, probe=block)
            assert ei.value.status == _abi.HJB_E_UNSUPPORTED


# ---- k_fill_separable / k_gather_bytes -------------------------------------------------------------------------------------
FILL_SHAPES = {1: (37,), 2: (9, 11), 3: (5, 7, 6), 4: (4, 5, 3, 6), 5: (3, 4, 5, 3, 4), 6: (3, 4, 3, 5, 3, 4)}


def _fill_spec(hjbdp, n, storage, seed=0):
    from problems import random_problem
    dtype = np.float64 if storage == "f64" else np.float32
    spec = random_problem(2000 + seed, n, (2,), dtype=dtype)
    if storage == "f16s":
        spec = hjbdp.ProblemSpec(spec.knots, spec.m, spec.next_terms, spec.cost_terms, dtype=np.float32, j_storage=np.float16)
    return spec


def _fill_vecs(rng, n, dtype):
    """Values of mixed sign and size, so that the order of the adds and the one rounding to the storage type matter."""
    return [((rng.standard_normal(x) * 10.0 ** rng.integers(-2, 3, x)) * (1.0 + a)).astype(dtype) for a, x in enumerate(n)]


def _fill_check(spec, vecs, got, sel=None):
    """The ordered sum in the arithmetic type rounded once to storage, bit for bit; against the float64 sum to
    D float units of the sum of |v| plus half a unit of the storage type."""
    full = separable_ref(vecs, spec.dtype, spec.j_dtype)
    ref = full if sel is None else full[sel]
    assert np.array_equal(got, ref)
    v64 = [np.asarray(v, dtype=np.float64) for v in vecs]
    s64 = separable_ref(v64, np.float64, np.float64)
    a64 = separable_ref([np.abs(v) for v in v64], np.float64, np.float64)
    if sel is not None:
        s64, a64 = s64[sel], a64[sel]
    tol = spec.D * np.finfo(spec.dtype).eps * a64 + 0.5 * np.finfo(spec.j_dtype).eps * np.abs(s64) + (6e-8 if spec.j_dtype == np.float16 else 0)
    assert np.all(np.abs(got.astype(np.float64) - s64) <= tol)


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_fill_separable_every_instantiation(env, D, storage):
    """k_fill_separable<float, _Float16>, <float, float>, <double, double> over small grids of every D: every
    element read back through hjb_device_gather (and a plain copy)."""
    hjbdp, _abi, c_oracle = env
    spec = _fill_spec(hjbdp, FILL_SHAPES[D], storage, seed=D)
    rng = np.random.default_rng(30 + D)
    vecs = _fill_vecs(rng, spec.n, spec.dtype)
    esz = np.dtype(spec.j_dtype).itemsize
    with hjbdp.Backup(spec) as bk, hjbdp.DeviceBuffer(spec.nS * esz) as dJ:
        bk.fill_separable(vecs, dJ)
        sel = rng.permutation(spec.nS)
        got = dJ.gather(spec.j_dtype, sel)
        _fill_check(spec, vecs, got, sel)
        _fill_check(spec, vecs, dJ.download(spec.j_dtype))


def test_fill_separable_above_2_24_states(env):
    """One float16-stored grid of 257 x 256 x 256 = 16.8M states (> 2^24; the fill's grid-stride walk takes four
    passes): a seeded sample of 10^5 states plus the first, the last and both sides of 2^24, bit for bit."""
    hjbdp, _abi, c_oracle = env
    spec = _fill_spec(hjbdp, (257, 256, 256), "f16s", seed=99)
    assert spec.nS > 2 ** 24
    rng = np.random.default_rng(31)
    vecs = [(rng.random(x) * (1.0 + a)).astype(np.float32) for a, x in enumerate(spec.n)]
    sel = np.concatenate([rng.integers(0, spec.nS, 100000), [0, spec.nS - 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1]])
    with hjbdp.Backup(spec) as bk, hjbdp.DeviceBuffer(spec.nS * 2) as dJ:
        bk.fill_separable(vecs, dJ)
        got = dJ.gather(np.float16, sel)
    idx = np.unravel_index(sel, spec.n, order="F")
    ref = ordered_sum([vecs[a][idx[a]] for a in range(3)], np.float32).astype(np.float16)
    assert np.array_equal(got, ref)
    s64 = sum(vecs[a][idx[a]].astype(np.float64) for a in range(3))
    assert np.all(np.abs(got - s64) <= 3 * np.finfo(np.float32).eps * s64 + 0.5 * np.finfo(np.float16).eps * s64)


@pytest.mark.parametrize("storage", STORAGE)
def test_rank_fill_three_slabs(env, storage):
    """hjb_rank_fill_separable on three slabs: each rank's haloed buffer equals planes [begin - halo_lo, end + halo_hi)
    of the whole-grid fill - halo planes included - and the ordered numpy sum."""
    hjbdp, _abi, c_oracle = env
    from problems import colsweep_problem
    dtype = np.float64 if storage == "f64" else np.float32
    spec = colsweep_problem(15, (36, 7, 9, 14), gax=2, dtype=dtype, j_storage=np.float16 if storage == "f16s" else None)
    rng = np.random.default_rng(32)
    vecs = _fill_vecs(rng, spec.n, spec.dtype)
    esz = np.dtype(spec.j_dtype).itemsize
    inner, nl = spec.nS // spec.n[-1], spec.n[-1]
    with hjbdp.Backup(spec) as bk, hjbdp.DeviceBuffer(spec.nS * esz) as dW:
        bk.fill_separable(vecs, dW)
        whole = dW.download(spec.j_dtype)
    _fill_check(spec, vecs, whole)
    whole = whole.reshape(inner, nl, order="F")
    seen = []
    for rank in range(3):
        rk = hjbdp.RankSlab(spec, 0, rank, 3)
        try:
            planes = rk.end - rk.begin + rk.halo_lo + rk.halo_hi
            with hjbdp.DeviceBuffer(inner * planes * esz) as dB:
                rk.fill_separable(vecs, dB)
                got = dB.download(spec.j_dtype).reshape(inner, planes, order="F")
            assert np.array_equal(got, whole[:, rk.begin - rk.halo_lo:rk.end + rk.halo_hi]), rank
            seen.append((rk.begin, rk.end, rk.halo_lo, rk.halo_hi))
        finally:
            rk.close()
    assert seen[0][0] == 0 and seen[-1][1] == nl and seen[1][2] > 0 and seen[1][3] > 0, seen


@pytest.mark.parametrize("eb", [1, 2, 4, 8])
def test_device_gather_every_element_size(env, eb):
    """hjb_device_gather at 1, 2, 4 and 8 bytes per element: unsorted and repeated selections, the first and last
    element; at 1 byte also more selections than one launch's 65,536 x 256 grid stride."""
    hjbdp, _abi, c_oracle = env
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[eb]
    rng = np.random.default_rng(40 + eb)
    N = 100003
    src = rng.integers(0, np.iinfo(dt).max, N, dtype=dt, endpoint=True)
    n_sel = 65536 * 256 + 333 if eb == 1 else 70001
    sel = rng.integers(0, N, n_sel)
    sel[:6] = [N - 1, 0, N - 1, 0, 5, 5]
    sel[-3:] = [0, N - 1, N // 2]
    with hjbdp.DeviceBuffer(N * eb) as d:
        d.upload(src)
        got = d.gather(dt, sel)
        assert got.dtype == dt and np.array_equal(got, src[sel])
        assert d.gather(dt, np.zeros(0, np.int64)).size == 0
