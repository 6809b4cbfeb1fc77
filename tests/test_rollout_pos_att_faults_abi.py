"""CPU tests of the pos-att fault campaign (hjb_rollout_set_pos_att_fault_controller / hjb_rollout_run_pos_att_faults,
csrc/kernels_rollout_pos_att_faults.h): the prototypes agree in both headers and are exported and bound; null objects are statuses;
every K23 instantiation compiles for gfx950 without spilling; the numpy twin the GPU tests hold K23 to
(tests/pos_att_fault_rollout_refs.py) equals K18's twin when nothing is set, and the scalar host loop
(hjbdp/rollout.py::pos_att_fault_path_fixed) equals the twin bit for bit."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np

import pos_att_fault_rollout_refs as fr
import pos_att_rollout_refs as pr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "optimal-control-dynamic-programming_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW_FNS = ("hjb_rollout_set_pos_att_fault_controller", "hjb_rollout_run_pos_att_faults")
KEYS = ("X_final", "X_path", "F_path", "FM_path")


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_fault_prototypes_are_identical_in_both_headers_and_bound(built):
    import hjbdp
    from hjbdp import _abi
    from test_abi import _prototypes
    lib = hjbdp.load_library()
    full = _prototypes((ROOT / "include" / "hjbdp.h").read_text())
    flat = _prototypes((ROOT / "include" / "hjbdp_matlab.h").read_text())
    for name in NEW_FNS:
        assert name in full and name in flat and full[name] == flat[name], name
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
        assert len(_abi.SYMBOLS[name][1]) == len(full[name]), name
    assert full["hjb_rollout_set_pos_att_fault_controller"] == ["void*", "void*"]
    assert full["hjb_rollout_run_pos_att_faults"] == ["void*", "int32_t", "int32_t*", "int64_t", "double*", "int32_t*", "int32_t*",
                                                      "int32_t*", "double", "double", "double*", "double*", "int32_t*", "double*",
                                                      "double*", "double*", "double*"]
    assert hasattr(hjbdp.Rollout, "set_pos_att_fault_controller") and hasattr(hjbdp.Rollout, "run_pos_att_faults")
    assert hasattr(hjbdp.Solver_pos_att, "get_fault_campaign")


def test_null_objects_are_statuses(built):
    import hjbdp
    from hjbdp import _abi
    lib = hjbdp.load_library()
    assert lib.hjb_rollout_set_pos_att_fault_controller(None, None) == _abi.HJB_E_INVALID
    assert b"null handle" in lib.hjb_rollout_last_error(None)
    X = np.zeros(13)
    p = X.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.hjb_rollout_run_pos_att_faults(None, 0, None, 1, p, None, None, None, 1.0, 1.0, p, None, None, None, None, None,
                                              None) == _abi.HJB_E_INVALID
    assert b"null handle" in lib.hjb_rollout_last_error(None)


def test_fault_kernel_register_budget(tmp_path):
    """every K23 instantiation (label type x LDS) compiled for gfx950: no VGPR spill, no private segment and no scratch or buffer
    access in any of the six, as K18's own metadata test asks of K18.  The VGPR counts are printed (DESIGN 4b records them)."""
    import __graft_entry__ as g
    asm = tmp_path / "paf.s"
    r = subprocess.run([HIPCC, *g.HIPCC_FLAGS, "-S", "--cuda-device-only", "-o", str(asm), str(CSRC / "rollout_pos_att_faults.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = asm.read_text()
    got = re.findall(r"\.name:\s+(_ZN3hjb24k_rollout_pos_att_faults\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                     r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(got) == 6, [k[0] for k in got]
    for name, scratch, vgprs, spills in got:
        print(name, "vgprs", vgprs, "private segment", scratch, "vgpr spills", spills)
        assert int(spills) == 0 and int(scratch) == 0, (name, scratch, vgprs, spills)
    bodies = re.findall(r"^(_ZN3hjb24k_rollout_pos_att_faults\S*):.*\n((?:.*\n)*?)\s+s_endpgm", text, flags=re.M)
    assert len(bodies) == 6
    for name, body in bodies:
        assert not re.search(r"\b(scratch_|buffer_(load|store))", body), name


def _random_channel(rng, n_labels, n_planes, knots_range=(4, 8)):
    from hjbdp.matlab_compat import sym_linspace_pos_att
    lo, hi = knots_range
    knots = [sym_linspace_pos_att(-0.2, 0.2, int(rng.integers(lo, hi))), sym_linspace_pos_att(-0.1, 0.1, int(rng.integers(lo, hi))),
             sym_linspace_pos_att(-0.1, 0.1, int(rng.integers(lo, hi))), sym_linspace_pos_att(-0.035, 0.035, int(rng.integers(lo, hi)))]
    shape = tuple(len(k) for k in knots)
    labels = rng.integers(1, 1 + n_labels, size=shape + ((n_planes,) if n_planes > 1 else ())).astype(np.uint8)
    ut = rng.choice([0.0, 0.13, -0.13], size=(n_labels, 4)) * rng.uniform(0.5, 1.0, size=(n_labels, 4))
    return knots, labels, ut


def _starts(rng, n):
    X = np.empty((13, n))
    X[0:3] = rng.uniform(-0.25, 0.25, size=(3, n))
    X[3:6] = rng.uniform(-0.12, 0.12, size=(3, n))
    ang = rng.uniform(-0.12, 0.12, size=(3, n))
    X[6:9] = np.sin(ang / 2)
    X[9] = np.sqrt(1.0 - (X[6:9] ** 2).sum(axis=0))
    X[10:13] = rng.uniform(-0.04, 0.04, size=(3, n))
    return X


def test_twin_with_nothing_set_equals_the_pos_att_twin_bit_for_bit(built):
    from hjbdp.rollout import pos_att_orbit_table
    rng = np.random.default_rng(230)
    chans = [c + (1,) for c in (_random_channel(rng, 20, 3) for _ in range(3))]
    fault = _random_channel(rng, 15, 3, (3, 6)) + (1,)
    J = np.array([[0.02852, -0.0000837, 0.000014], [-0.0000837, 0.028317, -0.00029], [0.000014, -0.00029, 0.0245]])
    X0 = _starts(rng, 40)
    for S in (1, 2):
        K, h = 20, 0.01
        planes = rng.integers(0, 3, size=K)
        rsw, coef = pos_att_orbit_table(K, h, S)
        ref = pr.rollout(chans, J, 4.16, 9.65e-2, h, S, rsw, coef, X0, planes)
        for fc, kw in ((None, {}), (fault, dict(switch_stage=np.full(40, K), fault_mask=np.zeros(40, int))),
                       (fault, dict(fault_mask=np.full(40, 0xFFF), fault_stage=np.full(40, K + 3)))):
            got = fr.rollout(chans, fc, J, 4.16, 9.65e-2, h, S, rsw, coef, X0, planes, **kw)
            for key, r in zip(KEYS, ref):
                assert _bits(got[key], r), (S, key)
            assert _bits(got["F_cmd"], got["F_path"]) and _bits(got["Fx_nominal"], got["F_path"][:, [0, 1, 6, 7]])
            assert (got["settle_stage"] == 0).all() and (got["impulse"] > 0).all()
            # 240 non-negative terms summed in another order: relative difference <= 240 * 2^-53 < 1e-13
            assert np.allclose(got["impulse"], np.abs(ref[2]).sum(axis=(1, 2)) * h, rtol=1e-13, atol=0)


def test_host_loop_equals_the_twin_bit_for_bit(built):
    """pos_att_fault_path_fixed against the twin on random small channels: 64 stages, 16 starts, mixed faults and hand-overs, both
    tolerances finite; with nothing set it returns pos_att_optimal_path_fixed's arrays."""
    import hjbdp
    from hjbdp.rollout import pos_att_fault_path_fixed, pos_att_optimal_path_fixed, pos_att_orbit_table
    rng = np.random.default_rng(231)
    pa = hjbdp.Solver_pos_att()
    names = ("channel_x_controller_1", "channel_y_controller_1", "channel_z_controller_1", "channel_x_controller_1_failure")
    raw = [_random_channel(rng, 20, 1) for _ in range(3)] + [_random_channel(rng, 12, 1, (3, 6))]
    raw[3][2][:, 0] = 0.0                                      # the failure controller never commands f0
    pa.controllers = {nm: {"GridVectors": k, "U_Optimal_id": lab, "f0_allcomb": ut[:, 0], "f1_allcomb": ut[:, 1], "f6_allcomb": ut[:, 2],
                           "f7_allcomb": ut[:, 3]} for nm, (k, lab, ut) in zip(names, raw)}
    n, K = 16, 64
    X0 = _starts(rng, n)
    mask = rng.integers(0, 4096, size=n)
    mask[::3] = 0
    f_at = rng.integers(0, K + 9, size=n)
    s_at = rng.integers(0, K + 9, size=n)
    chans = [c + (1,) for c in raw[:3]]
    fault = raw[3] + (1,)
    for S in (1, 2):
        rsw, coef = pos_att_orbit_table(K, pa.h, S)
        probe = fr.rollout(chans, fault, pa.InertiaM, pa.Mass, pa.T_dist, pa.h, S, rsw, coef, X0, np.zeros(K, int), mask, f_at, s_at)
        pos_tol = float(np.median(np.sqrt((probe["X_path"][:, 0:3] ** 2).sum(axis=1))))
        att_tol = float(np.percentile(np.sqrt((probe["X_path"][:, 6:9] ** 2).sum(axis=1)), 80))
        tw = fr.rollout(chans, fault, pa.InertiaM, pa.Mass, pa.T_dist, pa.h, S, rsw, coef, X0, np.zeros(K, int), mask, f_at, s_at,
                        pos_tol, att_tol)
        assert (tw["F_cmd"] != tw["F_path"]).any() and (tw["Fx_nominal"] != tw["F_cmd"][:, [0, 1, 6, 7]]).any()
        assert len(set(tw["settle_stage"].tolist())) >= 3, tw["settle_stage"]
        for i in range(n):
            T, X, F, FM, imp, settle = pos_att_fault_path_fixed(pa, X0[:, i], int(mask[i]), int(f_at[i]), int(s_at[i]), n_steps=K,
                                                                 substeps=S, pos_tol=pos_tol, att_tol=att_tol)
            assert X.shape == (K + 1, 13) and F.shape == (K + 1, 12) and FM.shape == (K + 1, 6) and not F[K].any() and not FM[K].any()
            assert _bits(tw["X_path"][i].T, X) and _bits(tw["F_path"][i].T, F[:K]) and _bits(tw["FM_path"][i].T, FM[:K]), (S, i)
            assert _bits(tw["impulse"][i], imp) and int(tw["settle_stage"][i]) == settle, (S, i, imp, settle)
        for i in range(3):
            base = pos_att_optimal_path_fixed(pa, X0[:, i], n_steps=K, substeps=S)
            for kw in (dict(fault_mask=None, fault_stage=None, switch_stage=None), dict(fault_mask=0, fault_stage=0, switch_stage=K),
                       dict(fault_mask=0xFFF, fault_stage=K, switch_stage=None)):
                got = pos_att_fault_path_fixed(pa, X0[:, i], n_steps=K, substeps=S, **kw)
                assert all(_bits(g, b) for g, b in zip(got[:4], base)), (S, i, kw)
                assert got[5] == 0
