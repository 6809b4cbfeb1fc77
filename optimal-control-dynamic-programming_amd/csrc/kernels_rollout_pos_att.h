// kernels_rollout_pos_att.h - K18: batched closed-loop rollouts of the 13-state pos-att loop (hjb_rollout_run_pos_att).
//
// pos-att/Solver_pos_att.m:452-730 (get_optimal_path after simplified_run) for many initial states at once: one thread per
// trajectory, all n_steps stages in one launch, everything in double, left to right, every product rounded (-ffp-contract=off).
// The state is the reference's X = [x(3) v(3) q(4) w(3)] (q4 scalar, x and v in the target's RSW frame).  Per stage k:
//   t_i = 2 * canon_asin(clamp(X[6+i], -1, 1)), i = 0..2 (:490-492; the clamp is ours, the reference would go complex);
//   E = ECI2body(q) (:825-829), M = E * RSW (RSW = RSW2ECI(R0, V0), constant: the model's), xb = M x, vb = M v (:411-415);
//   three 'nearest' lookups with K16's HJB_ROLLOUT_LOOKUP (D = 4, four thruster levels each) on plane plane_of_step[k]:
//     channel x at (xb0, vb0, t_y, w_y) -> f0 f1 f6 f7, y at (xb1, vb1, t_z, w_z) -> f2 f3 f8 f9,
//     z at (xb2, vb2, t_x, w_x) -> f4 f5 f10 f11 (:434-447);
//   to_Moments_Forces (:804-823): U_M = [(f4-f5+f10-f11) (f0-f1+f6-f7) (f2-f3+f8-f9)] * T_dist, a_body = thrust sums / Mass,
//     a = RSWinv * (inv3(E) * a_body): inv3 is the adjugate over the determinant below (E is only nearly orthogonal: q is not
//     renormalised in this loop, as in the reference), RSWinv = inv3(RSW) formed once by the same rule (pa_inv3, host side);
//   S classical RK4 sub-steps of hs = h / S with a and U_M held (:504, :705-727).  The right-hand side needs the target's orbit
//     only through five scalars of t (pa_rates); they come from the host-built table `coef` (hjbdp/orbit.py stays the only Kepler
//     solver): sub-step s of stage k reads nodes 2 (S k + s) + {0, 1, 1, 2}, five doubles each, the same for the whole wave.
//     w_dot = Jinv (U_M - w x (J w)), Jinv = inv3(J).  No quaternion renormalisation.
// Neither an RK4 temporary nor E is live across the lookups (E is formed again for the inverse).  Labels were range-checked by
// hjb_rollout_create and find_cell clamps every query (NaN -> cell 0), so a state that leaves the grids or stops being finite
// reads inside the label arrays.  The numpy restatement is tests/pos_att_rollout_refs.py, the scalar host loop
// hjbdp/rollout.py::pos_att_optimal_path_fixed.  The stage itself is kernels_rollout_pos_att_body.inc, shared with K23
// (kernels_rollout_pos_att_faults.h); this header keeps the structs, the helpers and the kernel's declaration.
#pragma once
#include "hjbdp_dev.h"
#include "kernels_rollout.h"
#include "kernels_rollout_attitude.h"   // canon_asin

namespace hjb {

#define HJB_PA_W 13                   // state width
#define HJB_PA_F 12                   // thrusters
#define HJB_PA_FM 6                   // Force_Moment row: a_x a_y a_z U_M

// One channel's policy: what HJB_ROLLOUT_LOOKUP reads of a DRollout at D = 4, without the affine model (A, B, c, q, r)
struct DPaChan {
    int32_t n[4], koff[4], uniform[4];
    double x0[4], inv_h[4];
    int64_t stride[4];
    int64_t nS;
    int32_t n_knots, n_labels, index_base, pad_;
    const double *knots, *rdx;        // [n_knots] each (global)
    const double *u_table;            // [n_labels, 4] column-major (global)
    const void *labels;               // [nS, n_planes] column-major, TL
    const int32_t *plane_of_step;     // [n_steps]
};

struct DPosAtt {
    double J[9], Jinv[9];             // row-major: J[3 r + c]
    double RSW[9], RSWinv[9];
    double mass, t_dist, hs;          // hs = h / substeps
    int32_t substeps, n_steps;
    const double *coef;               // [5, n_nodes] column-major (global)
};

// m^-1 = adj(m) / det(m), row-major, one fixed operation order (host and device; the twin repeats it)
__host__ __device__ __forceinline__ void pa_inv3(const double (&m)[9], double (&o)[9]) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[2] * m[7] - m[1] * m[8], c02 = m[1] * m[5] - m[2] * m[4];
    const double c10 = m[5] * m[6] - m[3] * m[8], c11 = m[0] * m[8] - m[2] * m[6], c12 = m[2] * m[3] - m[0] * m[5];
    const double c20 = m[3] * m[7] - m[4] * m[6], c21 = m[1] * m[6] - m[0] * m[7], c22 = m[0] * m[4] - m[1] * m[3];
    const double det = (m[0] * c00 + m[1] * c10) + m[2] * c20;
    o[0] = c00 / det;
    o[1] = c01 / det;
    o[2] = c02 / det;
    o[3] = c10 / det;
    o[4] = c11 / det;
    o[5] = c12 / det;
    o[6] = c20 / det;
    o[7] = c21 / det;
    o[8] = c22 / det;
}

__host__ __device__ __forceinline__ double pa_det3(const double (&m)[9]) {
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) + m[1] * (m[5] * m[6] - m[3] * m[8])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// y = m v, row-major m
__device__ __forceinline__ void pa_mul3(const double (&m)[9], double v0, double v1, double v2, double (&y)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = (m[3 * r] * v0 + m[3 * r + 1] * v1) + m[3 * r + 2] * v2;
}

// ECI2body(q) (:825-829), q = [q1 q2 q3 q4], q4 scalar
__device__ __forceinline__ void pa_eci2body(double q1, double q2, double q3, double q4, double (&E)[9]) {
    E[0] = 1.0 - 2.0 * (q2 * q2 + q3 * q3);
    E[1] = 2.0 * (q1 * q2 + q3 * q4);
    E[2] = 2.0 * (q1 * q3 - q2 * q4);
    E[3] = 2.0 * (q2 * q1 - q3 * q4);
    E[4] = 1.0 - 2.0 * (q1 * q1 + q3 * q3);
    E[5] = 2.0 * (q2 * q3 + q1 * q4);
    E[6] = 2.0 * (q3 * q1 + q2 * q4);
    E[7] = 2.0 * (q3 * q2 - q1 * q4);
    E[8] = 1.0 - 2.0 * (q1 * q1 + q2 * q2);
}

// f(X) of :705-727 at one table node c = [2mu/|R|^3 + H^2/|R|^4, 2 (R.V) H/|R|^4, 2H/|R|^2, mu/|R|^3 - H^2/|R|^4, mu/|R|^3]
__device__ __forceinline__ void pa_rates(const DPosAtt &M, const double *__restrict__ c, const double (&a)[3], const double (&um)[3],
                                         const double (&y)[HJB_PA_W], double (&f)[HJB_PA_W]) {
    const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4];
    f[0] = y[3];
    f[1] = y[4];
    f[2] = y[5];
    f[3] = ((c0 * y[0] - c1 * y[1]) + c2 * y[4]) + a[0];
    f[4] = ((c1 * y[0] - c3 * y[1]) - c2 * y[3]) + a[1];
    f[5] = a[2] - c4 * y[2];
    const double q1 = y[6], q2 = y[7], q3 = y[8], q4 = y[9], w1 = y[10], w2 = y[11], w3 = y[12];
    f[6] = 0.5 * (((w3 * q2) - (w2 * q3)) + (w1 * q4));
    f[7] = 0.5 * (((w1 * q3) - (w3 * q1)) + (w2 * q4));
    f[8] = 0.5 * (((w2 * q1) - (w1 * q2)) + (w3 * q4));
    f[9] = 0.5 * (((-(w1 * q1)) - (w2 * q2)) - (w3 * q3));
    double jw[3], t[3];
    pa_mul3(M.J, w1, w2, w3, jw);
    t[0] = um[0] - (w2 * jw[2] - w3 * jw[1]);
    t[1] = um[1] - (w3 * jw[0] - w1 * jw[2]);
    t[2] = um[2] - (w1 * jw[1] - w2 * jw[0]);
    double wd[3];
    pa_mul3(M.Jinv, t[0], t[1], t[2], wd);
    f[10] = wd[0];
    f[11] = wd[1];
    f[12] = wd[2];
}

template <typename TL, bool LDS>
__global__ void __launch_bounds__(256)
k_rollout_pos_att(const DPaChan CX, const DPaChan CY, const DPaChan CZ, const DPosAtt M, int64_t nc, const double *__restrict__ X0,
                  double *__restrict__ Xf, double *__restrict__ Xp, double *__restrict__ Fp, double *__restrict__ FMp) {
#define HJB_PA_BODY_FAULTS 0
#include "kernels_rollout_pos_att_body.inc"
#undef HJB_PA_BODY_FAULTS
}

// rollout_pos_att.hip instantiates the 6 kernels (label type x LDS) and launches the one asked for
hipError_t launch_rollout_pos_att(int idx_bytes, bool lds_on, const DPaChan &CX, const DPaChan &CY, const DPaChan &CZ, const DPosAtt &M,
                                  int64_t nc, size_t lds, hipStream_t st, const double *X0, double *Xf, double *Xp, double *Fp,
                                  double *FMp);

}  // namespace hjb
