// kernels_rollout_pos_att_body.inc - the pos-att stage: the body of k_rollout_pos_att (K18, kernels_rollout_pos_att.h) and of
// k_rollout_pos_att_faults (K23, kernels_rollout_pos_att_faults.h), written once.
//
// Included between the braces of each kernel's definition with HJB_PA_BODY_FAULTS set to 0 (K18) or 1 (K23); it reads the
// includer's parameters (CX CY CZ M nc X0 Xf Xp Fp FMp, and CXF Q when the switch is on) and template arguments (TL, LDS).  The
// parts under the switch are all there is to K23: the fourth channel's staging and pointers, the three per-trajectory inputs, the
// hand-over branch around channel x's lookup, the dead-thruster select, the impulse sum, last_outside and the two tail stores.
// Shared as text, not as a function: behind a force-inlined template both kernels are allocated fewer registers and run more
// instructions, and one __global__ template with a FAULTS argument moves K18's kernel arguments and renames both kernels; with the
// switch off the preprocessed text is K18 as it was written out, and each kernel's code object is what its own copy gave.
    extern __shared__ double smem[];
    const double *knx, *rdx_, *utx, *kny, *rdy, *uty, *knz, *rdz, *utz;
    // per channel [knots | 1/dx | u_table], x then y then z then the fault controller (nothing of it when none is attached)
    HJB_ROLLOUT_PLACE(x, CX, 4, smem)
    HJB_ROLLOUT_PLACE(y, CY, 4, HJB_ROLLOUT_PLACE_END(x))
    HJB_ROLLOUT_PLACE(z, CZ, 4, HJB_ROLLOUT_PLACE_END(y))
#if HJB_PA_BODY_FAULTS
    const double *knf, *rdf, *utf;
    HJB_ROLLOUT_PLACE(f, CXF, 4, HJB_ROLLOUT_PLACE_END(z))
#endif
    HJB_ROLLOUT_STAGE(LDS, x, CX, knx, rdx_, utx)
    HJB_ROLLOUT_STAGE(LDS, y, CY, kny, rdy, uty)
    HJB_ROLLOUT_STAGE(LDS, z, CZ, knz, rdz, utz)
#if HJB_PA_BODY_FAULTS
    HJB_ROLLOUT_STAGE(LDS, f, CXF, knf, rdf, utf)
#endif
    if constexpr (LDS) __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const TL *__restrict__ labx = static_cast<const TL *>(CX.labels);
    const TL *__restrict__ laby = static_cast<const TL *>(CY.labels);
    const TL *__restrict__ labz = static_cast<const TL *>(CZ.labels);
    const int64_t nlx = CX.n_labels, nly = CY.n_labels, nlz = CZ.n_labels;
    const double hs = M.hs;
    const int S = M.substeps;
#if HJB_PA_BODY_FAULTS
    const TL *__restrict__ labf = static_cast<const TL *>(CXF.labels);
    const int64_t nlf = CXF.n_labels;
    const int n_steps = M.n_steps;
    // a stage that never comes is n_steps: the host let a hand-over before n_steps through only with a fault controller attached
    const int mask = Q.mask ? Q.mask[i] : 0;
    const int fault_at = Q.fault_stage ? Q.fault_stage[i] : 0;
    const int switch_at = Q.switch_stage ? Q.switch_stage[i] : n_steps;
#endif
    double x[HJB_PA_W];
#pragma unroll
    for (int a = 0; a < HJB_PA_W; ++a) x[a] = X0[a + (int64_t)HJB_PA_W * i];
    if (Xp) {
#pragma unroll
        for (int a = 0; a < HJB_PA_W; ++a) Xp[i + nc * a] = x[a];
    }
#if HJB_PA_BODY_FAULTS
    double imp = 0.0;
    int last_outside = pa_inside(x, Q.p2, Q.a2) ? -1 : 0;
#endif
    for (int k = 0; k < M.n_steps; ++k) {
        double th[3], xb[3], vb[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = x[6 + j];
            s = s > 1.0 ? 1.0 : s < -1.0 ? -1.0 : s;
            th[j] = 2.0 * canon_asin(s);
        }
        {
            double E[9], R[9];
            pa_eci2body(x[6], x[7], x[8], x[9], E);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) R[3 * r + c] = (E[3 * r] * M.RSW[c] + E[3 * r + 1] * M.RSW[3 + c]) + E[3 * r + 2] * M.RSW[6 + c];
            }
            pa_mul3(R, x[0], x[1], x[2], xb);
            pa_mul3(R, x[3], x[4], x[5], vb);
        }
        double f[HJB_PA_F];
        {
            const double p[4] = {xb[0], vb[0], th[1], x[11]};
#if HJB_PA_BODY_FAULTS
            if (switch_at <= k) {                                  // the fault controller has taken over
                HJB_ROLLOUT_LOOKUP(4, 4, HJB_LOOKUP_NEAREST, CXF, knf, rdf, utf, labf, k, p, 4, nlf, u)
                f[0] = u[0];
                f[1] = u[1];
                f[6] = u[2];
                f[7] = u[3];
            } else
#endif
            {
                HJB_ROLLOUT_LOOKUP(4, 4, HJB_LOOKUP_NEAREST, CX, knx, rdx_, utx, labx, k, p, 4, nlx, u)
                f[0] = u[0];
                f[1] = u[1];
                f[6] = u[2];
                f[7] = u[3];
            }
        }
        {
            const double p[4] = {xb[1], vb[1], th[2], x[12]};
            HJB_ROLLOUT_LOOKUP(4, 4, HJB_LOOKUP_NEAREST, CY, kny, rdy, uty, laby, k, p, 4, nly, u)
            f[2] = u[0];
            f[3] = u[1];
            f[8] = u[2];
            f[9] = u[3];
        }
        {
            const double p[4] = {xb[2], vb[2], th[0], x[10]};
            HJB_ROLLOUT_LOOKUP(4, 4, HJB_LOOKUP_NEAREST, CZ, knz, rdz, utz, labz, k, p, 4, nlz, u)
            f[4] = u[0];
            f[5] = u[1];
            f[10] = u[2];
            f[11] = u[3];
        }
#if HJB_PA_BODY_FAULTS
        // what the plant gets: a dead thruster applies +0.0
        {
            const int dead = fault_at <= k ? mask : 0;
#pragma unroll
            for (int j = 0; j < HJB_PA_F; ++j) f[j] = ((dead >> j) & 1) ? 0.0 : f[j];
        }
        {
            double s = fabs(f[0]) + fabs(f[1]);
#pragma unroll
            for (int j = 2; j < HJB_PA_F; ++j) s = s + fabs(f[j]);
            imp = imp + s;
        }
#endif
        double um[3], acc3[3];
        um[0] = (((f[4] - f[5]) + f[10]) - f[11]) * M.t_dist;
        um[1] = (((f[0] - f[1]) + f[6]) - f[7]) * M.t_dist;
        um[2] = (((f[2] - f[3]) + f[8]) - f[9]) * M.t_dist;
        {
            const double ab0 = (((f[0] + f[1]) + f[6]) + f[7]) / M.mass;
            const double ab1 = (((f[2] + f[3]) + f[8]) + f[9]) / M.mass;
            const double ab2 = (((f[4] + f[5]) + f[10]) + f[11]) / M.mass;
            double E[9], Ei[9], ae[3];
            pa_eci2body(x[6], x[7], x[8], x[9], E);
            pa_inv3(E, Ei);
            pa_mul3(Ei, ab0, ab1, ab2, ae);
            pa_mul3(M.RSWinv, ae[0], ae[1], ae[2], acc3);
        }
        if (Fp) {
#pragma unroll
            for (int j = 0; j < HJB_PA_F; ++j) Fp[i + nc * (j + (int64_t)HJB_PA_F * k)] = f[j];
        }
        if (FMp) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                FMp[i + nc * (j + (int64_t)HJB_PA_FM * k)] = acc3[j];
                FMp[i + nc * (3 + j + (int64_t)HJB_PA_FM * k)] = um[j];
            }
        }
        for (int s = 0; s < S; ++s) {
            const double *c = M.coef + 5 * (2 * ((int64_t)S * k + s));
#define HJB_PA_RHS(j_, y_, r_) pa_rates(M, c + 5 * ((j_ + 1) / 2), acc3, um, y_, r_)      /* nodes c + 5 * {0, 1, 1, 2} */
            HJB_ROLLOUT_RK4_STEP(HJB_PA_W, x, x, hs, HJB_PA_RHS)
#undef HJB_PA_RHS
        }
        if (Xp) {
#pragma unroll
            for (int a = 0; a < HJB_PA_W; ++a) Xp[i + nc * (a + (int64_t)HJB_PA_W * (k + 1))] = x[a];
        }
#if HJB_PA_BODY_FAULTS
        if (!pa_inside(x, Q.p2, Q.a2)) last_outside = k + 1;
#endif
    }
#pragma unroll
    for (int a = 0; a < HJB_PA_W; ++a) Xf[a + (int64_t)HJB_PA_W * i] = x[a];
#if HJB_PA_BODY_FAULTS
    if (Q.impulse) Q.impulse[i] = imp * Q.h;
    if (Q.settle) Q.settle[i] = last_outside + 1;
#endif
