// kernels_rollout_lookahead_campaign_body.inc - K29's flight: the body of k_rollout_lookahead_campaign
// (kernels_rollout_lookahead_campaign.h) and of k_rollout_lookahead_campaign_hist (K30, kernels_rollout_lookahead_campaign_hist.h)
// up to the block partial, written once.
//
// Included between the braces of each kernel's definition.  It reads the includer's K (a DLookCampaignArgs: the kernel's argument,
// or the first member of it - the record is reread where it lies, at the start of the argument segment) and template arguments
// (D, TV, LDS), and leaves behind K0 (the record in the argument segment), t, lb, slot, G, s, m, live, the slot values v
// (campaign_padding() in a lane that flew nothing), f_exceed, f_settled and n_out.  Shared as text, the way
// kernels_rollout_campaign_body.inc is and for its reason.
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, K.R, K.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, K.R, kn, rd, ut)
    HJB_ROLLOUT_STAGE_NOISE(LDS, p, K.N, nt)
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DLookCampaignArgs KArgs;
    const KArgs &K0 = *(const KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t lb, s, m;
    int slot, G;
    const bool live = campaign_lane(record_reread(K0).C, t, lb, slot, G, s, m);
    CampVals v = campaign_padding();
    bool f_exceed = false, f_settled = false;
    uint32_t n_out = 0u;                                      // 1 once a visited state lay outside the grid, as a word per lane: a vector register,
                                                              // where a flag carried round the step loop is a pair of scalar ones
    if (live) {
        double x[D];
        uint64_t stream;
        {
            const KArgs &Kk = record_reread(K0);
            stream = Kk.N.first + (uint64_t)(s * Kk.C.M + m);
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = Kk.X0[a + (int64_t)D * s];
#pragma unroll
            for (int a = 0; a < D; ++a) n_out |= campaign_outside(x[a], Kk.C.lo[a], Kk.C.hi[a]) ? 1u : 0u;
        }
        uint32_t rw[4] = {0u, 0u, 0u, 0u};
        double J = 0.0;
        for (int k = 0; k < record_reread(K0).R.n_steps; ++k) {
            double u[HJB_ROLLOUT_MAX_U], g, best;
            int label;
            {
                const KArgs &Kk = record_reread(K0);
                const int32_t p = Kk.R.plane_of_step[k];
                const TV *plane = p < 0 ? nullptr : static_cast<const TV *>(Kk.values) + (int64_t)p * Kk.R.nS;
                look_step<D, TV>(K0.R, K0.L, kn, rd, ut, plane, x, u, g, label, best);
            }
            J = J + g;
            {
                const KArgs &Kn = record_reread(K0);              // the flight set
                int w;
                // the global form takes the block from the record here: it holds no pointer to it across look_step
                HJB_ROLLOUT_NOISE_STEP(D, Kn.N.seed, stream, k, rw, (LDS ? nt : Kn.N.tab), (LDS ? nt : Kn.N.tab) + (Kn.N.n_nodes - 1),
                                       Kn.N.n_nodes, Kn.N.mask, x, w)
            }
            const KArgs &Kc = record_reread(K0);              // the grid's extent
#pragma unroll
            for (int a = 0; a < D; ++a) n_out |= campaign_outside(x[a], Kc.C.lo[a], Kc.C.hi[a]) ? 1u : 0u;
        }
        const KArgs &Kk = record_reread(K0);
        (void)campaign_lane(Kk.C, t, lb, slot, G, s, m);          // the start again: not held across the flight
        double tol[D];
#pragma unroll
        for (int a = 0; a < D; ++a) tol[a] = Kk.C.tol[a];
        f_settled = campaign_settled(D, x, Kk.C.has_tol ? tol : nullptr);
        f_exceed = campaign_exceeds(J, Kk.C.threshold != nullptr, Kk.C.threshold ? Kk.C.threshold[s] : 0.0);
        v = campaign_slot(J, f_settled);
    }
