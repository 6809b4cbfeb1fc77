// kernels_rollout_campaign_body.inc - K28's flight: the body of k_rollout_campaign (kernels_rollout_campaign.h) and of
// k_rollout_campaign_hist (K30, kernels_rollout_campaign_hist.h) up to the block partial, written once.
//
// Included between the braces of each kernel's definition.  It reads the includer's K (a DCampaignArgs: the kernel's argument, or
// the first member of it - the record is reread where it lies, at the start of the argument segment) and template arguments
// (D, TL, METHOD, LDS), and leaves behind what the tail of a campaign kernel needs: K0 (the record in the argument segment), t, lb,
// slot, G, s, m, live, the slot values v (campaign_padding() in a lane that flew nothing) and the three flags.  Shared as text, the
// way kernels_rollout_pos_att_body.inc is and for its reason: the preprocessed text of k_rollout_campaign is what it was written
// out, and its code objects are instruction for instruction what its own copy gave.
    extern __shared__ double smem[];
    const double *kn, *rd, *ut, *nt;
    HJB_ROLLOUT_PLACE(p, K.R, K.R.n_u, smem)
    HJB_ROLLOUT_STAGE(LDS, p, K.R, kn, rd, ut)
    HJB_ROLLOUT_STAGE_NOISE(LDS, p, K.N, nt)
    if constexpr (LDS) __syncthreads();
    typedef __attribute__((address_space(4))) DCampaignArgs KArgs;
    const KArgs &K0 = *(const KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t lb, s, m;
    int slot, G;
    const bool live = campaign_lane(record_reread(K0).C, t, lb, slot, G, s, m);
    CampVals v = campaign_padding();
    bool f_exceed = false, f_left = false, f_settled = false;
    if (live) {
        double x[D];
        uint64_t stream;
        {
            const KArgs &Kk = record_reread(K0);
            stream = Kk.N.first + (uint64_t)(s * Kk.C.M + m);
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = Kk.X0[a + (int64_t)D * s];
#pragma unroll
            for (int a = 0; a < D; ++a) f_left = f_left || campaign_outside(x[a], Kk.C.lo[a], Kk.C.hi[a]);
        }
        uint32_t rw[4] = {0u, 0u, 0u, 0u};
        double J = 0.0;
        for (int k = 0; k < record_reread(K0).R.n_steps; ++k) {
            const KArgs &Kl = record_reread(K0);              // the lookup's part of the record
            const TL *__restrict__ lab = static_cast<const TL *>(Kl.R.labels);
            const int nu = Kl.R.n_u;
            const int64_t nl = Kl.R.n_labels;
            HJB_ROLLOUT_LOOKUP(D, HJB_ROLLOUT_MAX_U, METHOD, Kl.R, kn, rd, ut, lab, k, x, nu, nl, u)
            // the record again for the cost, and again for each row of A and of B
            HJB_ROLLOUT_AFFINE_STEP(D, HJB_ROLLOUT_MAX_U, campaign_reread_in_step<D>(K0, Kl).R, campaign_reread_in_step<D>(K0, Kl).R,
                                    x, u, nu, g, xn)
            J = J + g;
            const KArgs &Kn = campaign_reread_in_step<D>(K0, Kl);      // the noise set and the grid's extent
            const int n_nodes = Kn.N.n_nodes;
            int w;
            HJB_ROLLOUT_NOISE_STEP(D, Kn.N.seed, stream, k, rw, nt, nt + (n_nodes - 1), n_nodes, Kn.N.mask, xn, w)
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = xn[a];
#pragma unroll
            for (int a = 0; a < D; ++a) f_left = f_left || campaign_outside(x[a], Kn.C.lo[a], Kn.C.hi[a]);
        }
        const KArgs &Kk = record_reread(K0);
        double tol[D];
#pragma unroll
        for (int a = 0; a < D; ++a) tol[a] = Kk.C.tol[a];
        f_settled = campaign_settled(D, x, Kk.C.has_tol ? tol : nullptr);
        f_exceed = campaign_exceeds(J, Kk.C.threshold != nullptr, Kk.C.threshold ? Kk.C.threshold[s] : 0.0);
        v = campaign_slot(J, f_settled);
    }
