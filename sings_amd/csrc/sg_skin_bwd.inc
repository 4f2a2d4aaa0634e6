// The single-frame skinned per-Gaussian backward (LBS^T) of sg_skin.hip, included there twice: SG_SKBWD_AUX 0 defines
// sg_skin_bwd_kernel<D, ACC>, SG_SKBWD_AUX 1 sg_skin_bwd_aux_kernel<D> (gradients written), whose POSED mean gradient also takes
// the depth map's dL/dz (plane `dzp`, one float per record slot, z = view row 2 . posed mean) before LBS^T takes it to xyz_canon,
// A and transl.
// (no include guard: included once per variant)
#if SG_SKBWD_AUX
// (the same register budget)
template <int D>
__global__ void __launch_bounds__(SG_SKIN_THREADS) __attribute__((amdgpu_waves_per_eu(D == 0 ? 3 : 1, D == 0 ? 3 : 10)))
sg_skin_bwd_aux_kernel(SG_SKBWD_PARAMS, const float *__restrict__ dzp)
#else
// D = 0 (what SinGS trains at): three waves per SIMD.  Unconstrained hipcc takes 196 registers = two waves per SIMD = 2 048 resident
// waves, and an avatar of 150 k Gaussians is 2 344 waves: a second, 14 %-full round (the kernel is latency-bound: a round costs what
// a wave costs).  With the hint it fits 168 registers without scratch.  D >= 1 would spill (36-52 B at D = 1): left alone.
template <int D, bool ACC>
__global__ void __launch_bounds__(SG_SKIN_THREADS) __attribute__((amdgpu_waves_per_eu(D == 0 ? 3 : 1, D == 0 ? 3 : 10)))
sg_skin_bwd_kernel(SG_SKBWD_PARAMS)
#endif
{
    constexpr bool AUX = SG_SKBWD_AUX;
#if SG_SKBWD_AUX
    constexpr bool ACC = false;
#else
    const float *const dzp = nullptr;
#endif
    constexpr bool accumulate = ACC;                            // (compile-time: see sg_preprocess_bwd_kernel)
    __shared__ float sA[SG_JMAX * 16];
    // per wave: [weights tile | T transpose scratch, later the dT tile]; between the two uses the whole 2 x 4.3 KB is
    // the staging buffer of the record sums and of the dL/dsh rows
    __shared__ float sWT[SG_SKIN_WAVES][2 * 64 * SG_WSTRIDE];
    static_assert(2 * 64 * SG_WSTRIDE >= SG_REC_CHUNK * 12 && 2 * 64 * SG_WSTRIDE >= 32 * SG_ROW_LDS, "staging buffer size");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *const sWw = sWT[wave], *const sTw = sWT[wave] + 64 * SG_WSTRIDE;
    const int g0 = (blockIdx.x * SG_SKIN_WAVES + wave) * 64;
    const int idx = g0 + lane;
    sg_load_A(k, sA);
    __syncthreads();
    float T[12];
    sg_skin_T(k.lbs_w, k.J, P, g0, lane, sA, sWw, sTw, T);
    const bool live = idx < P;
    float dT[12];
#pragma unroll
    for (int i = 0; i < 12; i++) dT[i] = 0.0f;
    float dtr[3] = { 0, 0, 0 };
    const int Mrows = c.M;
    constexpr int nc = (D + 1) * (D + 1);
    // this Gaussian's gradient records: wave-cooperative, coalesced (as in sg_preprocess_bwd_kernel)
    const bool vis = live && radii[idx] > 0 && header[1] == 0u;     // forward overflowed: zero gradients (see sg_preprocess.hip)
    float4 rc = make_float4(0, 0, 0, 0);
    if (vis) { const uint2 sl = g.slot[idx]; rc.y = __uint_as_float(sl.x); rc.w = __uint_as_float(sl.y); }
    float a9[9];
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    sg_sum_records_coop(grec, cap, vis, rc, lane, sWw, a9, rec_valid);
    const float dz = AUX ? sg_sum_dz(dzp, cap, vis, rc, rec_valid) : 0.0f;
    float dsh[nc * 3];
#pragma unroll
    for (int i = 0; i < nc * 3; i++) dsh[i] = 0.0f;
    if (live) {
        float dxc[3] = { 0, 0, 0 }, dRc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, dsc[3] = { 0, 0, 0 }, dop = 0, g2[2] = { 0, 0 };
        const bool have_in = dposed_xyz_in != nullptr || dposed_rotq_in != nullptr;
        if (vis || have_in) {
            SgPosed ps;
            sg_pose_gaussian(k, idx, T, scales, ps);
            SgGaussGrad G;
#pragma unroll
            for (int i = 0; i < 3; i++) { G.dmean[i] = 0; G.dsc[i] = 0; G.dcol[i] = 0; }
#pragma unroll
            for (int i = 0; i < 4; i++) G.drot[i] = 0;
            G.g2[0] = G.g2[1] = 0; G.dop = 0;
            if (vis)
                sg_project_bwd<D>(c, ps.p, ps.s3, ps.q, nullptr, shs + (size_t)idx * Mrows * 3, g.flags[idx], a9, true, dsh, G);
            if (AUX && vis) {
#pragma unroll
                for (int i = 0; i < 3; i++) G.dmean[i] = fmaf(dz, c.view[4 * i + 2], G.dmean[i]);
            }
            if (dposed_xyz_in) {
#pragma unroll
                for (int i = 0; i < 3; i++) G.dmean[i] += dposed_xyz_in[3 * idx + i];
            }
            if (dposed_rotq_in) {
#pragma unroll
                for (int i = 0; i < 4; i++) G.drot[i] += dposed_rotq_in[4 * idx + i];
            }
            g2[0] = G.g2[0]; g2[1] = G.g2[1]; dop = G.dop;
            // scales_posed = scales * s ; p = (T33 x + t) * s + transl
#pragma unroll
            for (int i = 0; i < 3; i++) { dsc[i] = G.dsc[i] * ps.sc; dtr[i] = G.dmean[i]; }
            float dps[3] = { G.dmean[0] * ps.sc, G.dmean[1] * ps.sc, G.dmean[2] * ps.sc };
            float dRd[9];
            sg_m2q_bwd(ps.q, ps.best, ps.qab, G.drot, dRd);
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int kx = 0; kx < 3; kx++) {
                    // dT33 = dp x^T + dRdef Rc^T
                    dT[4 * i + kx] = dps[i] * ps.x[kx] + dRd[3 * i] * ps.Rc[3 * kx] + dRd[3 * i + 1] * ps.Rc[3 * kx + 1] + dRd[3 * i + 2] * ps.Rc[3 * kx + 2];
                }
                dT[4 * i + 3] = dps[i];
            }
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
                dxc[kx] = T[kx] * dps[0] + T[4 + kx] * dps[1] + T[8 + kx] * dps[2];
#pragma unroll
                for (int j = 0; j < 3; j++)      // dRc = T33^T dRdef
                    dRc[3 * kx + j] = T[kx] * dRd[j] + T[4 + kx] * dRd[3 + j] + T[8 + kx] * dRd[6 + j];
            }
        }
        // accumulate: the frames of one optimisation step share ONE canonical-gradient buffer (sg_skinned_backward_gaussians)
        if (accumulate) {
#pragma unroll
            for (int i = 0; i < 3; i++) { dxc[i] += dL_dxyz_canon[3 * idx + i]; dsc[i] += dL_dscales[3 * idx + i]; }
            dop += dL_dopacity[idx];
        }
        dL_dxyz_canon[3 * idx] = dxc[0]; dL_dxyz_canon[3 * idx + 1] = dxc[1]; dL_dxyz_canon[3 * idx + 2] = dxc[2];
        if (dL_drot_canon) {
            if (k.rot6d) {
                float d6[6], dd[6];
#pragma unroll
                for (int i = 0; i < 6; i++) d6[i] = k.rot_canon[6 * (size_t)idx + i];
                sg_r6d2m_bwd(d6, dRc, dd);
#pragma unroll
                for (int i = 0; i < 6; i++) dL_drot_canon[6 * (size_t)idx + i] = dd[i] + (accumulate ? dL_drot_canon[6 * (size_t)idx + i] : 0.0f);
            } else {
#pragma unroll
                for (int i = 0; i < 9; i++) dL_drot_canon[9 * (size_t)idx + i] = dRc[i] + (accumulate ? dL_drot_canon[9 * (size_t)idx + i] : 0.0f);
            }
        }
        dL_dscales[3 * idx] = dsc[0]; dL_dscales[3 * idx + 1] = dsc[1]; dL_dscales[3 * idx + 2] = dsc[2];
        dL_dopacity[idx] = dop;
        dL_dmeans2D[3 * idx] = g2[0]; dL_dmeans2D[3 * idx + 1] = g2[1]; dL_dmeans2D[3 * idx + 2] = 0.0f;
    }
    // dL/dsh: planes, or the reference's rows: every one of the M rows is written (accumulate: the (D+1)^2 in use are added to)
    sg_skin_store_dsh<D, accumulate, !accumulate>(dsh, c.flags & SG_FLAG_SH_PLANAR, Mrows == 16, Mrows, P, idx, g0, lane, live, dL_dsh, sWw);
    // ---- dA[J x 16] += W^T[J x 64] . dT[64 x 16] on the matrix cores
    float *sdT = sTw;
#pragma unroll
    for (int i = 0; i < 12; i++) sdT[lane * SG_WSTRIDE + i] = dT[i];
#pragma unroll
    for (int i = 12; i < 16; i++) sdT[lane * SG_WSTRIDE + i] = 0.0f;
    const int nchunk = (k.J + 15) >> 4;
    // every wave owns one slab row (no cross-wave stage): [Jp x 16] dA partials + 3 dtransl partials
    float *out = slab + ((size_t)blockIdx.x * SG_SKIN_WAVES + wave) * slab_stride;
    const bool vec = (k.J & 3) == 0;
    float4 wv[4];
    if (vec) sg_w_fetch(k.lbs_w, k.J, P, g0, 0, lane, wv);
    for (int cch = 0; cch < nchunk; cch++) {
        if (vec) {
            sg_w_stash(wv, lane, sWw);
            if (cch + 1 < nchunk) sg_w_fetch(k.lbs_w, k.J, P, g0, cch + 1, lane, wv);
            __builtin_amdgcn_s_waitcnt(0xC07F);
        } else {
            sg_stage_w_chunk(k.lbs_w, k.J, P, g0, cch, lane, sWw);
            __builtin_amdgcn_s_waitcnt(0);
        }
        __builtin_amdgcn_wave_barrier();
        f32x4 acc = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            float av = sWw[(4 * kk + (lane >> 4)) * SG_WSTRIDE + (lane & 15)];     // W^T[joint lane&15][gaussian]
            float bv = sdT[(4 * kk + (lane >> 4)) * SG_WSTRIDE + (lane & 15)];          // dT[gaussian][entry lane&15]
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
        // acc[r] = dA[joint 16c + 4(lane>>4) + r][entry lane&15]
#pragma unroll
        for (int r = 0; r < 4; r++) out[(16 * cch + 4 * (lane >> 4) + r) * 16 + (lane & 15)] = acc[r];
        __builtin_amdgcn_wave_barrier();
    }
    sg_skin_store_dtransl(dtr, lane, out);
}
