// The single-camera per-Gaussian backward of sg_preprocess.hip, included there twice: SG_PBWD_AUX 0 defines
// sg_preprocess_bwd_kernel<D, ACC>, SG_PBWD_AUX 1 sg_preprocess_bwd_aux_kernel<D> (gradients written), whose mean gradient also
// takes the depth map's dL/dz: the plane `dzp` (one float per record slot) summed like the records, through z = view row 2 . mean.
// (no include guard: included once per variant)
#if SG_PBWD_AUX
template <int D>
__global__ void __launch_bounds__(256)
sg_preprocess_bwd_aux_kernel(SG_PBWD_PARAMS, const float *__restrict__ dzp)
#else
template <int D, bool ACC>
__global__ void __launch_bounds__(256)
sg_preprocess_bwd_kernel(SG_PBWD_PARAMS)
#endif
{
    constexpr bool AUX = SG_PBWD_AUX;
#if SG_PBWD_AUX
    constexpr bool ACC = false;
#else
    const float *const dzp = nullptr;
#endif
    constexpr bool accumulate = ACC;
    __shared__ float lds_all[4][32 * SG_ROW_LDS];         // 6.5 KiB per wave: record chunks, then dL/dsh rows out
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = idx - lane;
    if (g0 >= P) return;                                    // whole wave out of range
    float *L = lds_all[wave];
    const bool live = idx < P;
    SgGaussGrad G;
#pragma unroll
    for (int k = 0; k < 3; k++) { G.dmean[k] = 0; G.dcol[k] = 0; G.dsc[k] = 0; }
#pragma unroll
    for (int k = 0; k < 4; k++) G.drot[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) G.g6[k] = 0;
    G.g2[0] = G.g2[1] = 0; G.dop = 0;
    // after a forward that overflowed (header[1] != 0) the backward composite wrote no records: every gradient is ZERO, the
    // stale contents of the record buffer are never summed (asynchronous overflow check: rasterizer.py)
    const bool vis = live && radii[idx] > 0 && header[1] == 0u;
    const int Mrows = c.M;
    constexpr int nc = (D + 1) * (D + 1);
    const bool staged = D == 3 && Mrows == 16 && shs != nullptr && dL_dsh != nullptr;
    // 0. issue every load that does not depend on another one up front (one memory round trip, not four)
    float4 rc = make_float4(0, 0, 0, 0);
    float p[3] = { 0, 0, 0 }, s3[3] = { 0, 0, 0 }, q[4] = { 0, 0, 0, 0 }, sh[nc * 3], dsh[nc * 3];
    uint32_t flags = 0;
#pragma unroll
    for (int k = 0; k < nc * 3; k++) { sh[k] = 0.0f; dsh[k] = 0.0f; }
    if (vis) {
        { const uint2 sl = g.slot[idx]; rc.y = __uint_as_float(sl.x); rc.w = __uint_as_float(sl.y); }
        flags = g.flags[idx];
        p[0] = means3D[3 * idx]; p[1] = means3D[3 * idx + 1]; p[2] = means3D[3 * idx + 2];
        if (!cov3D_precomp) {
            s3[0] = scales[3 * idx]; s3[1] = scales[3 * idx + 1]; s3[2] = scales[3 * idx + 2];
            q[0] = rotations[4 * idx]; q[1] = rotations[4 * idx + 1]; q[2] = rotations[4 * idx + 2]; q[3] = rotations[4 * idx + 3];
        }
        if (shs) {
            const float *src = shs + (size_t)idx * Mrows * 3;
            if (staged) {
#pragma unroll
                for (int k = 0; k < nc * 3 / 4; k++) {
                    float4 v = ((const float4 *)src)[k];
                    sh[4 * k] = v.x; sh[4 * k + 1] = v.y; sh[4 * k + 2] = v.z; sh[4 * k + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < nc * 3; k++) sh[k] = src[k];
            }
        }
    }
    // 1. this Gaussian's gradient records (wave-cooperative, coalesced)
    float a9[9];
    sg_sum_records_coop(grec, cap, vis, rc, lane, L, a9, rec_valid);
    const float dz = AUX ? sg_sum_dz(dzp, cap, vis, rc, rec_valid) : 0.0f;
    // 2. the chain rule
    if (vis)
        sg_project_bwd<D>(c, p, s3, q, cov3D_precomp ? cov3D_precomp + 6 * (size_t)idx : nullptr, sh, flags, a9,
                          dL_dsh != nullptr, dsh, G);
    if (AUX && vis) {
#pragma unroll
        for (int k = 0; k < 3; k++) G.dmean[k] = fmaf(dz, c.view[4 * k + 2], G.dmean[k]);
    }
    // 3. dL/dsh out: coefficient-major planes [M][P][3], only the (D+1)^2 in use (SG_FLAG_SH_PLANAR); or the reference's rows
    //    (every one of the M rows is written; coalesced through LDS when staged)
    if (dL_dsh && (c.flags & SG_FLAG_SH_PLANAR)) {
        if (live) {
#pragma unroll
            for (int kq = 0; kq < nc; kq++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    float *d = dL_dsh + ((size_t)kq * P + idx) * 3 + ch;
                    *d = accumulate ? dsh[3 * kq + ch] + *d : dsh[3 * kq + ch];
                }
        }
    } else if (dL_dsh) {
        if (staged) {
#pragma unroll
            for (int h = 0; h < 2; h++) {                    // 32 rows at a time (keeps LDS at 6.5 KiB per wave)
                if ((lane >> 5) == h) {
#pragma unroll
                    for (int k = 0; k < 12; k++)
                        *(float4 *)(L + (lane & 31) * SG_ROW_LDS + 4 * k) = make_float4(dsh[4 * k], dsh[4 * k + 1], dsh[4 * k + 2], dsh[4 * k + 3]);
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
                sg_rows48_store(dL_dsh, g0 + 32 * h, P, lane, L, 32, accumulate != 0);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
            }
        } else if (live) {
            float *dsh_row = dL_dsh + (size_t)idx * Mrows * 3;
            if (accumulate) {
#pragma unroll
                for (int k = 0; k < nc * 3; k++) dsh_row[k] += dsh[k];
            } else {
#pragma unroll
                for (int k = 0; k < nc * 3; k++) dsh_row[k] = dsh[k];
                for (int k = nc * 3; k < Mrows * 3; k++) dsh_row[k] = 0.0f;
            }
        }
    }
    if (!live) return;
    // the screen-space gradient is per VIEW (the densifier's statistic): never accumulated
    dL_dmeans2D[3 * idx] = G.g2[0]; dL_dmeans2D[3 * idx + 1] = G.g2[1]; dL_dmeans2D[3 * idx + 2] = 0.0f;
    if (accumulate) {
        // the views of one optimisation step share ONE gradient buffer: this view adds to what the views in front of it in the
        // step's chain left there (the old values are requested together, here: one more memory round trip per wave)
        float o3[3], os[3], orr[4], oc[3], og[6], oo;
#pragma unroll
        for (int k = 0; k < 3; k++) o3[k] = dL_dmeans3D[3 * idx + k];
        oo = dL_dopacity[idx];
#pragma unroll
        for (int k = 0; k < 3; k++) { oc[k] = dL_dcolors ? dL_dcolors[3 * idx + k] : 0.0f; os[k] = dL_dscales ? dL_dscales[3 * idx + k] : 0.0f; }
#pragma unroll
        for (int k = 0; k < 4; k++) orr[k] = dL_drots ? dL_drots[4 * idx + k] : 0.0f;
#pragma unroll
        for (int k = 0; k < 6; k++) og[k] = dL_dcov3D ? dL_dcov3D[6 * idx + k] : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) { G.dmean[k] += o3[k]; G.dcol[k] += oc[k]; G.dsc[k] += os[k]; }
#pragma unroll
        for (int k = 0; k < 4; k++) G.drot[k] += orr[k];
#pragma unroll
        for (int k = 0; k < 6; k++) G.g6[k] += og[k];
        G.dop += oo;
    }
    dL_dmeans3D[3 * idx] = G.dmean[0]; dL_dmeans3D[3 * idx + 1] = G.dmean[1]; dL_dmeans3D[3 * idx + 2] = G.dmean[2];
    dL_dopacity[idx] = G.dop;
    if (dL_dcolors) { dL_dcolors[3 * idx] = G.dcol[0]; dL_dcolors[3 * idx + 1] = G.dcol[1]; dL_dcolors[3 * idx + 2] = G.dcol[2]; }
    if (dL_dscales) { dL_dscales[3 * idx] = G.dsc[0]; dL_dscales[3 * idx + 1] = G.dsc[1]; dL_dscales[3 * idx + 2] = G.dsc[2]; }
    if (dL_drots) { dL_drots[4 * idx] = G.drot[0]; dL_drots[4 * idx + 1] = G.drot[1]; dL_drots[4 * idx + 2] = G.drot[2]; dL_drots[4 * idx + 3] = G.drot[3]; }
    if (dL_dcov3D) {
#pragma unroll
        for (int k = 0; k < 6; k++) dL_dcov3D[6 * idx + k] = G.g6[k];
    }
}
