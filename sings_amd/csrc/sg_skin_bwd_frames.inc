// The K-frame skinned per-Gaussian backward (LBS^T) of sg_skin.hip, included there twice: SG_SKFBWD_AUX 0 defines
// sg_skin_bwd_frames_kernel<D, ACC>, SG_SKFBWD_AUX 1 sg_skin_bwd_frames_aux_kernel<D> (gradients written), whose posed mean
// gradient of frame f also takes that frame's dL/dz (the spare float of its record-sum block: sg_record_sums_aux_kernel) along the
// frame's view row of z before LBS^T takes it to xyz_canon, A_f and transl_f -- sg_skin_bwd.inc's single-frame AUX term.  One
// source included twice, so that the plain kernel keeps its instructions.
// (no include guard: included once per variant)
#if SG_SKFBWD_AUX
// (accumulate = 0: the gradients are written, as by the single-frame AUX kernel)
template <int D>
__global__ void __launch_bounds__(SG_SKIN_THREADS) __attribute__((amdgpu_waves_per_eu(D <= 1 ? 2 : 1, 2)))
sg_skin_bwd_frames_aux_kernel(SgCam c0, SgBatch bt, int P, SgSkin k0, const float *__restrict__ shs, const float *__restrict__ scales,
#else
template <int D, bool ACC>
__global__ void __launch_bounds__(SG_SKIN_THREADS) __attribute__((amdgpu_waves_per_eu(D <= 1 ? 2 : 1, 2)))   // (D = 0: 255 VGPRs, no spills)
sg_skin_bwd_frames_kernel(SgCam c0, SgBatch bt, int P, SgSkin k0, const float *__restrict__ shs, const float *__restrict__ scales,
#endif
                          const int32_t *__restrict__ radii0, SgGeom g0_, SgRec grec0, size_t cap,
                          const uint32_t *__restrict__ header0, const float *__restrict__ dposed_xyz_in, const float *__restrict__ dposed_rotq_in,
                          float *__restrict__ dL_dxyz_canon, float *__restrict__ dL_drot_canon,
                          float *__restrict__ dL_dscales, float *__restrict__ dL_dopacity, float *__restrict__ dL_dsh,
                          float *__restrict__ dL_dmeans2D, float *__restrict__ slab, int slab_stride, size_t slab_frame,
                          const float4 *__restrict__ a9in)
{
#if SG_SKFBWD_AUX
    constexpr bool ACC = false, AUX = true;
#else
    constexpr bool AUX = false;
#endif
    constexpr bool accumulate = ACC;
    extern __shared__ float sg_skin_lds[];                      // [sA 64 x 16][per wave: W tile 64 x WP | scratch 64 x 17]
    const int J = k0.J, WP = J + 1;
    const int wave_size = 64 * WP + 64 * SG_WSTRIDE;
    float *const sA = sg_skin_lds;
    const int wave_all = threadIdx.x >> 6, lane_all = threadIdx.x & 63;
    const int g0_all = (blockIdx.x * SG_SKIN_WAVES + wave_all) * 64;
    const int idx_all = g0_all + lane_all;
    const bool live = idx_all < P;
    const int Mrows = c0.M;
    constexpr int nc = (D + 1) * (D + 1);
    const bool have_in = dposed_xyz_in != nullptr || dposed_rotq_in != nullptr;
    const int nchunk = (J + 15) >> 4;
    // ---- once per K frames: the wave's weight tile into LDS (coalesced: the tile's 64 rows are one contiguous range)
    {
        float *const sW = sg_skin_lds + SG_JMAX * 16 + wave_all * wave_size;
        const int rows = P - g0_all < 64 ? (P - g0_all > 0 ? P - g0_all : 0) : 64;
        const int total = rows * J;
        const float *src = k0.lbs_w + (size_t)g0_all * J;
        if (((J & 3) == 0)) {
            // every load of the tile is issued before the first LDS write: ONE memory round trip (64 x 64 floats = 16 float4 per lane)
            float4 v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int e = 4 * (64 * u + lane_all);
                v[u] = e < total ? *(const float4 *)(src + e) : make_float4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int e = 4 * (64 * u + lane_all);
                if (e < total) {
                    const int r = e / J, cc = e - r * J;              // (J % 4 == 0: the four values share a row)
                    float *d = sW + r * WP + cc;
                    d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
                }
            }
        } else {
            for (int e = lane_all; e < total; e += 64) { const int r = e / J; sW[r * WP + (e - r * J)] = src[e]; }
        }
        for (int e = total + lane_all; e < 64 * J; e += 64) { const int r = e / J; sW[r * WP + (e - r * J)] = 0.0f; }   // rows beyond P
    }
    // ---- once per K frames: the canonical inputs of this lane's Gaussian
    float cx[3] = { 0, 0, 0 }, cs[3] = { 0, 0, 0 }, cRc[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, d6[6] = { 0, 0, 0, 0, 0, 0 };
    if (live) {
        cx[0] = k0.xyz_canon[3 * idx_all]; cx[1] = k0.xyz_canon[3 * idx_all + 1]; cx[2] = k0.xyz_canon[3 * idx_all + 2];
        cs[0] = scales[3 * idx_all]; cs[1] = scales[3 * idx_all + 1]; cs[2] = scales[3 * idx_all + 2];
        if (k0.rot_canon) {
            if (k0.rot6d) {
#pragma unroll
                for (int i = 0; i < 6; i++) d6[i] = k0.rot_canon[6 * (size_t)idx_all + i];
                sg_r6d2m(d6, cRc);
            } else {
#pragma unroll
                for (int i = 0; i < 9; i++) cRc[i] = k0.rot_canon[9 * (size_t)idx_all + i];
            }
        }
    }
    const float csc = k0.smpl_scale ? k0.smpl_scale[0] : 1.0f;
    // ---- sums over the frames; ACC: they start from what the gradient buffer holds
    float dxc[3] = { 0, 0, 0 }, dRc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, dsc[3] = { 0, 0, 0 }, dop = 0;
    float dsh[nc * 3];
#pragma unroll
    for (int i = 0; i < nc * 3; i++) dsh[i] = 0.0f;
    if (accumulate && live) {
#pragma unroll
        for (int i = 0; i < 3; i++) { dxc[i] = dL_dxyz_canon[3 * idx_all + i]; dsc[i] = dL_dscales[3 * idx_all + i]; }
        dop = dL_dopacity[idx_all];
        if (dL_drot_canon) {
            const int rw = k0.rot6d ? 6 : 9;
            for (int i = 0; i < rw; i++) dRc[i] = dL_drot_canon[(size_t)rw * idx_all + i];
        }
        const bool planar = c0.flags & SG_FLAG_SH_PLANAR;
#pragma unroll
        for (int i = 0; i < nc * 3; i++)
            dsh[i] = planar ? dL_dsh[((size_t)(i / 3) * P + idx_all) * 3 + i % 3] : dL_dsh[(size_t)idx_all * Mrows * 3 + i];
    }
    // frame 0's joint transforms; (visible, slot, flags) of frame 0
    for (int i = threadIdx.x; i < SG_JMAX * 16; i += SG_SKIN_THREADS) sA[i] = i < J * 16 ? k0.A[i] : 0.0f;
    bool vis_n = live && radii0[idx_all] > 0 && header0[1] == 0u;
    uint32_t fl_n = 0u;
    if (vis_n) fl_n = g0_.flags[idx_all];
    __syncthreads();
#pragma unroll 1
    for (int f = 0; f < bt.K; f++) {
        // lane / wave / Gaussian index are made opaque per trip: hipcc otherwise hoists everything of the loop body that depends on
        // them only (LDS addresses, shuffle lane indices, per-frame array addresses) in front of the loop and keeps it live across
        // it -- 330 VGPRs instead of ~250, one wave per SIMD instead of two
        int idx = idx_all, lane = lane_all, wave = wave_all;
        asm volatile("" : "+v"(idx), "+v"(lane), "+v"(wave));
        float *const sW = sg_skin_lds + SG_JMAX * 16 + wave * wave_size, *const sTw = sW + 64 * WP;
        const SgCam c = sg_frame(c0, f, bt.cam_stride);
        const float *transl = k0.transl ? k0.transl + (size_t)f * bt.transl_stride : nullptr;
        // next frame's joint transforms: requested now, written to LDS when every wave is done with this frame's
        float4 an = make_float4(0, 0, 0, 0);
        const bool more = f + 1 < bt.K;
        if (more) {
            const int i4 = 4 * (int)threadIdx.x;                  // SG_JMAX * 16 = 1024 floats = one float4 per thread
            if (i4 < J * 16) an = *(const float4 *)(k0.A + (size_t)(f + 1) * J * 16 + i4);
        }
        float T[12];
        sg_skin_T_resident(sW, WP, J, lane, sA, sTw, T);
        const bool vis = vis_n;
        const uint32_t flags = fl_n;
        if (more) {
            const SgGeom gn = sg_frame(g0_, (size_t)(f + 1) * bt.geom);
            vis_n = live && radii0[(size_t)(f + 1) * bt.P + idx] > 0 && sg_at(header0, (size_t)(f + 1) * bt.bin)[1] == 0u;
            fl_n = 0u;
            if (vis_n) fl_n = gn.flags[idx];
        }
        // this frame's record sums (sg_record_sums_kernel): 48 contiguous bytes per Gaussian; AUX: + its dL/dz in the spare float
        float a9[9];
        float dz = 0.0f;
        {
            const float4 *src = a9in + 3 * ((size_t)f * bt.P + idx);
            float4 r0 = make_float4(0, 0, 0, 0), r1 = r0, r2 = r0;
            if (vis) { r0 = src[0]; r1 = src[1]; r2 = src[2]; }
            a9[0] = r0.x; a9[1] = r0.y; a9[2] = r0.z; a9[3] = r0.w; a9[4] = r1.x; a9[5] = r1.y; a9[6] = r1.z; a9[7] = r1.w; a9[8] = r2.x;
            if (AUX) dz = r2.y;
        }
        float dT[12];
#pragma unroll
        for (int i = 0; i < 12; i++) dT[i] = 0.0f;
        float dtr[3] = { 0, 0, 0 };
        if (live) {
            float fxc[3] = { 0, 0, 0 }, fRc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, fsc[3] = { 0, 0, 0 }, fop = 0, g2[2] = { 0, 0 };
            if (vis || have_in) {
                // sings_hybrid.py:400-419 for this Gaussian (sg_pose_gaussian without the loads and without ext_tfs)
                float pp[3], s3[3], Rdef[9], q[4];
#pragma unroll
                for (int i = 0; i < 3; i++) pp[i] = T[4 * i] * cx[0] + T[4 * i + 1] * cx[1] + T[4 * i + 2] * cx[2] + T[4 * i + 3];
                s3[0] = cs[0]; s3[1] = cs[1]; s3[2] = cs[2];
                if (k0.smpl_scale) {
#pragma unroll
                    for (int i = 0; i < 3; i++) { pp[i] = pp[i] * csc; s3[i] = s3[i] * csc; }
                }
                if (transl) {
#pragma unroll
                    for (int i = 0; i < 3; i++) pp[i] = pp[i] + transl[i];
                }
                if (k0.rot_canon) {
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++)
                            Rdef[3 * i + j] = T[4 * i] * cRc[j] + T[4 * i + 1] * cRc[3 + j] + T[4 * i + 2] * cRc[6 + j];
                } else {
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++) Rdef[3 * i + j] = T[4 * i + j];
                }
                int best; float qab;
                sg_m2q(Rdef, q, best, qab);
                SgGaussGrad G;
#pragma unroll
                for (int i = 0; i < 3; i++) { G.dmean[i] = 0; G.dsc[i] = 0; G.dcol[i] = 0; }
#pragma unroll
                for (int i = 0; i < 4; i++) G.drot[i] = 0;
                G.g2[0] = G.g2[1] = 0; G.dop = 0;
                if (vis)
                    sg_project_bwd<D>(c, pp, s3, q, nullptr, shs + (size_t)idx * Mrows * 3, flags, a9, true, dsh, G, !accumulate && f == 0);
                if (AUX && vis) {                                // depth map: dL/dz along this frame's view row of z (sg_skin_bwd.inc)
#pragma unroll
                    for (int i = 0; i < 3; i++) G.dmean[i] = fmaf(dz, c.view[4 * i + 2], G.dmean[i]);
                }
                if (dposed_xyz_in) {
#pragma unroll
                    for (int i = 0; i < 3; i++) G.dmean[i] += dposed_xyz_in[3 * ((size_t)f * bt.P + idx) + i];
                }
                if (dposed_rotq_in) {
#pragma unroll
                    for (int i = 0; i < 4; i++) G.drot[i] += dposed_rotq_in[4 * ((size_t)f * bt.P + idx) + i];
                }
                g2[0] = G.g2[0]; g2[1] = G.g2[1]; fop = G.dop;
#pragma unroll
                for (int i = 0; i < 3; i++) { fsc[i] = G.dsc[i] * csc; dtr[i] = G.dmean[i]; }
                float dps[3] = { G.dmean[0] * csc, G.dmean[1] * csc, G.dmean[2] * csc };
                float dRd[9];
                sg_m2q_bwd(q, best, qab, G.drot, dRd);
#pragma unroll
                for (int i = 0; i < 3; i++) {
#pragma unroll
                    for (int kx = 0; kx < 3; kx++)
                        dT[4 * i + kx] = dps[i] * cx[kx] + dRd[3 * i] * cRc[3 * kx] + dRd[3 * i + 1] * cRc[3 * kx + 1] + dRd[3 * i + 2] * cRc[3 * kx + 2];
                    dT[4 * i + 3] = dps[i];
                }
#pragma unroll
                for (int kx = 0; kx < 3; kx++) {
                    fxc[kx] = T[kx] * dps[0] + T[4 + kx] * dps[1] + T[8 + kx] * dps[2];
#pragma unroll
                    for (int j = 0; j < 3; j++) fRc[3 * kx + j] = T[kx] * dRd[j] + T[4 + kx] * dRd[3 + j] + T[8 + kx] * dRd[6 + j];
                }
            }
            // the decoder's 6-D rotations: every frame's dL/dR_canon goes through the Gram-Schmidt backward on its own, as in a
            // single-frame call (the map is linear in dR, but J (a + b) and J a + J b differ in the last bit)
            if (dL_drot_canon && k0.rot6d) {
                float dd[6];
                sg_r6d2m_bwd(d6, fRc, dd);
#pragma unroll
                for (int i = 0; i < 6; i++) fRc[i] = dd[i];
            }
            if (!accumulate && f == 0) {
#pragma unroll
                for (int i = 0; i < 3; i++) { dxc[i] = fxc[i]; dsc[i] = fsc[i]; }
#pragma unroll
                for (int i = 0; i < 9; i++) dRc[i] = fRc[i];
                dop = fop;
            } else {
                // (operand order of the single-frame accumulate: new + old)
#pragma unroll
                for (int i = 0; i < 3; i++) { dxc[i] = fxc[i] + dxc[i]; dsc[i] = fsc[i] + dsc[i]; }
#pragma unroll
                for (int i = 0; i < 9; i++) dRc[i] = fRc[i] + dRc[i];
                dop = fop + dop;
            }
            float *m2 = dL_dmeans2D + 3 * ((size_t)f * bt.P + idx);
            m2[0] = g2[0]; m2[1] = g2[1]; m2[2] = 0.0f;
        }
        // ---- dA[J x 16] = W^T[J x 64] . dT[64 x 16] on the matrix cores, W from the resident tile
        float *sdT = sTw;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 12; i++) sdT[lane * SG_WSTRIDE + i] = dT[i];
#pragma unroll
        for (int i = 12; i < 16; i++) sdT[lane * SG_WSTRIDE + i] = 0.0f;
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        float *out = slab + (size_t)f * slab_frame + ((size_t)blockIdx.x * SG_SKIN_WAVES + wave) * slab_stride;
        for (int cch = 0; cch < nchunk; cch++) {
            f32x4 acc = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
            // (joints >= J of the last chunk: the column index is clamped -- those rows of dA are written with whatever comes out
            //  and never read: sg_skin_reduce2_kernel sums J x 16 columns)
            const int col = 16 * cch + (lane & 15) < J ? 16 * cch + (lane & 15) : J - 1;
#pragma unroll
            for (int k4 = 0; k4 < 4; k4++) {
                float av[4], bv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int kk = 4 * k4 + u;
                    av[u] = sW[(4 * kk + (lane >> 4)) * WP + col];                          // W^T[joint][gaussian 4 kk + (lane >> 4)]
                    bv[u] = sdT[(4 * kk + (lane >> 4)) * SG_WSTRIDE + (lane & 15)];          // dT[gaussian][entry lane & 15]
                }
#pragma unroll
                for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) out[(16 * cch + 4 * (lane >> 4) + r) * 16 + (lane & 15)] = acc[r];
        }
        sg_skin_store_dtransl(dtr, lane, out);
        if (more) {
            __syncthreads();                                     // every wave is done with this frame's joint transforms
            *(float4 *)(sA + 4 * (int)threadIdx.x) = an;
            __syncthreads();
        }
    }
    // ---- the canonical-Gaussian gradients, once for the K frames (ACC: the sums already include what the buffer held)
    const int idx = idx_all, lane = lane_all, g0 = g0_all;
    float *const sWw = sg_skin_lds + SG_JMAX * 16 + wave_all * wave_size;      // (the weight tile is dead: staging for the SH rows)
    if (live) {
        dL_dxyz_canon[3 * idx] = dxc[0]; dL_dxyz_canon[3 * idx + 1] = dxc[1]; dL_dxyz_canon[3 * idx + 2] = dxc[2];
        if (dL_drot_canon) {
            const int rw = k0.rot6d ? 6 : 9;
            for (int i = 0; i < rw; i++) dL_drot_canon[(size_t)rw * idx + i] = dRc[i];
        }
        dL_dscales[3 * idx] = dsc[0]; dL_dscales[3 * idx + 1] = dsc[1]; dL_dscales[3 * idx + 2] = dsc[2];
        dL_dopacity[idx] = dop;
    }
    // dL/dsh rows: every one of the M rows is written (through LDS as 16-B-per-lane coalesced stores when M == 16); ACC: only the
    // (D+1)^2 rows in use are rewritten -- the others keep what the step's first call wrote
    // (the sums are stored, never added; the LDS path writes all 16 rows: not under ACC with rows out of use, and only where the
    // weight tile holds 32 staged rows)
    __builtin_amdgcn_wave_barrier();
    sg_skin_store_dsh<D, false, !accumulate>(dsh, c0.flags & SG_FLAG_SH_PLANAR,
                                             Mrows == 16 && (!accumulate || nc == 16) && 64 * WP >= 32 * SG_ROW_LDS, Mrows, P, idx, g0, lane,
                                             live, dL_dsh, sWw);
}
