// Plain (un-skinned) per-Gaussian kernels: the GaussianRasterizer surface.
//
// Replaces preprocessCUDA<3> (+ computeCov2DCUDA in backward) of the rasterizer the reference
// calls at sings/rec/renderer/gs_renderer_single.py:87-95; algorithm per SURVEY.md App. A.1/A.5.
// One lane per Gaussian; 256-thread workgroups; grid = ceil(P/256) >> 256 CUs at P >= 1e5.
// HBM-bound streaming kernels: forward reads `in` bytes per Gaussian and writes a 56-B projected
// record; backward re-reads the inputs, sums the Gaussian's gradient records and writes 248 B.
#include "sg_project.h"
#include "sg_host.h"

// NOBIN (include/sings_order.h): everything but the pair expansion, which sg_bin_ordered_kernel does in work order behind this kernel.
// (A compile-time switch: the instantiation that bins keeps its code.)
template <int D, bool NOBIN>
__global__ void __launch_bounds__(256)
sg_preprocess_fwd_kernel(SgCam c, SgBatch bt, int P, const float *__restrict__ means3D,
                         const float *__restrict__ shs, const float *__restrict__ colors_precomp,
                         const float *__restrict__ opacities, const float *__restrict__ scales,
                         const float *__restrict__ rotations, const float *__restrict__ cov3D_precomp,
                         SgGeom g, SgBin bn, uint32_t cap, int32_t *__restrict__ radii, int hist_tiles, int nblocks)
{
    extern __shared__ uint32_t sg_hist_lds[];               // hist_tiles words (0: per-pair global atomics)
    __shared__ uint32_t scratch_all[4][NOBIN ? 1 : 256];
    // (Gaussian block, camera) of this workgroup: the K cameras of one block run back to back on ONE XCD (sg_block_frame)
    int gblock, frame;
    if (!sg_block_frame((int)blockIdx.x, bt.K, nblocks, gblock, frame)) return;
    c = sg_frame(c, frame, bt.cam_stride); g = sg_frame(g, (size_t)frame * bt.geom); bn = sg_frame(bn, (size_t)frame * bt.bin);
    radii += (size_t)frame * bt.P;
    const int idx = gblock * 256 + (int)threadIdx.x;
    const int wave = threadIdx.x >> 6;
    const bool live = idx < P;
    constexpr int nc = (D + 1) * (D + 1);
    float sh[nc * 3];
    if (shs && live) {
        const float *src = shs + (size_t)idx * c.M * 3;
        if (D == 3 && c.M == 16) {
            // the reference's layout [P,16,3]: a row is 192 B, 16-B aligned -> twelve 16-B loads per lane.  (Staging the
            // wave's 64 rows through LDS as coalesced 1-KiB pieces was measured too: 39.4 vs 39.0 us -- the one-row-per-lane
            // form does not bound this kernel; the pair expansion's scattered returning atomics do: 16 of its 39 us.)
#pragma unroll
            for (int k = 0; k < nc * 3 / 4; k++) {
                const float4 v = ((const float4 *)src)[k];
                sh[4 * k] = v.x; sh[4 * k + 1] = v.y; sh[4 * k + 2] = v.z; sh[4 * k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < nc * 3; k++) sh[k] = src[k];
        }
    }
    SgProj o;
    o.mr = 0; o.tt = 0; o.clampbits = 0; o.x0 = o.y0 = o.x1 = o.y1 = 0;
    o.pix[0] = o.pix[1] = 0; o.conic[0] = o.conic[1] = o.conic[2] = 0; o.rgb[0] = o.rgb[1] = o.rgb[2] = 0; o.depth = 0;
    float opac = 0.0f;
    if (live) {
        float p[3] = { means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2] };
        float s3[3] = { 0, 0, 0 }, q[4] = { 0, 0, 0, 0 };
        if (!cov3D_precomp) {
            s3[0] = scales[3 * idx]; s3[1] = scales[3 * idx + 1]; s3[2] = scales[3 * idx + 2];
            q[0] = rotations[4 * idx]; q[1] = rotations[4 * idx + 1]; q[2] = rotations[4 * idx + 2]; q[3] = rotations[4 * idx + 3];
        }
        sg_project_fwd<D>(c, p, s3, q, cov3D_precomp ? cov3D_precomp + 6 * (size_t)idx : nullptr,
                          colors_precomp ? colors_precomp + 3 * (size_t)idx : nullptr, sh, o);
        opac = opacities[idx];
    }
    if constexpr (NOBIN)
        sg_store_proj_nobin(live, idx, o, opac, g, bn, radii);
    else
    sg_store_proj(live, idx, o, opac, g, bn, c.gx, cap, radii, scratch_all[wave], hist_tiles ? sg_hist_lds : nullptr, hist_tiles,
                  sg_key_pitch_of(hist_tiles != 0, c.flags));
}

// ---- K cameras per launch in work order: the forward twin of sg_gauss_frames_bwd_kernel -------------------------------------------
// What sg_preprocess_fwd_kernel<D, true> does for K frames, with the workgroup turned by 90 degrees: 64 consecutive Gaussians x K
// frames, K waves, wave f is frame f (camera, geometry and allocator pointers stay wave-uniform), lane = Gaussian; grid ceil(P / 64).
//  1. The 64 Gaussians' inputs are requested ONCE per workgroup: all K waves fill SG_GFF_PITCH-float rows of LDS with coalesced
//     loads (16 bytes per lane where the coefficient rows are one contiguous block), one barrier, and every lane takes its row.
//     (One workgroup per (256 Gaussians, frame) asked for every 192-byte coefficient row K times, at a 192-byte lane stride: from
//     HBM once and from the XCD's L2 K - 1 times.)  An odd pitch: lane-strided reads hit distinct banks.
//         0-47 SH coefficients ((D+1)^2 x 3 in use) | 48-50 position | 51-53 scale | 54-57 rotation | 58 opacity
//     cov3D_precomp / colors_precomp rows are read by sg_project_fwd where it uses them, as in the single-camera kernel.
//  2. sg_project_fwd<D> -- the coefficients are read from the row where sg_eval_sh uses them, by the Gaussians that get that far:
//     not 48 registers held across the projection --, then sg_store_proj_wave: a wave holds one frame's 64 Gaussians, so its
//     record slots need no other wave.
// No wave leaves between kernel entry and the barrier.
#define SG_GFF_PITCH 59
#define SG_GFF_POS 48
#define SG_GFF_SCALE 51
#define SG_GFF_ROT 54
#define SG_GFF_OPAC 58
template <int D>
__global__ void __launch_bounds__(1024)
sg_gauss_frames_fwd_kernel(SgCam c, SgBatch bt, int P, const float *__restrict__ means3D, const float *__restrict__ shs,
                           const float *__restrict__ colors_precomp, const float *__restrict__ opacities,
                           const float *__restrict__ scales, const float *__restrict__ rotations,
                           const float *__restrict__ cov3D_precomp, SgGeom g, SgBin bn, int32_t *__restrict__ radii)
{
    extern __shared__ float sg_gff_lds[];                   // 64 rows of SG_GFF_PITCH floats
    const int lane = threadIdx.x & 63;
    const int frame = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (scalar: the frame's pointers stay in SGPRs)
    const int g0 = (int)blockIdx.x * 64;
    const int tid = (int)threadIdx.x, nthr = bt.K * 64;     // (K >= 2: at least 128 threads share the fill)
    const int nlive = P - g0 < 64 ? P - g0 : 64;
    constexpr int nc = (D + 1) * (D + 1);
    const bool want_sh = shs != nullptr && colors_precomp == nullptr;
    {
        // ---- 1. the fill: every request goes out before the first value is written
        // coefficient rows: with M = (D+1)^2 the 64 rows are ONE block of nlive * nc * 3 floats (16-byte aligned: g0 is a multiple
        // of 64), taken as 16-byte vectors; what is left (no whole vector, or rows of M > (D+1)^2 coefficients) goes by the float
        const int nsh = want_sh ? nlive * nc * 3 : 0;
        const int nv4 = c.M == nc && ((uintptr_t)shs & 15u) == 0 ? nsh >> 2 : 0;
        const float4 *src4 = (const float4 *)(shs + (size_t)g0 * nc * 3);
        float4 v4[6];                                       // 64 * 48 / 4 = 768 vectors over >= 128 threads
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const int f = tid + i * nthr;
            if (f < nv4) v4[i] = src4[f];
        }
        float vp[2], vs[2], vq[2], vo = 0.0f;               // 192, 192, 256 and 64 floats over >= 128 threads
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int t = tid + i * nthr;
            if (t < nlive * 3) vp[i] = means3D[3 * (size_t)g0 + t];
            if (!cov3D_precomp) {
                if (t < nlive * 3) vs[i] = scales[3 * (size_t)g0 + t];
                if (t < nlive * 4) vq[i] = rotations[4 * (size_t)g0 + t];
            }
        }
        if (tid < nlive) vo = opacities[g0 + tid];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const int f = tid + i * nthr;
            if (f < nv4) {
                const float e[4] = { v4[i].x, v4[i].y, v4[i].z, v4[i].w };
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int t = 4 * f + u, j = t / (nc * 3);
                    sg_gff_lds[j * SG_GFF_PITCH + (t - j * nc * 3)] = e[u];
                }
            }
        }
        for (int t = 4 * nv4 + tid; t < nsh; t += nthr) {
            const int j = t / (nc * 3), k = t - j * nc * 3;
            sg_gff_lds[j * SG_GFF_PITCH + k] = shs[(size_t)(g0 + j) * c.M * 3 + k];
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int t = tid + i * nthr;
            if (t < nlive * 3) sg_gff_lds[(t / 3) * SG_GFF_PITCH + SG_GFF_POS + t % 3] = vp[i];
            if (!cov3D_precomp) {
                if (t < nlive * 3) sg_gff_lds[(t / 3) * SG_GFF_PITCH + SG_GFF_SCALE + t % 3] = vs[i];
                if (t < nlive * 4) sg_gff_lds[(t >> 2) * SG_GFF_PITCH + SG_GFF_ROT + (t & 3)] = vq[i];
            }
        }
        if (tid < nlive) sg_gff_lds[tid * SG_GFF_PITCH + SG_GFF_OPAC] = vo;
    }
    __syncthreads();                                        // every wave of the workgroup arrives (no return above)
    // ---- 2. frame `frame` of Gaussian g0 + lane
    const SgCam cf = sg_frame(c, frame, bt.cam_stride);
    const SgGeom gf = sg_frame(g, (size_t)frame * bt.geom);
    const SgBin bf = sg_frame(bn, (size_t)frame * bt.bin);
    const int idx = g0 + lane;
    const bool live = idx < P;
    const float *row = sg_gff_lds + lane * SG_GFF_PITCH;
    SgProj o;
    o.mr = 0; o.tt = 0; o.clampbits = 0; o.x0 = o.y0 = o.x1 = o.y1 = 0;
    o.pix[0] = o.pix[1] = 0; o.conic[0] = o.conic[1] = o.conic[2] = 0; o.rgb[0] = o.rgb[1] = o.rgb[2] = 0; o.depth = 0;
    float opac = 0.0f;
    if (live) {
        float p[3] = { row[SG_GFF_POS], row[SG_GFF_POS + 1], row[SG_GFF_POS + 2] };
        float s3[3] = { 0, 0, 0 }, q[4] = { 0, 0, 0, 0 };
        if (!cov3D_precomp) {
            s3[0] = row[SG_GFF_SCALE]; s3[1] = row[SG_GFF_SCALE + 1]; s3[2] = row[SG_GFF_SCALE + 2];
            q[0] = row[SG_GFF_ROT]; q[1] = row[SG_GFF_ROT + 1]; q[2] = row[SG_GFF_ROT + 2]; q[3] = row[SG_GFF_ROT + 3];
        }
        sg_project_fwd<D>(cf, p, s3, q, cov3D_precomp ? cov3D_precomp + 6 * (size_t)idx : nullptr,
                          colors_precomp ? colors_precomp + 3 * (size_t)idx : nullptr, row, o);
        opac = row[SG_GFF_OPAC];
    }
    sg_store_proj_wave(live, idx, o, opac, gf, bf, radii + (size_t)frame * bt.P);
}

// The pair expansion of a NOBIN launch, in work order: lane i reads the rectangle (recC) and the depth bits behind it (sg_rec_pad)
// of Gaussian order[i] -- 32 contiguous bytes of one line of what the kernels above stored -- and bins it (sg_bin_ordered).
// Grid: Gaussian blocks x frames.  An entry >= P is never dereferenced: its lane is idle.
__global__ void __launch_bounds__(256)
sg_bin_ordered_kernel(SgBatch bt, int P, SgGeom g, SgBin bn, int gx, uint32_t key_pitch, const uint32_t *__restrict__ order)
{
    __shared__ uint32_t scratch_all[4][320];
    const int frame = blockIdx.y;
    g = sg_frame(g, (size_t)frame * bt.geom); bn = sg_frame(bn, (size_t)frame * bt.bin);
    const int pos = blockIdx.x * 256 + (int)threadIdx.x, wave = threadIdx.x >> 6;
    uint32_t gid = pos < P ? order[pos] : 0xffffffffu;
    uint32_t rmin = 0u, rwh = 0u, dep = 0u;
    if (gid < (uint32_t)P) {
        const float4 rc = g.recC[SG_REC_STRIDE * (size_t)gid], pad = *sg_rec_pad(g, (size_t)gid);
        rmin = __float_as_uint(rc.z); rwh = __float_as_uint(rc.w);
        dep = __float_as_uint(pad.x);
    } else gid = 0u;
    sg_bin_ordered(gid, rmin, rwh, dep, bn, gx, scratch_all[wave], scratch_all[wave] + 256, key_pitch);
}

void sg_launch_preprocess_fwd(const SgCam &c, const SgBatch &bt, int P, const float *means3D, const float *shs,
                              const float *colors_precomp, const float *opacities, const float *scales,
                              const float *rotations, const float *cov3D_precomp, SgGeom g, SgBin b,
                              size_t cap, int32_t *radii, hipStream_t st)
{
    sg_launch_preprocess_fwd_ordered(c, bt, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, g, b, cap,
                                     radii, nullptr, st);
}

// order != null (P entries) takes effect where sg_order_applies says so; elsewhere the launch is the unordered one
void sg_launch_preprocess_fwd_ordered(const SgCam &c, const SgBatch &bt, int P, const float *means3D, const float *shs,
                                      const float *colors_precomp, const float *opacities, const float *scales,
                                      const float *rotations, const float *cov3D_precomp, SgGeom g, SgBin b,
                                      size_t cap, int32_t *radii, const uint32_t *order, hipStream_t st)
{
    if (P <= 0) return;
    const int nblocks = (P + 255) / 256;
    dim3 grid(sg_frame_grid(nblocks, bt.K)), block(256);
    const int ht = sg_lds_hist(c.gx, c.gy) ? (int)sg_ctr_count((uint32_t)c.gx, (uint32_t)c.gy) : 0;     // histogram words (= tile counters)
    const bool ord = order && sg_order_applies(c);
#define SG_PPO(DD, OO) hipLaunchKernelGGL((sg_preprocess_fwd_kernel<DD, OO>), grid, block, (size_t)ht * 4, st, c, bt, P, means3D, shs, \
                                     colors_precomp, opacities, scales, rotations, cov3D_precomp, g, b, sg_cap32(cap), radii, ht, nblocks)
// K > 1 in work order: 64 Gaussians x K frames per workgroup, K waves, the inputs staged once in LDS
#define SG_PPK(DD) hipLaunchKernelGGL((sg_gauss_frames_fwd_kernel<DD>), dim3((P + 63) / 64), dim3(64 * bt.K), 64 * SG_GFF_PITCH * sizeof(float), \
                                     st, c, bt, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, g, b, radii)
#define SG_PP(DD) do { if (ord && bt.K > 1) SG_PPK(DD); else if (ord) SG_PPO(DD, true); else SG_PPO(DD, false); } while (0)
    int D = colors_precomp ? 0 : c.D;
    sg_prof_begin(SG_K_PREPROCESS_FWD, st);
    switch (D) { case 0: SG_PP(0); break; case 1: SG_PP(1); break; case 2: SG_PP(2); break; default: SG_PP(3); break; }
    if (ord)
        hipLaunchKernelGGL(sg_bin_ordered_kernel, dim3(nblocks, bt.K), block, 0, st, bt, P, g, b, c.gx, sg_key_pitch_of(false, c.flags), order);
    sg_prof_end(SG_K_PREPROCESS_FWD, st);
#undef SG_PP
#undef SG_PPK
#undef SG_PPO
}

// ------------------------------------------------------------------------------------------
// ACC: add to the gradient outputs instead of writing them (a compile-time switch: as a runtime flag the untaken branches cost
// the plain kernel 3.8 us of its 33 -- same-box A/B)
#define SG_PBWD_PARAMS SgCam c, int P, const float *__restrict__ means3D, const float *__restrict__ shs,                              \
                       const float *__restrict__ colors_precomp, const float *__restrict__ scales,                                \
                       const float *__restrict__ rotations, const float *__restrict__ cov3D_precomp,                              \
                       const int32_t *__restrict__ radii, SgGeom g, SgRec grec,                                                   \
                       size_t cap, const uint32_t *__restrict__ header, const uint8_t *__restrict__ rec_valid, float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dmeans2D, \
                       float *__restrict__ dL_dsh, float *__restrict__ dL_dcolors,                                                \
                       float *__restrict__ dL_dopacity, float *__restrict__ dL_dscales,                                           \
                       float *__restrict__ dL_drots, float *__restrict__ dL_dcov3D
// The single-camera kernel and (SG_PBWD_AUX 1) its variant for the depth / alpha maps (sg_rasterize_backward_aux).  One source,
// included twice: as an inlined body the plain kernel compiled to different code.
#define SG_PBWD_AUX 0
#include "sg_preprocess_bwd.inc"
#undef SG_PBWD_AUX
#define SG_PBWD_AUX 1
#include "sg_preprocess_bwd.inc"
#undef SG_PBWD_AUX

// ---- K cameras per launch (round 4; one kernel, the frames summed in LDS, since round 13) ---------------------------------------
// K cameras (bt.K frames) of the SAME Gaussians: the K gradients of a Gaussian are summed in frame order (frame 0 assigns, frame
// f > 0 adds: bit for bit what K single-camera calls leave behind when the first writes the gradient buffer and the others run with
// accumulate = 1) and the 248-byte gradient row is written ONCE: K - 1 read-modify-write passes over the buffer less (at cfg3
// 2 x 47 MB per view).  dL_dmeans2D (the densifier's per-view statistic) is per frame.
//
// Only the ADDITIONS are ordered; what a frame contributes depends on that frame alone.  sg_gauss_frames_bwd_kernel: a workgroup is
// 64 consecutive Gaussians x K frames, K waves; wave f works on frame f (camera, geometry, record and header pointers stay
// wave-uniform), lane = Gaussian.  The K waves read the same positions, scales, rotations and SH rows: from HBM once, from the
// CU's cache K - 1 times.
//  1. per wave: steps 0-2 of the single-camera kernel -- visibility, sg_sum_records_coop, sg_project_bwd -- without forming dL/dsh.
//     The wave stores the frame's dL_dmeans2D row and leaves one row per (frame, Gaussian) in ITS block of LDS (the record-chunk
//     block, free once the record loop is over; SG_GF_PITCH floats, an odd pitch: lane-strided writes hit distinct banks):
//         0-2 dmean, 3 dop | 4-6 dsc, 7-10 drot (cov3D_precomp: 4-9 the six g6) | 11-13 dRGB | 14-29 sg_sh_basis(dir) | 30 visible
//     dRGB: the colour gradient after the clamp mask (no SH rows: the plain colour gradient).  A frame that does not see the
//     Gaussian leaves +0 in slots 0-13 and `visible` = 0.
//  2. behind ONE workgroup barrier the 64 K threads share the 64 Gaussians' outputs, dealt so that consecutive lanes hold
//     consecutive floats of an output array (whole lines are stored): per (Gaussian, coefficient) the three dL/dsh channels, per
//     (Gaussian, value) a geometry sum.  Each walks the frames 0 .. K - 1 in order with the single-camera accumulate's expressions
//     (geometry: new + old, an invisible frame enters as +0; dL/dsh = basis * dRGB, an invisible frame leaves the sums alone).
// No wave leaves between kernel entry and the barrier: a wave whose 64 Gaussians lie behind P, that sees nothing
// (sg_sum_records_coop returns to its caller, not from the kernel) or whose frame overflowed (header[1]) still writes its 64
// `visible` words and arrives.
// (Rounds 4-11 held the chain rule INSIDE a frame loop: 168 registers, 48 KiB of LDS, two waves per SIMD.  Round 12 split it into
//  a per-(Gaussian, frame) kernel that wrote 64-byte rows to memory and a sum kernel that read them back: K P 128 bytes of traffic
//  and a launch that existed only to order K additions -- LAB.md.)
#define SG_GF_PITCH 31                                      // floats per (frame, Gaussian) row in LDS
#define SG_GF_BLOCK 2048                                    // floats per wave: 64 rows (1 984), or a record chunk (SG_REC_CHUNK * 12)
#define SG_GF_RGB 11
#define SG_GF_BAS 14
#define SG_GF_VIS 30
#define SG_GF_BATCH 8                                       // frames whose rows step 2 reads at once
static_assert(64 * SG_GF_PITCH <= SG_GF_BLOCK && SG_REC_CHUNK * 12 <= SG_GF_BLOCK, "a wave's LDS block holds its rows and a record chunk");
// ACC: the sums START from what the gradient buffer holds (read once, in step 2), so that the K frames are added in the order K
// single-camera calls with accumulate = 1 would add them: ((old + g0) + g1) + ...; otherwise frame 0 ASSIGNS (a -0 survives).
template <int D, bool ACC>
__global__ void __launch_bounds__(1024)
sg_gauss_frames_bwd_kernel(SgCam c, SgBatch bt, int P, const float *__restrict__ means3D, const float *__restrict__ shs,
                           const float *__restrict__ scales, const float *__restrict__ rotations,
                           const float *__restrict__ cov3D_precomp, const int32_t *__restrict__ radii, SgGeom g, SgRec grec,
                           size_t cap, const uint32_t *__restrict__ header, const uint8_t *__restrict__ rec_valid,
                           float *__restrict__ dL_dmeans2D, float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dsh,
                           float *__restrict__ dL_dcolors, float *__restrict__ dL_dopacity, float *__restrict__ dL_dscales,
                           float *__restrict__ dL_drots, float *__restrict__ dL_dcov3D)
{
    extern __shared__ float sg_gf_lds[];                    // K blocks of SG_GF_BLOCK floats
    const int lane = threadIdx.x & 63;
    const int frame = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (scalar: the frame's pointers stay in SGPRs)
    const int g0 = (int)blockIdx.x * 64;
    constexpr int nc = (D + 1) * (D + 1);
    const bool want_sh = shs != nullptr;
    {
        // ---- 1. frame `frame` of Gaussian g0 + lane
        const int idx = g0 + lane;
        float *L = sg_gf_lds + frame * SG_GF_BLOCK;
        const SgCam cf = sg_frame(c, frame, bt.cam_stride);
        const SgGeom gf = sg_frame(g, (size_t)frame * bt.geom);
        const SgRec grf = sg_frame(grec, (size_t)frame * bt.rec);
        const uint32_t *hf = sg_at(header, (size_t)frame * bt.bin);
        const uint8_t *rvf = sg_at(rec_valid, (size_t)frame * bt.bin);
        const int32_t *rad = radii + (size_t)frame * bt.P;
        const bool live = idx < P;
        // after a forward that overflowed (header[1] != 0) the backward composite wrote no records: the frame contributes nothing
        const bool vis = live && rad[idx] > 0 && hf[1] == 0u;
        const int Mrows = cf.M;
        // 0. every load that does not depend on another one up front
        float4 rc = make_float4(0, 0, 0, 0);
        float p[3] = { 0, 0, 0 }, s3[3] = { 0, 0, 0 }, q[4] = { 0, 0, 0, 0 }, sh[nc * 3];
        uint32_t flags = 0;
        if (vis) {
            { const uint2 sl = gf.slot[idx]; rc.y = __uint_as_float(sl.x); rc.w = __uint_as_float(sl.y); }
            flags = gf.flags[idx];
            p[0] = means3D[3 * idx]; p[1] = means3D[3 * idx + 1]; p[2] = means3D[3 * idx + 2];
            if (!cov3D_precomp) {
                s3[0] = scales[3 * idx]; s3[1] = scales[3 * idx + 1]; s3[2] = scales[3 * idx + 2];
                q[0] = rotations[4 * idx]; q[1] = rotations[4 * idx + 1]; q[2] = rotations[4 * idx + 2]; q[3] = rotations[4 * idx + 3];
            }
        }
        // 1. this Gaussian's gradient records of this frame (wave-cooperative, coalesced)
        float a9[9];
        sg_sum_records_coop(grf, cap, vis, rc, lane, L, a9, rvf);
        float *row = L + lane * SG_GF_PITCH;                // (the record loop is over: the block is this wave's to reuse)
        row[SG_GF_VIS] = vis ? 1.0f : 0.0f;
        if (!vis) {                                         // the geometry slots of a frame that does not see the Gaussian: +0
#pragma unroll
            for (int k = 0; k < SG_GF_BAS; k++) row[k] = 0.0f;
        }
        if (live) {
            // the screen-space gradient is per VIEW (the densifier's statistic): zeros for a Gaussian this frame does not see
            float *m2 = dL_dmeans2D + 3 * ((size_t)frame * bt.P + idx);
            if (!vis) { m2[0] = 0.0f; m2[1] = 0.0f; m2[2] = 0.0f; }
        }
        if (vis) {
            float *m2 = dL_dmeans2D + 3 * ((size_t)frame * bt.P + idx);
            // 2. the chain rule without its SH block (dL/dsh is NOT formed: the row carries dRGB and the basis, step 2 multiplies)
            SgGaussGrad G;
            sg_project_bwd<D>(cf, p, s3, q, cov3D_precomp ? cov3D_precomp + 6 * (size_t)idx : nullptr, nullptr, flags, a9, false, nullptr, G);
            m2[0] = G.g2[0]; m2[1] = G.g2[1]; m2[2] = 0.0f;
            float dRGB[3] = { G.dcol[0], G.dcol[1], G.dcol[2] };
            if (want_sh) {
                // the SH block of sg_project_bwd, its expressions in its order: dL/ddir and its share of dL/dmean.  The coefficient
                // row is requested HERE (opaque index: not in front of the record loop or the cov2D / cov3D chain, where its 48
                // registers would be live across both) and consumed in order by the dL/ddir sums.
                int ish = idx;
                asm volatile("" : "+v"(ish), "+v"(G.dmean[2]), "+v"(G.drot[3]));
                const float *src = shs + (size_t)ish * Mrows * 3;
                if (D == 3 && Mrows == 16) {
#pragma unroll
                    for (int k = 0; k < nc * 3 / 4; k++) {
                        const float4 v = ((const float4 *)src)[k];
                        sh[4 * k] = v.x; sh[4 * k + 1] = v.y; sh[4 * k + 2] = v.z; sh[4 * k + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < nc * 3; k++) sh[k] = src[k];
                }
                float dorig[3] = { p[0] - cf.campos[0], p[1] - cf.campos[1], p[2] - cf.campos[2] };
                float sum2 = dorig[0] * dorig[0] + dorig[1] * dorig[1] + dorig[2] * dorig[2];
                float len = sqrtf(sum2);
                float dir[3] = { dorig[0] / len, dorig[1] / len, dorig[2] / len };
                {
                    float bas[16];
                    sg_sh_basis<D>(dir, bas);
#pragma unroll
                    for (int k = 0; k < nc; k++) row[SG_GF_BAS + k] = bas[k];
                }
                float db[48];
                sg_sh_basis_grad<D>(dir, db);
#pragma unroll
                for (int ch = 0; ch < 3; ch++) dRGB[ch] = (flags >> ch) & 1u ? 0.0f : G.dcol[ch];
                float ddir[3] = { 0, 0, 0 };
#pragma unroll
                for (int k = 1; k < nc; k++)
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        float sv = sh[3 * k + ch] * dRGB[ch];
                        ddir[0] += db[3 * k] * sv; ddir[1] += db[3 * k + 1] * sv; ddir[2] += db[3 * k + 2] * sv;
                    }
                float inv32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
                float vx = dorig[0], vy = dorig[1], vz = dorig[2];
                G.dmean[0] += ((sum2 - vx * vx) * ddir[0] - vy * vx * ddir[1] - vz * vx * ddir[2]) * inv32;
                G.dmean[1] += (-vx * vy * ddir[0] + (sum2 - vy * vy) * ddir[1] - vz * vy * ddir[2]) * inv32;
                G.dmean[2] += (-vx * vz * ddir[0] - vy * vz * ddir[1] + (sum2 - vz * vz) * ddir[2]) * inv32;
            }
            row[0] = G.dmean[0]; row[1] = G.dmean[1]; row[2] = G.dmean[2]; row[3] = G.dop;
            if (cov3D_precomp) {
#pragma unroll
                for (int k = 0; k < 6; k++) row[4 + k] = G.g6[k];
            } else {
                row[4] = G.dsc[0]; row[5] = G.dsc[1]; row[6] = G.dsc[2];
                row[7] = G.drot[0]; row[8] = G.drot[1]; row[9] = G.drot[2]; row[10] = G.drot[3];
            }
            row[SG_GF_RGB] = dRGB[0]; row[SG_GF_RGB + 1] = dRGB[1]; row[SG_GF_RGB + 2] = dRGB[2];
        }
    }
    __syncthreads();                                        // every wave of the workgroup arrives (no return above)
    // ---- 2. the sums over the frames, in frame order; thread t takes items t, t + 64 K, ...
    const int tid = (int)threadIdx.x, nthr = bt.K * 64, nframes = bt.K;
    const int nlive = P - g0 < 64 ? P - g0 : 64;
    if (want_sh) {
        // an item: the three channels of (Gaussian j, coefficient k).  Coefficient-major planes [M][P][3], only the (D+1)^2 in use
        // (SG_FLAG_SH_PLANAR), or the reference's rows [P][M][3]: every one of the M rows is written (ACC: those in use)
        const bool planar = c.flags & SG_FLAG_SH_PLANAR;
        const int Mrows = c.M;
        const int nitems = 64 * (planar ? nc : Mrows);
        for (int it = tid; it < nitems; it += nthr) {
            int j, k;
            float *dst;
            if (planar) { k = it >> 6; j = it & 63; dst = dL_dsh + ((size_t)k * P + (size_t)(g0 + j)) * 3; }
            else { j = it / Mrows; k = it - j * Mrows; dst = dL_dsh + ((size_t)(g0 + j) * Mrows + k) * 3; }
            if (j >= nlive) continue;
            if (k >= nc) {
                if (!ACC) { dst[0] = 0.0f; dst[1] = 0.0f; dst[2] = 0.0f; }
                continue;
            }
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            if (ACC) { a0 = dst[0]; a1 = dst[1]; a2 = dst[2]; }
            const float *r = sg_gf_lds + j * SG_GF_PITCH;
            // SG_GF_BATCH frames at a time: every read of the batch goes out before the first value is used (the opaque point
            // below; as a plain loop hipcc tested `visible` per frame and read dRGB under the branch: two LDS round trips per
            // frame and item).  A frame index past K is clamped to K - 1 (a valid row, its values unused); an invisible frame's
            // row holds stale record bytes behind slot SG_GF_BAS -- read, multiplied and dropped by the select.
            for (int f0 = 0; f0 < nframes; f0 += SG_GF_BATCH) {
                float vv[SG_GF_BATCH], bb[SG_GF_BATCH], d0[SG_GF_BATCH], d1[SG_GF_BATCH], d2[SG_GF_BATCH];
#pragma unroll
                for (int u = 0; u < SG_GF_BATCH; u++) {
                    const float *rf = r + (f0 + u < nframes ? f0 + u : nframes - 1) * SG_GF_BLOCK;
                    vv[u] = rf[SG_GF_VIS]; bb[u] = rf[SG_GF_BAS + k];
                    d0[u] = rf[SG_GF_RGB]; d1[u] = rf[SG_GF_RGB + 1]; d2[u] = rf[SG_GF_RGB + 2];
                }
#pragma unroll
                for (int u = 0; u < SG_GF_BATCH; u++) asm volatile("" : "+v"(vv[u]), "+v"(bb[u]), "+v"(d0[u]), "+v"(d1[u]), "+v"(d2[u]));
#pragma unroll
                for (int u = 0; u < SG_GF_BATCH; u++) {
                    const bool seen = f0 + u < nframes && vv[u] != 0.0f, first = !ACC && f0 + u == 0;
                    const float p0 = bb[u] * d0[u], p1 = bb[u] * d1[u], p2 = bb[u] * d2[u];
                    a0 = seen ? (first ? p0 : a0 + p0) : a0;
                    a1 = seen ? (first ? p1 : a1 + p1) : a1;
                    a2 = seen ? (first ? p2 : a2 + p2) : a2;
                }
            }
            dst[0] = a0; dst[1] = a1; dst[2] = a2;
        }
    }
    // an item: one geometry value of one Gaussian, in the order of the output arrays (means | opacity | scales, rotations or the six
    // covariances | colours), float t of an array's 64-Gaussian piece on consecutive lanes
    const bool g6rows = cov3D_precomp != nullptr;
    const int nB = g6rows ? 6 * 64 : 3 * 64, nC = g6rows ? 0 : 4 * 64;
    const int ngeo = 3 * 64 + 64 + nB + nC + (dL_dcolors ? 3 * 64 : 0);
    for (int it = tid; it < ngeo; it += nthr) {
        int t = it, j, s;
        float *dst;
        if (t < 3 * 64) { j = t / 3; s = t - 3 * j; dst = dL_dmeans3D + 3 * (size_t)g0 + t; }
        else if ((t -= 3 * 64) < 64) { j = t; s = 3; dst = dL_dopacity + (size_t)g0 + t; }
        else if ((t -= 64) < nB) {
            if (g6rows) { j = t / 6; s = 4 + t - 6 * j; dst = dL_dcov3D ? dL_dcov3D + 6 * (size_t)g0 + t : nullptr; }
            else { j = t / 3; s = 4 + t - 3 * j; dst = dL_dscales ? dL_dscales + 3 * (size_t)g0 + t : nullptr; }
        }
        else if ((t -= nB) < nC) { j = t >> 2; s = 7 + (t & 3); dst = dL_drots ? dL_drots + 4 * (size_t)g0 + t : nullptr; }
        else { t -= nC; j = t / 3; s = SG_GF_RGB + t - 3 * j; dst = dL_dcolors + 3 * (size_t)g0 + t; }
        if (!dst || j >= nlive) continue;
        float a = 0.0f;
        if (ACC) a = *dst;
        const float *r = sg_gf_lds + j * SG_GF_PITCH;
        // (operand order of the single-camera accumulate: new + old)
        // (an invisible frame's row holds +0 in the geometry slots: what the single-camera kernel adds for it)
        for (int f0 = 0; f0 < nframes; f0 += SG_GF_BATCH) {
            float v[SG_GF_BATCH];
#pragma unroll
            for (int u = 0; u < SG_GF_BATCH; u++) v[u] = r[(f0 + u < nframes ? f0 + u : nframes - 1) * SG_GF_BLOCK + s];
#pragma unroll
            for (int u = 0; u < SG_GF_BATCH; u++) asm volatile("" : "+v"(v[u]));
#pragma unroll
            for (int u = 0; u < SG_GF_BATCH; u++)
                if (f0 + u < nframes) a = (!ACC && f0 + u == 0) ? v[u] : v[u] + a;
        }
        *dst = a;
    }
}
// the kernel's dynamic LDS (K blocks) is above the default 64-KiB limit from K = 9 on: raised once per device, to the K = 16 size
template <int D, bool ACC> static bool sg_gauss_frames_lds(size_t bytes)
{
    static SgLdsLimit limit;
    return bytes <= 64 * 1024 ||
           sg_dyn_lds_limit(limit, (const void *)sg_gauss_frames_bwd_kernel<D, ACC>, SG_MAX_FRAMES * SG_GF_BLOCK * 4);
}
static bool sg_gauss_frames_fit(int D, bool acc, size_t bytes)
{
#define SG_GF_FIT(DD) (acc ? sg_gauss_frames_lds<DD, true>(bytes) : sg_gauss_frames_lds<DD, false>(bytes))
    switch (D) { case 0: return SG_GF_FIT(0); case 1: return SG_GF_FIT(1); case 2: return SG_GF_FIT(2); default: return SG_GF_FIT(3); }
#undef SG_GF_FIT
}

void sg_launch_preprocess_bwd(const SgCam &c, const SgBatch &bt, int P, const float *means3D, const float *shs,
                              const float *colors_precomp, const float *opacities, const float *scales,
                              const float *rotations, const float *cov3D_precomp,
                              const int32_t *radii, SgGeom g, SgRec grec, size_t cap, const uint32_t *header, const uint8_t *rec_valid,
                              float4 *a9buf, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dsh,
                              float *dL_dcolors, float *dL_dopacity, float *dL_dscales,
                              float *dL_drots, float *dL_dcov3D, int accumulate, hipStream_t st, const float *dz)
{
    (void)opacities; (void)a9buf;                           // (a9buf: the skinned path's block; the raster path sums in LDS)
    if (P <= 0) return;
    const int nblocks = (P + 255) / 256;
    dim3 grid(nblocks), block(256);
    int D = shs ? c.D : 0;
    // K > 1 with an output the LDS rows do not carry (dL_dcolors beside SH rows; dL_dcov3D without cov3D_precomp -- no caller of
    // the project asks for either), or on a device whose runtime refuses the kernel its LDS: the chain of K single-camera
    // launches the kernel is defined by
    const size_t lds = (size_t)bt.K * SG_GF_BLOCK * sizeof(float);
    if (bt.K > 1 && ((shs && dL_dcolors) || (!cov3D_precomp && dL_dcov3D) || !sg_gauss_frames_fit(D, accumulate != 0, lds))) {
        SgBatch one = bt;
        one.K = 1;
        for (int f = 0; f < bt.K; f++)
            sg_launch_preprocess_bwd(sg_frame(c, f, bt.cam_stride), one, P, means3D, shs, colors_precomp, opacities, scales, rotations,
                                     cov3D_precomp, radii + (size_t)f * bt.P, sg_frame(g, (size_t)f * bt.geom),
                                     sg_frame(grec, (size_t)f * bt.rec), cap, sg_at(header, (size_t)f * bt.bin),
                                     sg_at(rec_valid, (size_t)f * bt.bin), nullptr, dL_dmeans3D, dL_dmeans2D + 3 * (size_t)f * bt.P,
                                     dL_dsh, dL_dcolors, dL_dopacity, dL_dscales, dL_drots, dL_dcov3D, accumulate || f > 0, st, nullptr);
        return;
    }
#define SG_PB1(DD, AA) hipLaunchKernelGGL((sg_preprocess_bwd_kernel<DD, AA>), grid, block, 0, st, c, P, means3D, shs, \
                                     colors_precomp, scales, rotations, cov3D_precomp, radii, g,            \
                                     grec, cap, header, rec_valid, dL_dmeans3D, dL_dmeans2D, dL_dsh, dL_dcolors, \
                                     dL_dopacity, dL_dscales, dL_drots, dL_dcov3D)
// K > 1: 64 Gaussians x K frames per workgroup, K waves, the frames' gradients summed through LDS
#define SG_PBK(DD, AA) hipLaunchKernelGGL((sg_gauss_frames_bwd_kernel<DD, AA>), dim3((P + 63) / 64), dim3(64 * bt.K), lds, st, c, bt, P,  \
                                     means3D, shs, scales, rotations, cov3D_precomp, radii, g, grec, cap, header, rec_valid,          \
                                     dL_dmeans2D, dL_dmeans3D, dL_dsh, dL_dcolors, dL_dopacity, dL_dscales, dL_drots, dL_dcov3D)
#define SG_PB2(DD, AA) do { if (bt.K == 1) SG_PB1(DD, AA); else SG_PBK(DD, AA); } while (0)      // (K = 1: the round-3 kernel, untouched)
#define SG_PB(DD) do { if (accumulate) SG_PB2(DD, true); else SG_PB2(DD, false); } while (0)
    sg_prof_begin(SG_K_PREPROCESS_BWD, st);
#define SG_PBA(DD) hipLaunchKernelGGL((sg_preprocess_bwd_aux_kernel<DD>), grid, block, 0, st, c, P, means3D, shs,            \
                                     colors_precomp, scales, rotations, cov3D_precomp, radii, g,            \
                                     grec, cap, header, rec_valid, dL_dmeans3D, dL_dmeans2D, dL_dsh, dL_dcolors, \
                                     dL_dopacity, dL_dscales, dL_drots, dL_dcov3D, dz)
    if (dz)       // (the aux entry point: K = 1, accumulate = 0)
        switch (D) { case 0: SG_PBA(0); break; case 1: SG_PBA(1); break; case 2: SG_PBA(2); break; default: SG_PBA(3); break; }
    else
    switch (D) { case 0: SG_PB(0); break; case 1: SG_PB(1); break; case 2: SG_PB(2); break; default: SG_PB(3); break; }
#undef SG_PBA
    sg_prof_end(SG_K_PREPROCESS_BWD, st);
#undef SG_PB
#undef SG_PB2
#undef SG_PB1
#undef SG_PBK
}
