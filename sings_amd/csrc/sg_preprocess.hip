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

// The pair expansion of a NOBIN launch, in work order: lane i reads the rectangle (recC) and the depth of Gaussian order[i] -- what
// the kernel above stored -- and bins it (sg_bin_ordered).  Grid: Gaussian blocks x frames.  An entry >= P is never dereferenced:
// its lane is idle.
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
        const float4 rc = g.recC[SG_REC_STRIDE * (size_t)gid];
        rmin = __float_as_uint(rc.z); rwh = __float_as_uint(rc.w);
        dep = __float_as_uint(g.depth[gid]);
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
#define SG_PP(DD) do { if (ord) SG_PPO(DD, true); else SG_PPO(DD, false); } while (0)
    int D = colors_precomp ? 0 : c.D;
    sg_prof_begin(SG_K_PREPROCESS_FWD, st);
    switch (D) { case 0: SG_PP(0); break; case 1: SG_PP(1); break; case 2: SG_PP(2); break; default: SG_PP(3); break; }
    if (ord)
        hipLaunchKernelGGL(sg_bin_ordered_kernel, dim3(nblocks, bt.K), block, 0, st, bt, P, g, b, c.gx, sg_key_pitch_of(false, c.flags), order);
    sg_prof_end(SG_K_PREPROCESS_FWD, st);
#undef SG_PP
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

// ---- K cameras per launch (round 4; two kernels since round 12) ---------------------------------------------------------------
// K cameras (bt.K frames) of the SAME Gaussians: the K gradients of a Gaussian are summed in frame order (frame 0 assigns, frame
// f > 0 adds: bit for bit what K single-camera calls leave behind when the first writes the gradient buffer and the others run with
// accumulate = 1) and the 248-byte gradient row is written ONCE: K - 1 read-modify-write passes over the buffer less (at cfg3
// 2 x 47 MB per view).  dL_dmeans2D (the densifier's per-view statistic) is per frame.
//
// Only the ADDITIONS are ordered; what a frame contributes depends on that frame alone.  So the work is two kernels:
//  1. sg_gauss_frame_bwd_kernel: one (Gaussian, frame) per lane at full grid, in the (block, frame) order of the forward
//     (sg_block_frame: the K frames of a block back to back on one XCD -- positions, scales, rotations and SH rows come from HBM
//     once and from L2 K - 1 times).  Steps 0-2 of the single-camera kernel -- visibility, sg_sum_records_coop, sg_project_bwd --
//     without forming dL/dsh: it writes the frame's dL_dmeans2D row and one 64-byte row per VISIBLE (frame, Gaussian) into the
//     block behind the K record buffers (sg_a9_bytes):
//         vector 0: dmean.xyz, dop      vector 1: dsc.xyz, -      vector 2: drot.xyzw      vector 3: dRGB.xyz, -
//     dRGB: the colour gradient after the clamp mask (no SH rows: the plain colour gradient); with cov3D_precomp the six g6 values
//     take vectors 1-2 instead (g6[0..3] | g6[4], g6[5], -, -).
//  2. sg_gauss_sum_frames_kernel: one Gaussian per lane, the ordered part and nothing else.  It walks the K rows of its Gaussian
//     (the next one requested ahead), adds the geometry values as the single-camera accumulate does (new + old) and forms
//     dL/dsh = basis(dir_f) * dRGB_f from the position and the frame's camera centre -- the expressions of sg_project_bwd --
//     in 48 registers: no SH coefficient, record, slot or flag word is read here.
// (The one-kernel form this replaces held the chain rule INSIDE the frame loop: 168 registers and 48 KiB of LDS per workgroup,
//  two waves per SIMD, the 192-byte SH row re-read per trip: 119 us + 63 us of record sums at cfg3, K = 8 -- LAB.md.)
#define SG_GROW_VEC 4                                       // 16-byte vectors per (frame, Gaussian) row
template <int D>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
sg_gauss_frame_bwd_kernel(SgCam c, SgBatch bt, int P, const float *__restrict__ means3D, const float *__restrict__ shs,
                          const float *__restrict__ scales, const float *__restrict__ rotations,
                          const float *__restrict__ cov3D_precomp, const int32_t *__restrict__ radii, SgGeom g, SgRec grec,
                          size_t cap, const uint32_t *__restrict__ header, const uint8_t *__restrict__ rec_valid,
                          float4 *__restrict__ rows, float *__restrict__ dL_dmeans2D, int nblocks)
{
    __shared__ float lds_all[4][32 * SG_ROW_LDS];          // 6.5 KiB per wave: the record chunks
    int gblock, frame;
    if (!sg_block_frame((int)blockIdx.x, bt.K, nblocks, gblock, frame)) return;
    c = sg_frame(c, frame, bt.cam_stride); g = sg_frame(g, (size_t)frame * bt.geom); grec = sg_frame(grec, (size_t)frame * bt.rec);
    header = sg_at(header, (size_t)frame * bt.bin); rec_valid = sg_at(rec_valid, (size_t)frame * bt.bin);
    radii += (size_t)frame * bt.P;
    const int idx = gblock * 256 + (int)threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (idx - lane >= P) return;                            // whole wave out of range
    const bool live = idx < P;
    // after a forward that overflowed (header[1] != 0) the backward composite wrote no records: the frame contributes nothing
    const bool vis = live && radii[idx] > 0 && header[1] == 0u;
    const int Mrows = c.M;
    constexpr int nc = (D + 1) * (D + 1);
    const bool want_sh = shs != nullptr;
    // 0. every load that does not depend on another one up front
    float4 rc = make_float4(0, 0, 0, 0);
    float p[3] = { 0, 0, 0 }, s3[3] = { 0, 0, 0 }, q[4] = { 0, 0, 0, 0 }, sh[nc * 3];
    uint32_t flags = 0;
    if (vis) {
        { const uint2 sl = g.slot[idx]; rc.y = __uint_as_float(sl.x); rc.w = __uint_as_float(sl.y); }
        flags = g.flags[idx];
        p[0] = means3D[3 * idx]; p[1] = means3D[3 * idx + 1]; p[2] = means3D[3 * idx + 2];
        if (!cov3D_precomp) {
            s3[0] = scales[3 * idx]; s3[1] = scales[3 * idx + 1]; s3[2] = scales[3 * idx + 2];
            q[0] = rotations[4 * idx]; q[1] = rotations[4 * idx + 1]; q[2] = rotations[4 * idx + 2]; q[3] = rotations[4 * idx + 3];
        }
    }
    // 1. this Gaussian's gradient records of this frame (wave-cooperative, coalesced)
    float a9[9];
    sg_sum_records_coop(grec, cap, vis, rc, lane, lds_all[wave], a9, rec_valid);
    if (!live) return;
    // the screen-space gradient is per VIEW (the densifier's statistic): zeros for a Gaussian this frame does not see
    float *m2 = dL_dmeans2D + 3 * ((size_t)frame * bt.P + idx);
    if (!vis) { m2[0] = 0.0f; m2[1] = 0.0f; m2[2] = 0.0f; return; }
    // 2. the chain rule without its SH block (dL/dsh is NOT formed: the rows below carry dRGB, the sum kernel multiplies by the basis)
    SgGaussGrad G;
    sg_project_bwd<D>(c, p, s3, q, cov3D_precomp ? cov3D_precomp + 6 * (size_t)idx : nullptr, nullptr, flags, a9, false, nullptr, G);
    m2[0] = G.g2[0]; m2[1] = G.g2[1]; m2[2] = 0.0f;
    float dRGB[3] = { G.dcol[0], G.dcol[1], G.dcol[2] };
    if (want_sh) {
        // the SH block of sg_project_bwd, its expressions in its order: dL/ddir and its share of dL/dmean.  The coefficient row is
        // requested HERE (opaque index: not in front of the record loop or the cov2D / cov3D chain, where its 48 registers would be
        // live across both) and consumed in order by the dL/ddir sums.
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
        float dorig[3] = { p[0] - c.campos[0], p[1] - c.campos[1], p[2] - c.campos[2] };
        float sum2 = dorig[0] * dorig[0] + dorig[1] * dorig[1] + dorig[2] * dorig[2];
        float len = sqrtf(sum2);
        float dir[3] = { dorig[0] / len, dorig[1] / len, dorig[2] / len };
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
    float4 *o = rows + SG_GROW_VEC * ((size_t)frame * bt.P + idx);
    o[0] = make_float4(G.dmean[0], G.dmean[1], G.dmean[2], G.dop);
    if (cov3D_precomp) {
        o[1] = make_float4(G.g6[0], G.g6[1], G.g6[2], G.g6[3]);
        o[2] = make_float4(G.g6[4], G.g6[5], 0.0f, 0.0f);
    } else {
        o[1] = make_float4(G.dsc[0], G.dsc[1], G.dsc[2], 0.0f);
        o[2] = make_float4(G.drot[0], G.drot[1], G.drot[2], G.drot[3]);
    }
    o[3] = make_float4(dRGB[0], dRGB[1], dRGB[2], 0.0f);
}

// ACC: the sums START from what the gradient buffer holds (read once, here), so that the K frames are added in the order K
// single-camera calls with accumulate = 1 would add them: ((old + g0) + g1) + ...; otherwise frame 0 ASSIGNS (a -0 survives).
// A frame that does not see the Gaussian enters the geometry sums as +0 -- what the single-camera kernel adds for it -- and
// leaves the dL/dsh sums alone.
template <int D, bool ACC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
sg_gauss_sum_frames_kernel(SgCam c0, SgBatch bt, int P, const float *__restrict__ means3D, const int32_t *__restrict__ radii0,
                           const uint32_t *__restrict__ header0, const float4 *__restrict__ rows, int g6rows,
                           float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dsh, float *__restrict__ dL_dcolors,
                           float *__restrict__ dL_dopacity, float *__restrict__ dL_dscales, float *__restrict__ dL_drots,
                           float *__restrict__ dL_dcov3D)
{
    __shared__ float lds_all[4][32 * SG_ROW_LDS];          // the staging rows of the dL/dsh store
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = idx - lane;
    if (g0 >= P) return;                                    // whole wave out of range
    const bool live = idx < P;
    const int Mrows = c0.M;
    const int nframes = bt.K;
    constexpr int nc = (D + 1) * (D + 1);
    const bool want_sh = dL_dsh != nullptr;
    const bool planar = c0.flags & SG_FLAG_SH_PLANAR;
    const bool staged = D == 3 && Mrows == 16 && want_sh && !planar;
    // frame f + 1's (visible, row) are requested while frame f is added; frame 0's go out with the position
    bool vis_n = live && radii0[idx] > 0 && header0[1] == 0u;
    const float4 z4 = make_float4(0, 0, 0, 0);
    float4 n[SG_GROW_VEC] = { z4, z4, z4, z4 };
    if (vis_n) {
        const float4 *src = rows + SG_GROW_VEC * (size_t)idx;
#pragma unroll
        for (int v = 0; v < SG_GROW_VEC; v++) n[v] = src[v];
    }
    float p[3] = { 0, 0, 0 };
    if (live) { p[0] = means3D[3 * idx]; p[1] = means3D[3 * idx + 1]; p[2] = means3D[3 * idx + 2]; }
    // the sums over the frames.  Geometry, in the rows' layout: A[0..3] = dmean.xyz, dop; A[4..11] = dsc.xyz, -, drot.xyzw (g6rows:
    // the six g6, -, -); A[12..14] = the colour gradient -- kept in the wave's LDS block while the frames are walked ([value][lane]:
    // conflict-free; the dL/dsh sums, the requested row and the basis take the 128 registers of four waves per SIMD)
    constexpr int NA = 4 * SG_GROW_VEC - 1;
    static_assert(NA * 64 <= 32 * SG_ROW_LDS, "the geometry sums fit the wave's staging block");
    float *sA = lds_all[wave] + lane;
    float A[NA];
#pragma unroll
    for (int k = 0; k < NA; k++) A[k] = 0.0f;
    float acc[nc * 3];
#pragma unroll
    for (int k = 0; k < nc * 3; k++) acc[k] = 0.0f;
    if (ACC && live) {
#pragma unroll
        for (int k = 0; k < 3; k++) A[k] = dL_dmeans3D[3 * idx + k];
        A[3] = dL_dopacity[idx];
        if (g6rows) {
#pragma unroll
            for (int k = 0; k < 6; k++) A[4 + k] = dL_dcov3D ? dL_dcov3D[6 * idx + k] : 0.0f;
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) A[4 + k] = dL_dscales ? dL_dscales[3 * idx + k] : 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) A[8 + k] = dL_drots ? dL_drots[4 * idx + k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) A[12 + k] = dL_dcolors ? dL_dcolors[3 * idx + k] : 0.0f;
        if (want_sh) {
            const float *row = dL_dsh + (size_t)idx * Mrows * 3;
#pragma unroll
            for (int k = 0; k < nc * 3; k++) acc[k] = planar ? dL_dsh[((size_t)(k / 3) * P + idx) * 3 + k % 3] : row[k];
        }
    }
#pragma unroll
    for (int k = 0; k < NA; k++) sA[64 * k] = A[k];
#pragma unroll 1
    for (int f = 0; f < nframes; f++) {
        const bool vis = vis_n;
        const bool first = !ACC && f == 0;
        // (opaque per trip: keeps hipcc from promoting the LDS sums to registers across the loop)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        float *sAf = lds_all[wave] + ln;
        // (operand order of the single-camera accumulate: new + old)
#pragma unroll
        for (int v = 0; v < SG_GROW_VEC; v++) {
            const float r[4] = { n[v].x, n[v].y, n[v].z, n[v].w };
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (4 * v + k < NA) sAf[64 * (4 * v + k)] = first ? r[k] : r[k] + sAf[64 * (4 * v + k)];
        }
        const float dRGB[3] = { n[3].x, n[3].y, n[3].z };
        if (f + 1 < nframes) {
            vis_n = live && radii0[(size_t)(f + 1) * bt.P + idx] > 0 && sg_at(header0, (size_t)(f + 1) * bt.bin)[1] == 0u;
#pragma unroll
            for (int v = 0; v < SG_GROW_VEC; v++) n[v] = z4;
            if (vis_n) {
                const float4 *src = rows + SG_GROW_VEC * ((size_t)(f + 1) * bt.P + idx);
#pragma unroll
                for (int v = 0; v < SG_GROW_VEC; v++) n[v] = src[v];
            }
        }
        if (want_sh && vis) {
            // the view direction and the basis: sg_project_bwd's expressions
            const float *campos = c0.campos + 3 * (size_t)f * (size_t)bt.cam_stride;
            float dorig[3] = { p[0] - campos[0], p[1] - campos[1], p[2] - campos[2] };
            float sum2 = dorig[0] * dorig[0] + dorig[1] * dorig[1] + dorig[2] * dorig[2];
            float len = sqrtf(sum2);
            float dir[3] = { dorig[0] / len, dorig[1] / len, dorig[2] / len };
            float bas[16];
            sg_sh_basis<D>(dir, bas);
#pragma unroll
            for (int k = 0; k < nc; k++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++)
                    acc[3 * k + ch] = first ? bas[k] * dRGB[ch] : acc[3 * k + ch] + bas[k] * dRGB[ch];
        }
    }
#pragma unroll
    for (int k = 0; k < NA; k++) A[k] = sA[64 * k];
    __builtin_amdgcn_s_waitcnt(0xC07F);                     // every lane holds its sums: the block is free for the staging rows
    __builtin_amdgcn_wave_barrier();
    // dL/dsh out: coefficient-major planes [M][P][3], only the (D+1)^2 in use (SG_FLAG_SH_PLANAR); or the reference's rows
    // (every one of the M rows is written; coalesced through LDS when staged).  (ACC: the sums already hold old + frames)
    if (want_sh && planar) {
        if (live) {
#pragma unroll
            for (int k = 0; k < nc * 3; k++) dL_dsh[((size_t)(k / 3) * P + idx) * 3 + k % 3] = acc[k];
        }
    } else if (want_sh) {
        if (staged) {
            float *L = lds_all[wave];
#pragma unroll
            for (int h = 0; h < 2; h++) {                    // 32 rows at a time
                if ((lane >> 5) == h) {
#pragma unroll
                    for (int k = 0; k < nc * 3 / 4; k++)
                        *(float4 *)(L + (lane & 31) * SG_ROW_LDS + 4 * k) = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
                sg_rows48_store(dL_dsh, g0 + 32 * h, P, lane, L, 32, false);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
            }
        } else if (live) {
            float *dsh_row = dL_dsh + (size_t)idx * Mrows * 3;
#pragma unroll
            for (int k = 0; k < nc * 3; k++) dsh_row[k] = acc[k];
            if (!ACC)
                for (int k = nc * 3; k < Mrows * 3; k++) dsh_row[k] = 0.0f;
        }
    }
    if (!live) return;
    dL_dmeans3D[3 * idx] = A[0]; dL_dmeans3D[3 * idx + 1] = A[1]; dL_dmeans3D[3 * idx + 2] = A[2];
    dL_dopacity[idx] = A[3];
    if (dL_dcolors) { dL_dcolors[3 * idx] = A[12]; dL_dcolors[3 * idx + 1] = A[13]; dL_dcolors[3 * idx + 2] = A[14]; }
    if (g6rows) {
        if (dL_dcov3D) {
#pragma unroll
            for (int k = 0; k < 6; k++) dL_dcov3D[6 * idx + k] = A[4 + k];
        }
    } else {
        if (dL_dscales) { dL_dscales[3 * idx] = A[4]; dL_dscales[3 * idx + 1] = A[5]; dL_dscales[3 * idx + 2] = A[6]; }
        if (dL_drots) { dL_drots[4 * idx] = A[8]; dL_drots[4 * idx + 1] = A[9]; dL_drots[4 * idx + 2] = A[10]; dL_drots[4 * idx + 3] = A[11]; }
    }
}

void sg_launch_preprocess_bwd(const SgCam &c, const SgBatch &bt, int P, const float *means3D, const float *shs,
                              const float *colors_precomp, const float *opacities, const float *scales,
                              const float *rotations, const float *cov3D_precomp,
                              const int32_t *radii, SgGeom g, SgRec grec, size_t cap, const uint32_t *header, const uint8_t *rec_valid,
                              float4 *a9buf, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dsh,
                              float *dL_dcolors, float *dL_dopacity, float *dL_dscales,
                              float *dL_drots, float *dL_dcov3D, int accumulate, hipStream_t st, const float *dz)
{
    (void)opacities;
    if (P <= 0) return;
    const int nblocks = (P + 255) / 256;
    dim3 grid(nblocks), block(256);
    int D = shs ? c.D : 0;
    // K > 1 with an output the 64-byte rows have no room for (dL_dcolors beside SH rows; dL_dcov3D without cov3D_precomp -- no
    // caller of the project asks for either): the chain of K single-camera launches the two kernels are defined by
    if (bt.K > 1 && ((shs && dL_dcolors) || (!cov3D_precomp && dL_dcov3D))) {
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
// K > 1: the per-(Gaussian, frame) chain rule at full grid (rows [K][P][4] vectors behind the K record buffers), then the ordered sums
#define SG_PBK(DD, AA) do {                                                                                                        \
        hipLaunchKernelGGL((sg_gauss_frame_bwd_kernel<DD>), dim3(sg_frame_grid(nblocks, bt.K)), block, 0, st, c, bt, P, means3D,   \
                           shs, scales, rotations, cov3D_precomp, radii, g, grec, cap, header, rec_valid, a9buf, dL_dmeans2D,      \
                           nblocks);                                                                                               \
        hipLaunchKernelGGL((sg_gauss_sum_frames_kernel<DD, AA>), grid, block, 0, st, c, bt, P, means3D, radii, header, a9buf,      \
                           cov3D_precomp != nullptr, dL_dmeans3D, dL_dsh, dL_dcolors, dL_dopacity, dL_dscales, dL_drots,           \
                           dL_dcov3D);                                                                                             \
    } while (0)
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
