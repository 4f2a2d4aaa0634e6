// SMPL linear-blend-skinning fused with the projection preprocess (forward and backward).
//
// Replaces the LBS block of SinGS.forward -- sings/rec/models/sings_hybrid.py:398-428 with
// sings/rec/utils/body_model/lbs.py:59-74 (T = W . A, v' = T [v;1]) and
// sings/rec/utils/geometry/rotations.py:98-149 (matrix_to_quaternion) -- and feeds the posed
// mean / rotation / scale straight into the projection of sg_project.h, so the posed means and
// quaternions, T[N,4,4] and the ~15 eager kernels of the reference never touch HBM.
//
// The only dense contraction on the path, T[64 x 16] = W[64 x J] . A[J x 16] per wave, runs on the
// matrix cores with v_mfma_f32_16x16x4_f32 (exact fp32, bitwise a k-ordered fmaf chain); its
// transpose dA[J x 16] = W^T . dT in backward likewise.  W is streamed once per pass in 64-B row
// segments through LDS (HBM-bound: 4J bytes per Gaussian dominate).
#include "sg_project.h"
#include "sg_rot.h"
#include "../../include/sings_scene.h"
#include "sg_skin.h"

struct SgSkin {
    int J, rot6d;            // rot6d: rot_canon is [P,6] (Zhou et al. 6-D form, rotation_6d_to_matrix fused in)
    const float *xyz_canon, *rot_canon, *lbs_w, *A, *smpl_scale, *transl, *ext_trans, *ext_rot, *ext_scale;
};
// from an SgSkinInputs or an SgSceneAvatar (the same fields under the same names)
template <typename In>
static SgSkin sg_skin_of(const In &in)
{
    return SgSkin{ in.J, in.rot_format == SG_ROT_CANON_6D, in.xyz_canon, in.rot_canon, in.lbs_weights, in.A, in.smpl_scale,
                   in.transl, in.ext_trans, in.ext_rot, in.ext_scale };
}

// T rows 0..2 (12 floats, row-major 3x4) of this lane's Gaussian g0 + lane.
// sA: [Jp][16] joint transforms (zero padded to a multiple of 16 rows), sW / sT: this wave's scratch.
__device__ __forceinline__ void sg_skin_T(const float *__restrict__ W, int J, int P, int g0, int lane,
                                          const float *__restrict__ sA, float *__restrict__ sW,
                                          float *__restrict__ sT, float T[12])
{
    f32x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; b++) acc[b] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
    const int nchunk = (J + 15) >> 4;
    const bool vec = (J & 3) == 0;
    float4 wv[4];
    if (vec) sg_w_fetch(W, J, P, g0, 0, lane, wv);
    for (int c = 0; c < nchunk; c++) {
        if (vec) {
            sg_w_stash(wv, lane, sW);
            if (c + 1 < nchunk) sg_w_fetch(W, J, P, g0, c + 1, lane, wv);
            __builtin_amdgcn_s_waitcnt(0xC07F);             // LDS only: the next chunk's global loads stay in flight
        } else {
            sg_stage_w_chunk(W, J, P, g0, c, lane, sW);
            __builtin_amdgcn_s_waitcnt(0);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            float bv = sA[(c * 16 + 4 * kk + (lane >> 4)) * 16 + (lane & 15)];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                float av = sW[(16 * b + (lane & 15)) * SG_WSTRIDE + 4 * kk + (lane >> 4)];
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[b], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // acc[b][r] = T[gaussian 16b + 4(lane>>4) + r][entry lane&15]  ->  transpose through LDS
    if ((lane & 15) < 12) {
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) sT[(16 * b + 4 * (lane >> 4) + r) * 13 + (lane & 15)] = acc[b][r];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = sT[lane * 13 + i];
    __builtin_amdgcn_wave_barrier();
}

struct SgPosed { float p[3], q[4], s3[3], Rdef[9], x[3], Rc[9], sc; int best; float qab; };

// sings_hybrid.py:400-428 for one Gaussian, given its blended transform T (3x4)
__device__ __forceinline__ void sg_pose_gaussian(const SgSkin &k, int idx, const float T[12],
                                                 const float *__restrict__ scales, SgPosed &o)
{
    o.x[0] = k.xyz_canon[3 * idx]; o.x[1] = k.xyz_canon[3 * idx + 1]; o.x[2] = k.xyz_canon[3 * idx + 2];
#pragma unroll
    for (int i = 0; i < 3; i++) o.p[i] = T[4 * i] * o.x[0] + T[4 * i + 1] * o.x[1] + T[4 * i + 2] * o.x[2] + T[4 * i + 3];
    o.s3[0] = scales[3 * idx]; o.s3[1] = scales[3 * idx + 1]; o.s3[2] = scales[3 * idx + 2];
    o.sc = k.smpl_scale ? k.smpl_scale[0] : 1.0f;
    if (k.smpl_scale) {
#pragma unroll
        for (int i = 0; i < 3; i++) { o.p[i] = o.p[i] * o.sc; o.s3[i] = o.s3[i] * o.sc; }
    }
    if (k.transl) {
#pragma unroll
        for (int i = 0; i < 3; i++) o.p[i] = o.p[i] + k.transl[i];
    }
    if (k.rot_canon) {
        if (k.rot6d) {       // sings_hybrid.py:356-357 fused in: the [N,3,3] matrices never exist in HBM
            float d6[6];
#pragma unroll
            for (int i = 0; i < 6; i++) d6[i] = k.rot_canon[6 * (size_t)idx + i];
            sg_r6d2m(d6, o.Rc);
        } else {
#pragma unroll
            for (int i = 0; i < 9; i++) o.Rc[i] = k.rot_canon[9 * (size_t)idx + i];
        }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                o.Rdef[3 * i + j] = T[4 * i] * o.Rc[j] + T[4 * i + 1] * o.Rc[3 + j] + T[4 * i + 2] * o.Rc[6 + j];
    } else {                    // isotropic: R_canon = I (sings_hybrid.py:358-361)
#pragma unroll
        for (int i = 0; i < 9; i++) o.Rc[i] = (i % 4 == 0) ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) o.Rdef[3 * i + j] = T[4 * i + j];
    }
    sg_m2q(o.Rdef, o.q, o.best, o.qab);
    if (k.ext_rot) {            // sings_hybrid.py:421-428 (animation only; forward)
        float e = k.ext_scale[0], pr[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
            pr[i] = k.ext_rot[3 * i] * o.p[0] + k.ext_rot[3 * i + 1] * o.p[1] + k.ext_rot[3 * i + 2] * o.p[2];
#pragma unroll
        for (int i = 0; i < 3; i++) { o.p[i] = k.ext_trans[i] + e * pr[i]; o.s3[i] = e * o.s3[i]; }
        float er[9], qe[4], qo[4]; int bb; float qq;
#pragma unroll
        for (int i = 0; i < 9; i++) er[i] = k.ext_rot[i];
        sg_m2q(er, qe, bb, qq);
        sg_qmul_std(qe, o.q, qo);
        o.q[0] = qo[0]; o.q[1] = qo[1]; o.q[2] = qo[2]; o.q[3] = qo[3];
    }
}

__device__ __forceinline__ void sg_load_A(const SgSkin &k, float *__restrict__ sA)
{
    const int Jp = ((k.J + 15) >> 4) << 4;
    for (int i = threadIdx.x; i < Jp * 16; i += blockDim.x) sA[i] = i < k.J * 16 ? k.A[i] : 0.0f;
}

// frame f of a launch of bt.K frames: joint transforms A + 16 J f, translation + transl_stride f, and with the SG_PLACEMENT_* bits
// (forward only) ext_tfs + (3, 9, 1) f and smpl_scale + f (sg_frame for the rest)
__device__ __forceinline__ SgSkin sg_skin_frame(SgSkin k, int frame, const SgBatch &bt)
{
    k.A += (size_t)frame * k.J * 16;
    if (k.transl) k.transl += (size_t)frame * bt.transl_stride;
    if ((bt.placement & SG_PLACEMENT_EXT_TFS) && k.ext_rot) {
        k.ext_trans += 3 * frame; k.ext_rot += 9 * frame; k.ext_scale += frame;
    }
    if ((bt.placement & SG_PLACEMENT_SMPL_SCALE) && k.smpl_scale) k.smpl_scale += frame;
    return k;
}

// What a workgroup of the two forward kernels below does once it knows its frame and its avatar: block `lblock` (256 Gaussians) of
// an avatar of P Gaussians, skinned with the frame's k, projected, and stored as the Gaussian ids start + local of frame `frame`.
template <int D>
__device__ __forceinline__ void sg_skin_fwd_block(SgCam c, const SgBatch &bt, int frame, const SgSkin &k, int P, int lblock, int start,
                                                  const float *__restrict__ shs, const float *__restrict__ opacities,
                                                  const float *__restrict__ scales, SgGeom g, SgBin bn, uint32_t cap,
                                                  int32_t *__restrict__ radii, float *__restrict__ posed_xyz,
                                                  float *__restrict__ posed_rotq, float *__restrict__ posed_scales, int hist_tiles)
{
    __shared__ float sA[SG_JMAX * 16];
    __shared__ float sW[SG_SKIN_WAVES][64 * SG_WSTRIDE];
    __shared__ float sT[SG_SKIN_WAVES][64 * 13];
    static_assert(SG_SKIN_WAVES * 64 * SG_WSTRIDE >= SG_HIST_TILES_MAX, "the weight tiles double as the per-tile histogram");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    c = sg_frame(c, frame, bt.cam_stride);
    g = sg_frame(g, (size_t)frame * bt.geom); bn = sg_frame(bn, (size_t)frame * bt.bin);
    radii += (size_t)frame * bt.P;
    if (posed_xyz) posed_xyz += 3 * (size_t)frame * bt.P;
    if (posed_rotq) posed_rotq += 4 * (size_t)frame * bt.P;
    if (posed_scales) posed_scales += 3 * (size_t)frame * bt.P;
    const int g0 = (lblock * SG_SKIN_WAVES + wave) * 64;                     // of the avatar's own Gaussians
    const int local = g0 + lane, idx = start + local;                        // ... and the launch's id
    sg_load_A(k, sA);
    __syncthreads();
    float T[12];
    sg_skin_T(k.lbs_w, k.J, P, g0, lane, sA, sW[wave], sT[wave], T);
    const bool live = local < P;
    SgProj o;
    o.mr = 0; o.tt = 0; o.clampbits = 0; o.x0 = o.y0 = o.x1 = o.y1 = 0;
    o.pix[0] = o.pix[1] = 0; o.conic[0] = o.conic[1] = o.conic[2] = 0; o.rgb[0] = o.rgb[1] = o.rgb[2] = 0; o.depth = 0;
    float opac = 0.0f;
    if (live) {
        SgPosed ps;
        sg_pose_gaussian(k, local, T, scales, ps);
        sg_project_fwd<D>(c, ps.p, ps.s3, ps.q, nullptr, nullptr, shs + (size_t)local * c.M * 3, o);
        opac = opacities[local];
        if (posed_xyz) { posed_xyz[3 * (size_t)idx] = ps.p[0]; posed_xyz[3 * (size_t)idx + 1] = ps.p[1]; posed_xyz[3 * (size_t)idx + 2] = ps.p[2]; }
        if (posed_rotq) { posed_rotq[4 * (size_t)idx] = ps.q[0]; posed_rotq[4 * (size_t)idx + 1] = ps.q[1]; posed_rotq[4 * (size_t)idx + 2] = ps.q[2]; posed_rotq[4 * (size_t)idx + 3] = ps.q[3]; }
        if (posed_scales) { posed_scales[3 * (size_t)idx] = ps.s3[0]; posed_scales[3 * (size_t)idx + 1] = ps.s3[1]; posed_scales[3 * (size_t)idx + 2] = ps.s3[2]; }
    }
    uint32_t *hist = nullptr;
    if (hist_tiles) {                                         // the skinning-weight tiles are dead: reuse them as histogram
        __syncthreads();
        hist = (uint32_t *)&sW[0][0];
    }
    sg_store_proj(live, idx, o, opac, g, bn, c.gx, cap, radii, (uint32_t *)sT[wave], hist, hist_tiles, sg_key_pitch_of(hist_tiles != 0, c.flags));
}

template <int D>
__global__ void __launch_bounds__(SG_SKIN_THREADS)
sg_skin_fwd_kernel(SgCam c, SgBatch bt, int P, SgSkin k, const float *__restrict__ shs, const float *__restrict__ opacities,
                   const float *__restrict__ scales, SgGeom g, SgBin bn, uint32_t cap,
                   int32_t *__restrict__ radii, float *__restrict__ posed_xyz, float *__restrict__ posed_rotq,
                   float *__restrict__ posed_scales, int hist_tiles, int nblocks)
{
    // (Gaussian block, frame): the K poses of one block of 256 Gaussians run back to back on one XCD -- its skinning weights
    // (4 J bytes per Gaussian: the largest input), means, scales and SH rows come from HBM once and from that L2 K - 1 times
    int gblock, frame;
    if (!sg_block_frame((int)blockIdx.x, bt.K, nblocks, gblock, frame)) return;
    sg_skin_fwd_block<D>(c, bt, frame, sg_skin_frame(k, frame, bt), P, gblock, 0, shs, opacities, scales, g, bn, cap, radii, posed_xyz,
                         posed_rotq, posed_scales, hist_tiles);
}

// ---- several avatars in one launch (include/sings_scene.h) -----------------------------------------------------------------------
// The reference poses every avatar, concatenates the posed sets -- SH block included: 192 B per Gaussian at M = 16 -- and rasterizes
// once (gs_renderer_multiple.py:12-68).  Here a workgroup of the kernel above first looks up which avatar its block of 256 Gaussians
// belongs to: the avatars (at most SG_SCENE_MAX_AVATARS) ride in the kernel arguments with the first block of each, so the segment
// is found with S - 1 workgroup-uniform compares.  It then skins with that avatar's J, A of the frame, weights and placement -- the
// very body of sg_skin_fwd_kernel (sg_skin_fwd_block): the same bits -- and writes the records of the scene's Gaussian ids
// start_s + local.  A segment's blocks start at its own Gaussian 0, so a wave's 64 ids are consecutive (sg_store_proj: g0 = idx -
// lane) and only a segment's last block has dead lanes; they reach every barrier of sg_store_proj as the dead lanes of the
// single-avatar kernel's last block do.  Every per-frame array has K rows: no placement bits.
struct SgSceneSeg {
    SgSkin k;                                                  // (A, transl, smpl_scale, ext_*: frame 0's)
    const float *shs, *opacities, *scales;
    int P, start, block0, pad;                                 // Gaussians, first Gaussian id, first block of 256
};
struct SgScene { int S; SgSceneSeg seg[SG_SCENE_MAX_AVATARS]; };

template <int D>
__global__ void __launch_bounds__(SG_SKIN_THREADS)
sg_scene_fwd_kernel(SgCam c, SgBatch bt, SgScene sc, SgGeom g, SgBin bn, uint32_t cap, int32_t *__restrict__ radii,
                    float *__restrict__ posed_xyz, float *__restrict__ posed_rotq, float *__restrict__ posed_scales,
                    int hist_tiles, int nblocks)
{
    int gblock, frame;
    if (!sg_block_frame((int)blockIdx.x, bt.K, nblocks, gblock, frame)) return;
    int s = 0;                                                 // (workgroup-uniform; block0 ascends)
#pragma unroll
    for (int t = 1; t < SG_SCENE_MAX_AVATARS; t++)
        if (t < sc.S && gblock >= sc.seg[t].block0) s = t;
    const SgSceneSeg &sg = sc.seg[s];
    SgSkin k = sg.k;
    k.A += (size_t)frame * k.J * 16;
    if (k.transl) k.transl += 3 * (size_t)frame;
    if (k.smpl_scale) k.smpl_scale += frame;
    if (k.ext_rot) { k.ext_trans += 3 * (size_t)frame; k.ext_rot += 9 * (size_t)frame; k.ext_scale += frame; }
    sg_skin_fwd_block<D>(c, bt, frame, k, sg.P, gblock - sg.block0, sg.start, sg.shs, sg.opacities, sg.scales, g, bn, cap, radii,
                         posed_xyz, posed_rotq, posed_scales, hist_tiles);
}

// Backward: LBS^T.  Per Gaussian: dL/dxyz_canon, dL/dR_canon, dL/dscales, dL/dopacity, dL/dsh;
// per workgroup: partial dL/dA [Jp x 16] (matrix cores) and dL/dtransl [3] written to a slab
// (reduced by sg_skin_reduce_kernel -- no atomics, deterministic).
//
// ---- what the single-frame and the K-frame kernel (sg_skin_bwd.inc, sg_skin_bwd_frames.inc) share ---------------------------------
// The two stores below, and nothing else: the per-Gaussian chain rule (SgGaussGrad -> dT, dxc, dRc, dsc, dtr) is spelled out in
// both files on purpose.  As a shared inlined function -- with or without the sg_project_bwd call in it -- it cost registers: 8 to
// 44 more in the single-frame kernels at D >= 2, 20 bytes more scratch in the frames kernels at D = 1 (LAB.md).
//
// dL/dsh of the wave's 64 Gaussians (g0 + lane = idx) from the lanes' dsh [(D+1)^2 x 3]: coefficient-major planes [M][P][3], only the
// (D+1)^2 in use (`planar`, SG_FLAG_SH_PLANAR: 12-byte stores, coalesced across the lanes); or the reference's rows -- `rows_lds`
// (M == 16): all 16 rows through `stage` (32 x SG_ROW_LDS floats of the wave's LDS) as 16-B-per-lane coalesced stores; otherwise
// lane by lane.  ADD: added to what the buffer holds; ZERO_TAIL: the lane-by-lane path also zeroes the rows not in use.
template <int D, bool ADD, bool ZERO_TAIL>
__device__ __forceinline__ void sg_skin_store_dsh(const float *dsh, bool planar, bool rows_lds, int Mrows, int P, int idx, int g0, int lane,
                                                  bool live, float *__restrict__ dL_dsh, float *__restrict__ stage)
{
    constexpr int nc = (D + 1) * (D + 1);
    if (planar) {
        if (live) {
#pragma unroll
            for (int kq = 0; kq < nc; kq++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    float *d = dL_dsh + ((size_t)kq * P + idx) * 3 + ch;
                    *d = ADD ? dsh[3 * kq + ch] + *d : dsh[3 * kq + ch];
                }
        }
    } else if (rows_lds) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if ((lane >> 5) == h) {
                float *row = stage + (lane & 31) * SG_ROW_LDS;
#pragma unroll
                for (int i = 0; i < 48; i++) row[i] = i < nc * 3 ? dsh[i < nc * 3 ? i : 0] : 0.0f;
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            sg_rows48_store(dL_dsh, g0 + 32 * h, P, lane, stage, 32, ADD);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
        }
    } else if (live) {
        float *dsh_row = dL_dsh + (size_t)idx * Mrows * 3;
#pragma unroll
        for (int i = 0; i < nc * 3; i++) dsh_row[i] = ADD ? dsh_row[i] + dsh[i] : dsh[i];
        if (ZERO_TAIL)
            for (int i = nc * 3; i < Mrows * 3; i++) dsh_row[i] = 0.0f;
    }
}

// dL/dtransl of the wave's 64 Gaussians: wave sum into the three floats behind the dA partials of its slab row `out`
__device__ __forceinline__ void sg_skin_store_dtransl(const float dtr[3], int lane, float *__restrict__ out)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float v = dtr[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) out[SG_JMAX * 16 + i] = v;
    }
}

#define SG_SKBWD_PARAMS SgCam c, int P, SgSkin k, const float *__restrict__ shs, const float *__restrict__ scales,                      \
                   const int32_t *__restrict__ radii, SgGeom g, SgRec grec, size_t cap,                                              \
                   const uint32_t *__restrict__ header, const uint8_t *__restrict__ rec_valid, const float *__restrict__ dposed_xyz_in, const float *__restrict__ dposed_rotq_in, \
                   float *__restrict__ dL_dxyz_canon, float *__restrict__ dL_drot_canon,                                             \
                   float *__restrict__ dL_dscales, float *__restrict__ dL_dopacity, float *__restrict__ dL_dsh,                      \
                   float *__restrict__ dL_dmeans2D, float *__restrict__ slab, int slab_stride
// The single-frame kernel and (SG_SKBWD_AUX 1) its variant for the depth / alpha maps (sg_skinned_backward_aux).  One source,
// included twice: as an inlined body the plain kernel compiled to different code.
#define SG_SKBWD_AUX 0
#include "sg_skin_bwd.inc"
#undef SG_SKBWD_AUX
#define SG_SKBWD_AUX 1
#include "sg_skin_bwd.inc"
#undef SG_SKBWD_AUX

// ---- K frames per launch (round 4) -----------------------------------------------------------------------------------------
// bt.K frames of the SAME canonical Gaussians: the wave walks the frames -- blend T with frame f's joint transforms, sum frame f's
// gradient records, chain rule, dA partials of frame f into frame f's slab row -- and sums the canonical-Gaussian gradients of the
// K frames in registers, in frame order: frame 0 assigns (ACC: adds to what the gradient buffer holds, read ONCE in front of the
// loop), frame f > 0 adds -- bit for bit what K single-frame calls leave behind when they share one gradient buffer (first call
// accumulate = 0 resp. 1, the others 1).  The gradient row -- 55 floats per Gaussian on the avatar, 48 of them the SH block -- is
// written ONCE per K frames instead of being read and rewritten by every frame.  dL_dmeans2D, dL_dA, dL_dtransl are per frame.
//
// What a frame costs here is dependent memory round trips, not arithmetic (6.3e6 VALU instructions per frame = 9 us of issue; the
// single-frame kernel takes 43 us, the first version of this loop 38 us per frame: A_f -> LDS, 4 weight chunks for T, slot / flags,
// 3 record chunks, the canonical inputs, 4 weight chunks again for W^T dT).  So, per wave:
//  * the skinning-weight tile (64 x J floats, the largest input: 4 J bytes per Gaussian) is read from HBM ONCE and stays in LDS
//    for all K frames and both contractions (row pitch J + 1: conflict-free for the [gaussian][joint] reads of W.A and the
//    [joint][gaussian] reads of W^T.dT alike);
//  * the canonical inputs (mean, scales, SH rows in use, 6-D rotation) are read once, in front of the loop;
//  * frame f + 1's joint transforms and (visible, record slot, clamp flags) are requested while frame f is worked on.
// LDS: 4 waves x (64 (J + 1) + 64 x 17) floats + 4 KB of joint transforms = 76 KB at J = 52: two workgroups per CU, as many
// waves per SIMD as the kernel's ~250 registers allow anyway.
// T rows 0..2 of this lane's Gaussian from the wave's RESIDENT weight tile sW [64][WP] (WP = J + 1) and the frame's sA.
// The same k-ordered fp32 MFMA chain as sg_skin_T (joints in ascending order, zero weights for the padding joints of the last
// chunk): the same T, bit for bit.
__device__ __forceinline__ void sg_skin_T_resident(const float *__restrict__ sW, int WP, int J, int lane, const float *__restrict__ sA,
                                                   float *__restrict__ sT, float T[12])
{
    f32x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; b++) acc[b] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
    // k-steps of 4 joints; a step whose joints are all padding (J % 16 != 0: the tail of the last chunk) is skipped -- its weights are
    // zero and A is finite, so acc + 0 x b = acc exactly: the same T as sg_skin_T, bit for bit; the operands of a step are
    // requested together, in front of its four MFMAs (one LDS latency per step, not one per MFMA)
    const int nsteps = (J + 3) >> 2;
    for (int st = 0; st < nsteps; st++) {
        const int col = 4 * st + (lane >> 4);
        const float bv = sA[col * 16 + (lane & 15)];
        float av[4];
#pragma unroll
        for (int b = 0; b < 4; b++) av[b] = sW[(16 * b + (lane & 15)) * WP + (col < J ? col : 0)];
#pragma unroll
        for (int b = 0; b < 4; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(col < J ? av[b] : 0.0f, bv, acc[b], 0, 0, 0);
    }
    if ((lane & 15) < 12) {
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) sT[(16 * b + 4 * (lane >> 4) + r) * 13 + (lane & 15)] = acc[b][r];
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = sT[lane * 13 + i];
    __builtin_amdgcn_wave_barrier();
}

// Record sums of ALL frames as a kernel of their own (grid: Gaussian blocks x K): a9 [K][P][12] (9 sums + padding: three 16-byte
// vectors per Gaussian).  Inside the frame loop below the sums were the largest item -- five dependent round trips (load -> LDS ->
// sum) per wave and frame, 98 of the loop kernel's 320 us at K = 8 (timing-only ablation builds, tools/ablate.py) -- because that
// kernel runs two waves per SIMD and nothing hides a round trip; here the same coalesced chunk loop runs at full occupancy (40
// registers) next to thousands of other waves, and the loop kernel reads 48 contiguous bytes per Gaussian and frame instead.  The
// order of the additions per Gaussian is sg_sum_records_coop's: the same sums, bit for bit.
// AUX, the depth / alpha maps: frame f's dL/dz sum (its dz plane at dz0 + f dz_stride bytes: sg_aux_bytes) goes to the spare float
// of the block, summed by sg_sum_dz -- in the order of the single-frame AUX kernels, so K = 1 is their value bit for bit.  (A kernel
// of its own below: the plain one keeps its instructions.)
template <bool AUX>
__device__ __forceinline__ void sg_record_sums_block(const SgBatch &bt, int P, const int32_t *__restrict__ radii0, SgGeom g0_, SgRec grec0,
                                                     size_t cap, const uint32_t *__restrict__ header0,
                                                     const uint8_t *__restrict__ rec_valid, float4 *__restrict__ a9out,
                                                     const float *__restrict__ dz0, size_t dz_stride)
{
    __shared__ float lds_all[4][SG_REC_CHUNK * 12];
    const int f = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (idx - lane >= P) return;
    const bool live = idx < P;
    const SgGeom g = sg_frame(g0_, (size_t)f * bt.geom);
    const SgRec grec = sg_frame(grec0, (size_t)f * bt.rec);
    const bool vis = live && radii0[(size_t)f * bt.P + idx] > 0 && sg_at(header0, (size_t)f * bt.bin)[1] == 0u;
    float4 rc = make_float4(0, 0, 0, 0);
    if (vis) { const uint2 sl = g.slot[idx]; rc.y = __uint_as_float(sl.x); rc.w = __uint_as_float(sl.y); }
    float a9[9];
    sg_sum_records_coop(grec, cap, vis, rc, lane, lds_all[wave], a9, sg_at(rec_valid, (size_t)f * bt.bin));
    const float dz = AUX ? sg_sum_dz(sg_at(dz0, (size_t)f * dz_stride), cap, vis, rc, sg_at(rec_valid, (size_t)f * bt.bin)) : 0.0f;
    if (live) {
        float4 *o = a9out + 3 * ((size_t)f * bt.P + idx);
        o[0] = make_float4(a9[0], a9[1], a9[2], a9[3]); o[1] = make_float4(a9[4], a9[5], a9[6], a9[7]);
        o[2] = make_float4(a9[8], dz, 0.0f, 0.0f);
    }
}
__global__ void __launch_bounds__(256)
sg_record_sums_kernel(SgBatch bt, int P, const int32_t *__restrict__ radii0, SgGeom g0_, SgRec grec0, size_t cap,
                      const uint32_t *__restrict__ header0, const uint8_t *__restrict__ rec_valid, float4 *__restrict__ a9out)
{
    sg_record_sums_block<false>(bt, P, radii0, g0_, grec0, cap, header0, rec_valid, a9out, nullptr, 0);
}
__global__ void __launch_bounds__(256)
sg_record_sums_aux_kernel(SgBatch bt, int P, const int32_t *__restrict__ radii0, SgGeom g0_, SgRec grec0, size_t cap,
                          const uint32_t *__restrict__ header0, const uint8_t *__restrict__ rec_valid, float4 *__restrict__ a9out,
                          const float *__restrict__ dz0, size_t dz_stride)
{
    sg_record_sums_block<true>(bt, P, radii0, g0_, grec0, cap, header0, rec_valid, a9out, dz0, dz_stride);
}

void sg_launch_record_sums(const SgBatch &bt, int P, const int32_t *radii, SgGeom g, SgRec grec, size_t cap, const uint32_t *header,
                           const uint8_t *rec_valid, float4 *a9out, hipStream_t st, const float *dz, size_t dz_stride)
{
    if (P <= 0) return;
    if (dz)
        hipLaunchKernelGGL(sg_record_sums_aux_kernel, dim3((P + 255) / 256, bt.K), dim3(256), 0, st, bt, P, radii, g, grec, cap, header,
                           rec_valid, a9out, dz, dz_stride);
    else
        hipLaunchKernelGGL(sg_record_sums_kernel, dim3((P + 255) / 256, bt.K), dim3(256), 0, st, bt, P, radii, g, grec, cap, header,
                           rec_valid, a9out);
}

#define SG_SKFBWD_AUX 0
#include "sg_skin_bwd_frames.inc"
#undef SG_SKFBWD_AUX
#define SG_SKFBWD_AUX 1
#include "sg_skin_bwd_frames.inc"
#undef SG_SKFBWD_AUX

// sums the per-wave slab rows in a fixed order: dL_dA [J,16] and dL_dtransl [3].  Two passes so that the
// ~10 MB of slabs are read by thousands of waves with 256-B coalesced rows (a single 53-block pass took 44 us):
//  pass 1: grid (column blocks of 64, SG_RED_GROUPS/4); wave = row group rg sums rows rg, rg + G, ... into part[rg]
//  pass 2: one thread per column sums the G partial rows.
#define SG_RED_GROUPS 64        // (32 / 64 / 128 groups: pass 1 + pass 2 = 8.5 + 4.7 / 5.6 + 4.9 / 4.9 + 6.8 us on the avatar frame)
__global__ void __launch_bounds__(256)
sg_skin_reduce1_kernel(const float *__restrict__ slab, int nrows, int slab_stride, float *__restrict__ part, size_t slab_frame)
{
    slab += (size_t)blockIdx.z * slab_frame;                   // frame blockIdx.z: its slab rows -> its SG_RED_GROUPS partial rows
    part += (size_t)blockIdx.z * SG_RED_GROUPS * slab_stride;
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rg = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (col >= slab_stride) return;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int b = rg;
    for (; b + 3 * SG_RED_GROUPS < nrows; b += 4 * SG_RED_GROUPS) {
        s0 += slab[(size_t)b * slab_stride + col];
        s1 += slab[(size_t)(b + SG_RED_GROUPS) * slab_stride + col];
        s2 += slab[(size_t)(b + 2 * SG_RED_GROUPS) * slab_stride + col];
        s3 += slab[(size_t)(b + 3 * SG_RED_GROUPS) * slab_stride + col];
    }
    for (; b < nrows; b += SG_RED_GROUPS) s0 += slab[(size_t)b * slab_stride + col];
    part[(size_t)rg * slab_stride + col] = (s0 + s1) + (s2 + s3);
}

__global__ void __launch_bounds__(64)
sg_skin_reduce2_kernel(const float *__restrict__ part, int slab_stride, int J, float *__restrict__ dL_dA,
                       float *__restrict__ dL_dtransl)
{
    part += (size_t)blockIdx.z * SG_RED_GROUPS * slab_stride;  // frame blockIdx.z -> dL_dA [K,J,16], dL_dtransl [K,3]
    dL_dA += (size_t)blockIdx.z * J * 16;
    if (dL_dtransl) dL_dtransl += 3 * (size_t)blockIdx.z;
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int nA = J * 16;
    if (i >= nA + 3) return;
    const int col = i < nA ? i : SG_JMAX * 16 + (i - nA);
    float t = 0.0f;
#pragma unroll 8
    for (int r = 0; r < SG_RED_GROUPS; r++) t += part[(size_t)r * slab_stride + col];
    if (i < nA) dL_dA[i] = t;
    else if (dL_dtransl) dL_dtransl[i - nA] = t;
}

// ---- launchers ---------------------------------------------------------------------------
void sg_launch_skin_fwd(const SgCam &c, const SgBatch &bt, int P, const SgSkinInputs *in, const float *shs, const float *opacities,
                        const float *scales, SgGeom g, SgBin b, size_t cap, int32_t *radii, float *posed_xyz,
                        float *posed_rotq, float *posed_scales, hipStream_t st)
{
    if (P <= 0) return;
    const SgSkin k = sg_skin_of(*in);
    const int nblocks = (P + SG_SKIN_THREADS - 1) / SG_SKIN_THREADS;
    dim3 grid(sg_frame_grid(nblocks, bt.K)), block(SG_SKIN_THREADS);
    const int ht = sg_lds_hist(c.gx, c.gy) ? (int)sg_ctr_count((uint32_t)c.gx, (uint32_t)c.gy) : 0;     // histogram words (= tile counters)
#define SG_SF(DD) hipLaunchKernelGGL(sg_skin_fwd_kernel<DD>, grid, block, 0, st, c, bt, P, k, shs, opacities, scales, g, \
                                     b, sg_cap32(cap), radii, posed_xyz, posed_rotq, posed_scales, ht, nblocks)
    sg_prof_begin(SG_K_PREPROCESS_FWD, st);
    switch (c.D) { case 0: SG_SF(0); break; case 1: SG_SF(1); break; case 2: SG_SF(2); break; default: SG_SF(3); break; }
    sg_prof_end(SG_K_PREPROCESS_FWD, st);
#undef SG_SF
}

void sg_launch_scene_fwd(const SgCam &c, const SgBatch &bt, int S, const SgSceneAvatar *avatars, SgGeom g, SgBin b, size_t cap,
                         int32_t *radii, float *posed_xyz, float *posed_rotq, float *posed_scales, hipStream_t st)
{
    SgScene sc = {};
    sc.S = S;
    int nblocks = 0, start = 0;
    for (int s = 0; s < S; s++) {
        const SgSceneAvatar &a = avatars[s];
        SgSceneSeg &q = sc.seg[s];
        q.k = sg_skin_of(a);
        q.shs = a.shs; q.opacities = a.opacities; q.scales = a.scales;
        q.P = a.P; q.start = start; q.block0 = nblocks; q.pad = 0;
        start += a.P;
        nblocks += (a.P + SG_SKIN_THREADS - 1) / SG_SKIN_THREADS;
    }
    if (nblocks <= 0) return;
    dim3 grid(sg_frame_grid(nblocks, bt.K)), block(SG_SKIN_THREADS);
    const int ht = sg_lds_hist(c.gx, c.gy) ? (int)sg_ctr_count((uint32_t)c.gx, (uint32_t)c.gy) : 0;     // histogram words (= tile counters)
#define SG_SCF(DD) hipLaunchKernelGGL(sg_scene_fwd_kernel<DD>, grid, block, 0, st, c, bt, sc, g, b, sg_cap32(cap), radii, posed_xyz, \
                                      posed_rotq, posed_scales, ht, nblocks)
    sg_prof_begin(SG_K_PREPROCESS_FWD, st);
    switch (c.D) { case 0: SG_SCF(0); break; case 1: SG_SCF(1); break; case 2: SG_SCF(2); break; default: SG_SCF(3); break; }
    sg_prof_end(SG_K_PREPROCESS_FWD, st);
#undef SG_SCF
}

// dynamic LDS above 64 KB needs the kernel's limit raised (once per kernel and process; J = 64: 88 KB)
static void sg_skin_frames_lds(const void *fn, size_t bytes)
{
    if (bytes > 64 * 1024) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// per frame: the per-wave slabs, followed (after the slabs of ALL frames) by the SG_RED_GROUPS partial rows of every frame
static size_t sg_skin_slab_rows(int P) { return (size_t)((P + SG_SKIN_THREADS - 1) / SG_SKIN_THREADS) * SG_SKIN_WAVES; }
size_t sg_skin_slab_floats(int P, int K)
{
    const size_t k = (size_t)(K > 0 ? K : 1);
    // (+ the record sums of the K-frame backward: 12 floats per frame and Gaussian, 16-byte aligned behind the partial rows)
    return (sg_skin_slab_rows(P) + SG_RED_GROUPS) * k * (SG_JMAX * 16 + 4) + (k > 1 ? k * 12 * (size_t)P + 4 : 0);
}

// the `nrows` per-wave slab rows of each of K frames (frame f's at slab + f nrows stride) -> dL_dA [K,J,16], dL_dtransl [K,3] (or
// NULL); the SG_RED_GROUPS partial rows of every frame lie behind the slabs of all frames
void sg_launch_skin_reduce(float *slab, int nrows, int stride, int J, int K, float *dL_dA, float *dL_dtransl, hipStream_t st)
{
    const size_t slab_frame = (size_t)nrows * stride;
    float *part = slab + slab_frame * K;
    hipLaunchKernelGGL(sg_skin_reduce1_kernel, dim3((stride + 63) / 64, SG_RED_GROUPS / 4, K), dim3(256), 0, st, slab, nrows, stride,
                       part, slab_frame);
    hipLaunchKernelGGL(sg_skin_reduce2_kernel, dim3((J * 16 + 3 + 63) / 64, 1, K), dim3(64), 0, st, part, stride, J, dL_dA, dL_dtransl);
}

// what sg_launch_skin_bwd hands to the kernel that (D, accumulate, depth / alpha maps) and K select
struct SgSkinBwdCall {
    SgCam c; SgBatch bt; int P; SgSkin k;
    const float *shs, *scales; const int32_t *radii; SgGeom g; SgRec grec; size_t cap;
    const uint32_t *header; const uint8_t *rec_valid; const float *dposed_xyz_in, *dposed_rotq_in;
    float *dL_dxyz_canon, *dL_drot_canon, *dL_dscales, *dL_dopacity, *dL_dsh, *dL_dmeans2D, *slab;
    int stride; size_t slab_frame; const float4 *a9buf; const float *dz; hipStream_t st;
};
template <int D, bool ACC, bool AUX>
static void sg_skin_bwd_launch(const SgSkinBwdCall &a)
{
    const dim3 grid((a.P + SG_SKIN_THREADS - 1) / SG_SKIN_THREADS), block(SG_SKIN_THREADS);
    // the frames kernel: sA + 4 waves x (resident weight tile 64 x (J + 1) + scratch 64 x 17) floats of dynamic LDS
    const size_t dyn = ((size_t)SG_JMAX * 16 + (size_t)SG_SKIN_WAVES * (64 * (a.k.J + 1) + 64 * SG_WSTRIDE)) * sizeof(float);
    auto one = [&](auto kernel, auto... dz) {
        hipLaunchKernelGGL(kernel, grid, block, 0, a.st, a.c, a.P, a.k, a.shs, a.scales, a.radii, a.g, a.grec, a.cap, a.header, a.rec_valid,
                           a.dposed_xyz_in, a.dposed_rotq_in, a.dL_dxyz_canon, a.dL_drot_canon, a.dL_dscales, a.dL_dopacity, a.dL_dsh,
                           a.dL_dmeans2D, a.slab, a.stride, dz...);
    };
    auto frames = [&](auto kernel) {
        sg_skin_frames_lds((const void *)kernel, dyn);
        hipLaunchKernelGGL(kernel, grid, block, dyn, a.st, a.c, a.bt, a.P, a.k, a.shs, a.scales, a.radii, a.g, a.grec, a.cap, a.header,
                           a.dposed_xyz_in, a.dposed_rotq_in, a.dL_dxyz_canon, a.dL_drot_canon, a.dL_dscales, a.dL_dopacity, a.dL_dsh,
                           a.dL_dmeans2D, a.slab, a.stride, a.slab_frame, a.a9buf);
    };
    if constexpr (AUX) {
        if (a.bt.K == 1) one(sg_skin_bwd_aux_kernel<D>, a.dz); else frames(sg_skin_bwd_frames_aux_kernel<D>);
    } else {
        if (a.bt.K == 1) one(sg_skin_bwd_kernel<D, ACC>); else frames(sg_skin_bwd_frames_kernel<D, ACC>);
    }
}
template <int D>
static void sg_skin_bwd_launch(const SgSkinBwdCall &a, int accumulate)
{
    if (a.dz) sg_skin_bwd_launch<D, false, true>(a);             // (the aux entry points: accumulate = 0)
    else if (accumulate) sg_skin_bwd_launch<D, true, false>(a);
    else sg_skin_bwd_launch<D, false, false>(a);
}

void sg_launch_skin_bwd(const SgCam &c, const SgBatch &bt, int P, const SgSkinInputs *in, const float *shs, const float *scales,
                        const int32_t *radii, SgGeom g, SgRec grec, size_t cap, const uint32_t *header, const uint8_t *rec_valid,
                        const float *dposed_xyz_in, const float *dposed_rotq_in, float *slab, float *dL_dxyz_canon, float *dL_drot_canon,
                        float *dL_dscales, float *dL_dopacity, float *dL_dsh, float *dL_dmeans2D, float *dL_dA,
                        float *dL_dtransl, int accumulate, hipStream_t st, const float *dz, size_t dz_stride)
{
    if (P <= 0) return;
    SgSkin k = sg_skin_of(*in);
    k.ext_trans = k.ext_rot = k.ext_scale = nullptr;             // (animation only; forward)
    const int stride = SG_JMAX * 16 + 4;
    const size_t slab_frame = sg_skin_slab_rows(P) * stride;
    // K > 1: the record sums of all frames first, as a kernel of their own (a9 [K][P][12] behind the slabs and partial rows)
    const float4 *a9buf = (const float4 *)(slab + (slab_frame + (size_t)SG_RED_GROUPS * stride) * bt.K);
    const SgSkinBwdCall a = { c, bt, P, k, shs, scales, radii, g, grec, cap, header, rec_valid, dposed_xyz_in, dposed_rotq_in,
                              dL_dxyz_canon, dL_drot_canon, dL_dscales, dL_dopacity, dL_dsh, dL_dmeans2D, slab, stride, slab_frame,
                              a9buf, dz, st };
    sg_prof_begin(SG_K_PREPROCESS_BWD, st);
    // (depth / alpha maps, dz != null: frame f's dL/dz plane at dz + f dz_stride bytes; its sums ride in the a9 block)
    if (bt.K > 1)
        sg_launch_record_sums(bt, P, radii, g, grec, cap, header, rec_valid, (float4 *)a9buf, st, dz, dz_stride);
    switch (c.D) {
    case 0: sg_skin_bwd_launch<0>(a, accumulate); break;
    case 1: sg_skin_bwd_launch<1>(a, accumulate); break;
    case 2: sg_skin_bwd_launch<2>(a, accumulate); break;
    default: sg_skin_bwd_launch<3>(a, accumulate); break;
    }
    sg_launch_skin_reduce(slab, (int)sg_skin_slab_rows(P), stride, in->J, bt.K, dL_dA, dL_dtransl, st);
    sg_prof_end(SG_K_PREPROCESS_BWD, st);
}

