// The SMPL(-H) kinematic chain and the learned per-frame pose tables: pose -> joint transforms A [B,J,16], value and gradient
// (sg_joint_transforms[_backward], sg_pose_transforms[_backward]).  One wave per frame; the rotation math is sg_rot.h's.
#include "sg_rot.h"

// ---- SMPL(-H) kinematic chain (sings/rec/utils/body_model/smpl.py:415-513) ------------------------------------
// pose [B,J,3] axis-angle + rest joints [J,3] + parents -> A [B,J,16] = G - pad(G [J;0]) (x post[j] if given: the
// per-joint inv(A_t2cano) of sings_hybrid.py:398-399).  torch runs this as ~100 tiny launches per call (Rodrigues, J - 1
// dependent 4x4 products, the correction) and three times that for autograd: launch latency, ~1 ms per frame.  Here:
// one wave per frame, lane = joint; the chain is walked in joint order (parents[i] < i) through LDS.
struct SgRod { float R[9], th, d[3], s, c; };
__device__ __forceinline__ void sg_rodrigues(const float v[3], SgRod &o)
{
    // batch_rodrigues (smpl.py:415-446): angle = |v + 1e-8|, axis = v / angle
    const float a0 = v[0] + 1e-8f, a1 = v[1] + 1e-8f, a2 = v[2] + 1e-8f;
    o.th = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
    o.d[0] = v[0] / o.th; o.d[1] = v[1] / o.th; o.d[2] = v[2] / o.th;
    o.s = sinf(o.th); o.c = cosf(o.th);
    const float K[9] = { 0, -o.d[2], o.d[1], o.d[2], 0, -o.d[0], -o.d[1], o.d[0], 0 };
    const float oc = 1.0f - o.c;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int cc = 0; cc < 3; cc++) {
            const float kk = K[3 * r] * K[cc] + K[3 * r + 1] * K[3 + cc] + K[3 * r + 2] * K[6 + cc];
            o.R[3 * r + cc] = (r == cc ? 1.0f : 0.0f) + o.s * K[3 * r + cc] + oc * kk;
        }
}
// dL/dR [9] -> dL/dv [3]
__device__ __forceinline__ void sg_rodrigues_bwd(const float v[3], const SgRod &o, const float M[9], float dv[3])
{
    const float K[9] = { 0, -o.d[2], o.d[1], o.d[2], 0, -o.d[0], -o.d[1], o.d[0], 0 };
    float K2[9], mk = 0.0f, mk2 = 0.0f;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int cc = 0; cc < 3; cc++) {
            K2[3 * r + cc] = K[3 * r] * K[cc] + K[3 * r + 1] * K[3 + cc] + K[3 * r + 2] * K[6 + cc];
            mk += M[3 * r + cc] * K[3 * r + cc]; mk2 += M[3 * r + cc] * K2[3 * r + cc];
        }
    const float oc = 1.0f - o.c;
    float dK[9];                                                  // s M + (1 - c) (M K^T + K^T M)
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int cc = 0; cc < 3; cc++) {
            float a = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) a += M[3 * r + k] * K[3 * cc + k] + K[3 * k + r] * M[3 * k + cc];
            dK[3 * r + cc] = o.s * M[3 * r + cc] + oc * a;
        }
    const float dd[3] = { dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1] };
    float dth = o.c * mk + o.s * mk2;
    const float ith = 1.0f / o.th;
#pragma unroll
    for (int k = 0; k < 3; k++) dth -= dd[k] * v[k] * ith * ith;
#pragma unroll
    for (int k = 0; k < 3; k++) dv[k] = dd[k] * ith + dth * (v[k] + 1e-8f) * ith;
}
// C[3x4] = A[3x4] o B[3x4] as rigid 4x4 products (bottom rows 0 0 0 1)
__device__ __forceinline__ void sg_mul34(const float *A, const float *B, float *Cm)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int cc = 0; cc < 4; cc++)
            Cm[4 * r + cc] = (A[4 * r] * B[cc] + A[4 * r + 1] * B[4 + cc]) + A[4 * r + 2] * B[8 + cc] + (cc == 3 ? A[4 * r + 3] : 0.0f);
    }
}
// The chain of one frame, one wave: lane j holds joint j's axis-angle v -> its row `o` [16] of A.  sG: the wave's LDS scratch.
__device__ __forceinline__ void sg_chain_fwd(float (*sG)[13], int J, int j, bool on, const float v[3], const float *__restrict__ joints,
                                             const int *__restrict__ parents, const float *__restrict__ post, float *__restrict__ o)
{
    float T[12], G[12];
    const int par = on ? parents[j] : -1;
    float Jj[3] = { 0, 0, 0 };
    if (on) {
        SgRod ro;
        sg_rodrigues(v, ro);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Jj[k] = joints[3 * j + k];
            T[4 * k] = ro.R[3 * k]; T[4 * k + 1] = ro.R[3 * k + 1]; T[4 * k + 2] = ro.R[3 * k + 2];
            T[4 * k + 3] = Jj[k] - (par >= 0 ? joints[3 * par + k] : 0.0f);
        }
    }
    for (int i = 0; i < J; i++) {
        if (j == i) {
            if (par < 0) {
#pragma unroll
                for (int k = 0; k < 12; k++) G[k] = T[k];
            } else {
                float P[12];
#pragma unroll
                for (int k = 0; k < 12; k++) P[k] = sG[par][k];
                sg_mul34(P, T, G);
            }
#pragma unroll
            for (int k = 0; k < 12; k++) sG[j][k] = G[k];
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
    }
    if (!on) return;
    // A = G - pad(G [J;0]): same rotation, translation t - R J
#pragma unroll
    for (int r = 0; r < 3; r++) G[4 * r + 3] -= (G[4 * r] * Jj[0] + G[4 * r + 1] * Jj[1]) + G[4 * r + 2] * Jj[2];
    if (post) {
        const float *Pm = post + (size_t)j * 16;                  // full 4x4: A (bottom row 0 0 0 1) @ post
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int cc = 0; cc < 4; cc++)
                o[4 * r + cc] = ((G[4 * r] * Pm[cc] + G[4 * r + 1] * Pm[4 + cc]) + G[4 * r + 2] * Pm[8 + cc]) + G[4 * r + 3] * Pm[12 + cc];
#pragma unroll
        for (int cc = 0; cc < 4; cc++) o[12 + cc] = Pm[12 + cc];
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) o[k] = G[k];
        o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
    }
}
__global__ void __launch_bounds__(64)
sg_joint_transforms_fwd_kernel(int J, const float *__restrict__ pose, const float *__restrict__ joints, const int *__restrict__ parents,
                               const float *__restrict__ post, float *__restrict__ A_out)
{
    __shared__ float sG[64][13];
    const int b = blockIdx.x, j = threadIdx.x;
    const bool on = j < J;
    float v[3] = { 0, 0, 0 };
    if (on) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = pose[((size_t)b * J + j) * 3 + k];
    }
    sg_chain_fwd(sG, J, j, on, v, joints, parents, post, A_out + ((size_t)b * J + (on ? j : 0)) * 16);
}
// The chain's gradient for one frame: lane j's row g [16] of dA -> dv [3] (its axis-angle) and dJ [3] (its rest joint; lanes j < J)
__device__ __forceinline__ void sg_chain_bwd(float (*sG)[13], float (*sD)[13], float (*sJ)[4], int J, int j, bool on, const float v[3],
                                             const float *__restrict__ joints, const int *__restrict__ parents,
                                             const float *__restrict__ post, const float *__restrict__ g, float dv[3], float dJo[3])
{
    float T[12], G[12], dG[12];
    const int par = on ? parents[j] : -1;
    float Jj[3] = { 0, 0, 0 };
    SgRod ro;
    if (on) {
        sg_rodrigues(v, ro);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Jj[k] = joints[3 * j + k];
            T[4 * k] = ro.R[3 * k]; T[4 * k + 1] = ro.R[3 * k + 1]; T[4 * k + 2] = ro.R[3 * k + 2];
            T[4 * k + 3] = Jj[k] - (par >= 0 ? joints[3 * par + k] : 0.0f);
        }
    }
    for (int i = 0; i < J; i++) {                                 // forward chain again (G into LDS)
        if (j == i) {
            if (par < 0) {
#pragma unroll
                for (int k = 0; k < 12; k++) G[k] = T[k];
            } else {
                float P[12];
#pragma unroll
                for (int k = 0; k < 12; k++) P[k] = sG[par][k];
                sg_mul34(P, T, G);
            }
#pragma unroll
            for (int k = 0; k < 12; k++) sG[j][k] = G[k];
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
    }
    // dA (after post) -> dA of the un-multiplied transform (top three rows) -> dG, direct dJ
    float dJ[3] = { 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < 12; k++) dG[k] = 0.0f;
    if (on) {
        float dAp[12];
        if (post) {
            const float *Pm = post + (size_t)j * 16;              // d(A) = dOut @ post^T, rows 0..2
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 4; k++)
                    dAp[4 * r + k] = ((g[4 * r] * Pm[4 * k] + g[4 * r + 1] * Pm[4 * k + 1]) + g[4 * r + 2] * Pm[4 * k + 2]) + g[4 * r + 3] * Pm[4 * k + 3];
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) dAp[k] = g[k];
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int cc = 0; cc < 3; cc++) {
                dG[4 * r + cc] = dAp[4 * r + cc] - dAp[4 * r + 3] * Jj[cc];
                dJ[cc] -= G[4 * r + cc] * dAp[4 * r + 3];
            }
            dG[4 * r + 3] = dAp[4 * r + 3];
        }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) sD[j][k] = dG[k];
    sJ[j][0] = 0.0f; sJ[j][1] = 0.0f; sJ[j][2] = 0.0f;
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    float dT[12];
#pragma unroll
    for (int k = 0; k < 12; k++) dT[k] = 0.0f;
    for (int i = J - 1; i >= 0; i--) {                            // reverse chain: children have larger indices
        if (j == i) {
#pragma unroll
            for (int k = 0; k < 12; k++) dG[k] = sD[j][k];
            if (par < 0) {
#pragma unroll
                for (int k = 0; k < 12; k++) dT[k] = dG[k];
            } else {
                float P[12];
#pragma unroll
                for (int k = 0; k < 12; k++) P[k] = sG[par][k];
                // G = P o T:  dT.R = P.R^T dG.R, dT.t = P.R^T dG.t;  dP.R += dG.R T.R^T + dG.t T.t^T, dP.t += dG.t
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int cc = 0; cc < 4; cc++)
                        dT[4 * r + cc] = (P[r] * dG[cc] + P[4 + r] * dG[4 + cc]) + P[8 + r] * dG[8 + cc];
#pragma unroll
                for (int r = 0; r < 3; r++) {
#pragma unroll
                    for (int cc = 0; cc < 3; cc++)
                        sD[par][4 * r + cc] += ((dG[4 * r] * T[4 * cc] + dG[4 * r + 1] * T[4 * cc + 1]) + dG[4 * r + 2] * T[4 * cc + 2]) +
                                               dG[4 * r + 3] * T[4 * cc + 3];
                    sD[par][4 * r + 3] += dG[4 * r + 3];
                }
                // T.t = J_j - J_parent
#pragma unroll
                for (int k = 0; k < 3; k++) sJ[par][k] -= dT[4 * k + 3];
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
    }
    if (!on) return;
    const float M[9] = { dT[0], dT[1], dT[2], dT[4], dT[5], dT[6], dT[8], dT[9], dT[10] };
    sg_rodrigues_bwd(v, ro, M, dv);
#pragma unroll
    for (int k = 0; k < 3; k++) dJo[k] = dJ[k] + dT[4 * k + 3] + sJ[j][k];
}
// dA [B,J,16] -> dpose [B,J,3], djoints [B,J,3] (per frame; the caller sums over B)
__global__ void __launch_bounds__(64)
sg_joint_transforms_bwd_kernel(int J, const float *__restrict__ pose, const float *__restrict__ joints, const int *__restrict__ parents,
                               const float *__restrict__ post, const float *__restrict__ dA, float *__restrict__ dpose,
                               float *__restrict__ djoints)
{
    __shared__ float sG[64][13], sD[64][13], sJ[64][4];
    const int b = blockIdx.x, j = threadIdx.x;
    const bool on = j < J;
    float v[3] = { 0, 0, 0 }, dv[3], dJ[3];
    if (on) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = pose[((size_t)b * J + j) * 3 + k];
    }
    sg_chain_bwd(sG, sD, sJ, J, j, on, v, joints, parents, post, dA + ((size_t)b * J + (on ? j : 0)) * 16, dv, dJ);
    if (!on) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        dpose[((size_t)b * J + j) * 3 + k] = dv[k];
        if (djoints) djoints[((size_t)b * J + j) * 3 + k] = dJ[k];
    }
}
void sg_launch_joint_transforms(int B, int J, const float *pose, const float *joints, const int *parents, const float *post,
                                const float *dA, float *out0, float *out1, hipStream_t st)
{
    if (B <= 0) return;
    if (dA) hipLaunchKernelGGL(sg_joint_transforms_bwd_kernel, dim3(B), dim3(64), 0, st, J, pose, joints, parents, post, dA, out0, out1);
    else hipLaunchKernelGGL(sg_joint_transforms_fwd_kernel, dim3(B), dim3(64), 0, st, J, pose, joints, parents, post, out0);
}

// ---- learned per-frame poses: 6-D table row -> A (sings_hybrid.py:142-150, 370-399) ---------------------------------------
// rotation_6d_to_axis_angle (rotations.py:601-603) = rotation_6d_to_matrix -> matrix_to_quaternion -> quaternion_to_axis_angle per
// joint, then the chain above: the same device functions, in the same order, as the stand-alone kernels, so a table row gives bit
// for bit what those give when they are composed.  Forward: one wave per frame of the step, lane = joint; the row is named by
// frame_idx[k] in DEVICE memory (a captured launch follows the index).  Backward: one wave per TABLE row; it walks frame_idx in
// ascending position and adds the frames that name its row (none: zeros), so the gradient tables are dense, written entirely by
// this launch, free of atomics and reproducible bit for bit.
__device__ __forceinline__ void sg_r6d2aa(const float d[6], float v[3])
{
    float m[9], q[4], qab;
    int best;
    sg_r6d2m(d, m);
    sg_m2q(m, q, best, qab);
    sg_q2aa(q, v);
}
__device__ __forceinline__ void sg_r6d2aa_bwd(const float d[6], const float dv[3], float dd[6])
{
    float m[9], q[4], qab, dq[4], dm[9];
    int best;
    sg_r6d2m(d, m);
    sg_m2q(m, q, best, qab);
    sg_q2aa_bwd(q, dv, dq);
    sg_m2q_bwd(q, best, qab, dq, dm);
    sg_r6d2m_bwd(d, dm, dd);
}
// an index outside [0, F) reads (and, in backward, credits) the nearest row: nothing out of bounds is touched
__device__ __forceinline__ int sg_pose_row(const int *__restrict__ frame_idx, int k, int F)
{
    const int f = frame_idx[k];
    return f < 0 ? 0 : (f >= F ? F - 1 : f);
}
__global__ void __launch_bounds__(64)
sg_pose_transforms_fwd_kernel(int F, int J, int NBu, const int *__restrict__ frame_idx, const float *__restrict__ global_orient,
                              const float *__restrict__ body_pose, const float *__restrict__ tail_pose, const float *__restrict__ transl,
                              const float *__restrict__ joints, const int *__restrict__ parents, const float *__restrict__ post,
                              float *__restrict__ A_out, float *__restrict__ aa_out, float *__restrict__ transl_out)
{
    __shared__ float sG[64][13];
    const int k = blockIdx.x, j = threadIdx.x;
    const bool on = j < J;
    const int f = sg_pose_row(frame_idx, k, F);
    float v[3] = { 0, 0, 0 };
    if (on) {
        if (j <= NBu) {
            const float *src = j == 0 ? global_orient + (size_t)f * 6 : body_pose + ((size_t)f * SG_POSE_NB + (j - 1)) * 6;
            float d[6];
#pragma unroll
            for (int c = 0; c < 6; c++) d[c] = src[c];
            sg_r6d2aa(d, v);
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = tail_pose[(size_t)(j - 1 - NBu) * 3 + c];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) aa_out[((size_t)k * J + j) * 3 + c] = v[c];
    }
    if (transl && j < 3) transl_out[(size_t)k * 3 + j] = transl[(size_t)f * 3 + j];
    sg_chain_fwd(sG, J, j, on, v, joints, parents, post, A_out + ((size_t)k * J + (on ? j : 0)) * 16);
}
__global__ void __launch_bounds__(64)
sg_pose_transforms_bwd_kernel(int K, int F, int J, int NBu, const int *__restrict__ frame_idx, const float *__restrict__ global_orient,
                              const float *__restrict__ body_pose, const float *__restrict__ aa, const float *__restrict__ joints,
                              const int *__restrict__ parents, const float *__restrict__ post, const float *__restrict__ dA,
                              const float *__restrict__ d_transl_rows, float *__restrict__ d_global_orient,
                              float *__restrict__ d_body_pose, float *__restrict__ d_transl)
{
    __shared__ float sG[64][13], sD[64][13], sJ[64][4];
    const int f = blockIdx.x, j = threadIdx.x;
    const bool on = j < J, learned = on && j <= NBu;
    float acc[6] = { 0, 0, 0, 0, 0, 0 }, acc_t = 0.0f;
    bool named = false;                                           // (the first frame is stored, not added to 0: a -0 stays a -0)
    for (int k = 0; k < K; k++) {                                 // ascending position: a row named twice is a fixed-order sum
        if (sg_pose_row(frame_idx, k, F) != f) continue;          // (wave-uniform)
        float v[3] = { 0, 0, 0 }, dv[3] = { 0, 0, 0 }, dJ[3];
        if (on) {
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = aa[((size_t)k * J + j) * 3 + c];
        }
        sg_chain_bwd(sG, sD, sJ, J, j, on, v, joints, parents, post, dA + ((size_t)k * J + (on ? j : 0)) * 16, dv, dJ);
        if (learned) {
            const float *src = j == 0 ? global_orient + (size_t)f * 6 : body_pose + ((size_t)f * SG_POSE_NB + (j - 1)) * 6;
            float d[6], dd[6];
#pragma unroll
            for (int c = 0; c < 6; c++) d[c] = src[c];
            sg_r6d2aa_bwd(d, dv, dd);
#pragma unroll
            for (int c = 0; c < 6; c++) acc[c] = named ? acc[c] + dd[c] : dd[c];
        }
        if (d_transl && j < 3) acc_t = named ? acc_t + d_transl_rows[(size_t)k * 3 + j] : d_transl_rows[(size_t)k * 3 + j];
        named = true;
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();                          // (the next frame of this row reuses the scratch)
    }
    // every entry of row f, also of the body joints the layout does not drive (SMPL-H: 22 and 23)
    if (j <= SG_POSE_NB) {
        float *dst = j == 0 ? d_global_orient + (size_t)f * 6 : d_body_pose + ((size_t)f * SG_POSE_NB + (j - 1)) * 6;
#pragma unroll
        for (int c = 0; c < 6; c++) dst[c] = learned ? acc[c] : 0.0f;
    }
    if (d_transl && j < 3) d_transl[(size_t)f * 3 + j] = acc_t;
}
void sg_launch_pose_transforms(int K, int F, int J, int NBu, const int *frame_idx, const float *global_orient, const float *body_pose,
                               const float *tail_pose, const float *transl, const float *joints, const int *parents, const float *post,
                               float *A_out, float *aa_out, float *transl_out, hipStream_t st)
{
    hipLaunchKernelGGL(sg_pose_transforms_fwd_kernel, dim3(K), dim3(64), 0, st, F, J, NBu, frame_idx, global_orient, body_pose, tail_pose,
                       transl, joints, parents, post, A_out, aa_out, transl_out);
}
void sg_launch_pose_transforms_bwd(int K, int F, int J, int NBu, const int *frame_idx, const float *global_orient, const float *body_pose,
                                   const float *aa, const float *joints, const int *parents, const float *post, const float *dA,
                                   const float *d_transl_rows, float *d_global_orient, float *d_body_pose, float *d_transl, hipStream_t st)
{
    hipLaunchKernelGGL(sg_pose_transforms_bwd_kernel, dim3(F), dim3(64), 0, st, K, F, J, NBu, frame_idx, global_orient, body_pose, aa, joints,
                       parents, post, dA, d_transl_rows, d_global_orient, d_body_pose, d_transl);
}
