// A decoder without a gradient in ONE launch (include/sings_frozen.h): tri-plane features in, attributes out, every hidden layer
// in LDS.  The reference's first opt_geo_from / opt_app_from iterations run the decoders under torch.no_grad()
// (sings_hybrid.py:265-277); the per-layer kernels of sg_linear.hip write each hidden h and its gelu'(z) for a backward that never
// comes -- at 150 k points six 77-MB arrays for the geometry decoder, to produce under 2 MB of outputs.
//
// A workgroup (four waves) owns SG_FROZEN_BLOCK = 128 points.  Their activations are ONE LDS image [128][XS], XS = widest layer
// + 4 floats (the pad that spreads the rows over the banks for ds_read_b128), and every layer works IN PLACE on it:
//     all four waves multiply (reads only) -> barrier -> bias + GELU from the accumulators into the same rows -> barrier.
// A product is sg_linear.hip's narrow form: the weights are the MFMA A operand (lane: output column 32 cb + j), the points the B
// operand, read with one ds_read_b128 per four v_mfma_f32_32x32x2_f32 from the permuted reduction index (step s multiplies inputs s
// and CK/2 + s).  The accumulator of a 32 x 32 tile then holds, per lane, four times four CONSECUTIVE output columns of ONE point:
// the next layer's input row leaves as 16-B LDS stores, a head's columns as that point's few global stores.  A layer of TO = Cout / 32
// column blocks gives each wave one block of TO of the four 32-point tiles (16 TO accumulator registers, TO independent MFMA
// chains); a narrow head is one padded column block, one point tile per wave.  The heads that read the trunk (xyz_offsets +
// rotations: 9 columns; shs + opacity: 49) are stacked into one product; in the geometry decoder they run BEFORE scales.0
// overwrites the trunk.
//
// The block size is the one decision.  Weights do not fit beside 64 accumulator registers at two waves per SIMD, so a lane
// fetches its 16 bytes of W per four MFMAs from L2 (two steps ahead), i.e. a workgroup re-reads every layer's weights once
// (once per wave that shares a column block).  Shipped widths, geometry, Cin = 96, hidden 128:
//     weights per workgroup    (96 + 128 + 128) x 128 x 4 B + 4 x (9 + 1) x 128 x 4 B       = 196 KiB from L2 (all of it resident: 4 MiB)
//     what it replaces, HBM    per point 3 hidden layers x 512 B x (h written + gelu' written + h read back; the trunk twice)
//                              = 5 KiB, x 128 points                                        = 640 KiB
// so the L2 re-read is under a third of the HBM traffic it removes, and the kernel's own HBM traffic is the 384-B feature row
// and 36 - 60 B of outputs per point.  At 64 points the re-read would be 60 % of it; 256 points need 132 KiB of LDS (one workgroup
// per CU) and 128 accumulator registers.  LDS: 128 x 132 x 4 B = 66 KiB, two workgroups per CU within the 160 KiB; <= 256 registers.
// The arithmetic is the floor: 45 k multiply-adds per point on the fp32 matrix cores (64 FLOP / clk / SIMD), ~90 us at 150 k points.
#include "sg_host.h"
#include "sg_act.h"
#include "../../include/sings_frozen.h"

#include <atomic>

#define FZ_R SG_FROZEN_BLOCK
#define FZ_MAXC 128

// The GELU of sg_linear_forward's epilogue: the same sg_gelu_both, its derivative dropped, so the two paths round a hidden
// activation to the same bits from the same sum.
__device__ __forceinline__ float fz_gelu(float z)
{
    float h, dh;
    sg_gelu_both(z, h, dh);
    return h;
}

// up to two weight matrices [rows, CK] stacked into one product: output column c < rows0 is row c of W0, then rows of W1
struct FzStack { const float *W0, *W1; int rows0, rows1; };

// acc[i] = W(32 cb + .., :) . X(tile tg TO + i)^T for this wave's column block cb = wave % TO and its TO point tiles.
// sX [FZ_R][XS]; columns CK .. CKP - 1 of it are zero (CKP = CK rounded up to 8).  Reads only.
template <int TO>
__device__ __forceinline__ void fz_product(const float *sX, int XS, int CK, const FzStack &L, int wave, int lane, sg_v16f (&acc)[TO])
{
    const int CKP = (CK + 7) & ~7, HALF = CKP >> 1, NQ = CKP >> 3;
    const int cb = wave % TO, tg = wave / TO, j = lane & 31, h = lane >> 5;
    const int co = 32 * cb + j;
    const float *wrow = nullptr;
    if (co < L.rows0) wrow = L.W0 + (size_t)co * CK;
    else if (co < L.rows0 + L.rows1) wrow = L.W1 + (size_t)(co - L.rows0) * CK;
    auto ldw = [&](int q) {                                                // W(co, h HALF + 4 q ..+3): whole or not at all (CK % 4 == 0)
        const int k = h * HALF + 4 * q;
        return (wrow && q < NQ && k < CK) ? *(const float4 *)(wrow + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
#pragma unroll
    for (int i = 0; i < TO; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.0f;
    const float *xb = sX + (32 * tg * TO + j) * XS + h * HALF;             // B operand: X[point j of the tile][h HALF + s]
    float4 wa = ldw(0), wb = ldw(1);
    for (int q = 0; q < NQ; q++) {
        const float4 wc = ldw(q + 2);                                      // two steps ahead: an L2 round trip under 8 TO MFMAs
        float4 b[TO];
#pragma unroll
        for (int i = 0; i < TO; i++) b[i] = *(const float4 *)(xb + i * 32 * XS + 4 * q);
#pragma unroll
        for (int i = 0; i < TO; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.x, b[i].x, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TO; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.y, b[i].y, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TO; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.z, b[i].z, acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TO; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.w, b[i].w, acc[i], 0, 0, 0);
        wa = wb; wb = wc;
    }
}

// A hidden layer of 32 TO columns, in place: product, barrier (every wave has read the old rows), gelu(acc + bias) into columns
// 0 .. 32 TO - 1 of the same rows, barrier.
template <int TO>
__device__ __forceinline__ void fz_hidden(float *sX, int XS, int CK, const float *__restrict__ W, const float *__restrict__ bias,
                                          int wave, int lane)
{
    sg_v16f acc[TO];
    const FzStack L = { W, nullptr, 32 * TO, 0 };
    fz_product<TO>(sX, XS, CK, L, wave, lane, acc);
    const int cb = wave % TO, tg = wave / TO, j = lane & 31, h = lane >> 5;
    float bv[16];
#pragma unroll
    for (int r = 0; r < 16; r++) bv[r] = bias[32 * cb + 8 * (r >> 2) + 4 * h + (r & 3)];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TO; i++) {
        float *row = sX + (32 * (tg * TO + i) + j) * XS + 32 * cb + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; g++)
            *(float4 *)(row + 8 * g) = make_float4(fz_gelu(acc[i][4 * g] + bv[4 * g]), fz_gelu(acc[i][4 * g + 1] + bv[4 * g + 1]),
                                                   fz_gelu(acc[i][4 * g + 2] + bv[4 * g + 2]), fz_gelu(acc[i][4 * g + 3] + bv[4 * g + 3]));
    }
    __syncthreads();
}

// the workgroup's feature rows into LDS: 16-B loads, rows beyond N and columns Cin .. CKP - 1 zero
__device__ __forceinline__ void fz_load_features(float *sX, int XS, int N, int Cin, const float *__restrict__ X, int n0, int tid)
{
    const int f4row = ((Cin + 7) & ~7) >> 2;
    for (int f = tid; f < FZ_R * f4row; f += 256) {
        const int row = f / f4row, c = 4 * (f - row * f4row), n = n0 + row;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (n < N && c < Cin) v = *(const float4 *)(X + (size_t)n * Cin + c);
        *(float4 *)(sX + row * XS + c) = v;
    }
    __syncthreads();
}

struct FzGeoArgs {
    int N, Cin, H, aniso, XS;
    const float *X, *W0, *b0, *W2, *b2, *Ws0, *bs0, *Ws2, *bs2, *Wxyz, *bxyz, *Wrot, *brot;
    float *xyz, *scales, *aux, *rot;
};

template <int TH>                         // hidden / 32
__global__ void __launch_bounds__(256, 2)
sg_frozen_geometry_kernel(FzGeoArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float fz_sX[];
    float *sX = fz_sX;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * FZ_R, H = 32 * TH, XS = a.XS;
    fz_load_features(sX, XS, a.N, a.Cin, a.X, n0, tid);
    fz_hidden<TH>(sX, XS, a.Cin, a.W0, a.b0, wave, lane);
    fz_hidden<TH>(sX, XS, H, a.W2, a.b2, wave, lane);
    const int n = n0 + 32 * wave + j;                                      // a narrow head: point tile `wave`, this lane's point
    {   // xyz_offsets (3) and rotations (6) on the trunk, before scales.0 overwrites it
        const int nrot = a.aniso ? 6 : 0;
        sg_v16f acc[1];
        const FzStack L = { a.Wxyz, a.Wrot, 3, nrot };
        fz_product<1>(sX, XS, H, L, wave, lane, acc);
        if (n < a.N) {
#pragma unroll
            for (int g = 0; g < 2; g++)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int c = 8 * g + 4 * h + u;
                    if (c < 3) a.xyz[(size_t)n * 3 + c] = acc[0][4 * g + u] + a.bxyz[c];
                    else if (c < 3 + nrot) a.rot[(size_t)n * 6 + (c - 3)] = acc[0][4 * g + u] + a.brot[c - 3];
                }
        }
    }
    fz_hidden<TH>(sX, XS, H, a.Ws0, a.bs0, wave, lane);                    // (its first barrier: every wave is done with the trunk)
    {   // scales.2: z -> scales_aux, log(exp(z) + 1) -> scales (the isotropic column three times: sg_scales_head_forward)
        const int ns = a.aniso ? 3 : 1;
        sg_v16f acc[1];
        const FzStack L = { a.Ws2, nullptr, ns, 0 };
        fz_product<1>(sX, XS, H, L, wave, lane, acc);
        if (n < a.N && h == 0) {                                           // columns 0..3: register 0..3 of the lower half
            const float z0 = acc[0][0] + a.bs2[0];
            const float z1 = a.aniso ? acc[0][1] + a.bs2[1] : z0, z2 = a.aniso ? acc[0][2] + a.bs2[2] : z0;
            const float s0 = sg_softplus(z0);
            const float s1 = a.aniso ? sg_softplus(z1) : s0, s2 = a.aniso ? sg_softplus(z2) : s0;
            float *ps = a.scales + (size_t)n * 3, *pa = a.aux + (size_t)n * 3;
            ps[0] = s0; ps[1] = s1; ps[2] = s2;
            pa[0] = z0; pa[1] = z1; pa[2] = z2;
        }
    }
}

struct FzAppArgs {
    int N, Cin, H, XS;
    const float *X, *W0, *b0, *W2, *b2, *Wshs, *bshs, *Wop, *bop, *off;
    float *shs, *opacity;
};

template <int TH>
__global__ void __launch_bounds__(256, 2)
sg_frozen_appearance_kernel(FzAppArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float fz_sX[];
    float *sX = fz_sX;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * FZ_R, H = 32 * TH, XS = a.XS;
    fz_load_features(sX, XS, a.N, a.Cin, a.X, n0, tid);
    fz_hidden<TH>(sX, XS, a.Cin, a.W0, a.b0, wave, lane);
    fz_hidden<TH>(sX, XS, H, a.W2, a.b2, wave, lane);
    // shs (48) and opacity (1) stacked: two column blocks, two point tiles per wave
    sg_v16f acc[2];
    const FzStack L = { a.Wshs, a.Wop, SG_FROZEN_SHS, a.Wop ? 1 : 0 };
    fz_product<2>(sX, XS, H, L, wave, lane, acc);
    const int cb = wave % 2, tg = wave / 2;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int n = n0 + 32 * (2 * tg + i) + j;
        if (n >= a.N) continue;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c = 32 * cb + 8 * g + 4 * h;
            if (c < SG_FROZEN_SHS) {
                const float4 bb = *(const float4 *)(a.bshs + c);
                *(float4 *)(a.shs + (size_t)n * SG_FROZEN_SHS + c) =
                    make_float4(acc[i][4 * g] + bb.x, acc[i][4 * g + 1] + bb.y, acc[i][4 * g + 2] + bb.z, acc[i][4 * g + 3] + bb.w);
            } else if (c == SG_FROZEN_SHS && a.Wop) {                      // sigmoid(z + offset): sg_linear_forward's act 2
                const float ro = a.off ? a.off[n] : 0.0f;
                a.opacity[n] = sg_sigmoid((acc[i][4 * g] + a.bop[0]) + ro);
            }
        }
    }
}

// the kernels' dynamic LDS is above the 64 KiB a launch gets unasked at the widest layers: raised once per (kernel, device)
static bool fz_lds_limit(int which, const void *fn, int bytes)
{
    static std::atomic<signed char> state[4][64];                // 0 unknown, 1 granted, -1 refused
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess || ((void)hipGetLastError(), false);
    signed char st = state[which][dev].load(std::memory_order_acquire);
    if (st == 0) {
        st = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 1 : -1;
        if (st < 0) (void)hipGetLastError();
        state[which][dev].store(st, std::memory_order_release);
    }
    return st > 0;
}

// the checks both entry points share; 0 or the refusal's status
static int fz_check_sizes(const char *who, int N, int Cin, int hidden)
{
    if (N < 1) return sg_failf("%s: N = %d, at least one point is needed", who, N);
    if (Cin < 4 || Cin > FZ_MAXC || (Cin & 3)) return sg_failf("%s: Cin = %d is not a multiple of 4 in 4..%d", who, Cin, FZ_MAXC);
    if (hidden != 64 && hidden != 128) return sg_failf("%s: hidden = %d is neither 64 nor 128", who, hidden);
    return 0;
}
// a required pointer; wide: read or written 16 bytes at a time (features, weight rows, shs and its bias), otherwise by element
struct FzPtr { const char *name; const void *p; bool wide; };
static int fz_check_pointers(const char *who, const FzPtr *ptrs, int n)
{
    for (int i = 0; i < n; i++) {
        const unsigned align = ptrs[i].wide ? 16u : 4u;
        if (!ptrs[i].p) return sg_failf("%s: %s is a null pointer", who, ptrs[i].name);
        if ((uintptr_t)ptrs[i].p & (align - 1u)) return sg_failf("%s: %s is not %u-byte aligned", who, ptrs[i].name, align);
    }
    return 0;
}
static inline int fz_row_floats(int Cin, int hidden) { const int ckp = (Cin + 7) & ~7; return (ckp > hidden ? ckp : hidden) + 4; }

extern "C" int sg_frozen_geometry(int N, int Cin, int hidden, int anisotropic, const float *feats, const float *W_net0,
                                  const float *b_net0, const float *W_net2, const float *b_net2, const float *W_scales0,
                                  const float *b_scales0, const float *W_scales2, const float *b_scales2, const float *W_xyz,
                                  const float *b_xyz, const float *W_rot, const float *b_rot, float *xyz_offsets, float *scales,
                                  float *scales_aux, float *rotations, void *stream)
{
    const char *who = "sg_frozen_geometry";
    if (fz_check_sizes(who, N, Cin, hidden)) return 1;
    const FzPtr need[] = { { "feats", feats, true }, { "W_net0", W_net0, true }, { "b_net0", b_net0, false }, { "W_net2", W_net2, true }, { "b_net2", b_net2, false },
                           { "W_scales0", W_scales0, true }, { "b_scales0", b_scales0, false }, { "W_scales2", W_scales2, true },
                           { "b_scales2", b_scales2, false }, { "W_xyz", W_xyz, true }, { "b_xyz", b_xyz, false }, { "xyz_offsets", xyz_offsets, false },
                           { "scales", scales, false }, { "scales_aux", scales_aux, false } };
    if (fz_check_pointers(who, need, (int)(sizeof need / sizeof need[0]))) return 1;
    const FzPtr rot[] = { { "W_rot", W_rot, true }, { "b_rot", b_rot, false }, { "rotations", rotations, false } };
    if (anisotropic && fz_check_pointers(who, rot, 3)) return 1;
    FzGeoArgs a = { N, Cin, hidden, anisotropic ? 1 : 0, fz_row_floats(Cin, hidden), feats, W_net0, b_net0, W_net2, b_net2,
                    W_scales0, b_scales0, W_scales2, b_scales2, W_xyz, b_xyz, W_rot, b_rot, xyz_offsets, scales, scales_aux, rotations };
    const int lds = FZ_R * a.XS * (int)sizeof(float), grid = (N + FZ_R - 1) / FZ_R;
    const void *fn = hidden == 128 ? (const void *)sg_frozen_geometry_kernel<4> : (const void *)sg_frozen_geometry_kernel<2>;
    if (lds > 64 * 1024 && !fz_lds_limit(hidden == 128 ? 0 : 1, fn, lds))
        return sg_failf("%s: the device refuses %d bytes of LDS per workgroup", who, lds);
    if (hidden == 128) hipLaunchKernelGGL(sg_frozen_geometry_kernel<4>, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(sg_frozen_geometry_kernel<2>, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
    return sg_launched(who);
}

extern "C" int sg_frozen_appearance(int N, int Cin, int hidden, const float *feats, const float *W_net0, const float *b_net0,
                                    const float *W_net2, const float *b_net2, const float *W_shs, const float *b_shs,
                                    const float *W_opacity, const float *b_opacity, const float *opacity_offset, float *shs,
                                    float *opacity, void *stream)
{
    const char *who = "sg_frozen_appearance";
    if (fz_check_sizes(who, N, Cin, hidden)) return 1;
    const FzPtr need[] = { { "feats", feats, true }, { "W_net0", W_net0, true }, { "b_net0", b_net0, false }, { "W_net2", W_net2, true }, { "b_net2", b_net2, false },
                           { "W_shs", W_shs, true }, { "b_shs", b_shs, true }, { "shs", shs, true } };
    if (fz_check_pointers(who, need, (int)(sizeof need / sizeof need[0]))) return 1;
    const FzPtr op[] = { { "W_opacity", W_opacity, true }, { "b_opacity", b_opacity, false }, { "opacity", opacity, false } };
    if (W_opacity && fz_check_pointers(who, op, 3)) return 1;
    FzAppArgs a = { N, Cin, hidden, fz_row_floats(Cin, hidden), feats, W_net0, b_net0, W_net2, b_net2, W_shs, b_shs, W_opacity,
                    b_opacity, W_opacity ? opacity_offset : nullptr, shs, opacity };
    const int lds = FZ_R * a.XS * (int)sizeof(float), grid = (N + FZ_R - 1) / FZ_R;
    const void *fn = hidden == 128 ? (const void *)sg_frozen_appearance_kernel<4> : (const void *)sg_frozen_appearance_kernel<2>;
    if (lds > 64 * 1024 && !fz_lds_limit(hidden == 128 ? 2 : 3, fn, lds))
        return sg_failf("%s: the device refuses %d bytes of LDS per workgroup", who, lds);
    if (hidden == 128) hipLaunchKernelGGL(sg_frozen_appearance_kernel<4>, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(sg_frozen_appearance_kernel<2>, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
    return sg_launched(who);
}
