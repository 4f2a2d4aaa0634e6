// One (pixel, face) pair of the soft silhouette (include/sings_silhouette.h), stated ONCE: the forward and the backward composite of
// sg_silhouette.hip take the same threshold decisions because they run the same instructions.  `silhouette_host` of
// sings_amd/pose_refine.py operation for operation (the build has -ffp-contract=off and correctly rounded divisions).
#pragma once
#include "sg_common.h"

struct SgSilScalars { float s2, r, sigma; };     // (2 / min(H, W))^2;  ln(1 / 1e-4 - 1) sigma;  sigma

struct SgSilPair {
    bool on;         // blended: inside, or the squared distance within the band
    float x;         // signed squared distance / sigma (NDC): q = sigmoid(x), prob = 1 - q
    float sign;      // -1 inside, +1 outside
    int edge;        // the nearest edge e: from corner e to corner (e + 1) % 3
    float t, dx, dy; // the clamped parameter on it and pixel - nearest point, in pixels
};

// ra = (u0, v0, u1, v1), rb = (u2, v2, -, -) in pixels; (px, py) the pixel centre
__device__ __forceinline__ SgSilPair sg_sil_pair(float px, float py, const float4 ra, const float4 rb, const SgSilScalars c)
{
    const float ux[3] = {ra.x, ra.z, rb.x}, uy[3] = {ra.y, ra.w, rb.y};
    SgSilPair p;
    bool pos = true, neg = true;
    float best = 0.0f;
    p.edge = 0; p.t = 0.0f; p.dx = 0.0f; p.dy = 0.0f;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const int b = (e + 1) % 3;
        const float ex = ux[b] - ux[e], ey = uy[b] - uy[e];
        const float wx = px - ux[e], wy = py - uy[e];
        const float cr = ex * wy - ey * wx;
        pos = pos && cr > 0.0f;
        neg = neg && cr < 0.0f;
        const float t = fminf(fmaxf((wx * ex + wy * ey) / (ex * ex + ey * ey), 0.0f), 1.0f);
        const float dx = wx - t * ex, dy = wy - t * ey;
        const float d2 = dx * dx + dy * dy;
        if (e == 0 || d2 < best) { best = d2; p.edge = e; p.t = t; p.dx = dx; p.dy = dy; }
    }
    const float d2n = best * c.s2;
    const bool inside = pos || neg;
    p.on = inside || d2n < c.r;
    p.sign = inside ? -1.0f : 1.0f;
    p.x = (inside ? -d2n : d2n) / c.sigma;
    return p;
}

// prob = 1 / (1 + exp(x)), the face's coverage of the pixel; q = 1 - prob is what the blend multiplies up
__device__ __forceinline__ float sg_sil_prob(float x) { return 1.0f / (1.0f + expf(x)); }
