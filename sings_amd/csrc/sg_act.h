// The decoders' activations, once: the element-wise kernels of sg_decode.hip, the fused layers of sg_linear.hip and the frozen
// decoders of sg_decode_frozen.hip all compute them from here, so the paths that must agree bit for bit (per-layer forward against
// frozen decode) run the same operations by construction.  Device bodies only.
#pragma once
#include "sg_common.h"

// activation codes of sg_bias_act_* / sg_linear_* (ABI: include/sings_hip.h)
#define SG_ACT_NONE 0
#define SG_ACT_GELU 1                  // GELU (erf)
#define SG_ACT_SIGMOID 2               // sigmoid(z + row_offset)
#define SG_ACT_SOFTPLUS 3              // log(exp(z) + 1)

__device__ __forceinline__ float sg_gelu(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f)); }
__device__ __forceinline__ float sg_gelu_grad(float z)
{
    const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
    return cdf + z * 0.39894228040143267794f * __expf(-0.5f * z * z);
}
// GELU and its derivative from ONE evaluation of erf: h = z Phi(z), h' = Phi(z) + z phi(z), Phi = (1 + erf(z / sqrt 2)) / 2.
// erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, i.e. fp32 round-off of Phi): 1 - (a1 t + ... + a5 t^5) e^(-x^2),
// t = 1 / (1 + p |x|); the e^(-x^2) = e^(-z^2 / 2) it needs is the one phi(z) needs.  The fused layers' forward epilogue and the
// frozen decoders' hidden layers (which drop dh) both call this: they round a hidden activation to the same bits from the same sum.
__device__ __forceinline__ void sg_gelu_both(float z, float &h, float &dh)
{
    const float x = fabsf(z) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, x, 1.0f));
    const float e = __expf(-x * x);
    const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
    const float erfa = fmaf(-poly, e, 1.0f);                               // erf(|x|)
    const float cdf = 0.5f * (1.0f + copysignf(erfa, z));
    h = z * cdf;
    dh = fmaf(z * 0.39894228040143267794f, e, cdf);
}
__device__ __forceinline__ float sg_sigmoid(float t) { return 1.0f / (1.0f + expf(-t)); }
__device__ __forceinline__ float sg_softplus(float z) { return logf(expf(z) + 1.0f); }
__device__ __forceinline__ float sg_softplus_grad(float z) { const float e = expf(z); return e / (e + 1.0f); }

// h = act(z); ro: the row's offset inside the sigmoid (0 without one)
__device__ __forceinline__ float sg_act(int act, float z, float ro)
{
    if (act == SG_ACT_GELU) return sg_gelu(z);
    if (act == SG_ACT_SIGMOID) return sg_sigmoid(z + ro);
    if (act == SG_ACT_SOFTPLUS) return sg_softplus(z);
    return z;
}
// The derivative comes in two shapes that do NOT round alike; each caller keeps its own.
// sg_linear: a FACTOR from the forward's aux value -- GELU: aux = gelu'(z); sigmoid: aux = h; softplus: aux = z
__device__ __forceinline__ float sg_act_grad_aux(int act, float aux)
{
    if (act == SG_ACT_GELU) return aux;
    if (act == SG_ACT_SIGMOID) return aux * (1.0f - aux);
    if (act == SG_ACT_SOFTPLUS) return sg_softplus_grad(aux);
    return 1.0f;
}
// sg_bias_act_*: dz = g act'(z) from z itself, g multiplied in FIRST -- (g s) (1 - s), (g e) / (e + 1)
__device__ __forceinline__ float sg_act_bwd(int act, float g, float z, float ro)
{
    if (act == SG_ACT_GELU) return g * sg_gelu_grad(z);
    if (act == SG_ACT_SIGMOID) { const float s = sg_sigmoid(z + ro); return g * s * (1.0f - s); }
    if (act == SG_ACT_SOFTPLUS) { const float e = expf(z); return g * e / (e + 1.0f); }
    return g;
}
