// Host side of the extern "C" boundary: what every entry point shares (the formatted refusal, the launch epilogue) and the
// launcher prototypes that sg_common.h does not carry.  Host only; included by the translation units that define entry points.
#pragma once
#include "sg_common.h"

#include <atomic>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

// sg_set_error of an argument error whose text is formatted (the entry point's name first: "%s: ...", who)
static inline int sg_failf(const char *fmt, ...)
{
    char msg[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return sg_set_error(msg, hipSuccess);
}

// the end of an entry point that launches and returns: 0, or the launch error under `what`
static inline int sg_launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_set_error(what, e);
}

// Raising a kernel's dynamic-LDS limit is a host-side call into the runtime (a table update under a lock): asked ONCE per
// (kernel, device) and remembered per device id -- not in a process-wide flag (a second GPU used from the same process must get
// its own call), and a refusal is remembered too (the callers then take their fallback paths).  Round 3 asked on every forward.
// One SgLdsLimit (static storage: zeroes) per kernel.
struct SgLdsLimit { std::atomic<signed char> state[64]; };       // per device: 0 unknown, 1 granted, -1 refused
static inline bool sg_dyn_lds_limit(SgLdsLimit &m, const void *fn, int bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess || ((void)hipGetLastError(), false);
    signed char st = m.state[dev].load(std::memory_order_acquire);
    if (st == 0) {
        st = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 1 : -1;
        if (st < 0) (void)hipGetLastError();
        m.state[dev].store(st, std::memory_order_release);
    }
    return st > 0;
}

// The reference's 11-tap SSIM window (losses/utils.py:28-30): the fp32 values exp(-(x-5)^2 / (2 * 1.5^2)) divided by their sum AS
// torch.Tensor.sum() GIVES IT -- the correctly rounded sum (0x1.e12e8ap+1: summed in fp64, rounded once), not the left-to-right fp32 sum
// (one ulp less: nine weights one ulp larger, the window's sum 1 + 8.9e-8 instead of 1 - 6.2e-8 -- on a smooth frame, where
// 2 sigma12 + C2 is a small difference of window sums, that moves the SSIM mean by 5e-6 to 1e-5: LAB.md "Validation on the device",
// "Photometric loss on smooth frames").  The one copy: the training loss (sg_loss.hip) and the validation metrics (sg_metrics.hip)
// weigh a frame with the same bits, those of tests/golden/photo_loss_golden.npz `window_1d`.
static inline void sg_ssim_window(float w[11])
{
    float g[11];
    double s = 0.0;
    for (int x = 0; x < 11; x++) { g[x] = (float)exp(-(double)((x - 5) * (x - 5)) / (2.0 * 1.5 * 1.5)); s += (double)g[x]; }
    for (int x = 0; x < 11; x++) w[x] = g[x] / (float)s;
}

// between the launches of one entry point: return on a launch error; SgRasterSettings.debug also waits for the kernel
#define SG_CHECK_LAST(what, s, st)                                           \
    do {                                                                     \
        hipError_t e_ = hipGetLastError();                                   \
        if (e_ != hipSuccess) return sg_set_error(what, e_);                 \
        if ((s)->debug) {                                                    \
            e_ = hipStreamSynchronize(st);                                   \
            if (e_ != hipSuccess) return sg_set_error(what, e_);             \
        }                                                                    \
    } while (0)

// (declared here, not in sg_common.h: that header is one of the sources the committed PMC profiles are keyed on)
int sg_launch_linear_bwd_fan(int N, int Cin, int Cout, int act, const float *z, const float *dh, const float *W, float *dz_out,
                             float *dx_out, const SgLinearSide *side, hipStream_t st);
void sg_launch_scales_head(int N, const float *z, float *scales, float *aux, const float *dscales, const float *daux, float *dz,
                           hipStream_t st);

// ---- work order (include/sings_order.h) ----
// Where a work order takes effect: many-tile frames binned directly (SG_FLAG_SHORT_LISTS, no whole-image histogram).  Elsewhere the
// launch is the unordered one -- any order is correct, so is none.
static inline bool sg_order_applies(const SgCam &c) { return !sg_lds_hist(c.gx, c.gy) && sg_key_pitch_of(false, c.flags) != 0u; }
void sg_launch_preprocess_fwd_ordered(const SgCam &c, const SgBatch &bt, int P, const float *means3D, const float *shs,
                                      const float *colors_precomp, const float *opacities, const float *scales,
                                      const float *rotations, const float *cov3D_precomp, SgGeom g, SgBin b,
                                      size_t cap, int32_t *radii, const uint32_t *order, hipStream_t st);
void sg_launch_morton_codes(int P, const float *means3D, float *box, uint32_t *codes, hipStream_t st);
