"""Times LPIPS-VGG (sings_amd.lpips, csrc/sg_lpips.hip) on the GPU box:  python tools/lpips_time.py [--iters N]

  1. the training term's shape: forward on 4 pred + 4 gt 128^2 patches and the input gradient of the 4 pred patches (per step)
  2. a 512x896 full-frame forward (the validation metric)
  3. the same shapes through torch F.conv2d (the library convolutions) for comparison
and, from a torch.profiler kernel trace of one step of (1), the achieved fraction of the fp32 matrix peak (157.3 TFLOP/s) per VGG
level, forward and input-gradient convs together.  Weights: the test oracle's random VGG16-shaped weights (timing does not depend
on their values)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                                      # noqa: E402
import torch.nn.functional as F                                   # noqa: E402

import lpips_case as lc                                           # noqa: E402
from sings_amd import lpips as L                                  # noqa: E402

PEAK = 157.3e12
LEVEL = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def conv_flops(H, W, images):
    """-> per conv layer l >= 1: FLOPs of one direction on `images` images of H x W."""
    out = {}
    for l in range(1, 13):
        v = LEVEL[l]
        h, w = H >> v, W >> v
        ci, co = L.CONV_CHANNELS[l]
        out[l] = 2.0 * h * w * ci * co * 9 * images
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    wt = lc.make_weights(0)
    m = L.LPIPS.from_tensors(wt["convs"], wt["lins"], wt["shift"], wt["scale"], device=dev)
    g = torch.Generator(dev).manual_seed(0)
    pred = torch.rand(4, 3, 128, 128, device=dev, generator=g); gt = torch.rand(4, 3, 128, 128, device=dev, generator=g)
    full0 = torch.rand(1, 3, 512, 896, device=dev, generator=g); full1 = torch.rand(1, 3, 512, 896, device=dev, generator=g)

    def step():
        x = pred.clone().requires_grad_(True)
        m(x, gt).mean().backward()
        return x.grad

    def full():
        with torch.no_grad():
            return m(full0, full1)

    ms_step = timed(step, a.iters)
    ms_full = timed(full, max(3, a.iters // 4))
    print(f"sings_amd LPIPS: 4+4 x 128^2 forward + input gradient {ms_step:.3f} ms per step; 512x896 forward {ms_full:.3f} ms")

    # torch F.conv2d on the same trunk (fp32, library defaults), the head in torch
    tw = [(w.to(dev), b.to(dev)) for w, b in wt["convs"]]
    tl = [x.to(dev) for x in wt["lins"]]
    sh, sc = wt["shift"].to(dev), wt["scale"].to(dev)

    def feats(x):
        outs, l = [], 0
        for k, n in enumerate(L.SLICE_CONVS):
            if k:
                x = F.max_pool2d(x, 2, 2)
            for _ in range(n):
                x = F.relu(F.conv2d(x, tw[l][0], tw[l][1], padding=1)); l += 1
            outs.append(x)
        return outs

    def torch_lpips(x0, x1):
        f0, f1 = feats((x0 - sh) / sc), feats((x1 - sh) / sc)
        v = 0
        for k in range(5):
            n0 = f0[k] / (f0[k].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            n1 = f1[k] / (f1[k].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            v = v + F.conv2d((n0 - n1) ** 2, tl[k]).mean([2, 3], keepdim=True)
        return v

    def t_step():
        x = pred.clone().requires_grad_(True)
        torch_lpips(x, gt).mean().backward(inputs=[x])
        return x.grad

    def t_full():
        with torch.no_grad():
            return torch_lpips(full0, full1)

    tms_step = timed(t_step, a.iters)
    tms_full = timed(t_full, max(3, a.iters // 4))
    print(f"torch F.conv2d LPIPS: 4+4 x 128^2 forward + input gradient {tms_step:.3f} ms per step; 512x896 forward {tms_full:.3f} ms")

    # per-level matrix-peak fraction from a kernel trace of one step
    from torch.profiler import ProfilerActivity, profile
    step(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(); torch.cuda.synchronize()
    ev = [e for e in prof.events() if "lp_conv3x3" in e.name]
    ev.sort(key=lambda e: e.time_range.start)
    if len(ev) != 24:
        print(f"per-level fractions: unmeasured (the trace holds {len(ev)} conv kernels, expected 24)")
        return
    fwd_f, bwd_f = conv_flops(128, 128, 8), conv_flops(128, 128, 4)
    layers = list(range(1, 13)) + list(range(12, 0, -1))
    lv_t, lv_f = [0.0] * 5, [0.0] * 5
    for i, (e, l) in enumerate(zip(ev, layers)):
        dur = (e.time_range.end - e.time_range.start) * 1e-6                    # us -> s
        lv_t[LEVEL[l]] += dur
        lv_f[LEVEL[l]] += fwd_f[l] if i < 12 else bwd_f[l]
    for v in range(5):
        print(f"level {v + 1}: {lv_f[v] / 1e9:7.2f} GFLOP in {lv_t[v] * 1e3:7.3f} ms = {lv_f[v] / lv_t[v] / 1e12:6.1f} TFLOP/s, "
              f"{lv_f[v] / lv_t[v] / PEAK:.2f} of the fp32 matrix peak (MFMA convs; conv1_1 excluded)")
    tot_t = sum(lv_t)
    print(f"MFMA convs total {tot_t * 1e3:.3f} ms of the {ms_step:.3f}-ms step")


if __name__ == "__main__":
    main()
