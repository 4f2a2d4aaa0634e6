"""Times a checkpoint of the bench's training workload on the GPU box:  python tools/checkpoint_time.py [--reps N] [--out FILE]

The trainer of tools/density_stats_time.py (``avatar_scene(150000, J=52)``, fused optimiser, learned poses of 300 frames, captured step)
after a few steps: ``AvatarTrainer.state_dict()`` (device -> host copies of the anchors, the 33 MB of planes, both moment buffers, the
statistics and the pose tables), ``save_checkpoint`` (the same plus ``torch.save`` into a temporary file and ``os.replace``), the file's size,
and ``load_checkpoint`` into the same trainer (validation, host -> device, one rebuild).  Wall clock, ``--reps`` times each; the median
and the spread.  None of it is on a step's path: a run saves every few thousand iterations.

Writes profiles/checkpoint_time.json (``--out``)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch                                                      # noqa: E402

from density_stats_time import build_trainer, warm_up            # noqa: E402
from sings_amd import grad_arena, overflow                        # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=150000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "checkpoint_time.py needs the GPU"
    dev = torch.device("cuda:0")
    out = {"reps": a.reps, "N": a.n, "device_name": torch.cuda.get_device_name(0)}
    try:
        tr, step = build_trainer(dev, a.n, 1)
        warm_up(tr, step)
        ms = {"state_dict_ms": [], "save_checkpoint_ms": [], "load_checkpoint_ms": []}
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "human_000006.pth")
            for _ in range(a.reps):
                ms["state_dict_ms"].append(timed(tr.state_dict)[0])
                ms["save_checkpoint_ms"].append(timed(lambda: tr.save_checkpoint(path))[0])
            out["file_bytes"] = os.path.getsize(path)
            for _ in range(a.reps):
                ms["load_checkpoint_ms"].append(timed(lambda: tr.load_checkpoint(path))[0])
            assert tr.iteration == 6 and tr.captured is None
            warm_up(tr, step)                                     # (the loaded trainer sizes and captures again, and steps)
            assert tr.captured is not None
        out.update({k: stats(v) for k, v in ms.items()})
    finally:
        overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
        grad_arena.set_gradient_arena(None, None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
