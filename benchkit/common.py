"""Small helpers shared by the legs of bench.py."""
import ctypes as C
import json
import sys


def _release():
    """Between legs of one process: drop what the finished leg allocated (its locals are gone) and reset the library's global modes."""
    import gc
    import torch
    from sings_amd import rasterizer as _rz
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    _rz.set_overflow_check("sync")
    _rz.reset_overflow_state()


def _tile_list_stats(eng, W, H):
    """mean / max length of the per-tile depth-sorted lists of the engine's last forward (reported with
    every number); read from the tile ranges in the binning workspace."""
    import torch
    T = ((W + 15) // 16) * ((H + 15) // 16)
    rg = eng.binning[eng.L.bin_ranges:eng.L.bin_ranges + 8 * T].view(torch.int32).view(T, 2)
    n = (rg[:, 1] - rg[:, 0]).clamp_(min=0)
    return float(n.float().mean().item()), int(n.max().item())


DUMP_BUDGET_BYTES = 60_000_000      # --dump-outputs: all arrays together (the .npy headers ride on the remaining 4 MB of 64 MB)
DUMP_SEED = 20240901


def dump_plan(sizes, budget=DUMP_BUDGET_BYTES):
    """{name: (elements, itemsize)} -> {name: elements written}: the budget is shared out smallest array first, each taking at
    most an equal part of what is left, so small arrays are written whole and the larger ones share the rest equally."""
    plan, left = {}, int(budget)
    order = sorted(sizes, key=lambda k: (sizes[k][0] * sizes[k][1], k))
    for i, name in enumerate(order):
        n, item = sizes[name]
        take = min(n, left // (len(order) - i) // item)
        plan[name] = take
        left -= take * item
    return plan


def sample_index(name, n, k):
    """The fixed sample of a flat array of n elements of which k are written: [0, n) cut into k equal blocks, one index drawn in each
    with a seed that depends on the name and size only -- k sorted distinct indices, the same in every run and every build."""
    import zlib
    import numpy as np
    if k >= n:
        return None
    rng = np.random.default_rng([DUMP_SEED, zlib.crc32(name.encode()), n])
    bounds = np.arange(k + 1, dtype=np.int64) * n // k
    return bounds[:-1] + (rng.random(k) * (bounds[1:] - bounds[:-1])).astype(np.int64)


def dump_outputs(directory, arrays, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: write `arrays` ({name: torch tensor or numpy array}) as DIRECTORY/<name>.npy, float64 ones as float64 and
    everything else as float32, at most `budget` bytes in all (dump_plan); an array larger than its share is written as the fixed
    sample sample_index() picks from its flattened values.  -> {name: {shape, dtype, written, sampled}} for the JSON line."""
    import os
    import numpy as np
    import torch
    os.makedirs(directory, exist_ok=True)
    item = {k: 8 if v.dtype in (torch.float64, np.float64) else 4 for k, v in arrays.items()}
    plan = dump_plan({k: (int(v.numel() if torch.is_tensor(v) else v.size), item[k]) for k, v in arrays.items()}, budget)
    manifest = {}
    for name, v in arrays.items():
        n = int(v.numel() if torch.is_tensor(v) else v.size)
        idx = sample_index(name, n, plan[name])
        flat = v.detach().reshape(-1) if torch.is_tensor(v) else np.asarray(v).reshape(-1)
        if idx is not None:
            flat = flat[torch.from_numpy(idx).to(flat.device)] if torch.is_tensor(flat) else flat[idx]
        if torch.is_tensor(flat):
            flat = flat.cpu().numpy()
        out = flat.astype(np.float64 if item[name] == 8 else np.float32)
        np.save(os.path.join(directory, name + ".npy"), out if idx is not None else out.reshape(tuple(v.shape)))
        manifest[name] = {"shape": list(v.shape), "dtype": str(out.dtype), "written": int(out.size),
                          "sampled": None if idx is None else f"sorted distinct flat indices, common.sample_index({name!r}, {n}, {plan[name]})"}
    return manifest


def _emit(obj):
    """Print the result as the LAST line of stdout: text that native libraries (RCCL) left in the C stdio buffer is
    flushed first, otherwise it would come out at process exit, after the JSON line."""
    try:
        C.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    print(json.dumps(obj), flush=True)
