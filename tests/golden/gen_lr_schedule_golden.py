"""Generates tests/golden/lr_schedule_golden.npz by IMPORTING the reference's own ``get_expon_lr_func`` / ``get_cosine_annealing_lr``
(sings/rec/utils/general.py:76-126, read-only at /root/reference) in the build container; only inputs and outputs ship.

    python tests/golden/gen_lr_schedule_golden.py

The module imports loguru, omegaconf and PIL at its top for functions that are not used here: whichever is absent is stubbed.
The cases are the schedules ``setup_optimizer`` builds (sings_hybrid.py:785-809) with the numbers of defaults/config.py:62-84, plus an
exponential one with a delay (the reference's default passes none), on steps 0 .. 30 000 every 250 plus the edges and the delay
boundaries.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

for name, attrs in (("loguru", ("logger",)), ("omegaconf", ("OmegaConf",)), ("PIL", ("Image", "ImageDraw", "ImageFont"))):
    try:
        importlib.import_module(name)
    except ImportError:
        stub = types.ModuleType(name)
        for a in attrs:
            setattr(stub, a, types.SimpleNamespace())
        sys.modules[name] = stub
spec = importlib.util.spec_from_file_location("ref_general", os.path.join(REF, "sings/rec/utils/general.py"))
gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)

# defaults/config.py:62-84
position_init, position_final, position_delay_mult, position_max_steps, smpl_spatial = 0.00016, 0.0000016, 0.01, 30_000, 2.0
vembed = geometry = appearance = 1e-3
mlp_max_steps = 16000

steps = sorted(set(range(0, 30001, 250)) | {-1, 0, 1, 999, 1000, 1001, 7999, 8000, 8001, 15999, 16000, 16001, 29999, 30000, 30001, 40000})
out = {"steps": np.array(steps, np.int64)}
# columns of *_params: lr_init, lr_final, lr_delay_steps, lr_delay_mult, max_steps
expon = {"xyz": (position_init * smpl_spatial, position_final * smpl_spatial, 0, position_delay_mult, position_max_steps),
         "xyz_delayed": (position_init * smpl_spatial, position_final * smpl_spatial, 1000, position_delay_mult, position_max_steps)}
for name, (a, b, ds, dm, ms) in expon.items():
    fn = gen.get_expon_lr_func(lr_init=a, lr_final=b, lr_delay_steps=ds, lr_delay_mult=dm, max_steps=ms)
    out[f"expon_{name}_params"] = np.array([a, b, ds, dm, ms], np.float64)
    out[f"expon_{name}_lr"] = np.array([float(fn(s)) for s in steps], np.float64)
# columns of *_params: lr_init, lr_final, lr_delay_steps, T_max
cosine = {"v_embed": (vembed, vembed / 5., 0, mlp_max_steps), "geometry": (geometry, geometry / 5., mlp_max_steps // 2, mlp_max_steps),
          "appearance": (appearance, appearance / 5., mlp_max_steps // 2, mlp_max_steps)}
for name, (a, b, ds, tm) in cosine.items():
    fn = gen.get_cosine_annealing_lr(lr_init=a, lr_final=b, lr_delay_steps=ds, T_max=tm)
    out[f"cosine_{name}_params"] = np.array([a, b, ds, tm], np.float64)
    out[f"cosine_{name}_lr"] = np.array([float(fn(s)) for s in steps], np.float64)

dst = os.path.join(ROOT, "tests", "golden", "lr_schedule_golden.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst), "bytes", {k: v.shape for k, v in out.items()})
