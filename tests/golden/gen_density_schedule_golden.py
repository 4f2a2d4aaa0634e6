"""Golden event lists for ``sings_amd.density.HybridDensitySchedule``: the REFERENCE's own ``GaussianTrainer._adjust_density``
(sings/rec/trainer/gs_trainer.py:280-325) executed on the CPU.  The method's source is cut out of the file at generation time and
exec'd as a plain function (nothing of it is stored); ``self`` is a stub whose ``densify_or_prune_hybrid`` records ``(t, mode)``
instead of touching a model, the render package and the model output are stubs that answer the few attribute reads the method makes.
Only the recorded lists and the final ``densify_interval`` are written.

    python tests/golden/gen_density_schedule_golden.py <path to the reference checkout>

The three configurations (``from`` / ``until`` / ``interval``):

    human_male   the ``density_control.hybrid`` block of sings/rec/cfgs/train/beta/human_male.yaml -- prune 1998 / 6000 / 2000, densify
                 3999 / 10000 / 1500 -- over the 8 999 iterations t = 0 .. 8998
    defaults     sings/rec/defaults/config.py:119-128 -- prune 1999 / 12000 / 2000, densify 1999 / 12000 / 2000 -- over its
                 ``num_steps`` = 30 000
    compressed   prune 3 / 12 / 4, densify 5 / 14 / 3 over 16: every branch of the rule (a first densification at ``from``, a prune and a
                 densification on one iteration, the longer interval behind it, both windows closing) inside a test-sized run
"""
import json
import os
import re
import sys
import textwrap
import types

HERE = os.path.dirname(os.path.abspath(__file__))

CONFIGS = {
    "human_male": dict(steps=8999, prune_from_iter=1998, prune_until_iter=6000, prune_interval=2000, densify_from_iter=3999,
                       densify_until_iter=10000, densify_interval=1500),
    "defaults": dict(steps=30000, prune_from_iter=1999, prune_until_iter=12000, prune_interval=2000, densify_from_iter=1999,
                     densify_until_iter=12000, densify_interval=2000),
    "compressed": dict(steps=16, prune_from_iter=3, prune_until_iter=12, prune_interval=4, densify_from_iter=5, densify_until_iter=14,
                       densify_interval=3),
}


def _adjust_density_of(reference_root):
    src = open(os.path.join(reference_root, "sings", "rec", "trainer", "gs_trainer.py")).read()
    m = re.search(r"^    def _adjust_density\(self.*?(?=^    def )", src, flags=re.S | re.M)
    assert m, "gs_trainer.py has no _adjust_density"
    scope = {"torch": types.SimpleNamespace(no_grad=_NoGrad), "print": lambda *a, **k: None}
    exec(compile(textwrap.dedent(m.group(0)), "gs_trainer.py:_adjust_density", "exec"), scope)
    return scope["_adjust_density"]


class _NoGrad:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class _Points:                                                   # render_pkg['viewspace_points']: sliced, and its .grad sliced
    grad = None

    def __getitem__(self, _):
        return _Points()


_Points.grad = _Points()


def run(adjust, cfg):
    hybrid = types.SimpleNamespace(**{k: v for k, v in cfg.items() if k != "steps"})
    events = []
    stub = types.SimpleNamespace(
        cfg=types.SimpleNamespace(human=types.SimpleNamespace(density_control=types.SimpleNamespace(strategy="hybrid", hybrid=hybrid))),
        densify_or_prune_hybrid=lambda mode, **kw: events.append([t, mode]))
    out = {"xyz": types.SimpleNamespace(shape=(4,))}
    for t in range(cfg["steps"]):
        pkg = {"viewspace_points": _Points(), "human_visibility_filter": None, "human_radii": None}
        adjust(stub, t, pkg, out)
    return {"config": cfg, "events": events, "densify_interval": hybrid.densify_interval}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    adjust = _adjust_density_of(sys.argv[1])
    golden = {name: run(adjust, dict(cfg)) for name, cfg in CONFIGS.items()}
    with open(os.path.join(HERE, "density_schedule_golden.json"), "w") as f:
        json.dump(golden, f, indent=1)
        f.write("\n")
    for name, g in golden.items():
        print(name, g["events"], "densify_interval", g["densify_interval"])
