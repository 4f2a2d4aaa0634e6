"""sings_amd.decode after its split (grad_arena, side_launch, triplane, linear_layers): every public name callers import from
``sings_amd.decode`` is still there, as the SAME object as in its home module; and the gradient arena is plain torch -- it imports and
runs on host tensors where no HIP library exists.  No GPU, no library."""
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what benchkit/, tests/, tools/ and INTEGRATION.md import from sings_amd.decode, by home module
EXPORTS = {
    "sings_amd.grad_arena": ["set_gradient_arena", "invalidate_gradient_arena", "arena_sync"],
    "sings_amd.side_launch": ["overlap_weight_grads", "prepare_triplane_backward_early", "prepare_triplane_backward_late",
                              "flush_triplane_prepare", "reset_deferred"],
    "sings_amd.triplane": ["HexPlaneField", "init_grid_param", "triplane_features_nograd"],
    "sings_amd.linear_layers": ["ACT_NONE", "ACT_GELU", "ACT_SIGMOID", "ACT_SOFTPLUS_REF", "linear_act", "linear_act_shared",
                                "linear_fan", "fuse_fan_backward"],
    "sings_amd.decode": ["AppearanceDecoder", "GeometryDecoder", "decode_attributes", "decode_frozen", "frozen_geometry",
                         "frozen_appearance"],
}


_ARENA_SCRIPT = r"""
import os, sys
sys.path.insert(0, %r)
assert not os.path.exists(os.environ["SINGS_HIP_LIB"])
import torch
from sings_amd import grad_arena as ga
assert "sings_amd._lib" not in sys.modules and "sings_amd.decode" not in sys.modules
assert ga.arena_registration() == ({}, None)
a, b = torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(5))
flat = torch.zeros(17)
views = ga.set_gradient_arena([a, b], flat)
slots, params = ga.arena_registration()
assert sorted(slots) == sorted([a.data_ptr(), b.data_ptr()]) and [r() for r in params] == [a, b]
slots.clear()                                                   # a copy: the registration is not the caller's to change
assert len(ga.arena_registration()[0]) == 2
a.grad, b.grad = torch.ones(4, 3), torch.full((5,), 2.0)
assert ga.arena_sync([a, b], views, True) == 2
assert torch.equal(flat, torch.cat([torch.ones(12), torch.full((5,), 2.0)]))
flat.mul_(0.5)
assert ga.arena_sync([a, b], views, False) == 2 and float(a.grad.sum()) == 6.0 and float(b.grad.sum()) == 5.0
g = ga.arena_out(b)                                             # b.grad is set: not the slot
assert g.data_ptr() != views[1].data_ptr()
b.grad = None
g = ga.arena_out(b)
assert g.data_ptr() == views[1].data_ptr() and g.shape == b.shape
assert ga.set_gradient_arena(None, None) == [] and ga.arena_registration() == ({}, None)
assert "sings_amd._lib" not in sys.modules
print("arena ok")
"""


def test_decode_keeps_its_exports_and_the_gradient_arena_needs_no_library(tmp_path):
    from sings_amd import decode
    for home, names in EXPORTS.items():
        mod = importlib.import_module(home)
        for name in names:
            obj = getattr(decode, name)
            assert obj is getattr(mod, name), (home, name)
            if callable(obj):
                assert obj.__module__ == home, (name, obj.__module__)      # defined there, not merely passed through
    assert (decode.ACT_NONE, decode.ACT_GELU, decode.ACT_SIGMOID, decode.ACT_SOFTPLUS_REF) == (0, 1, 2, 3)
    # the arena, in a child process whose SINGS_HIP_LIB names a file that does not exist
    env = dict(os.environ, SINGS_HIP_LIB=str(tmp_path / "no_such_dir" / "libsings_hip.so"))
    p = subprocess.run([sys.executable, "-c", _ARENA_SCRIPT % ROOT], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "arena ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
