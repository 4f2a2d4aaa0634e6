"""CPU tests of the fused Adam step's host side (sings_amd/optim.py, sg_adam_step): the two learning-rate schedules against the
reference's own (tests/golden/lr_schedule_golden.npz), the fp64 restatement of the contract (tests/adam_case.py) against
``torch.optim.Adam``, the segment / chunk tables, the per-group row, and what is refused without a launch."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest
import torch

import adam_case as ac


def _golden(repo_root):
    return np.load(os.path.join(repo_root, "tests", "golden", "lr_schedule_golden.npz"))


def test_schedules_reproduce_the_reference(repo_root):
    """Double-precision host arithmetic on both sides: 1e-12 relative."""
    from sings_amd.optim import cosine_annealing_lr, expon_lr
    g = _golden(repo_root)
    steps = [int(s) for s in g["steps"]]
    assert -1 in steps and 0 in steps and 30000 in steps and 8000 in steps and 7999 in steps and len(steps) > 120
    n = 0
    for key in g.files:
        if not key.endswith("_params"):
            continue
        kind, want = key.split("_")[0], g[key[:-len("_params")] + "_lr"]
        q = g[key]
        if kind == "expon":
            fn = expon_lr(q[0], q[1], lr_delay_steps=int(q[2]), lr_delay_mult=q[3], max_steps=int(q[4]))
        else:
            fn = cosine_annealing_lr(q[0], q[1], int(q[2]), int(q[3]))
        got = np.array([fn(s) for s in steps], np.float64)
        err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        err[(got == 0) & (want == 0)] = 0
        print(f"{key[:-7]}: max rel {err.max():.2e}")
        assert err.max() <= 1e-12, (key, steps[int(err.argmax())], err.max())
        n += 1
    assert n == 5
    assert expon_lr(0.0, 0.0)(10) == 0.0 and expon_lr(1e-3, 1e-5)(-1) == 0.0
    assert expon_lr(1e-3, 1e-5)(5) == expon_lr(1e-3, 1e-5, 0, 1.0, 1000000)(5)            # the reference's defaults


def test_fp64_restatement_is_torch_adam():
    """The four lines of the contract in fp64 against ``torch.optim.Adam(foreach=False)`` in fp64 on the recipe (60 steps, the rate
    changing every step): parameters within 1e-13 absolute, exp_avg within 1e-13 of max|g| per element, exp_avg_sq within 1e-13
    relative, zero-gradient elements bit-identical to their start."""
    n = 20000
    rec = ac.Recipe(n, seed=3)
    ref = ac.Reference(rec.p0, np.float64)
    p = torch.from_numpy(rec.p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1.0, betas=ac.BETAS, eps=ac.EPS, foreach=False)
    gmax = np.zeros(n)
    worst = [0.0, 0.0, 0.0]
    for t in range(1, ac.STEPS + 1):
        g = rec.gradient(t, np.float64)
        gmax = np.maximum(gmax, np.abs(g))
        opt.param_groups[0]["lr"] = ac.lr_of(t)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        ref.step(g)
        st = opt.state[p]
        ep = np.abs(p.detach().numpy() - ref.p).max()
        em = (np.abs(st["exp_avg"].numpy() - ref.m) / np.maximum(gmax, 1e-300)).max()
        v = st["exp_avg_sq"].numpy()
        ev = (np.abs(v - ref.v) / np.maximum(np.abs(ref.v), 1e-300))[ref.v != 0].max()
        worst = [max(a, b) for a, b in zip(worst, (ep, em, ev))]
        assert np.array_equal(v == 0, ref.v == 0)
    print(f"fp64 restatement vs torch.optim.Adam: param {worst[0]:.1e} abs, exp_avg {worst[1]:.1e} of max|g|, exp_avg_sq {worst[2]:.1e} rel")
    assert worst[0] <= 1e-13 and worst[1] <= 1e-13 and worst[2] <= 1e-13
    z = rec.zero
    assert z.sum() > n // 18
    assert np.array_equal(ref.p[z].view(np.int64), rec.p0[z].view(np.int64)) and np.array_equal(p.detach().numpy()[z], rec.p0[z])
    assert not ref.m[z].any() and not ref.v[z].any()
    # the band exists and is what it is for: (1 - beta2) g^2 is an fp32 denormal there
    gb = np.abs(rec.gradient(1, np.float32)[rec.band]); gb = gb[gb > 0]
    assert gb.size and (1e-3 * gb.astype(np.float64) ** 2 < np.finfo(np.float32).tiny).all()


def _covered(seg, chunks, chunk):
    """Element counts per segment from the chunk table: every element must be counted exactly once."""
    hits = [np.zeros(int(n), np.int32) for n in seg[:, 2]]
    for s, first in chunks:
        n = int(seg[s, 2])
        assert 0 <= first < n and first % chunk == 0
        hits[s][first:min(first + chunk, n)] += 1
    return hits


@pytest.mark.parametrize("numels", [[1], [3], [4095], [4097], [4096], [1, 3, 4095, 4097, 2, 8192, 7, 12289, 64, 5],
                                    [64, 0, 3]])
def test_tables_cover_every_element_exactly_once(numels):
    from sings_amd import _lib
    from sings_amd.optim import build_tables
    chunk = int(_lib.load().sg_adam_chunk_elements())
    assert chunk == 4096
    addresses = [0x10000 + 0x100000 * i + 4 * (i % 4) for i in range(len(numels))]
    groups = [i % 3 for i in range(len(numels))]
    seg, chunks = build_tables(addresses, numels, groups)
    assert seg.dtype == np.int64 and seg.shape == (len(numels), 4) and chunks.dtype == np.int32 and chunks.shape[1] == 2
    assert list(seg[:, 0]) == addresses and list(seg[:, 2]) == numels and list(seg[:, 3]) == groups
    assert list(seg[:, 1]) == [sum(numels[:i]) for i in range(len(numels))]           # arena offsets are sum(numel)
    for h in _covered(seg, chunks, chunk):
        assert (h == 1).all()
    assert len(chunks) == sum((n + chunk - 1) // chunk for n in numels)
    with pytest.raises(ValueError):
        build_tables([0x1000], [2 ** 31], [0])


def test_hyper_row_is_the_double_formulas_rounded_once():
    from sings_amd.optim import HYPER_COLUMNS, hyper_row
    for lr, b1, b2, eps, t in ((1e-3, 0.9, 0.999, 1e-15, 1), (3.2e-4, 0.9, 0.999, 1e-15, 7), (2e-3, 0.8, 0.99, 1e-8, 12345),
                               (1.6e-6, 0.9, 0.999, 1e-15, 30000)):
        r = hyper_row(lr, b1, b2, eps, t)
        assert r.dtype == np.float32 and r.shape == (HYPER_COLUMNS,)
        want = [1.0 - b1, b2, 1.0 - b2, math.sqrt(1.0 - b2 ** t), eps, -(lr / (1.0 - b1 ** t)), 0.0, 0.0]
        assert [float(x) for x in r] == [float(np.float32(w)) for w in want]
        assert np.array_equal(r[:6], ac.row(lr, t, np.float32, (b1, b2), eps))


def test_sg_adam_step_refuses_bad_arguments_without_launching():
    from sings_amd import _lib
    lib = _lib.load()
    assert "sg_adam_step" in _lib.EXPORTS and "sg_adam_chunk_elements" in _lib.EXPORTS and _lib.ABI_VERSION == 8
    a, b, c, d = (C.c_void_p(0x1000 * k) for k in (1, 2, 3, 4))                       # never dereferenced
    ok = dict(n_segments=1, n_chunks=1, n_groups=1, segments=a, chunks=a, hyper=a, grad=b, m=c, v=d)

    def call(**kw):
        q = dict(ok, **kw)
        return lib.sg_adam_step(q["n_segments"], q["n_chunks"], q["n_groups"], q["segments"], q["chunks"], q["hyper"], q["grad"], q["m"],
                                q["v"], None)
    for name in ("segments", "chunks", "hyper", "grad", "m", "v"):
        assert call(**{name: None}) != 0
        assert "sg_adam_step: null pointer" in lib.sg_last_error().decode()
    for kw in (dict(n_segments=-1), dict(n_chunks=-1), dict(n_groups=0), dict(n_segments=0)):
        assert call(**kw) != 0
        assert "sg_adam_step" in lib.sg_last_error().decode() and ">= 0" in lib.sg_last_error().decode()
    assert call(grad=C.c_void_p(0x2004)) != 0 and "16-byte aligned" in lib.sg_last_error().decode()
    assert call(m=b) != 0 and "three buffers" in lib.sg_last_error().decode()
    assert call(n_chunks=0) == 0                                                       # nothing to do: nothing launched


def test_fused_adam_has_no_cpu_fallback():
    from sings_amd._marshal import adam_step
    from sings_amd.optim import FusedAdam
    p = torch.zeros(8, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedAdam([{"params": [p], "lr": 1e-3, "name": "w"}], torch.zeros(8), [torch.zeros(8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        adam_step(torch.zeros((1, 4), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 8)),
                  torch.zeros(8), torch.zeros(8), torch.zeros(8))


def test_trainer_defaults_keep_todays_behaviour():
    from sings_amd.train_loop import AvatarTrainer
    sig = inspect.signature(AvatarTrainer.__init__).parameters
    assert sig["optimizer"].default == "torch" and sig["lr_schedules"].default is None
    assert sig["fp"].default is None and sig["use_graph"].default is False
