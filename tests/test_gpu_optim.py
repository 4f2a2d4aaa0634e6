"""The fused Adam step on the GPU (csrc/sg_optim.hip through sings_amd.optim.FusedAdam) against the fp32 restatement of its contract
(tests/adam_case.py): BIT equality after every step, whatever the segmentation; torch.optim.Adam's state format both ways; the
re-indexing of a densify; what it refuses; and a captured ``apply()`` replayed with a new learning rate every step."""
import copy

import numpy as np
import pytest
import torch

import adam_case as ac

pytestmark = pytest.mark.gpu

BIG = 2049 * 4096 + 5                      # more chunks than the launch has workgroups: the grid strides
# (group, kind, shape).  kind: "plain" a tensor of its own (256-B aligned); "plane" a feature-minor HexPlaneField plane; "match" a view
# whose pointer is misaligned by as many floats as its arena offset (head + quads + tail); "view" a view misaligned differently
SPEC = [(0, "plain", (BIG,)), (0, "plain", (1001, 3)),
        (1, "plane", (1, 32, 16, 16)), (1, "plain", (4097,)), (1, "match", (4097,)), (1, "plain", (4096,)),
        (2, "plain", (64, 64)), (2, "plain", (64,)), (2, "plain", (3, 64)), (2, "plain", (3,)), (2, "plain", (1,)), (2, "view", (4095,)),
        (3, "plain", (4095,)), (3, "plain", (4097,)), (3, "plain", (1,)), (3, "match", (8195,)), (3, "plain", (3,)), (3, "plain", (8192,))]
NAMES = ("xyz", "triplane", "geometry", "appearance")


def _small(spec, big=300001):
    return [(g, k, (big,) if s == (BIG,) else s) for g, k, s in spec]


class _Run:
    """Parameters built from a spec and a recipe, their arena, a FusedAdam.  The gradient arena is ONE global registration:
    ``step`` registers this run's before it applies, so that several runs can alternate."""

    def __init__(self, dev, spec, p0, n_groups=4, p_from=None):
        from sings_amd import decode
        from sings_amd.grad_arena import is_feature_minor
        from sings_amd.optim import FusedAdam
        self.dev, self.spec = dev, spec
        self.params, self.offsets, self.align = [], [], []
        groups = [{"params": [], "lr": 1e-3, "name": NAMES[k]} for k in range(n_groups)]
        o = 0
        for i, (gi, kind, shape) in enumerate(spec):
            n = int(np.prod(shape))
            vals = torch.from_numpy(np.asarray(p0[o:o + n], np.float32)).to(dev).view(shape)
            if kind == "plane":
                cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': shape[1], 'resolution': [shape[3]] * 3,
                       'multires': [1]}
                p = decode.HexPlaneField(cfg, device=dev, feature_minor=True).grids[0][0]
                assert tuple(p.shape) == tuple(shape) and is_feature_minor(p)
                with torch.no_grad():
                    p.copy_(vals)
            elif kind == "plain":
                p = vals.clone().requires_grad_(True)
            else:
                k = o % 4 if kind == "match" else ((o % 4 + 1) % 4 or 2)
                p = torch.zeros(n + 4, device=dev)[k:k + n].view(shape)
                p.copy_(vals)
                p = p.detach().requires_grad_(True)
            if p_from is not None:
                with torch.no_grad():
                    p.copy_(p_from[i])
            self.params.append(p); self.offsets.append(o)
            self.align.append(((p.data_ptr() // 4) % 4, o % 4, n))
            groups[min(gi, n_groups - 1)]["params"].append(p)
            o += n
        self.n = o
        self.bounds, a = [], 0
        for g in groups:
            b = a + sum(p.numel() for p in g["params"])
            self.bounds.append((a, b)); a = b
        self.flat = torch.zeros(o, device=dev)
        self.views = decode.set_gradient_arena(self.params, self.flat)
        self.opt = FusedAdam(groups, self.flat, self.views, betas=ac.BETAS, eps=ac.EPS)

    def set_grads(self, gflat):
        """``gflat``: a flat GPU tensor in the order of the spec (each parameter's elements in its logical order)."""
        for p, o in zip(self.params, self.offsets):
            p.grad = gflat[o:o + p.numel()].view(p.shape)

    def step(self, g, lrs):
        from sings_amd import decode
        decode.set_gradient_arena(self.params, self.flat)
        self.set_grads(torch.from_numpy(g).to(self.dev))
        for grp, lr in zip(self.opt.param_groups, lrs):
            grp["lr"] = lr
        self.opt.step()

    def flat_state(self):
        """(p, exp_avg, exp_avg_sq) as flat GPU tensors in the order of the spec, logical element order per parameter."""
        st = self.opt.state_dict()["state"]
        cat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs])
        return (cat(self.params), cat([st[i]["exp_avg"] for i in range(len(self.params))]),
                cat([st[i]["exp_avg_sq"] for i in range(len(self.params))]))


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _drop_arena():
    from sings_amd import decode
    decode.set_gradient_arena(None, None)


def test_sixty_steps_are_bit_identical_to_the_fp32_restatement():
    """Four groups, 18 segments (aligned, misaligned alike and misaligned differently; sizes 1 and 3; a feature-minor plane; 8.4 M
    elements in one), the denormal band inside: parameters and both moments after EVERY step, every element, no tolerance."""
    dev = torch.device("cuda:0")
    n = sum(int(np.prod(s)) for _, _, s in SPEC)
    rec = ac.Recipe(n, seed=1)
    try:
        run = _Run(dev, SPEC, rec.p0)
        assert len(run.opt.param_groups) == 4 and len(SPEC) >= 12
        kinds = {(ap == aa, ap != 0) for ap, aa, cnt in run.align if cnt >= 8}
        assert (True, False) in kinds and (True, True) in kinds and (False, False) in kinds and (False, True) in kinds, run.align
        assert run.align[0][:2] == (0, 0) and run.align[0][2] > 2048 * 4096              # the big segment takes the 16-byte path
        ref = ac.Reference(rec.p0, np.float32, bounds=run.bounds)
        assert ac.same_bits(run.flat_state()[0].cpu().numpy(), ref.p)
        denormal_seen = False
        for t in range(1, ac.STEPS + 1):
            g = rec.gradient(t, np.float32)
            run.step(g, [ac.lr_of(t, k) for k in range(4)])
            ref.step(g)
            assert run.opt.steps == [t] * 4
            for name, got, want in zip(("param", "exp_avg", "exp_avg_sq"), run.flat_state(), (ref.p, ref.m, ref.v)):
                got = got.cpu().numpy()
                if not ac.same_bits(got, want):
                    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
                    seg = int(np.searchsorted(run.offsets, bad[0], side="right")) - 1
                    pytest.fail(f"step {t}: {name} differs in {bad.size} of {n} elements, first at {bad[0]} (segment {seg} {SPEC[seg]}, "
                                f"alignment {run.align[seg]}): {got[bad[0]]!r} vs {want[bad[0]]!r}")
            vb = ref.v[rec.band]
            denormal_seen |= bool(((vb > 0) & (vb < np.finfo(np.float32).tiny)).any())
        assert denormal_seen, "the band's second moments are fp32 denormals"
        assert np.isfinite(ref.p).all() and not ref.m[rec.zero].any()
    finally:
        _drop_arena()


def test_one_segment_gives_the_same_bits():
    """The same elements as ONE parameter (one segment, one group) against the 17-segment, four-group set-up with every group at
    the same rate: chunking and alignment paths must not matter."""
    dev = torch.device("cuda:0")
    spec = [s for s in SPEC if s[1] != "plane"]                   # (one tensor has one memory order)
    n = sum(int(np.prod(s)) for _, _, s in spec)
    rec = ac.Recipe(n, seed=2)
    try:
        many = _Run(dev, spec, rec.p0)
        one = _Run(dev, [(0, "plain", (n,))], rec.p0, n_groups=1)
        for t in range(1, ac.STEPS + 1):
            g = rec.gradient(t, np.float32)
            many.step(g, [ac.lr_of(t)] * 4)
            one.step(g, [ac.lr_of(t)])
            for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), many.flat_state(), one.flat_state()):
                assert _bits_equal(a, b), (t, name, int((a.view(torch.int32) != b.view(torch.int32)).sum()))
    finally:
        _drop_arena()


def test_state_dict_round_trip_through_torch_adam():
    """FusedAdam -> torch.optim.Adam -> FusedAdam: bitwise the same state; the run that was loaded continues bit-identically to the
    uninterrupted one."""
    dev = torch.device("cuda:0")
    spec = _small(SPEC)
    n = sum(int(np.prod(s)) for _, _, s in spec)
    rec = ac.Recipe(n, seed=4)
    try:
        a = _Run(dev, spec, rec.p0)
        for t in range(1, 21):
            a.step(rec.gradient(t, np.float32), [ac.lr_of(t, k) for k in range(4)])
        sd = a.opt.state_dict()
        assert set(sd) == {"state", "param_groups"} and len(sd["state"]) == len(spec)
        assert all(float(s["step"]) == 20.0 for s in sd["state"].values())
        plane = [i for i, s in enumerate(spec) if s[1] == "plane"][0]
        assert sd["state"][plane]["exp_avg"].stride() == a.params[plane].stride()          # the parameter's own layout
        # into torch.optim.Adam over parameters of its own, and back out (a copy: torch adopts the dict's tensors and steps them in place)
        twins = [p.detach().clone().requires_grad_(True) for p in a.params]
        groups, k = [], 0
        for g in a.opt.param_groups:
            groups.append({"params": twins[k:k + len(g["params"])], "lr": 1.0, "name": g["name"]}); k += len(g["params"])
        adam = torch.optim.Adam(groups, betas=ac.BETAS, eps=ac.EPS)
        adam.load_state_dict(copy.deepcopy(sd))
        assert [g["lr"] for g in adam.param_groups] == [g["lr"] for g in a.opt.param_groups]
        for p in twins:
            p.grad = torch.zeros_like(p)
        adam.step()                                                                        # (torch accepts the loaded state: it steps)
        adam.load_state_dict(copy.deepcopy(sd))
        back = adam.state_dict()
        for i in range(len(spec)):
            assert float(back["state"][i]["step"]) == 20.0
            for key in ("exp_avg", "exp_avg_sq"):
                assert _bits_equal(back["state"][i][key], sd["state"][i][key]), (i, key)
        # a second FusedAdam over copies of the parameters takes torch's dict and continues
        b = _Run(dev, spec, rec.p0, p_from=[p.detach() for p in a.params])
        b.opt.load_state_dict(back)
        assert b.opt.steps == [20] * 4
        for x, y in zip(a.flat_state(), b.flat_state()):
            assert _bits_equal(x, y)
        for t in range(21, 41):
            g = rec.gradient(t, np.float32)
            lrs = [ac.lr_of(t, k) for k in range(4)]
            a.step(g, lrs); b.step(g, lrs)
            for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a.flat_state(), b.flat_state()):
                assert _bits_equal(x, y), (t, name)
        # ... and torch.optim.Adam's own dict of a run of its own loads too (state only for parameters that have stepped)
        fresh = torch.optim.Adam(groups, betas=ac.BETAS, eps=ac.EPS)
        b.opt.load_state_dict(fresh.state_dict())
        assert b.opt.steps == [0] * 4 and not b.opt.exp_avg.any() and not b.opt.exp_avg_sq.any()
    finally:
        _drop_arena()


def test_remap_rows_is_the_cat_keep_expression():
    from sings_amd import decode
    dev = torch.device("cuda:0")
    N = 1237
    spec = [(0, "plain", (N, 3)), (1, "plane", (1, 32, 16, 16)), (2, "plain", (64, 7)), (2, "plain", (7,)), (3, "plain", (5,))]
    n = sum(int(np.prod(s)) for _, _, s in spec)
    rec = ac.Recipe(n, seed=5)
    try:
        run = _Run(dev, spec, rec.p0)
        for t in range(1, 6):
            run.step(rec.gradient(t, np.float32), [ac.lr_of(t, k) for k in range(4)])
        before = run.opt.state_dict()["state"]
        gen = torch.Generator().manual_seed(9)
        clone = (torch.rand(N, generator=gen) < 0.1).to(dev)
        keep = (torch.rand(N + int(clone.sum()), generator=gen) > 0.05).to(dev)
        old = run.params[0]
        new = torch.cat([old.detach(), old.detach()[clone]])[keep].clone().requires_grad_(True)
        want = {k: torch.cat([before[0][k], torch.zeros_like(before[0][k][clone])])[keep] for k in ("exp_avg", "exp_avg_sq")}
        run.opt.remap_rows(old, new, clone, keep)
        assert run.opt.param_groups[0]["params"][0] is new and run.opt.steps == [5] * 4
        with pytest.raises(RuntimeError, match="stale"):
            run.opt.apply()                                                               # no arena for the new sizes yet
        params = [new] + run.params[1:]
        flat = torch.zeros(sum(p.numel() for p in params), device=dev)
        views = decode.set_gradient_arena(params, flat)
        run.opt.bind_arena(flat, views)
        after = run.opt.state_dict()["state"]
        assert int(new.shape[0]) != N and tuple(after[0]["exp_avg"].shape) == tuple(new.shape)
        for k in ("exp_avg", "exp_avg_sq"):
            assert _bits_equal(after[0][k], want[k]), k
            for i in range(1, len(spec)):
                assert _bits_equal(after[i][k], before[i][k]), (i, k)
        assert all(float(s["step"]) == 5.0 for s in after.values())
        # the next step runs on the new set: the contract, from the re-indexed moments
        g = (torch.randn(new.shape, generator=gen) * 1e-2).to(dev)
        p0 = new.detach().cpu().numpy().reshape(-1).copy()
        for p in params:
            p.grad = torch.zeros_like(p)
        new.grad = g
        run.opt.step()
        pw, mw, vw = ac.adam_update(p0, want["exp_avg"].cpu().numpy().reshape(-1), want["exp_avg_sq"].cpu().numpy().reshape(-1),
                                    g.cpu().numpy().reshape(-1), ac.row(run.opt.param_groups[0]["lr"], 6, np.float32))
        st = run.opt.state_dict()["state"][0]
        assert ac.same_bits(new.detach().cpu().numpy().reshape(-1), pw)
        assert ac.same_bits(st["exp_avg"].cpu().numpy().reshape(-1), mw) and ac.same_bits(st["exp_avg_sq"].cpu().numpy().reshape(-1), vw)
    finally:
        _drop_arena()


def test_stale_registration_and_missing_gradient_are_refused():
    dev = torch.device("cuda:0")
    spec = [(0, "plain", (50, 3)), (2, "plain", (8, 8)), (2, "plain", (8,))]
    rec = ac.Recipe(150 + 64 + 8, seed=6)
    try:
        run = _Run(dev, spec, rec.p0, n_groups=3)
        # a parameter that took no part in the backward: its arena slot would be stale
        run.set_grads(torch.zeros(run.n, device=dev))
        run.params[2].grad = None
        before = [p.detach().clone() for p in run.params]
        with pytest.raises(RuntimeError, match=r"geometry\[1\] has no gradient"):
            run.opt.step()
        torch.cuda.synchronize()
        assert all(_bits_equal(a, b.detach()) for a, b in zip(before, run.params)), "nothing was launched"
        run.step(rec.gradient(1, np.float32), [1e-3] * 3)
        # a registered parameter object replaced behind the optimiser's back
        run.opt.param_groups[0]["params"][0] = run.params[0].detach().clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="stale"):
            run.opt.apply()
    finally:
        _drop_arena()


def test_captured_apply_replays_with_a_new_rate_every_step():
    """``apply()`` captured with ``capture_step`` and replayed 10 times, ``advance()`` (and a new ``lr``) between the replays, against
    10 eager steps: bitwise."""
    from sings_amd import decode
    from sings_amd.train_step import capture_step
    dev = torch.device("cuda:0")
    spec = _small(SPEC, big=70001)
    n = sum(int(np.prod(s)) for _, _, s in spec)
    rec = ac.Recipe(n, seed=7)
    try:
        eager = _Run(dev, spec, rec.p0)
        graph = _Run(dev, spec, rec.p0)                              # (registered last: the capture's arena_sync sees its arena)
        gstat = torch.zeros(n, device=dev)
        graph.set_grads(gstat)                                       # the captured launch reads these addresses
        graph.opt.advance()                                          # a real row for the warm-up runs, then everything goes back
        keep = [x.clone() for x in [p.detach() for p in graph.params] + [graph.opt.exp_avg, graph.opt.exp_avg_sq]]
        steps = list(graph.opt.steps)

        def body():
            graph.opt.apply()
            return graph.opt.hyper.detach().clone()
        g, _ = capture_step(body, warmup=2, device=dev)
        for dst, src in zip([p.detach() for p in graph.params] + [graph.opt.exp_avg, graph.opt.exp_avg_sq], keep):
            dst.copy_(src)
        graph.opt.steps[:] = [s - 1 for s in steps]
        for t in range(1, 11):
            gt = rec.gradient(t, np.float32)
            lrs = [ac.lr_of(t, k) * (1 + 0.1 * t) for k in range(4)]
            eager.step(gt, lrs)
            gstat.copy_(torch.from_numpy(gt))
            for grp, lr in zip(graph.opt.param_groups, lrs):
                grp["lr"] = lr
            graph.opt.advance()
            g.replay()
            assert graph.opt.steps == [t] * 4
            for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), eager.flat_state(), graph.flat_state()):
                assert _bits_equal(x, y), (t, name)
        assert float(eager.flat_state()[1].abs().max()) > 0
    finally:
        decode.set_gradient_arena(None, None)
