"""The hybrid density schedule of ``GaussianTrainer`` and the statistics its decisions read (include/sings_density.h,
csrc/sg_density.hip).

``HybridDensitySchedule`` is the rule of gs_trainer.py:280-325 -- WHEN the set of Gaussians is pruned (``prune_and_simplify``) and
densified (``densify_and_subdivide``) -- with the two smaller rules that hang on the same iteration counter: which attributes the L2
term reads (gs_trainer.py:356-360) and when the SH degree goes up (:457-458).  It is plain Python: no tensor, no device.

``densify_stats`` is the reference's statistics update (gs_trainer.py:486-492, sings_hybrid.py:1013-1015) as one launch behind a gate
in device memory; ``densify_stats_host`` is the same rule in numpy fp64, the definition the kernel is held to.

The rule of the statistics, per Gaussian i, over the K frames of a step in ascending order: a frame with ``radii[k, i] > 0`` adds
``sqrt(gx^2 + gy^2)`` of ``grad[k, i, :2]`` to ``accum[i]`` and 1 to ``denom[i]`` and raises ``max_radii[i]`` to ``radii[k, i]``; a frame
with ``radii <= 0`` is skipped -- its gradient is not read, so a NaN there changes nothing (boolean indexing in the reference; a
multiplication by a zero mask would write the NaN).  The third column of ``grad`` is never read.
"""
import numpy as np

L2_KEYS_OPEN = ("xyz_offsets", "scales")                         # while a density window is open (gs_trainer.py:360)
L2_KEYS_ALL = ("xyz_offsets", "scales", "opacity")               # once both have closed (:358)


# ---- the statistics ---------------------------------------------------------------------------------------------------------------
def densify_stats(grad, radii, accum, denom, max_radii, gate=None):
    """``sg_density_stats``: the statistics of one step into ``accum`` / ``denom`` / ``max_radii`` ([N] or [N,1] fp32, in place).
    ``grad`` [N,3] or [K,N,3] fp32 (``viewspace_points.grad``), ``radii`` [N] or [K,N] int32.  ``gate``: an int32 device tensor [1] --
    at 0 the launch changes nothing -- or None: always accumulate.  One launch on torch's current stream, no host read, no
    allocation: legal under capture.  GPU tensors only (no CPU fallback: ``densify_stats_host`` is the numpy rule)."""
    from ._marshal import density_stats
    density_stats(grad, radii, gate, accum, denom, max_radii)


def densify_stats_host(grad, radii, accum, denom, max_radii, gate=None):
    """The rule in numpy fp64 -> (accum, denom, max_radii) as new float64 arrays of the inputs' shapes (the inputs are not written).
    ``gate``: None, or anything whose first element is the gate word."""
    g = np.asarray(grad)
    g = g.reshape((-1,) + g.shape[-2:])
    K, N = g.shape[0], g.shape[1]
    r = np.asarray(radii).reshape(K, N)
    out = [np.array(a, dtype=np.float64) for a in (accum, denom, max_radii)]
    if gate is not None and int(np.asarray(gate).reshape(-1)[0]) == 0:
        return tuple(out)
    a, d, m = (o.reshape(-1) for o in out)                       # (views: the results keep the inputs' shapes)
    total = np.zeros(N, np.float64)
    for k in range(K):
        vis = r[k] > 0
        gx, gy = g[k, vis, 0].astype(np.float64), g[k, vis, 1].astype(np.float64)
        total[vis] += np.sqrt(gx * gx + gy * gy)
        d[vis] += 1.0
        m[vis] = np.maximum(m[vis], r[k, vis].astype(np.float64))
    seen = (r > 0).any(0)
    a[seen] += total[seen]
    return tuple(out)


# ---- the schedule -----------------------------------------------------------------------------------------------------------------
class HybridDensitySchedule:
    """``cfg.human.density_control.hybrid`` with the reference's names, the thresholds its two calls take
    (gs_trainer.py:495-510: ``min_n_gaussians`` / ``max_n_gaussians`` are ``cfg.human.density_control``'s) and ``sh_up_every`` (the
    literal 1000 of gs_trainer.py:457).

    ``actions(t)`` -> a tuple of ``"prune"`` / ``"densify"`` in the order the reference takes them: gs_trainer.py:280-325 as written.

        prune     ``prune_from_iter <= t < prune_until_iter`` and ``(t - prune_from_iter) % prune_interval == 0``
        densify   ``densify_from_iter <= t < densify_until_iter`` and ``(t - densify_from_iter - densify_interval) % densify_interval
                  == 0`` -- so the first densification is at ``densify_from_iter`` itself
        both      ``densify_interval`` goes up by one AND the densification still runs: the reference prints "will not densify
                  right after prunning" and then densifies.  The later densifications follow the new interval.

    The object is therefore stateful: ``actions`` must be called once per iteration with ``t`` going up (``ValueError`` otherwise;
    iterations may be left out only where nothing was due -- the trainer leaves none out).  ``decides_at(t)`` is the same test without
    the state change: what the trainer asks BEFORE step ``t`` to open the statistics' gate.  ``densify_interval`` is the current value;
    ``state_dict()`` / ``load_state_dict()`` carry it and the last ``t`` seen.

    ``l2_keys(t)``: the attributes ``L2Norm`` reads at iteration ``t`` -- without ``opacity`` until ``t >= prune_until_iter and t >=
    densify_until_iter`` (gs_trainer.py:356-360).  ``sh_up(t)``: ``t % sh_up_every == 0 and t > 0`` (:457-458).

    One deviation, in the trainer that applies the schedule: on an iteration with a prune AND a densification the reference
    accumulates the statistics a second time, with the pre-prune visibility mask on the post-prune arrays (which raises as soon as the
    prune removed anything).  ``AvatarTrainer`` accumulates once per iteration; the densification decides on the statistics the prune
    kept."""

    def __init__(self, prune_from_iter, prune_until_iter, prune_interval, densify_from_iter, densify_until_iter, densify_interval,
                 prune_opacity_threshold=0.005, prune_scale_threshold=0.0005, prune_max_n_gs_once=5000, min_n_gaussians=100000,
                 densify_grad_threshold=0.001, densify_scale_threshold=0.01, densify_render_size_threshold=20,
                 max_n_gaussians=200000, sh_up_every=1000):
        self.prune_from_iter, self.prune_until_iter = int(prune_from_iter), int(prune_until_iter)
        self.densify_from_iter, self.densify_until_iter = int(densify_from_iter), int(densify_until_iter)
        self.prune_interval, self.densify_interval = int(prune_interval), int(densify_interval)
        if self.prune_interval < 1 or self.densify_interval < 1 or int(sh_up_every) < 1:
            raise ValueError("HybridDensitySchedule: prune_interval, densify_interval and sh_up_every must be positive")
        self.prune_opacity_threshold, self.prune_scale_threshold = prune_opacity_threshold, prune_scale_threshold
        self.prune_max_n_gs_once, self.min_n_gaussians = prune_max_n_gs_once, min_n_gaussians
        self.densify_grad_threshold, self.densify_scale_threshold = densify_grad_threshold, densify_scale_threshold
        self.densify_render_size_threshold, self.max_n_gaussians = densify_render_size_threshold, max_n_gaussians
        self.sh_up_every = int(sh_up_every)
        self._last_t = None

    def _due(self, t):
        """(prune, densify) of iteration ``t`` under the current ``densify_interval``."""
        prune = self.prune_from_iter <= t < self.prune_until_iter and (t - self.prune_from_iter) % self.prune_interval == 0
        densify = (self.densify_from_iter <= t < self.densify_until_iter
                   and (t - self.densify_from_iter - self.densify_interval) % self.densify_interval == 0)
        return prune, densify

    def decides_at(self, t):
        return any(self._due(int(t)))

    def actions(self, t):
        t = int(t)
        if self._last_t is not None and t <= self._last_t:
            raise ValueError(f"HybridDensitySchedule.actions: t = {t} after t = {self._last_t} (once per iteration, t going up: the "
                             "densify interval changes on the way)")
        self._last_t = t
        prune, densify = self._due(t)
        if prune and densify:
            self.densify_interval += 1                           # "will not densify right after prunning" -- and then it does
        return (("prune",) if prune else ()) + (("densify",) if densify else ())

    def l2_keys(self, t):
        return L2_KEYS_ALL if t >= self.prune_until_iter and t >= self.densify_until_iter else L2_KEYS_OPEN

    def sh_up(self, t):
        return t % self.sh_up_every == 0 and t > 0

    def prune_kwargs(self):
        """The keyword arguments of ``AvatarTrainer.prune_and_simplify`` (gs_trainer.py:496-502)."""
        return dict(opacity_threshold=self.prune_opacity_threshold, scale_threshold=self.prune_scale_threshold,
                    prune_max_n_gs_once=self.prune_max_n_gs_once, min_n_gs=self.min_n_gaussians)

    def densify_kwargs(self):
        """The keyword arguments of ``AvatarTrainer.densify_and_subdivide`` (gs_trainer.py:504-510)."""
        return dict(grad_threshold=self.densify_grad_threshold, scale_threshold=self.densify_scale_threshold,
                    max_screen_size=self.densify_render_size_threshold, max_n_gs=self.max_n_gaussians)

    def state_dict(self):
        return {"densify_interval": self.densify_interval, "last_t": self._last_t}

    def load_state_dict(self, sd):
        self.densify_interval = int(sd["densify_interval"])
        self._last_t = None if sd["last_t"] is None else int(sd["last_t"])
