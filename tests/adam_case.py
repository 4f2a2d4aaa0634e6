"""The contract of the fused Adam step (include/sings_hip.h, sg_adam_step) restated in numpy, generic in dtype, and the input recipe
its tests share: gradients over fourteen decades, exact zeros, a band whose second moment is an fp32 denormal, a learning rate
that changes every step."""
import math

import numpy as np

STEPS = 60
LRS = (1.6e-4, 1e-3, 5e-4, 2.5e-3)            # the rate of step t (1-based) of group k is LRS[(t - 1 + k) % 4]
BETAS, EPS = (0.9, 0.999), 1e-15


def lr_of(step, group=0):
    return LRS[(step - 1 + group) % 4]


def row(lr, step, dtype, betas=BETAS, eps=EPS):
    """The six multipliers of a group at step ``step`` (1-based): double formulas, rounded once to ``dtype``."""
    b1, b2 = betas
    return np.array([1.0 - b1, b2, 1.0 - b2, math.sqrt(1.0 - b2 ** step), eps, -(lr / (1.0 - b1 ** step))], np.float64).astype(dtype)


def adam_update(p, m, v, g, h):
    """One step in the dtype of the arrays (all of ONE dtype, ``h`` = ``row(..)`` of the same): every operation rounds once, in this
    order.  -> (p', m', v')."""
    w1, b2, w2, c2, eps, neg_step = h
    assert p.dtype == m.dtype == v.dtype == g.dtype == h.dtype
    with np.errstate(all="ignore"):
        m = m + (g - m) * w1
        v = v * b2 + (w2 * g) * g
        d = np.sqrt(v) / c2 + eps
        p = p + (neg_step * m) / d
    assert p.dtype == h.dtype and m.dtype == h.dtype and v.dtype == h.dtype
    return p, m, v


class Recipe:
    """n elements: a fixed per-element gradient scale 10**U(-12, 2); every 17th element's gradient exactly zero at every step; a band
    (elements n//3 .. n//3 + max(8, n//16)) with |g| around 1e-20, so that (1 - beta2) g^2 ~ 1e-43 is an fp32 denormal."""

    def __init__(self, n, seed=0):
        self.n, self.seed = int(n), int(seed)
        rng = np.random.default_rng([self.seed, 0])
        self.scale = 10.0 ** rng.uniform(-12.0, 2.0, self.n)
        b0 = self.n // 3
        self.band = slice(b0, min(self.n, b0 + max(8, self.n // 16)))
        self.scale[self.band] = 1e-20
        self.zero = np.arange(self.n) % 17 == 0
        self.p0 = rng.normal(0.0, 1.0, self.n)

    def gradient(self, step, dtype):
        """The gradient of step ``step`` (1-based), float64 values rounded once to ``dtype``."""
        g = self.scale * np.random.default_rng([self.seed, step]).standard_normal(self.n)
        g[self.zero] = 0.0
        return g.astype(dtype)


class Reference:
    """The restatement run over flat arrays; ``bounds``: [(start, stop)] of group 0, 1, ... (one range of elements per group, whose
    learning rate differs), default one group."""

    def __init__(self, p0, dtype, bounds=None):
        self.dtype = np.dtype(dtype)
        self.p = np.asarray(p0).astype(self.dtype)
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.bounds = [(0, self.p.size)] if bounds is None else list(bounds)
        self.t = 0

    def step(self, g, lrs=None):
        """``lrs``: the learning rate per group of this step (default: ``lr_of``)."""
        self.t += 1
        for k, (a, b) in enumerate(self.bounds):
            lr = lr_of(self.t, k) if lrs is None else lrs[k]
            self.p[a:b], self.m[a:b], self.v[a:b] = adam_update(self.p[a:b], self.m[a:b], self.v[a:b], g[a:b], row(lr, self.t, self.dtype))


def same_bits(a, b):
    """Bit equality of two fp32 arrays of one shape (NaNs of one payload equal, +0 and -0 differ)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
