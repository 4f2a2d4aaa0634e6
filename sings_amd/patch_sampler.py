"""The corners of the LPIPS patches, drawn on the device (include/sings_sampler.h, csrc/sg_sampler.hip).

``DevicePatchSampler`` stands where ``sings_amd.lpips.PatchSampler`` (utils/image/sampler.py) stands, with the mask left where it
lies: two launches, no copy to the host, no wait, and a counter in device memory that every call advances -- so ``origins(mask)`` may
sit inside a captured step, and every replay of that step draws fresh patches.  ``origins_host`` is the rule in numpy: the
definition the kernels are held to, integer for integer.

The rule.  Corners of frame ``k`` are a pure function of ``(mask_k, H, W, P, n, ratio_mask, seed, counter, k)``:

    o = P // 2; the crop is ``mask[o:H-o, o:W-o]``, ``Hc = H - P`` by ``Wc = W - P``; position q is row ``q // Wc``, column ``q % Wc``
    valid where ``mask > 0`` (NaN and negatives are not); M valid positions, ranked in row-major order (``np.where``'s)
    word(t) = word ``t % 4`` of Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)`` and counter
              ``(counter & 0xffffffff, counter >> 32, k, t // 4)``
    bounded(w, R) = ``(w * R) >> 32`` in 64 bits: a value in [0, R) whose bias is at most ``R / 2**32`` (below 2e-4 for a crop of
              a 1080p frame, against the 1 / M of a single pixel)
    masked branch, when ``word(0) < thr`` and ``M >= n``, ``thr = uint64(float64(float32(ratio_mask)) * 2**32)``: Floyd's subset
              sampling -- for i in 0..n-1: ``j = M - n + i``, ``t = bounded(word(1 + i), j + 1)``, ``t = j`` if t was chosen
              before; corner i = crop coordinates of the t-th valid position (indices into the CROP used as top-left corners
              in the full image, as in the reference: the patch is centred on the valid pixel)
    uniform branch: corner i = ``(bounded(word(1 + 2 i), H - P), bounded(word(2 + 2 i), W - P))``

Two deviations from the reference: the random stream (counter based; numpy's global stream cannot be drawn from on the device --
keep the host ``PatchSampler`` for a seeded parity run), and ``M < n`` in the masked branch: ``np.random.choice`` raises, the device
cannot, so the frame takes the uniform branch and is counted (``info[k, 1] == 2``, ``forced_uniform``).
"""
import numpy as np

from . import _lib

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32, _U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
BRANCH_MASKED, BRANCH_UNIFORM, BRANCH_FORCED = _lib.PATCH_BRANCH_MASKED, _lib.PATCH_BRANCH_UNIFORM, _lib.PATCH_BRANCH_FORCED


def philox4x32(counter, key):
    """Philox4x32-10: ``counter`` four and ``key`` two 32-bit words -> four 32-bit words (Random123's known answers hold)."""
    c0, c1, c2, c3 = (int(c) & _U32 for c in counter)
    k0, k1 = (int(k) & _U32 for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _U32, (p0 >> 32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return c0, c1, c2, c3


def threshold(ratio_mask):
    """``thr`` of the rule: 2**32 at 1.0 and above (always the masked branch), 0 at 0.0, below, and for a NaN."""
    r = float(np.float32(ratio_mask))
    return 1 << 32 if r >= 1.0 else int(r * 4294967296.0) if r > 0.0 else 0


def origins_host(mask, patch_size, num_patch, ratio_mask, seed, counter, frame=0):
    """The rule of this module's docstring in numpy -> ``(int32 [n,2] (row, col) corners, branch, M)``; ``mask`` [H,W] (or
    [1,H,W]), ``branch`` 0 masked / 1 uniform by the draw / 2 uniform because M < n."""
    m = np.asarray(mask)
    m = m.reshape(m.shape[-2], m.shape[-1])
    H, W = m.shape
    P, n = int(patch_size), int(num_patch)
    if P < 2 or P % 2 or H <= P or W <= P or not 1 <= n <= _lib.PATCH_MAX_N:
        raise ValueError("origins_host: an even patch size below H and W, and 1..%d patches" % _lib.PATCH_MAX_N)
    o, Wc = P // 2, W - P
    with np.errstate(invalid="ignore"):
        valid = np.flatnonzero(m[o:H - o, o:W - o] > 0)                           # row-major ranks -> crop positions
    M = int(valid.size)
    seed, counter = int(seed) & _U64, int(counter) & _U64
    key, blocks = (seed & _U32, seed >> 32), {}

    def word(t):
        if t // 4 not in blocks:
            blocks[t // 4] = philox4x32((counter & _U32, counter >> 32, int(frame), t // 4), key)
        return blocks[t // 4][t % 4]

    bounded = lambda w, R: (w * R) >> 32
    branch = BRANCH_UNIFORM if word(0) >= threshold(ratio_mask) else BRANCH_FORCED if M < n else BRANCH_MASKED
    if branch == BRANCH_MASKED:
        chosen = []
        for i in range(n):
            j = M - n + i
            t = bounded(word(1 + i), j + 1)
            chosen.append(j if t in chosen else t)
        q = valid[np.asarray(chosen, np.int64)]
        out = np.stack([q // Wc, q % Wc], 1)
    else:
        out = np.array([[bounded(word(1 + 2 * i), H - P), bounded(word(2 + 2 * i), W - P)] for i in range(n)])
    return out.astype(np.int32).reshape(n, 2), branch, M


class DevicePatchSampler:
    """``PatchSampler``'s arguments plus ``seed``.  ``origins(mask)`` -> device int32 [n,2] of (row, col) top-left corners for a
    mask [H,W] / [1,H,W], [K,n,2] for [K,H,W] (or for one mask and ``frames=K``: K draws from the same mask) -- in a tensor this
    object owns and reuses per shape (a stable address under capture); no host read, no allocation after the first call for a
    shape.  An fp32 contiguous mask is read in place; any other is converted on the device into a buffer kept per shape.

    ``info``: int32 [K,2] of the last call, (M, branch) per frame.  ``counter`` (the next call's) and ``forced_uniform`` (frames that
    took the uniform branch because M < n) read the device state: they synchronise -- for tests and checkpoints.
    ``state_dict()`` / ``load_state_dict()`` carry ``seed`` and ``counter``: a resumed run continues the patch sequence."""

    def __init__(self, num_patch=4, patch_size=20, ratio_mask=0.9, dilate=0, seed=0, device=None):
        import torch
        if patch_size % 2:
            raise ValueError("patch size has to be even")
        if dilate > 0:
            raise NotImplementedError("PatchSampler: dilate > 0 (cv2.dilate) is not provided; the reference's configs use 0")
        if not 1 <= int(num_patch) <= _lib.PATCH_MAX_N:
            raise ValueError(f"DevicePatchSampler: num_patch must be in 1..{_lib.PATCH_MAX_N}")
        self.n, self.patch_size, self.p, self.dilate = int(num_patch), int(patch_size), float(ratio_mask), dilate
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RuntimeError("DevicePatchSampler: the sampler lives on the GPU (no CPU fallback; origins_host is the numpy rule)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        seed = int(seed) & _U64
        self.state = torch.tensor([0, 0, seed - (1 << 64) if seed >> 63 else seed, 0], dtype=torch.int64, device=self.device)
        self._bufs, self.info, self.last_origins = {}, None, None

    # ---- the device state, read on the host
    def _word(self, i):
        return int(self.state[i].item()) & _U64

    seed = property(lambda self: self._word(2))
    counter = property(lambda self: self._word(0))
    forced_uniform = property(lambda self: self._word(3))

    def state_dict(self):
        return {"seed": self.seed, "counter": self.counter}

    def load_state_dict(self, sd):
        signed = lambda v: (int(v) & _U64) - (1 << 64) if (int(v) & _U64) >> 63 else int(v) & _U64
        self.state[0], self.state[2] = signed(sd["counter"]), signed(sd["seed"])

    def live_tensors(self):
        """What a draw changes besides its outputs (the counter): a caller that runs draws which must not count (a capture's warm-up
        runs draw patches too) clones these before and copies them back after."""
        return [self.state]

    # ---- the draw
    def origins(self, mask, frames=None):
        import torch
        from ._marshal import _ptr, _stream
        if not torch.is_tensor(mask) or mask.device != self.device:
            raise RuntimeError(f"DevicePatchSampler: the mask must be a tensor on {self.device} (no host round trip)")
        if mask.dim() not in (2, 3):
            raise ValueError("DevicePatchSampler: mask must be [H,W], [1,H,W] or [K,H,W]")
        H, W = int(mask.shape[-2]), int(mask.shape[-1])
        Km = 1 if mask.dim() == 2 else int(mask.shape[0])
        K = Km if frames is None else int(frames)
        if Km not in (1, K):
            raise ValueError(f"DevicePatchSampler: {Km} masks for {K} frames")
        key = (K, Km, H, W, Km > 1 or frames is not None)         # (the last: the result is [K,n,2], not [n,2])
        b = self._bufs.get(key)
        if b is None:
            lib = _lib.load()
            nbytes = int(lib.sg_patch_sampler_ws_bytes(K, H, W, self.patch_size))
            dev = self.device
            b = self._bufs[key] = {"ws": torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev),
                                   "origins": torch.zeros((K, self.n, 2), dtype=torch.int32, device=dev),
                                   "info": torch.zeros((K, 2), dtype=torch.int32, device=dev), "mask": None}
        if mask.dtype == torch.float32 and mask.is_contiguous():
            m = mask
        else:
            if b["mask"] is None:
                b["mask"] = torch.empty(mask.shape, dtype=torch.float32, device=self.device)
            m = b["mask"].copy_(mask)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().sg_patch_origins(K, H, W, self.patch_size, self.n, 0 if Km == 1 else H * W, self.p, _ptr(m),
                                                    _ptr(self.state), _ptr(b["ws"]), _ptr(b["origins"]), _ptr(b["info"]),
                                                    _stream(self.device)), "sg_patch_origins")
        self.info = b["info"]
        self.last_origins = b["origins"] if key[4] else b["origins"][0]
        return self.last_origins
