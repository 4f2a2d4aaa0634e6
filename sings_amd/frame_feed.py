"""The training frames on the device: stored as the bytes they came from, drawn and expanded inside the step (include/sings_feed.h,
csrc/sg_feed.hip).

``FrameStore`` stands where ``Customdataset.load_data_to_cuda`` stands: the reference caches four fp32 planes per frame (16 B per
pixel) for data that was born as 8-bit PNGs; the store keeps [F,H,W,4] bytes (R, G, B, mask: 4 B per pixel).  ``FrameFeed`` stands
where ``RandomIndexIterator`` (general.py:16-32) and ``bg_color = torch.rand(3)`` (gs_trainer.py:238) stand: ``draw()`` is two
launches -- the step's K frame indices and its background colour from a counter in device memory, then those frames expanded into
the fp32 planes the loss reads -- with no copy to the host, no wait and no allocation, so it may sit inside a captured step, and
every replay of that step draws the next frames.  The ``*_host`` functions are the rule in numpy: the definition the kernels are
held to, integer for integer.

The rule.

    word_s(c, t) = word ``t % 4`` of Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)`` and counter
              ``(c & 0xffffffff, c >> 32, s, t // 4)``; ``s = 0`` is the order stream, ``s = 1`` the background stream
    bounded(w, R) = ``(w * R) >> 32`` in 64 bits: a value in [0, R)
    order of epoch e over F frames: ``a[i] = i``; for ``i = F-1`` down to 1: ``j = bounded(word_0(e, F-1-i), i+1)``, swap ``a[i]``
              and ``a[j]`` -- a pure function of ``(F, seed, e)``: it starts from the identity, not from the previous epoch's order,
              so a resumed run can rebuild it
    draw number t (t = frames drawn so far) is ``order(t // F)[t % F]``; a step of K frames takes draws ``c .. c+K-1`` and leaves
              ``c + K`` (a chunk may straddle an epoch)
    background of a step that starts at counter c: channel i = ``(word_1(c, i) >> 8) * 2**-24``, in [0, 1); one colour per step,
              also for K > 1
    a stored byte v becomes ``float32(v) / float32(255)``, correctly rounded: ``(img / 255).astype(np.float32)`` for all 256
              values (``value_table``).  Multiplying by ``1 / 255`` is not that: it differs at 126 of the 256 values.

One deviation from the reference: the random streams are counter based, not Python's / torch's global ones.
"""
import numpy as np

from . import _lib
from .patch_sampler import philox4x32

_U32, _U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
MAX_FRAMES, MAX_K = _lib.FEED_MAX_FRAMES, _lib.FEED_MAX_K


# ---- the rule in numpy ------------------------------------------------------------------------------------------------------------
def _words(seed, c, stream, n):
    """word_stream(c, 0 .. n-1) as a list of ints."""
    seed, c = int(seed) & _U64, int(c) & _U64
    key, out = (seed & _U32, seed >> 32), []
    for b in range(-(-n // 4)):
        out.extend(philox4x32((c & _U32, c >> 32, stream, b), key))
    return out[:n]


def order_host(F, seed, epoch):
    """The order of epoch ``epoch`` over ``F`` frames -> int32 [F], a permutation of 0..F-1."""
    F = int(F)
    if not 1 <= F <= MAX_FRAMES:
        raise ValueError(f"order_host: F must be in 1..{MAX_FRAMES}")
    a, w = list(range(F)), _words(seed, epoch, 0, F - 1)
    for i in range(F - 1, 0, -1):
        j = (w[F - 1 - i] * (i + 1)) >> 32
        a[i], a[j] = a[j], a[i]
    return np.asarray(a, np.int32)


def indices_host(F, seed, counter, K):
    """Draws ``counter .. counter+K-1`` -> int32 [K]."""
    F, orders, out = int(F), {}, []
    for t in range(int(counter), int(counter) + int(K)):
        e = t // F
        if e not in orders:
            orders[e] = order_host(F, seed, e)
        out.append(orders[e][t % F])
    return np.asarray(out, np.int32)


def bg_host(seed, counter):
    """The background colour of a step that starts at ``counter`` -> float32 [3], multiples of 2**-24 in [0, 1)."""
    return np.asarray([(w >> 8) * 2.0 ** -24 for w in _words(seed, counter, 1, 3)], np.float32)


def value_table():
    """float32 [256]: what a stored byte becomes."""
    return np.arange(256, dtype=np.float32) / np.float32(255.0)


# ---- the objects ------------------------------------------------------------------------------------------------------------------
def _device(device):
    import torch
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("sings_amd.frame_feed: the frames live on the GPU (no CPU fallback; the *_host functions are the numpy rule)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _signed(v):
    v = int(v) & _U64
    return v - (1 << 64) if v >> 63 else v


class FrameStore:
    """``FrameStore(rgb_u8 [F,H,W,3], mask_u8 [F,H,W])``: the training set as uint8 [F,H,W,4] on the device (``data``; tensors or
    numpy arrays, copied).  ``frames(idx) -> (gt [n,3,H,W], mask [n,H,W])`` fp32 for any indices (an int, a sequence, a tensor),
    eagerly, in fresh tensors: what validation reads its ground truth with.  ``nbytes``: the store's size."""

    def __init__(self, rgb_u8, mask_u8, device=None):
        import torch
        dev = self.device = _device(device)
        rgb, mask = torch.as_tensor(rgb_u8), torch.as_tensor(mask_u8)
        if rgb.dtype != torch.uint8 or mask.dtype != torch.uint8:
            raise TypeError(f"FrameStore: uint8 frames and masks (got {rgb.dtype}, {mask.dtype}); floats go through FrameStore.from_float")
        if rgb.dim() != 4 or rgb.shape[3] != 3 or tuple(mask.shape) != tuple(rgb.shape[:3]) or min(rgb.shape[:3]) < 1:
            raise ValueError(f"FrameStore: rgb_u8 [F,H,W,3] and mask_u8 [F,H,W], got {tuple(rgb.shape)} and {tuple(mask.shape)}")
        self.F, self.H, self.W = (int(n) for n in rgb.shape[:3])
        if self.F > MAX_FRAMES or self.H * self.W >= 1 << 31:
            raise ValueError(f"FrameStore: at most {MAX_FRAMES} frames of fewer than 2**31 pixels")
        self.data = torch.empty((self.F, self.H, self.W, 4), dtype=torch.uint8, device=dev)
        self.data[..., :3] = rgb.to(dev)
        self.data[..., 3] = mask.to(dev)

    @classmethod
    def from_float(cls, rgb, mask, device=None):
        """From the reference's cache: ``rgb`` [F,3,H,W] and ``mask`` [F,H,W] floats that are bytes divided by 255.  Every element
        must be bit-equal to its byte's ``value_table()`` entry (checked on the device): ``ValueError`` with the count otherwise --
        the store is never silently lossy."""
        import torch
        dev = _device(device)
        rgb, mask = torch.as_tensor(rgb), torch.as_tensor(mask)
        if rgb.dim() != 4 or rgb.shape[1] != 3 or tuple(mask.shape) != (rgb.shape[0], rgb.shape[2], rgb.shape[3]):
            raise ValueError(f"FrameStore.from_float: rgb [F,3,H,W] and mask [F,H,W], got {tuple(rgb.shape)} and {tuple(mask.shape)}")
        table = torch.from_numpy(value_table()).to(dev).view(torch.int32)
        F, _, H, W = (int(n) for n in rgb.shape)
        rgb_u8 = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        mask_u8 = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
        bad = torch.zeros((), dtype=torch.int64, device=dev)

        def quantise(x):
            x = x.to(dev, torch.float32).contiguous()
            q = torch.nan_to_num(x * 255.0, nan=0.0).round().clamp(0.0, 255.0).to(torch.uint8)
            bad.add_((table[q.long()] != x.view(torch.int32)).sum())
            return q
        for f in range(F):                                               # (a frame at a time: the check's temporaries stay small)
            rgb_u8[f] = quantise(rgb[f]).permute(1, 2, 0)
            mask_u8[f] = quantise(mask[f])
        if int(bad.item()):
            raise ValueError(f"FrameStore.from_float: {int(bad.item())} of {F * 4 * H * W} elements are not a byte divided by 255 "
                             "(the store would be lossy)")
        return cls(rgb_u8, mask_u8, device=dev)

    @classmethod
    def from_png_files(cls, image_paths, mask_paths, device=None, verify_crc=True, max_workspace_bytes=1 << 31, checked=None):
        """From a kit's files: frame f is ``image_paths[f]`` (8-bit RGB or RGBA PNG; alpha is dropped) and ``mask_paths[f]`` (8-bit
        grey PNG), all of one size.  The store is allocated, then filled on the device by ``unpng.PngDecoder`` (the files' zlib
        streams are uploaded, not their pixels), in batches whose workspace stays below ``max_workspace_bytes``.  ``ValueError``
        naming the file for unequal counts, a file the decoder does not read, a size that is not the first image's, and every stream
        the device refuses.  ``checked``: what ``unpng.check_kit_files`` returned for these very lists, from a caller that has
        already read the headers (``load_kit``); they are not read again.

        Memory: while the load runs the device holds, beside the store, the decoder's workspace -- one slot of the largest file's
        ``H * (1 + W * channels)`` scanline bytes per stream of a batch, a mask's slot as large as an image's, ``max_workspace_bytes``
        at the most (2 GiB by default; a kit of 80 frames of 512 x 896 takes 220 MB) -- and the files' compressed bytes.  A smaller
        ``max_workspace_bytes`` means more batches, and a load is about as long as the longest stream of each of its batches.  The
        workspace goes back to torch's allocator when this returns."""
        import torch
        from . import unpng
        dev = _device(device)
        images, masks = [str(p) for p in image_paths], [str(p) for p in mask_paths]
        W, H, raw = checked if checked is not None else unpng.check_kit_files(images, masks)
        self = cls.__new__(cls)
        self.device, self.F, self.H, self.W = dev, len(images), H, W
        if self.F > MAX_FRAMES or self.H * self.W >= 1 << 31:
            raise ValueError(f"FrameStore: at most {MAX_FRAMES} frames of fewer than 2**31 pixels")
        self.data = torch.empty((self.F, self.H, self.W, 4), dtype=torch.uint8, device=dev)
        batch = max(1, min(2 * self.F, unpng.MAX_STREAMS, int(max_workspace_bytes) // raw))
        decoder = unpng.PngDecoder(dev, batch, raw, verify_crc=verify_crc)
        decoder.decode_into(self.data, images + masks, [4 * f for f in range(self.F)] + [4 * f + 3 for f in range(self.F)])
        return self

    nbytes = property(lambda self: self.data.numel())

    def expand(self, idx, gt, mask):
        """``sg_frame_expand``: frames ``idx`` (device int32 [K], K <= 16) into ``gt`` [K,3,H,W] and ``mask`` [K,H,W]; one launch."""
        import torch
        from ._marshal import _ptr, _stream
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().sg_frame_expand(int(idx.shape[0]), self.H, self.W, self.F, _ptr(self.data), _ptr(idx), _ptr(gt),
                                                   _ptr(mask), _stream(self.device)), "sg_frame_expand")

    def frames(self, idx):
        import torch
        idx = torch.as_tensor(idx).reshape(-1).to(self.device, torch.int32).contiguous()
        n = int(idx.shape[0])
        gt = torch.empty((n, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        mask = torch.empty((n, self.H, self.W), dtype=torch.float32, device=self.device)
        for k in range(0, n, MAX_K):
            self.expand(idx[k:k + MAX_K], gt[k:k + MAX_K], mask[k:k + MAX_K])
        return gt, mask


class FrameFeed:
    """``FrameFeed(store, seed=0, frames_per_step=1, random_bg=True)`` owns the device state (``state`` int64 [4]: next counter,
    seed, the epoch ``order`` holds or -1, the last call's counter; ``order`` int32 [F]) and the static outputs ``idx`` int32 [K],
    ``gt`` [K,3,H,W], ``mask`` [K,H,W], ``bg`` [3] (with ``random_bg=False`` the feed never writes ``bg``).

    ``draw()``: the next K frames into those tensors -- two launches, no host read, no allocation; legal under capture.
    ``state_dict()`` / ``load_state_dict()`` carry ``seed`` and ``counter``; loading sets the held epoch to -1, so the next draw
    rebuilds the order.  ``counter`` and ``last_indices`` read the device: they synchronise -- for tests and logs."""

    def __init__(self, store, seed=0, frames_per_step=1, random_bg=True):
        import torch
        K = int(frames_per_step)
        if not 1 <= K <= MAX_K:
            raise ValueError(f"FrameFeed: frames_per_step must be in 1..{MAX_K}")
        self.store, self.K, self.random_bg = store, K, bool(random_bg)
        dev = self.device = store.device
        self.state = torch.tensor([0, _signed(seed), -1, 0], dtype=torch.int64, device=dev)
        self.order = torch.zeros(store.F, dtype=torch.int32, device=dev)
        self.idx = torch.zeros(K, dtype=torch.int32, device=dev)
        self.gt = torch.zeros((K, 3, store.H, store.W), dtype=torch.float32, device=dev)
        self.mask = torch.zeros((K, store.H, store.W), dtype=torch.float32, device=dev)
        self.bg = torch.zeros(3, dtype=torch.float32, device=dev)

    def draw(self):
        import torch
        from ._marshal import _ptr, _stream
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().sg_frame_draw(self.store.F, self.K, int(self.random_bg), _ptr(self.state), _ptr(self.order),
                                                 _ptr(self.idx), _ptr(self.bg), _stream(self.device)), "sg_frame_draw")
        self.store.expand(self.idx, self.gt, self.mask)

    def live_tensors(self):
        """What a draw changes besides its outputs: a caller that runs draws which must not count (a capture's warm-up) clones
        these before and copies them back after.  (``order`` with ``state``: the state names the epoch the order holds.)"""
        return [self.state, self.order]

    # ---- the device state, read on the host
    seed = property(lambda self: int(self.state[1].item()) & _U64)
    counter = property(lambda self: int(self.state[0].item()) & _U64)
    last_indices = property(lambda self: self.idx.cpu().numpy().copy())

    def state_dict(self):
        return {"seed": self.seed, "counter": self.counter}

    def load_state_dict(self, sd):
        import torch
        self.state.copy_(torch.tensor([_signed(sd["counter"]), _signed(sd["seed"]), -1, 0], dtype=torch.int64))
