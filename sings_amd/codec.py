"""What the two device encoders share (``video.JpegEncoder``, ``png.PngEncoder``): K uint8 frames of W x H on the device to K complete
files per call, everything allocated up front.

A subclass sets ``W`` and ``H`` and its own options, then calls ``_FrameEncoder.__init__``; it names its header and library flag
(``_INCLUDE``, ``_FLAG``), its numpy twin (``_TWIN``), the layout word that is its default capacity (``_DEFAULT_CAPACITY``) and whether
``encode_to_host`` grows the buffer for a frame that does not fit (``_GROWS``) or raises, and gives ``_describe()`` -> (header ``bytes``,
table words uint32, the layout dict of ``_marshal``) and ``_launch(k, frames, bgr, buf, sizes, stream, **options)``: the library's entry
point on k contiguous frames, ``options`` being what ``encode`` was given beyond its own arguments.
"""
MAX_FRAMES = 16                      # SG_JPEG_MAX_FRAMES, SG_PNG_MAX_FRAMES


class _FrameEncoder:
    _INCLUDE = _FLAG = _TWIN = _DEFAULT_CAPACITY = None
    _GROWS = False

    def __init__(self, K, device, capacity=None):
        import torch
        from . import _lib
        name = type(self).__name__
        self.K = int(K)
        if not 1 <= self.K <= MAX_FRAMES:
            raise ValueError(f"{name}: K = {K} outside 1..{MAX_FRAMES}")
        if capacity is not None and int(capacity) < 1:
            raise ValueError(f"{name}: capacity = {capacity} bytes per frame")
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError(f"{type(self).__module__}.{name} runs on the MI355X only; there is no CPU fallback ({self._TWIN} is the "
                               "numpy restatement the tests compare it with)")
        _lib.load()
        if not getattr(_lib, self._FLAG):
            raise RuntimeError(f"{name}: the loaded library predates include/{self._INCLUDE} (no fallback): rebuild it")
        self.header, tables, self.layout = self._describe()
        with torch.cuda.device(self.dev):
            self._tables = torch.from_numpy(tables.view("int32")).to(self.dev)
            self._header = torch.frombuffer(bytearray(self.header), dtype=torch.uint8).to(self.dev)
            self._ws = torch.empty(self.layout["ws_bytes"], dtype=torch.uint8, device=self.dev)
            self.sizes = torch.zeros(self.K, dtype=torch.int32, device=self.dev)
        self.buf = None
        self._allocate(self.layout[self._DEFAULT_CAPACITY] if capacity is None else int(capacity))

    def _allocate(self, capacity):
        import torch
        if capacity < 1:
            raise ValueError(f"{type(self).__name__}: capacity = {capacity} bytes per frame")
        self.capacity = int(capacity)
        self.buf = None                                           # (drop the old buffer before the new one is sized)
        self.buf = torch.empty((self.K, self.capacity), dtype=torch.uint8, device=self.dev)

    def encode(self, frames_u8, bgr=False, stream=None, out=None, **options):
        """``frames_u8``: uint8 [k,H,W,3] on the device, k <= K -> (buf [k, capacity] uint8, sizes [k] int32), views of the encoder's
        own buffers: the next ``encode`` overwrites them.  ``sizes[i]`` bytes of row i are frame i's file; a negative size is minus
        the bytes that frame needs (nothing of it was written).  ``out``: (buf [K', capacity'] uint8, sizes int32) of the caller's to
        write instead (a buffer with a guard region behind it, in tests)."""
        import torch
        if (not torch.is_tensor(frames_u8) or frames_u8.device != self.dev or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4
                or tuple(frames_u8.shape[1:]) != (self.H, self.W, 3) or not 1 <= frames_u8.shape[0] <= self.K):
            raise ValueError(f"{type(self).__name__}.encode: uint8 [1..{self.K},{self.H},{self.W},3] on {self.dev} expected, got "
                             f"{getattr(frames_u8, 'dtype', type(frames_u8).__name__)} {tuple(getattr(frames_u8, 'shape', ()))}")
        x = frames_u8.contiguous()
        k = int(x.shape[0])
        buf, sizes = (self.buf, self.sizes) if out is None else out
        if stream is None:
            stream = torch.cuda.current_stream(self.dev)
        self._launch(k, x, bgr, buf, sizes, stream, **options)
        return buf[:k], sizes[:k]

    def encode_to_host(self, frames_u8, bgr=False, **options):
        """-> a list of k ``bytes``.  One copy of ``sizes``, then one copy of the used bytes to pinned memory.  A frame that overflows
        ``capacity``: with ``_GROWS`` the buffer grows to what the largest frame needs and the batch is encoded again, at most twice;
        RuntimeError after that, or at once without ``_GROWS``."""
        import torch
        name = type(self).__name__
        for attempt in range(3):
            buf, sizes = self.encode(frames_u8, bgr, **options)
            n = sizes.cpu().tolist()
            if min(n) >= 0:
                break
            if not self._GROWS:
                raise RuntimeError(f"{name}: a frame needs {-min(n)} bytes, the capacity is {self.capacity}")
            if attempt == 2:
                raise RuntimeError(f"{name}: frames still overflow {self.capacity} bytes after two retries (needed: {-min(n)})")
            torch.cuda.current_stream(self.dev).synchronize()     # (the buffer is about to be replaced)
            self._allocate(-min(n))
        m = max(n)
        host = torch.empty((len(n), m), dtype=torch.uint8).pin_memory()
        host.copy_(buf[:, :m])
        rows = host.numpy()
        return [rows[i, :n[i]].tobytes() for i in range(len(n))]
