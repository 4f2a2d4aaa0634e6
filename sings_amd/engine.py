"""Pre-allocated forward/backward driver over the C ABI (no autograd, no per-call allocation).

This is what a training loop that owns its buffers (and bench.py) calls: workspaces and the
flat gradient buffer are sized once for 288 GB-class HBM and reused every step, the capacity
for (tile, Gaussian) pairs is a fixed upper bound, and nothing synchronises inside a step.  The
gradient tensors are views into ONE flat fp32 buffer so that frame-parallel training can
all-reduce them with a single RCCL call (see sings_amd/dp.py).  The engines fill the structs of the C ABI through
sings_amd/_marshal.py, the same functions the autograd ops use.
"""
import ctypes as C
import os

import torch

from . import _lib
from . import work_order as _work_order
from ._marshal import _camera_stride, _frame_batch, _frame_rows, _ptr, _settings_struct, _skin_frames, _skin_struct
from ._marshal import _stream as _current_stream


# RasterFramesEngine(order=None): build and keep the Morton work order (SINGS_WORK_ORDER=0: no order unless the caller passes one)
_ORDER_BY_DEFAULT = os.environ.get("SINGS_WORK_ORDER", "1") != "0"


def _raster_fields(M):
    """Flat gradient layout of the un-skinned engines: (view, floats per Gaussian; None: no view, the attribute is None)."""
    return [("d_means3D", 3), ("d_scales", 3), ("d_rots", 4), ("d_opacity", 1), ("d_sh", 3 * M if M else None)]


def _skinned_fields(M, with_rot, rot_width):
    """... of the LBS-fused engines (the reference's tensor shapes); ``rot_width`` 9: rotation matrices, 6: the decoder's 6-D form."""
    return [("d_xyz", 3), ("d_scales", 3), ("d_opacity", 1), ("d_sh", 3 * M), ("d_rot", int(rot_width) if with_rot else None)]


class _Engine:
    """What every engine shares: the workspaces of its K frames (K = 1 for the single-frame engines), the flat gradient buffer and
    its views, the flag word of the forward, the settings struct and the ViewBatch chain of the backward."""

    def __init__(self, P, W, H, sh_coeffs, device, capacity_pairs, K=None):
        """``K`` None: a single-frame engine (K = 1; ``color``, ``radii`` and ``d_means2D`` have no frame axis).  The workspaces
        of K frames are K consecutive single-frame workspaces in one allocation each (``sg_frames_layout``)."""
        self.lib = _lib.load()
        if K is not None and not 1 <= K <= _lib.MAX_FRAMES:
            raise ValueError(f"K must be 1..{_lib.MAX_FRAMES}")
        self.P, self.W, self.H, self.M, self.cap = int(P), int(W), int(H), int(sh_coeffs), int(capacity_pairs)
        self.K = 1 if K is None else int(K)
        self.dev = torch.device(device)
        L = _lib.SgLayout()
        sizes = [C.c_size_t() for _ in range(4)]
        _lib.check(self.lib.sg_frames_layout(self.P, self.W, self.H, self.cap, self.K, C.byref(L), *[C.byref(x) for x in sizes]),
                   "sg_frames_layout")
        self.L = L
        u8 = dict(dtype=torch.uint8, device=self.dev)
        self.geom = torch.empty(sizes[0].value, **u8)
        self.binning = torch.empty(sizes[1].value, **u8)
        self.binning.view(self.K, L.bin_bytes)[:, :L.bin_ranges].zero_()     # counters zeroed ONCE; every forward leaves them zeroed
        self._clean = True                                                    # (SG_FLAG_WS_CLEAN: no per-call zeroing launch)
        self.img = torch.empty(sizes[2].value, **u8)
        self.bwd_ws = torch.empty(sizes[3].value, **u8)
        lead = () if K is None else (self.K,)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.color = torch.empty(lead + (3, self.H, self.W), **f32)
        self.radii = torch.empty(lead + (self.P,), dtype=torch.int32, device=self.dev)
        self.d_means2D = torch.empty(lead + (self.P, 3), **f32)     # densification statistic, not reduced as a weight grad
        self._keep, self._s = [], None
        self._rows = 0                    # list-length hints of set_camera (SG_FLAG_SHORT_LISTS / LONG_ROWS; read by the avatar parity)
        self._chain = None                # inside ViewBatch.run: callable -> (accumulate, wait-for event, done event)
        # SG_FLAG_THROUGHPUT (no latency-only work): K frames share the chip; a ViewBatch that keeps several views in flight sets it
        self.throughput = K is not None

    def _gradients(self, fields, grad_flat, sh_planar):
        """Carve the flat gradient buffer into ``fields`` (view, floats per Gaussian).  ``sh_planar``: the SH block is
        coefficient-major, [M,P,3] (SG_FLAG_SH_PLANAR), and LAST -- the kernels write only the (sh_degree + 1)^2 planes in use, so
        the step's gradient is the PREFIX ``grad_flat[:active_floats(deg)]`` (10 floats per Gaussian at degree 0 instead of 55 for
        the avatar): that prefix is what is folded and all-reduced; the rest stays zero (zeroed here, once, when the engine owns
        the buffer -- a caller-owned buffer must come zeroed).  ``grad_flat``: optional caller-owned storage (one row of a
        [views, P*per] buffer when several engines render the views of one step concurrently and their gradients are summed in
        one pass)."""
        self.sh_planar = bool(sh_planar)
        if self.sh_planar:
            fields = [f for f in fields if f[0] != "d_sh"] + [f for f in fields if f[0] == "d_sh"]
        self._fields = fields
        own = grad_flat is None
        self.rebind_gradients(torch.empty(self.P * sum(w or 0 for _, w in fields), dtype=torch.float32, device=self.dev) if own
                              else grad_flat)
        if own and self.sh_planar and self.d_sh is not None:
            self.d_sh.zero_()

    def rebind_gradients(self, grad_flat):
        """Point the gradient views at another flat buffer (several engines of one step sharing ONE buffer: FramePipeline)."""
        P, n = self.P, self.P * sum(w or 0 for _, w in self._fields)
        dev = self.geom.device            # (where the workspaces are: ``self.dev`` may name a device without its index, "cuda")
        if grad_flat.numel() != n or grad_flat.dtype != torch.float32 or not grad_flat.is_contiguous() or grad_flat.device != dev:
            raise ValueError(f"grad_flat must be a contiguous fp32 tensor of {n} elements on {dev}")
        self.grad_flat = grad_flat.view(-1)
        o = 0
        for name, w in self._fields:
            shape = ((self.M, P, 3) if self.sh_planar else (P, self.M, 3)) if name == "d_sh" else (P, w)
            setattr(self, name, None if w is None else self.grad_flat[o:o + P * w].view(shape))
            o += P * (w or 0)

    def active_floats(self, sh_degree):
        """Length of the prefix of ``grad_flat`` that carries the step's gradient (everything, unless ``sh_planar``)."""
        if not self.sh_planar:
            return self.grad_flat.numel()
        return self.P * sum(w or 0 for name, w in self._fields if name != "d_sh") + (int(sh_degree) + 1) ** 2 * self.P * 3

    def set_camera(self, raster_settings, long_rows=False):
        """``long_rows``: the caller knows (from a sizing pass) that no tile list exceeds 16384 entries: direct binning on images of
        few tiles (SG_FLAG_LONG_ROWS, include/sings_hip.h; a longer list: ``num_rendered()`` = NUM_RENDERED_LONG_LIST, the frame
        rendered the background: call set_camera again without the hint)."""
        self._camera(raster_settings, _lib.FLAG_LONG_ROWS if long_rows else 0)

    def _camera(self, raster_settings, rows):
        keep = []
        self._s = _settings_struct(raster_settings, self.dev, self.M, keep)
        self._keep, self._rows = keep, rows

    def _flags(self):
        """The flag word of a forward."""
        return (self._rows | (_lib.FLAG_SH_PLANAR if self.sh_planar else 0) | (_lib.FLAG_THROUGHPUT if self.throughput else 0)
                | (_lib.FLAG_WS_CLEAN if self._clean else 0))

    def _stream(self):
        return _current_stream(self.dev)

    def _chain_begin(self, accumulate):
        """Before the per-Gaussian half of a backward: (accumulate, done event).  Inside a ``ViewBatch`` whose views share a gradient
        row, the view ADDS to the row iff an earlier view of the step wrote it (``accumulate=1``), and with one row across streams it
        first waits for the per-Gaussian half of the view in front of it in the step's chain."""
        acc, after, done = self._chain() if self._chain is not None else (False, None, None)
        if after is not None:
            torch.cuda.current_stream(self.dev).wait_event(after)
        return bool(accumulate) or bool(acc), done

    def _chain_end(self, done):
        """After the per-Gaussian half: the next view of the chain may go."""
        if done is not None:
            done.record(torch.cuda.current_stream(self.dev))

    def num_rendered(self):
        nr = C.c_int64(0)
        _lib.check(self.lib.sg_read_num_rendered(_ptr(self.binning), C.byref(nr), self._stream()), "read R")
        return int(nr.value)


class RasterEngine(_Engine):
    """One view per call (sg_rasterize_*).  Flat gradient layout (floats per Gaussian): means3D 3, scales 3, rotations 4,
    opacity 1, sh 3*M."""

    def __init__(self, P, W, H, sh_coeffs, device, capacity_pairs, grad_flat=None):
        super().__init__(P, W, H, sh_coeffs, device, capacity_pairs)
        self._gradients(_raster_fields(self.M), grad_flat, sh_planar=False)

    def set_camera(self, raster_settings, short_lists=False, long_rows=False):
        """``short_lists``: the caller knows (from a sizing pass over this scene) that no tile list exceeds 1024 entries (what the
        compositing workgroups sort themselves); the two long-list sort launches are then skipped and, on images of many tiles, the
        frame is binned directly (SG_FLAG_SHORT_LISTS).  ``long_rows``: images of few tiles -- no list exceeds 16384 entries: direct
        binning there (SG_FLAG_LONG_ROWS).  A longer list makes ``num_rendered()`` return ``_lib.NUM_RENDERED_LONG_LIST`` (the frame
        rendered the background): call set_camera again without the hint."""
        self._camera(raster_settings, (_lib.FLAG_SHORT_LISTS if short_lists else 0) | (_lib.FLAG_LONG_ROWS if long_rows else 0))

    def forward(self, means3D, shs, opacities, scales, rotations, sync_num_rendered=False):
        nr = C.c_int64(-1)
        self._s.flags = self._flags()
        self._clean = False                                  # (stays False if the call below raises)
        _lib.check(self.lib.sg_rasterize_forward(
            C.byref(self._s), self.P, _ptr(means3D), _ptr(shs), None, _ptr(opacities), _ptr(scales), _ptr(rotations),
            None, _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.img), _ptr(self.color), _ptr(self.radii),
            0, C.byref(nr) if sync_num_rendered else None, self._stream()), "forward")
        self._clean = True
        return int(nr.value)

    def backward(self, means3D, shs, opacities, scales, rotations, dL_dcolor, accumulate=False):
        """Composite backward (gradient records of this view), then the per-Gaussian chain rule into the gradient buffer.
        ``accumulate``: ADD to the buffer (``sg_rasterize_backward_gaussians(accumulate=1)``); so does a view inside a ``ViewBatch``
        whose row an earlier view of the step wrote (see ``_chain_begin``)."""
        _lib.check(self.lib.sg_rasterize_backward_records(
            C.byref(self._s), self.P, _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.img), _ptr(self.bwd_ws),
            _ptr(dL_dcolor), self._stream()), "backward (records)")
        accumulate, done = self._chain_begin(accumulate)
        _lib.check(self.lib.sg_rasterize_backward_gaussians(
            C.byref(self._s), self.P, _ptr(means3D), _ptr(shs), None, _ptr(opacities), _ptr(scales), _ptr(rotations),
            None, _ptr(self.radii), _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.bwd_ws), int(accumulate),
            _ptr(self.d_means3D), _ptr(self.d_means2D), _ptr(self.d_sh), None, _ptr(self.d_opacity),
            _ptr(self.d_scales), _ptr(self.d_rots), None, self._stream()), "backward (gaussians)")
        self._chain_end(done)

    def capture(self, means3D, shs, opacities, scales, rotations, dL_dcolor=None):
        """Record one step (forward, + backward when dL_dcolor is given) into a HIP graph and return it; ``graph.replay()``
        re-runs the whole launch sequence with one host call.  Possible because nothing in a step synchronises or
        allocates: every buffer (inputs included -- update them IN PLACE between replays) is fixed, the camera is read
        from device memory.  Pays off when the step is launch-bound (small scenes, forward-only animation)."""
        torch.cuda.synchronize(self.dev)
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):                            # warm-up on the capture stream
            self.forward(means3D, shs, opacities, scales, rotations)
            if dL_dcolor is not None:
                self.backward(means3D, shs, opacities, scales, rotations, dL_dcolor)
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.forward(means3D, shs, opacities, scales, rotations)
            if dL_dcolor is not None:
                self.backward(means3D, shs, opacities, scales, rotations, dL_dcolor)
        return g


class SkinnedEngine(_Engine):
    """Same idea for the LBS-fused path (sg_skinned_forward / backward): canonical Gaussians + per-frame joint
    transforms in, image + flat canonical-Gaussian gradient buffer out.  Flat layout (floats): xyz_canon 3P,
    scales 3P, opacity P, sh 3MP, [rot_canon 9P] (``sh_planar``: the SH block last).  dL/dA [J,16] and dL/dtransl [3] are
    per-frame (not all-reduced)."""

    def __init__(self, P, J, W, H, sh_coeffs, device, capacity_pairs, with_rot=False, grad_flat=None, rot_width=9, sh_planar=False):
        super().__init__(P, W, H, sh_coeffs, device, capacity_pairs)
        self.J = int(J)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.skin_ws = torch.empty(int(self.lib.sg_skin_ws_floats(self.P)), **f32)
        self._gradients(_skinned_fields(self.M, with_rot, rot_width), grad_flat, sh_planar)
        self.d_A = torch.empty((self.J, 16), **f32); self.d_transl = torch.empty(3, **f32)
        self._k = None

    def set_frame(self, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs=None):
        self._kkeep = []
        self._k = _skin_struct(self.dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs, self._kkeep)

    def forward(self, shs, opacities, scales, sync_num_rendered=False, posed_out=None):
        """``posed_out``: optional (xyz [P,3], quaternions [P,4], scales [P,3]) fp32 tensors that also receive the posed values
        (what SinGS.forward returns: sings_hybrid.py:400-419); the render itself never reads them back."""
        nr = C.c_int64(-1)
        self._s.flags = self._flags()
        self._clean = False
        pxyz, pq, psc = posed_out if posed_out is not None else (None, None, None)
        _lib.check(self.lib.sg_skinned_forward(
            C.byref(self._s), self.P, C.byref(self._k), _ptr(shs), _ptr(opacities), _ptr(scales), _ptr(self.geom),
            _ptr(self.binning), self.cap, _ptr(self.img), _ptr(self.color), _ptr(self.radii), _ptr(pxyz), _ptr(pq), _ptr(psc),
            C.byref(nr) if sync_num_rendered else None, self._stream()), "skinned forward")
        self._clean = True
        return int(nr.value)

    def backward(self, shs, opacities, scales, dL_dcolor, accumulate=False):
        """As ``RasterEngine.backward``: records of this frame, then (chained inside a ``ViewBatch``) the per-Gaussian half."""
        _lib.check(self.lib.sg_rasterize_backward_records(
            C.byref(self._s), self.P, _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.img), _ptr(self.bwd_ws),
            _ptr(dL_dcolor), self._stream()), "skinned backward (records)")
        accumulate, done = self._chain_begin(accumulate)
        _lib.check(self.lib.sg_skinned_backward_gaussians(
            C.byref(self._s), self.P, C.byref(self._k), _ptr(shs), _ptr(opacities), _ptr(scales), _ptr(self.radii),
            _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.bwd_ws), _ptr(self.skin_ws), int(accumulate),
            None, None, _ptr(self.d_xyz), _ptr(self.d_rot), _ptr(self.d_scales), _ptr(self.d_opacity),
            _ptr(self.d_sh), _ptr(self.d_means2D), _ptr(self.d_A), _ptr(self.d_transl), self._stream()), "skinned backward (gaussians)")
        self._chain_end(done)


class ViewBatch:
    """The views (frames) of ONE optimisation step in flight on several HIP streams.

    One view is a chain of short launches: the binning kernels are latency-bound (a handful of waves) and the composite
    kernels end in tile-imbalance tails.  Views of the same step are independent until their gradients are summed, the
    library keeps no state between calls, and every engine owns its workspaces -- so the views are dealt round-robin to
    ``streams`` streams and fill each other's holes (one MI355X: +24 % views/s at cfg3, +77 % frames/s for the avatar),
    bit-identical to running them one after the other.  ``run`` forks from the caller's current stream, launches
    ``fn(v, engine)`` for every view on its stream and joins; nothing synchronises with the host.  (No further stream: the
    caller's + three rendering streams are the four hardware queues HIP schedules onto.)

    Where the sum over the views is formed (``grads`` is ``[rows, per_view]``; engine v is built on row ``v % rows``):

    * rows == streams (round 3, what bench.py uses): ONE gradient row per stream.  The first view of a stream WRITES the row,
      the later views of that stream ADD to it (``sg_*_backward_gaussians(accumulate=1)``; stream order is the only ordering
      needed), so after the join ``streams`` rows are folded instead of ``views`` rows: the serial tail of a cfg3 step of 8 views
      on 3 streams reads 3 x 47 MB instead of 8 x 47 MB (the bytes of the other five rows are read by the accumulating kernels,
      inside the overlapped part of the step).  Fixed assignment and order -> bitwise reproducible.
    * rows == 1 with several streams: every view adds to the same buffer; an event per view orders the per-Gaussian halves of
      consecutive views across the streams (no fold at all).  Measured slower than stream rows on the avatar step (the waits
      couple the streams: 3 821 vs 3 940 frames/s) and on par at cfg3; kept for memory-constrained callers.
    * rows == views: the round-2 scheme, every view writes its own row.

    Either way a ``FrameParallel`` all-reduces the summed buffer over the ranks, chunk by chunk behind the fold
    (sings_amd.dp.GradientPipeline).

        grads = ViewBatch.gradient_rows(streams, per_view_floats, device)
        engines = [RasterEngine(..., grad_flat=grads[v % streams]) for v in range(views)]     # or SkinnedEngine
        batch = ViewBatch(engines, grads, streams=streams, frame_parallel=FrameParallel())     # None on one GPU
        acc = batch.run(lambda v, e: (e.forward(...), e.backward(...)))               # summed over views and ranks -> optimiser
    """

    @staticmethod
    def gradient_rows(views, per_view, device, zero=True):
        """``zero`` (default): ``sh_planar`` engines write only the SH planes in use, and with one row the row IS the
        accumulator -- an uninitialised tail would reach the optimiser.  ``zero=False`` for engines that write every
        float of their row (the reference layout) and callers that want to skip the one-off fill."""
        alloc = torch.zeros if zero else torch.empty
        return alloc((int(views), int(per_view)), dtype=torch.float32, device=device)

    def __init__(self, engines, grads, streams=3, frame_parallel=None, chunks=4, active=None):
        from .dp import GradientPipeline
        self.engines = list(engines)
        if grads.dim() == 1:
            grads = grads.view(1, -1)
        self.rows = int(grads.shape[0])
        self.n = max(1, min(int(streams), len(self.engines)))
        if self.rows not in (1, self.n, len(self.engines)):
            raise ValueError("gradient rows must be 1, the number of streams or the number of views")
        for v, e in enumerate(self.engines):
            if e.grad_flat.data_ptr() != grads[v % self.rows].data_ptr():
                raise ValueError(f"engine {v} must be built on grad_flat = grads[{v % self.rows}]")
        self.chain = self.rows == 1 and self.n > 1 and len(self.engines) > 1      # one shared buffer across streams: events
        self.grads = grads
        self.dev = grads.device
        self.streams = [torch.cuda.Stream(self.dev) for _ in range(self.n)] if self.n > 1 else []
        # the rows are folded (one row: nothing to fold) and the sum is all-reduced chunk by chunk on the caller's stream once
        # the views have joined it: sings_amd.dp.GradientPipeline
        self.pipe = GradientPipeline(grads, frame_parallel, chunks=chunks, active=active)
        self.acc = self.pipe.acc
        self._active_given = active is not None
        self._events = [torch.cuda.Event() for _ in self.engines] if self.chain else None
        for e in self.engines:                                # several views in flight: no latency-only work (SG_FLAG_THROUGHPUT)
            e.throughput = self.n > 1 or e.K > 1

    def _link(self, v, e):
        # Resolved when the view's backward actually RUNS (engine.backward calls it once): the view adds to its row iff a
        # backward of this run has already written that row -- a forward-only view (fn skips the backward) therefore never makes
        # a later view add to an unwritten buffer (round 3 decided by the view index alone); with one row across several streams
        # the per-Gaussian half additionally waits for the last backward before it (events order only those last, short kernels).
        def resolve():
            row = v % self.rows
            acc = self._written[row]
            self._written[row] = True
            if not self.chain:
                return acc, None, None
            after, self._last_event = self._last_event, self._events[v]
            return acc, after, self._events[v]
        e._chain = resolve

    def set_active(self, sh_degree):
        """The engines' SH degree changed (``oneupSHdegree``): widen (or narrow) the prefix of the gradient rows that is folded and
        all-reduced to ``engine.active_floats(sh_degree)``.  Every rank calls it at the same step."""
        self.pipe.set_active(self.engines[0].active_floats(sh_degree))
        self._active_given = True

    def _check_active(self):
        """An ``sh_planar`` engine whose camera asks for more SH planes than the configured prefix covers would have its extra
        planes silently dropped by the fold and the collective: refuse (call ``set_active(sh_degree)``)."""
        if not self._active_given:
            return
        for e in self.engines:
            st = e._s
            if e.sh_planar and st is not None and e.active_floats(int(st.sh_degree)) > self.pipe.n:
                raise RuntimeError(f"ViewBatch: an engine renders at SH degree {int(st.sh_degree)} but only the first {self.pipe.n} "
                                   f"floats of a gradient row are folded / all-reduced: call set_active({int(st.sh_degree)})")

    def run_unreduced(self, fn):
        """Render the views only (rows left unfolded): the caller reduces them itself, e.g. ``pipe.one_shot()``.  ``fn(v, engine)``
        runs view v's forward and AT MOST ONE backward; every row must be written by at least one backward before the rows are
        folded (checked).  Outside ``run`` the engines are plain again (a later stand-alone backward writes, never adds)."""
        self._check_active()
        self._written = [False] * self.rows
        self._last_event = None
        try:
            if not self.streams:
                for v, e in enumerate(self.engines):
                    self._link(v, e)
                    fn(v, e)
            else:
                cur = torch.cuda.current_stream(self.dev)
                for st in self.streams:
                    st.wait_stream(cur)
                for v, e in enumerate(self.engines):
                    self._link(v, e)
                    with torch.cuda.stream(self.streams[v % self.n]):
                        fn(v, e)
                for st in self.streams:
                    cur.wait_stream(st)
        finally:
            for e in self.engines:
                e._chain = None
        if any(self._written) and not all(self._written):
            raise RuntimeError("ViewBatch: a gradient row was not written by any view of this step (every stream / row needs at "
                               "least one view that runs its backward); the fold would read an unwritten buffer")

    def run(self, fn):
        self.run_unreduced(fn)
        return self.pipe.reduce()


class _FramesEngine(_Engine):
    """K frames (poses and / or cameras) of the SAME Gaussians per call: ONE dispatch per kernel for the K frames (the ``*_frames``
    entry points of include/sings_hip.h).  The reference hands its model 16 frames per call (``SinGS.forward_chunk``,
    sings_hybrid.py:474-569) and then renders them one by one (gs_trainer.py:684-714); a frame-parallel step renders K frames of the
    same canonical Gaussians per rank.  The per-Gaussian backward sums the K frames' gradients in registers and writes the gradient
    row once, in frame order -- bit for bit what K single-frame calls leave behind when the first writes the buffer and the others
    add (``accumulate=1``).  ``set_camera``: one camera for all K frames ([4,4] matrices) or one per frame (``viewmatrix`` /
    ``projmatrix`` [K,4,4], ``campos`` [K,3]: the other fields are shared).  A batch of frames is one "view" of a ViewBatch."""
    _fb = None                            # the frame batch of the calls (RasterFramesEngine.set_camera, SkinnedFramesEngine.set_frames)
    _cam_stride = 0                       # 1: one camera per frame

    def _camera(self, raster_settings, rows):
        stride = _camera_stride(raster_settings, self.K, ValueError)
        super()._camera(raster_settings, rows)
        self._cam_stride = stride

    def num_rendered(self):
        nr = (C.c_int64 * self.K)()
        _lib.check(self.lib.sg_read_num_rendered_frames(_ptr(self.binning), self.P, self.W, self.H, self.cap, self.K, nr,
                                                        self._stream()), "read R")
        return [int(v) for v in nr]


class SkinnedFramesEngine(_FramesEngine):
    """LBS-fused path, K posed frames of the same canonical Gaussians per call.  Flat gradient layout as ``SkinnedEngine``
    (xyz_canon 3P, scales 3P, opacity P, sh 3MP, [rot_canon]); per frame: ``color`` [K,3,H,W], ``radii`` [K,P], ``d_means2D``
    [K,P,3], ``d_A`` [K,J,16], ``d_transl`` [K,3].  ``aux``: the forward also writes ``depth`` and ``alpha`` [K,1,H,W] (the
    ``*_frames_aux`` entry points: no ``phase`` split, no ``sh_planar``, the backward writes the gradients)."""

    def __init__(self, P, J, W, H, sh_coeffs, K, device, capacity_pairs, with_rot=False, grad_flat=None, rot_width=9, sh_planar=False,
                 aux=False):
        self.aux = bool(aux)
        if self.aux and sh_planar:
            raise ValueError("SkinnedFramesEngine: the depth / alpha maps (aux=True) do not support sh_planar")
        super().__init__(P, W, H, sh_coeffs, device, capacity_pairs, K)
        self.J = int(J)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.aux_ws = self.depth = self.alpha = None
        if self.aux:
            self.aux_ws = torch.empty(_lib.frames_aux_layout(self.P, self.W, self.H, self.cap, self.K), dtype=torch.uint8, device=self.dev)
            self.depth = torch.empty((self.K, 1, self.H, self.W), **f32)
            self.alpha = torch.empty((self.K, 1, self.H, self.W), **f32)
        self.skin_ws = torch.empty(int(self.lib.sg_skin_ws_floats_frames(self.P, self.K)), **f32)
        self._gradients(_skinned_fields(self.M, with_rot, rot_width), grad_flat, sh_planar)
        self.d_A = torch.empty((self.K, self.J, 16), **f32); self.d_transl = torch.empty((self.K, 3), **f32)
        self._k = None
        self._forward_only = False        # set_frames: the frames carry ext_tfs or a per-frame smpl_scale (no backward)

    def set_frames(self, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs=None):
        """``A``: [K,J,4,4] / [K,J,16] joint transforms of the K frames; ``transl``: [K,3] (one per frame), [3] (shared) or None.
        ``smpl_scale``: None, [1] (shared) or [K] / [K,1] (one per frame).  ``ext_tfs``: None or the placement (trans, rotmat, scale)
        of sings_hybrid.py:421-428, shared ([3], [3,3], [1], or with a leading 1) or one per frame ([K,3], [K,3,3], [K,1]); an
        ``.expand`` view (the reference's AnimDataset_opt.get_chunk) is passed as the one shared set it is.  Per-frame sets reach
        the kernels as SgFrameBatch.placement bits (include/sings_hip.h, SG_PLACEMENT_*).  A placement or a per-frame scale is
        forward-only, as in the reference (no_grad): ``backward*`` then raises."""
        A = A.reshape(self.K, -1, 16)
        if A.shape[1] != self.J:
            raise ValueError(f"A must be [{self.K},{self.J},16]")
        self._kkeep = []
        if transl is not None:
            transl = transl.contiguous().float()
        placement = 0
        if smpl_scale is not None:
            smpl_scale, per = _frame_rows(smpl_scale, self.K, 1, "smpl_scale")
            placement |= _lib.PLACEMENT_SMPL_SCALE if per else 0
        if ext_tfs is not None:
            rows = [_frame_rows(x, self.K, w, n) for x, w, n in zip(ext_tfs, (3, 9, 1), ("ext trans", "ext rotmat", "ext scale"))]
            if any(per for _, per in rows):                  # (one set per frame for all three: a shared one is repeated)
                ext_tfs = tuple(x if per else x.reshape(1, -1).expand(self.K, -1) for x, per in rows)
                placement |= _lib.PLACEMENT_EXT_TFS
            else:
                ext_tfs = tuple(x for x, _ in rows)
        self._k, self._fb, self._forward_only = _skin_frames(self.dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl,
                                                             ext_tfs, self._cam_stride, self._kkeep, ValueError, placement)

    def _check_backward(self):
        if self._forward_only:
            raise RuntimeError("SkinnedFramesEngine: these frames carry ext_tfs or a per-frame smpl_scale, which are forward-only "
                               "(set_frames without them to differentiate)")

    def forward(self, shs, opacities, scales, sync_num_rendered=False, phase=None, posed_out=None):
        """``phase``: None = the whole forward; "binning" / "composite" = its two halves as separate calls on the same workspaces
        (SG_FLAG_FORWARD_BINNING / _COMPOSITE), for a caller that runs them on different streams and orders them with events.
        ``posed_out``: optional (xyz [K,P,3], quaternions [K,P,4], scales [K,P,3]) fp32 tensors the posed values of the K frames are
        also written to (what forward_chunk returns, sings_hybrid.py:512-553; the render itself never reads them back).
        ``aux`` engines also write ``depth`` / ``alpha`` and take no ``phase``."""
        if self._s is None or self._fb is None or self._k is None:
            raise RuntimeError("SkinnedFramesEngine: set_camera() and set_frames() first")
        if self.aux and phase is not None:
            raise ValueError("SkinnedFramesEngine: the depth / alpha maps (aux=True) have no phase split")
        if posed_out is not None:
            for x, wdt in zip(posed_out, (3, 4, 3)):
                if (tuple(x.shape) != (self.K, self.P, wdt) or x.dtype != torch.float32 or not x.is_contiguous() or x.device != self.dev):
                    raise ValueError(f"posed_out: contiguous fp32 [{self.K},{self.P},3|4|3] tensors on {self.dev}")
        pxyz, pq, psc = posed_out if posed_out is not None else (None, None, None)
        nr = (C.c_int64 * self.K)()
        self._fb.camera_stride = self._cam_stride
        self._s.flags = self._flags() | {None: 0, "binning": _lib.FLAG_FORWARD_BINNING, "composite": _lib.FLAG_FORWARD_COMPOSITE}[phase]
        if phase == "composite":
            self._s.flags &= ~_lib.FLAG_WS_CLEAN
        self._clean = False
        args = (C.byref(self._s), C.byref(self._fb), self.P, C.byref(self._k), _ptr(shs), _ptr(opacities), _ptr(scales),
                _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.img), _ptr(self.color), _ptr(self.radii), _ptr(pxyz), _ptr(pq),
                _ptr(psc), nr if sync_num_rendered and phase != "composite" else None)
        if self.aux:
            _lib.check(self.lib.sg_skinned_forward_frames_aux(*args, _ptr(self.aux_ws), _ptr(self.depth), _ptr(self.alpha),
                                                              self._stream()), "skinned forward (frames, depth / alpha maps)")
        else:
            _lib.check(self.lib.sg_skinned_forward_frames(*args, self._stream()), "skinned forward (frames)")
        self._clean = phase != "binning"                      # (the COMPOSITE leaves the counters zeroed for the next forward)
        return [int(v) for v in nr] if sync_num_rendered and phase != "composite" else None

    def backward(self, shs, opacities, scales, dL_dcolor, accumulate=False, dL_ddepth=None, dL_dalpha=None):
        """``dL_dcolor`` [K,3,H,W].  ``accumulate``: the K frames' sum is ADDED to the gradient buffer (a later batch of the step).
        ``dL_ddepth`` / ``dL_dalpha``: [K,1,H,W] adjoints of the maps (``aux`` engines; None: zero)."""
        self.backward_records(dL_dcolor, dL_ddepth, dL_dalpha)
        self.backward_gaussians(shs, opacities, scales, accumulate)

    def backward_records(self, dL_dcolor, dL_ddepth=None, dL_dalpha=None):
        """First half of ``backward``: the per-tile composite backward of the K frames (VALU-bound).  ``aux`` engines also take the
        maps' adjoints (and write every frame's dL/dz plane into ``aux_ws``)."""
        self._check_backward()
        if not self.aux and (dL_ddepth is not None or dL_dalpha is not None):
            raise ValueError("SkinnedFramesEngine: dL_ddepth / dL_dalpha need an engine built with aux=True")
        args = (C.byref(self._s), C.byref(self._fb), self.P, _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.img),
                _ptr(self.bwd_ws), _ptr(dL_dcolor))
        if self.aux:
            _lib.check(self.lib.sg_rasterize_backward_records_frames_aux(*args, _ptr(self.aux_ws), _ptr(dL_ddepth), _ptr(dL_dalpha),
                                                                         self._stream()),
                       "skinned backward (records, frames, depth / alpha maps)")
        else:
            _lib.check(self.lib.sg_rasterize_backward_records_frames(*args, self._stream()), "skinned backward (records, frames)")

    def backward_gaussians(self, shs, opacities, scales, accumulate=False):
        """Second half: record sums + the per-Gaussian chain rule summed over the K frames (latency-bound).  ``aux`` engines add
        every frame's dL/dz to its posed means and write the gradients (no ``accumulate``)."""
        self._check_backward()
        accumulate, done = self._chain_begin(accumulate)
        if self.aux and accumulate:
            raise ValueError("SkinnedFramesEngine: the depth / alpha maps (aux=True) write the gradients (no accumulate)")
        args = (C.byref(self._s), C.byref(self._fb), self.P, C.byref(self._k), _ptr(shs), _ptr(opacities), _ptr(scales),
                _ptr(self.radii), _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.bwd_ws), _ptr(self.skin_ws),
                int(accumulate), None, None, _ptr(self.d_xyz), _ptr(self.d_rot), _ptr(self.d_scales), _ptr(self.d_opacity),
                _ptr(self.d_sh), _ptr(self.d_means2D), _ptr(self.d_A), _ptr(self.d_transl))
        if self.aux:
            _lib.check(self.lib.sg_skinned_backward_gaussians_frames_aux(*args, _ptr(self.aux_ws), self._stream()),
                       "skinned backward (gaussians, frames, depth / alpha maps)")
        else:
            _lib.check(self.lib.sg_skinned_backward_gaussians_frames(*args, self._stream()), "skinned backward (gaussians, frames)")
        self._chain_end(done)


class RasterFramesEngine(_FramesEngine):
    """Un-skinned path: K cameras of the same Gaussians per call (``sg_rasterize_*_frames``).  Flat gradient layout as
    ``RasterEngine`` (``sh_planar``: dL/dsh coefficient-major [M,P,3]); ``color`` [K,3,H,W], ``radii`` [K,P], ``d_means2D`` [K,P,3].

    ``order`` (include/sings_order.h, sings_amd/work_order.py): the work order the forward bins its pairs in.  None: the Morton order
    of the positions, built on the first ``forward`` whose frame is in the direct many-tile regime and kept until
    ``refresh_order()`` (call it when the Gaussians have moved far, or after a densification that keeps P) -- a stale order is
    still correct, only slower; an int32 tensor [P]: that permutation; False: no order (the unordered entry points).  The results
    are the same bits whichever is used."""

    def __init__(self, P, W, H, sh_coeffs, K, device, capacity_pairs, grad_flat=None, sh_planar=False, order=None):
        super().__init__(P, W, H, sh_coeffs, device, capacity_pairs, K)
        self._gradients(_raster_fields(self.M), grad_flat, sh_planar)
        self.set_order(order)

    def set_order(self, order):
        """``order`` as in the constructor: None (build and keep the Morton order), an int32 tensor [P], or False."""
        if order is None and not _ORDER_BY_DEFAULT:
            order = False
        self._order_auto = order is None
        self._order = None if order is None or order is False else _work_order.check_order(order, self.P, self.geom.device)

    def set_camera(self, raster_settings, short_lists=False, long_rows=False):
        """As ``RasterEngine.set_camera``, with one camera or K."""
        self._camera(raster_settings, (_lib.FLAG_SHORT_LISTS if short_lists else 0) | (_lib.FLAG_LONG_ROWS if long_rows else 0))
        self._fb = _frame_batch(self.K, self._cam_stride, 0)

    def refresh_order(self):
        """Drop the built order: the next ``forward`` builds it again from the positions it is given."""
        if self._order_auto:
            self._order = None

    def _order_for(self, means3D):
        """The order of this call (None: the unordered launch).  Built here once, outside any graph capture."""
        if self._order is not None and not _lib.HAS_ORDER:
            raise RuntimeError("RasterFramesEngine: this library predates include/sings_order.h and takes no work order")
        if (self._order is None and self._order_auto and _lib.HAS_ORDER and self.P > 0
                and _work_order.order_applies(self.W, self.H, self._rows)):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RasterFramesEngine: the work order is built on the first forward, which cannot be inside a graph "
                                   "capture (run one forward first, or pass order=False / order=<tensor>)")
            self._order = _work_order.build_order(means3D)
        return self._order

    def forward(self, means3D, shs, opacities, scales, rotations, sync_num_rendered=False):
        if self._s is None or self._fb is None:
            raise RuntimeError("RasterFramesEngine: set_camera() first")
        order = self._order_for(means3D)
        nr = (C.c_int64 * self.K)()
        self._s.flags = self._flags()
        self._clean = False
        args = (C.byref(self._s), C.byref(self._fb), self.P, _ptr(means3D), _ptr(shs), None, _ptr(opacities), _ptr(scales),
                _ptr(rotations), None, _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.img), _ptr(self.color),
                _ptr(self.radii), nr if sync_num_rendered else None)
        if order is None:
            _lib.check(self.lib.sg_rasterize_forward_frames(*args, self._stream()), "forward (frames)")
        else:
            _lib.check(self.lib.sg_rasterize_forward_frames_ordered(*args, _ptr(order), order.numel(), self._stream()),
                       "forward (frames, ordered)")
        self._clean = True
        return [int(v) for v in nr] if sync_num_rendered else None

    def backward(self, means3D, shs, opacities, scales, rotations, dL_dcolor, accumulate=False):
        _lib.check(self.lib.sg_rasterize_backward_records_frames(
            C.byref(self._s), C.byref(self._fb), self.P, _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.img),
            _ptr(self.bwd_ws), _ptr(dL_dcolor), self._stream()), "backward (records, frames)")
        accumulate, done = self._chain_begin(accumulate)
        _lib.check(self.lib.sg_rasterize_backward_gaussians_frames(
            C.byref(self._s), C.byref(self._fb), self.P, _ptr(means3D), _ptr(shs), None, _ptr(opacities), _ptr(scales),
            _ptr(rotations), None, _ptr(self.radii), _ptr(self.geom), _ptr(self.binning), self.cap, _ptr(self.bwd_ws),
            int(accumulate), _ptr(self.d_means3D), _ptr(self.d_means2D), _ptr(self.d_sh), None, _ptr(self.d_opacity),
            _ptr(self.d_scales), _ptr(self.d_rots), None, self._stream()), "backward (gaussians, frames)")
        self._chain_end(done)


class FramePipeline:
    """The batches of frames of ONE optimisation step on TWO streams, by kind of kernel instead of by batch.

    A frame's chain alternates between kernels that keep the vector ALUs busy (the two composite kernels: half of an avatar frame)
    and kernels that wait -- binning, long-list sort, loss, record sums, per-Gaussian backward: a handful of waves per SIMD in
    dependent chains, a fifth of the chip's issue slots.  Batch-per-stream scheduling (``ViewBatch``) overlaps them only by
    accident.  Here stream A runs nothing but the composite kernels of all batches, back to back; stream B (high priority, so that
    its short kernels get wave slots as soon as they are ready) runs everything else, issued in an order that always has the
    other batch's light work ready beside the running composite:

        B:  bin 0 | bin 1 | .. | loss 0 | loss 1 | .. | per-Gaussian 0 | per-Gaussian 1 | ..
        A:          fwd 0 | fwd 1 | ..   | records 0 | records 1 | ..

    (events order a batch's own phases across the streams).  The per-Gaussian halves run in batch order on B and share ONE gradient
    buffer -- batch 0 writes, the others add: bit for bit the sum that the same batches give one after the other on one stream.
    Engines: ``SkinnedFramesEngine`` objects bound to the same ``grad_flat`` (``rebind_gradients``)."""

    def __init__(self, engines, device):
        self.engines = list(engines)
        self.dev = torch.device(device)
        self.A = torch.cuda.Stream(self.dev)
        self.B = torch.cuda.Stream(self.dev, priority=-1)
        self.ev = [[torch.cuda.Event() for _ in range(4)] for _ in self.engines]
        for e in self.engines:
            e.throughput = True
            if e.grad_flat.data_ptr() != self.engines[0].grad_flat.data_ptr():
                raise ValueError("FramePipeline: every engine must be bound to the same gradient buffer (rebind_gradients)")

    def run(self, prepare, forward_args, loss):
        """``prepare(b, engine)``: set the batch's frames (runs on B); ``forward_args`` = (shs, opacities, scales);
        ``loss(b, engine)`` -> dL_dcolor [K,3,H,W] (runs on B, after the batch's composite)."""
        cur = torch.cuda.current_stream(self.dev)
        A, B, ev = self.A, self.B, self.ev
        A.wait_stream(cur); B.wait_stream(cur)
        for b, e in enumerate(self.engines):
            with torch.cuda.stream(B):
                prepare(b, e)
                e.forward(*forward_args, phase="binning")
                ev[b][0].record(B)
            with torch.cuda.stream(A):
                A.wait_event(ev[b][0])
                e.forward(*forward_args, phase="composite")
                ev[b][1].record(A)
        grads = []
        for b, e in enumerate(self.engines):
            with torch.cuda.stream(B):
                B.wait_event(ev[b][1])
                grads.append(loss(b, e))
                ev[b][2].record(B)
            with torch.cuda.stream(A):
                A.wait_event(ev[b][2])
                e.backward_records(grads[b])
                ev[b][3].record(A)
        for b, e in enumerate(self.engines):
            with torch.cuda.stream(B):
                B.wait_event(ev[b][3])
                e.backward_gaussians(*forward_args, accumulate=b > 0)
        cur.wait_stream(A); cur.wait_stream(B)
