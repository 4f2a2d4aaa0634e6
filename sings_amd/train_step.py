"""One SinGS training step on one posed frame, composed from the library's pieces (what ``scripts/train_avatar.py`` ->
``GaussianTrainer.train`` does per iteration, SURVEY.md 3.1, without the optimiser / densification bookkeeping):

    decode_attributes (tri-plane + decoders)          sings_hybrid.py:249-313      sings_amd/decode.py (triplane.py, linear_layers.py)
    fused LBS + projection + binning + composite      sings_hybrid.py:398-428, gs_renderer_single.py:12-107   sings_amd/skinned.py
    clamp + L1 + SSIM                                 losses/loss.py:55-69         sings_amd/photo_loss.py
    LPIPS-VGG patch term (optional)                   losses/loss.py:71-80         sings_amd/lpips.py
    regularisers (optional)                           gs_trainer.py:355-399        sings_amd/regularizers.py
    mesh terms (optional)                             gs_trainer.py:366-399        sings_amd/mesh_terms.py
    backward through all of it

Everything between the parameters and the scalar loss runs in HIP kernels (library GEMMs for the decoders' forward /
input-gradient products); torch autograd only strings the stages together.  The regularisers depend on the decoded
attributes only, not on the render: with ``overlap_regularisers`` (default) they run on a second HIP stream next to the
LBS + raster + photometric-loss chain, also inside a captured HIP graph.  WHERE they run decides what they cost
(profiles/r03_train_step_trace.log): the k-NN query keeps 9 waves per SIMD resident on every CU for 0.23 ms, and beside it the
raster forward's latency-bound chain took 2-7x as long per kernel (the long-list sort needs a nearly empty CU per workgroup:
146 us instead of 21).  With ``defer_regulariser_join`` the query is held until the raster forward has finished and is NOT
joined before the loss: ``forward`` returns the photometric and the regulariser loss as two roots (``extras["loss_roots"]``) and
``AvatarStep.backward`` STAGES the backward pass by hand (round 5): the render and the regularisers read detached views of the
decoded attributes; the photometric gradients (loss, composite, LBS: this stream) are one ``torch.autograd.grad`` call, L2Norm's
gradients -- computed by its kernel with the value, in front of the query on the side stream -- are added with one ``_foreach_add_``,
and the decoders' backward starts from the sums.  The k-NN regulariser's gradient (scales only) enters at an identity node placed on
the geometry decoder's outputs BEFORE the appearance decoder is issued: autograd visits the youngest nodes first, so the appearance
decoder's backward is issued -- and runs beside the query -- before the main stream waits for the side stream at that node.  The
order of the launches is then the order the graph executor needs to keep the critical chain on ONE queue (sings_amd/side_launch.py
"capture order"; 2.18 -> 1.97-2.05 ms per step with the deferred weight gradients, profiles/r05_graph_queues.log).
"""
import torch

from .decode import decode_attributes
from .grad_arena import invalidate_gradient_arena
from .lpips import lpips_patch_loss
from .photo_loss import photometric_loss, photometric_loss_frames
from .side_launch import flush_triplane_prepare, reset_deferred, triplane_prepare_held
from .skinned import rasterize_skinned_frames, rasterize_skinned_gaussians


class _AddScalars(torch.autograd.Function):
    """a + b of two 0-dim losses: ONE launch forward and none backward (torch.stack(...).sum() is a concatenation and a reduction
    forward, and autograd's sum / stack backward each way; between the loss kernels and the first backward kernel every such
    4-us launch sits on the step's critical path)."""

    @staticmethod
    def forward(ctx, a, b):
        return a + b

    @staticmethod
    def backward(ctx, g):
        return g, g


def _sum_terms(loss_dict):
    """The sum of a step's photometric terms: l1 + ssim first, under ONE node that hands both the same upstream tensor (the loss
    kernel's backward is then a multiplication: sings_amd.photo_loss), the rest added behind."""
    vals = [v.reshape(()) for v in loss_dict.values()]
    total = _AddScalars.apply(vals[0], vals[1]) if len(vals) >= 2 else vals[0]
    for v in vals[2:]:
        total = total + v
    return total


class _SumFrames(torch.autograd.Function):
    """(l1[K].sum(), ssim[K].sum()) in one node whose backward hands BOTH per-frame terms the SAME upstream tensor when the two sums got
    the same one (they do under ``_AddScalars``): the photometric loss then returns the gradient it computed in the forward, times
    that tensor, instead of marching over the K images again (sings_amd.photo_loss._PhotoLossFrames.backward)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.k = int(a.shape[0])
        return a.sum(), b.sum()

    @staticmethod
    def backward(ctx, ga, gb):
        ea = ga.expand(ctx.k)
        return ea, (ea if gb is ga else gb.expand(ctx.k))


class _Inject(torch.autograd.Function):
    """Identity in the forward; the backward ADDS a gradient that arrives late from another stream (``slot[key]``: a tensor or
    None, ``slot["ready"]``: the event behind the kernel that produces it).  Placed on the geometry decoder's outputs before the appearance decoder is
    issued, so autograd reaches it -- and waits for that stream -- only after the appearance decoder's backward has been issued."""

    @staticmethod
    def forward(ctx, x, slot, key):
        ctx.slot, ctx.key = slot, key
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        extra = ctx.slot.pop(ctx.key, None)
        if extra is not None:
            cur = torch.cuda.current_stream(g.device)
            cur.wait_event(ctx.slot["ready"])                    # (not the whole side stream: more may have been issued behind it)
            extra.record_stream(cur)
            g = g + extra
        return g, None, None


def _tensors_of(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors_of(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors_of(v)


def capture_step(fn, warmup=3, device=None):
    """``graph, outputs = capture_step(fn)``: record ``fn()`` -- one whole step: forward, backward, whatever it launches -- into
    a HIP graph the safe way.  On ROCm 7.2 ``hipStreamEndCapture`` SEGFAULTS (not an error code: the process dies) when
    something ``fn`` returned still carries its autograd graph at the end of the capture (gpurun_out/crash.log, round 3): the
    saved tensors of that graph live in the capture's private memory pool on several streams.  This wrapper therefore looks at
    what ``fn`` returned BEFORE it ends the capture: if any returned tensor requires grad / has a grad_fn, the references are
    dropped first, the capture is ended cleanly (the graph is discarded) and a RuntimeError says what to do -- return
    ``loss.detach()`` (or ``.detach().clone()``) from the captured callable.  ``warmup`` eager runs on a side stream come first
    (allocator warm-up, lazily created streams), as ``torch.cuda.graph`` requires."""
    import gc
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("capture_step: a capture is already in progress on this stream")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(max(0, int(warmup))):
            out = fn()
            n_bad = sum(1 for t_ in _tensors_of(out) if t_.requires_grad or t_.grad_fn is not None)
            del out
            if n_bad:
                torch.cuda.current_stream(dev).wait_stream(side)
                raise RuntimeError(f"capture_step: the callable returns {n_bad} tensor(s) that still carry an autograd graph; "
                                   "return detached values (loss.detach()) -- ending a HIP-graph capture with them alive "
                                   "crashes hipStreamEndCapture on ROCm 7.2")
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    n_bad = 0
    with torch.cuda.graph(graph):
        out = fn()
        n_bad = sum(1 for t_ in _tensors_of(out) if t_.requires_grad or t_.grad_fn is not None)
        if n_bad:                              # (only reachable with warmup = 0) drop every reference BEFORE the capture ends
            out = None
            gc.collect()
    if n_bad:
        del graph
        raise RuntimeError(f"capture_step: the callable returned {n_bad} tensor(s) that still carry an autograd graph; the capture "
                           "was discarded.  Return detached values (loss.detach())")
    return graph, out


class AvatarStep(torch.nn.Module):
    def __init__(self, xyz_anchor, lbs_weights, triplane, geometry_dec, appearance_dec, l1_w=0.8, ssim_w=0.2,
                 thickness_factor=1.0, scaling_multiplier=None, l2_norm=None, gaussian_connect=None, gaussian_connect_w=0.0,
                 overlap_regularisers=True, defer_regulariser_join=False, lpips=None, lpips_w=0.0, lpips_patch_size=128,
                 mesh_terms=None):
        super().__init__()
        # the mesh terms (gs_trainer.py:366-399): a sings_amd.mesh_terms.MeshTerms that has been reset() for these anchors' mesh, or None
        self.mesh_terms = mesh_terms
        # the LPIPS patch term (loss.py:71-80): a sings_amd.lpips.LPIPS, its weight (human.loss.lpips_w) and patch size
        self.lpips, self.lpips_w, self.lpips_patch_size = lpips, float(lpips_w), int(lpips_patch_size)
        self.overlap_regularisers, self._side = bool(overlap_regularisers), None
        self.defer_regulariser_join = bool(defer_regulariser_join)
        self.xyz = torch.nn.Parameter(xyz_anchor.detach().clone())
        self.register_buffer("lbs_weights", lbs_weights.detach().clone())
        self.triplane, self.geometry_dec, self.appearance_dec = triplane, geometry_dec, appearance_dec
        self.l1_w, self.ssim_w, self.thickness_factor = l1_w, ssim_w, thickness_factor
        self.scaling_multiplier = scaling_multiplier
        self.l2_norm, self.gaussian_connect, self.gaussian_connect_w = l2_norm, gaussian_connect, gaussian_connect_w
        # what was captured / sized for this set of Gaussians (sings_amd.train_loop): moves on with every densify / prune / SH-degree change
        self.topology_version = 0
        self.xyz_gradient_accum = self.denom = self.max_radii2D = None
        # the reference's opt_geo / opt_app of the iteration (gs_trainer.py:225-226): False = that decoder runs without a gradient
        self.opt_geo = self.opt_app = True
        # an int32 device tensor [1]: the statistics are ONE gated launch (sings_amd.density.densify_stats) that does nothing while
        # the word is 0 -- a captured step serves deciding and non-deciding iterations alike; None: the torch chain, every step
        self.stats_gate = None
        # the attributes the L2 term reads (gs_trainer.py:356-360 leaves `opacity` out while a density window is open)
        self.l2_keys = ("xyz_offsets", "scales", "opacity")

    # ---- densification statistics and topology (sings_hybrid.py:1013-1015, 930-932; gs_trainer.py:486-492)
    def enable_densification_stats(self):
        """(Re)allocate the statistics for the current set: from now on ``forward`` hands the rasterizer a ``means2D`` holder and
        ``add_densification_stats(extras)`` after the backward accumulates |screen-space gradient|, the visibility count and the
        largest radius per Gaussian."""
        n, dev = int(self.xyz.shape[0]), self.xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        self.denom = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        self.max_radii2D = torch.zeros(n, dtype=torch.float32, device=dev)

    def stats_tensors(self):
        """The three statistics, one row per Gaussian, in the fixed order (accum, denom, max radii); () before
        ``enable_densification_stats``.  Every run of a step's body adds to them: a run that is not a step (a capture's warm-up) is
        followed by putting them back."""
        return () if self.xyz_gradient_accum is None else (self.xyz_gradient_accum, self.denom, self.max_radii2D)

    def set_stats(self, triple):
        """Replace the three statistics (the order of ``stats_tensors``): the rows a change of the set carried over."""
        self.xyz_gradient_accum, self.denom, self.max_radii2D = triple

    def add_densification_stats(self, extras):
        """``xyz_gradient_accum[vis] += |viewspace_points.grad[vis, :2]|``, ``denom[vis] += 1``, ``max_radii2D[vis] = max(., radii[vis])``
        for every frame of the step.  Masked arithmetic instead of boolean indexing: the same sums without a host round trip, so the
        call may sit inside a captured step.

        With ``stats_gate`` set the same update is one launch of ``sings_amd.density.densify_stats`` behind that gate: nothing is
        accumulated while the word is 0, and an invisible frame is skipped instead of multiplied by zero."""
        if self.xyz_gradient_accum is None:
            return
        g, radii = extras["viewspace_points"].grad, extras["radii"]
        if g is None:
            raise RuntimeError("add_densification_stats: call it after the backward pass of the step (viewspace_points.grad is empty)")
        if self.stats_gate is not None:
            from .density import densify_stats
            densify_stats(g.contiguous(), radii.contiguous(), self.xyz_gradient_accum, self.denom, self.max_radii2D,
                          gate=self.stats_gate)
            return
        g, radii = g.reshape(-1, g.shape[-2], 3), radii.reshape(-1, radii.shape[-1])
        vis = (radii > 0).to(torch.float32)                                       # [K, N]
        self.xyz_gradient_accum.add_((torch.norm(g[..., :2], dim=-1) * vis).sum(0).unsqueeze(1))
        self.denom.add_(vis.sum(0).unsqueeze(1))
        torch.maximum(self.max_radii2D, radii.to(torch.float32).max(0).values, out=self.max_radii2D)

    def set_topology(self, xyz_anchor, lbs_weights, scaling_multiplier=None):
        """A new set of Gaussians (densify / prune): new anchor PARAMETER (the old object is dead: an optimiser, a gradient arena or a
        captured graph that still holds it must be rebuilt -- ``topology_version`` says so), new skinning weights, statistics reset."""
        if xyz_anchor.shape[0] != lbs_weights.shape[0] or xyz_anchor.dim() != 2 or xyz_anchor.shape[1] != 3:
            raise ValueError("set_topology: xyz_anchor [N,3] and lbs_weights [N,J] must describe the same N Gaussians")
        self.xyz = torch.nn.Parameter(xyz_anchor.detach().clone().contiguous())
        self.lbs_weights = lbs_weights.detach().clone().contiguous()
        if scaling_multiplier is not None:
            self.scaling_multiplier = scaling_multiplier
        elif torch.is_tensor(self.scaling_multiplier) and self.scaling_multiplier.dim() > 0 and self.scaling_multiplier.shape[0] != xyz_anchor.shape[0]:
            raise ValueError("set_topology: the per-Gaussian scaling_multiplier must be passed for the new set")
        self.topology_version += 1
        invalidate_gradient_arena()
        if self.xyz_gradient_accum is not None:
            self.enable_densification_stats()

    # ---- checkpoint: the model's entries of the reference's ``SinGS.state_dict()`` (sings_hybrid.py:169-199)
    def checkpoint_entries(self):
        """``xyz``, ``triplane`` / ``geometry_dec_0`` / ``appearance_dec_0`` (the modules' own ``state_dict()``s), ``scaling_multiplier`` (None,
        a number, or a tensor: [N,1] once a densification has made it per-Gaussian), the three statistics and ``lbs_weights`` -- the
        live objects, not copies (``sings_amd.checkpoint`` copies them to the host).  One entry is not the reference's: ``opacity_offset``,
        the [N,1] tensor the appearance decoder's ``reset_opacity`` leaves behind every change of the set (None before the first).  It
        is a plain attribute, in no module's ``state_dict()`` -- the reference's file loses it, and with it the opacities."""
        stats = self.stats_tensors() or (None, None, None)
        offset = getattr(self.appearance_dec, "opacity_offset", None)
        return {"xyz": self.xyz.detach(), "triplane": dict(self.triplane.state_dict()),
                "geometry_dec_0": dict(self.geometry_dec.state_dict()), "appearance_dec_0": dict(self.appearance_dec.state_dict()),
                "scaling_multiplier": self.scaling_multiplier, "xyz_gradient_accum": stats[0], "denom": stats[1], "max_radii2D": stats[2],
                "lbs_weights": self.lbs_weights, "opacity_offset": offset if torch.is_tensor(offset) else None}

    @torch.no_grad()
    def load_checkpoint_entries(self, entries, replace_set=None):
        """The reverse, for entries whose shapes the caller has checked (``checkpoint.validate_model``): the three modules load in place
        (their parameter objects stay), the set is replaced at the saved N -- through ``replace_set(xyz, lbs_weights,
        scaling_multiplier)`` when a trainer owns the optimiser and what is sized by N, else ``set_topology`` -- and the statistics, if
        the entries carry them, are put back behind it.  ``opacity_offset``: the saved tensor, or -- None, or a file of the
        reference's that has no such entry -- the decoder's initial 0, as a model the reference reloads has it."""
        dev = self.xyz.device
        self.triplane.load_state_dict(entries["triplane"])
        self.geometry_dec.load_state_dict(entries["geometry_dec_0"])
        self.appearance_dec.load_state_dict(entries["appearance_dec_0"])
        if not getattr(self.appearance_dec, "fixed_opacity", False):
            offset = entries.get("opacity_offset")
            self.appearance_dec.opacity_offset = 0 if offset is None else offset.to(dev, torch.float32).clone().contiguous()
        xyz, sm = entries["xyz"].to(dev), entries["scaling_multiplier"]
        n = int(xyz.shape[0])
        per_gaussian = torch.is_tensor(sm) and sm.dim() == 2 and tuple(sm.shape) == (n, 1) and n != 1
        if torch.is_tensor(sm):
            sm = sm.to(dev).clone()
        if not per_gaussian:
            self.scaling_multiplier, sm = sm, None               # (a scalar for every Gaussian: nothing to pass for the new set)
        if replace_set is not None:
            replace_set(xyz, entries["lbs_weights"].to(dev), sm)
        else:
            self.set_topology(xyz, entries["lbs_weights"].to(dev), scaling_multiplier=sm)
        stats = [entries.get(k) for k in ("xyz_gradient_accum", "denom", "max_radii2D")]
        if all(t is not None for t in stats):
            self.set_stats([t.to(dev, torch.float32).clone().contiguous() for t in stats])

    def set_trainable(self, opt_geo=True, opt_app=True):
        """The decoders that learn from now on (gs_trainer.py:225-226; sings_hybrid.py:265-277: a decoder whose flag is False is decoded
        under no_grad -- here by ``decode.decode_attributes(opt_geo=, opt_app=)``).  With both False the tri-plane gets no gradient
        either: only the anchors (and a learned pose) do.  A change moves ``topology_version`` on: the set of tensors that receive a
        gradient is part of a captured step, which is refused and captured again like after a densify."""
        flags = (bool(opt_geo), bool(opt_app))
        if flags != (self.opt_geo, self.opt_app):
            self.opt_geo, self.opt_app = flags
            self.topology_version += 1

    def forward(self, A_cano2pose, raster_settings, gt_rgb, mask, bg_color, smpl_scale=None, transl=None, lpips_origins=None,
                lpips_bg=None):
        """-> (loss, loss_dict, extras).  ``A_cano2pose`` [J,4,4]: one frame per step (the reference's step); [K,J,4,4]: a chunk
        of K <= 16 frames of the step's Gaussians -- ONE attribute decode, the K frames rendered, compared (``gt_rgb`` / ``mask``
        [K,...] or one for all) and differentiated in one call per direction, the photometric terms summed over the frames,
        the regularisers once (``transl`` [K,3] / [3]; cameras: one, or stacked [K,4,4] / [K,3] in ``raster_settings``).  With ``defer_regulariser_join`` (and gradients enabled, regularisers present) ``loss``
        is **None**: the photometric and the regulariser terms are two autograd roots (``extras["loss_roots"]``) -- call
        ``self.backward(loss_dict, extras)``, which runs both, joins the regularisers' side stream and fills
        ``loss_dict["loss"]``.  Until then the regulariser entries of ``loss_dict`` live on that UNJOINED stream: do not read
        them (``.item()``, logging) before ``backward`` -- or call ``self.join_regularisers(loss_dict)`` first.
        With ``lpips`` and ``lpips_w`` > 0 set, ``lpips_origins`` ([n,2] / [K,n,2] device int (row, col) patch corners:
        ``sings_amd.lpips.PatchSampler``) adds ``loss_dict['lpips_patch']``; ``lpips_bg`` is the random background of the
        term (the reference's ``torch.rand_like(pred_img)``; drawn here when None).
        Inside a HIP-graph capture: use ``sings_amd.train_step.capture_step`` (it refuses, with an error instead of a dead
        process, a captured callable that returns tensors still carrying their autograd graph), and keep the regularisers on
        the ONE side stream this module owns (``GaussiansEdgeLoss.finish`` refuses any other stream while capturing)."""
        has_knn = self.gaussian_connect is not None and self.gaussian_connect_w > 0
        has_reg = self.l2_norm is not None or has_knn or self.mesh_terms is not None
        overlap = has_reg and self.overlap_regularisers and self.xyz.is_cuda
        defer = (overlap and self.defer_regulariser_join and torch.is_grad_enabled() and has_knn
                 and hasattr(self.gaussian_connect, "prepare"))
        inject = {} if defer else None                           # the k-NN regulariser's gradient (scales only: its edge lengths are
        hook = (lambda x, sc: (x, _Inject.apply(sc, inject, "scales"))) if defer else None          # detached, loss_items.py:75)
        # the tri-plane backward's point sorts (side_launch.py: "the point-only half ... early") are held back: beside the first decoder
        # layers they cost the forward chain ~70 us (the first layer: 121 instead of 53 us); here they are issued on the regularisers'
        # stream behind the k-NN query, long before the tri-plane backward needs them
        with triplane_prepare_held(defer):                       # (also drops a preparation left behind by a forward that raised)
            attrs = self.decode(geometry_hook=hook, opt_geo=self.opt_geo, opt_app=self.opt_app)
        # Two roots (defer): the render and the regularisers read DETACHED views of the decoded attributes (`use`), so that the
        # backward pass can be staged by hand (AvatarStep.backward): photometric gradients on this stream, the regularisers' on the
        # side stream, one addition, then the decoders' backward -- in an order the graph executor turns into ONE queue for the
        # critical chain (sings_amd/side_launch.py "capture order").  One root: `use` IS `attrs`, plain autograd.
        use = attrs
        if defer:
            use = {k: (v.detach().requires_grad_(v.requires_grad) if torch.is_tensor(v) else v) for k, v in attrs.items()}
        reg = {}

        def regularisers():
            if self.l2_norm is not None:
                reg["l2"] = self._l2(use)
            if self.mesh_terms is not None:
                reg.update(self.mesh_terms(use))
            if has_knn:
                reg["gaussian_connect_loss"] = self.gaussian_connect_w * self.gaussian_connect(
                    {"xyz_canon": use["xyz_canon"], "scales": use["scales"]})

        side = cur = decoded = rendered = None
        if overlap:
            dev = attrs["xyz_canon"].device
            if self._side is None or self._side.device != dev:
                self._side = torch.cuda.Stream(dev)
            side, cur = self._side, torch.cuda.current_stream(dev)
            if defer:
                decoded = torch.cuda.Event()
                decoded.record(cur)                              # fork point; the side stream's work is ISSUED after the photometric loss
            else:
                side.wait_stream(cur)                            # fork: the decoded attributes are complete
                with torch.cuda.stream(side):
                    regularisers()
        frames = A_cano2pose.dim() == 4                          # [K,J,4,4]: a CHUNK of K frames of this step's Gaussians (round 4)
        # the screen-space gradient the densifier reads (gs_renderer_single.py:50-56): a holder per step, only when statistics are kept
        m2d = None
        if self.xyz_gradient_accum is not None and torch.is_grad_enabled():
            shape = (int(A_cano2pose.shape[0]), int(self.xyz.shape[0]), 3) if frames else (int(self.xyz.shape[0]), 3)
            m2d = torch.zeros(shape, dtype=torch.float32, device=self.xyz.device, requires_grad=True)
        # frames: one decode, K frames rendered and differentiated in one call per direction: the attribute decode -- 3/4 of a
        # one-frame step -- is paid once per step, not once per frame (gt_rgb / mask: [K,...] or one for all frames).
        # anisotropic: the decoder's 6-D rotations go to the fused kernels as they are (rotation_6d_to_matrix of
        # sings_hybrid.py:356-357 runs inside them); isotropic: None
        rasterize = rasterize_skinned_frames if frames else rasterize_skinned_gaussians
        color, radii = rasterize(use["xyz_canon"], use["rot6d_canon"], use["scales"], use["opacity"], use["shs"], self.lbs_weights,
                                 A_cano2pose, raster_settings, smpl_scale=smpl_scale, transl=transl, means2D=m2d)
        if defer:
            rendered = torch.cuda.Event()
            rendered.record(cur)
        if frames:
            per_frame, extras = photometric_loss_frames(color, gt_rgb, mask, bg_color, self.l1_w, self.ssim_w)
            if len(per_frame) == 2:                                         # the step's photometric terms: summed over its frames
                loss_dict = dict(zip(per_frame.keys(), _SumFrames.apply(*per_frame.values())))
            else:
                loss_dict = {k: v.sum() for k, v in per_frame.items()}
            extras = dict(extras, per_frame=per_frame)
        else:
            loss_dict, extras = photometric_loss(color, gt_rgb, mask, bg_color, self.l1_w, self.ssim_w)
        if self.lpips is not None and self.lpips_w > 0.0 and lpips_origins is not None:
            # behind the l1 / ssim pair: their shared _AddScalars node stays as it is, this term is added after it
            bg_rand = torch.rand_like(color) if lpips_bg is None else lpips_bg
            lp = lpips_patch_loss(color, gt_rgb, mask, bg_color, bg_rand, lpips_origins, self.lpips_patch_size, self.lpips,
                                  self.lpips_w)
            loss_dict["lpips_patch"] = lp.sum() if frames else lp
            if frames:
                extras["per_frame"] = dict(extras["per_frame"], lpips_patch=lp)
        if defer:
            self._finish_deferred(loss_dict, extras, attrs, use, inject, side, decoded, rendered)
            # a pose that is itself learned (sings_amd.pose.PoseTable): the staged backward hands its gradients on
            extras["pose_inputs"] = [t for t in (A_cano2pose, transl) if torch.is_tensor(t) and t.requires_grad]
        loss = None if defer else self._finish_joined(loss_dict, reg, regularisers, side)
        return loss, loss_dict, {"render_raw": color, "radii": radii, "attrs": attrs, "viewspace_points": m2d, **extras}

    def decode(self, geometry_hook=None, opt_geo=True, opt_app=True):
        """The decoded attributes of the current set (``decode.decode_attributes`` of this module's anchors, tri-plane and decoders).
        ``opt_geo`` / ``opt_app``: the training step passes its own flags; every other caller decodes as before."""
        return decode_attributes(self.xyz, self.triplane, self.geometry_dec, self.appearance_dec, self.thickness_factor,
                                 self.scaling_multiplier, geometry_hook=geometry_hook, opt_geo=opt_geo, opt_app=opt_app)

    def _l2(self, a):                                            # (`a`: the decoded attributes, or their detached copy)
        return self.l2_norm({k: a[k] for k in self.l2_keys})     # (without `opacity`: L2Norm leaves its term and its gradient out)

    def _finish_deferred(self, loss_dict, extras, attrs, use, inject, side, decoded, rendered):
        """The two-roots tail of ``forward``, no join: the regularisers' gradients are waited for where they are consumed
        (``AvatarStep.backward``).  ``decoded`` / ``rendered``: the main stream's events behind the decode and the raster forward."""
        photo_root = _sum_terms(loss_dict)
        # the regularisers, ISSUED last (the main chain keeps its queue in the graph executor, sings_amd/side_launch.py "capture
        # order") but waiting only for what they read: L2Norm and the k-NN grids for the decode, the k-NN QUERY -- 9 waves per
        # SIMD on every CU for 0.23 ms -- for the raster forward.  (Measured, profiles/r05_graph_queues.log: the executor starts
        # a second queue's chain 60-160 us after its dependency is met, so part of the query is still exposed behind the
        # backward composite; issued FIRST, as in round 4, the chain starts at once and the raster forward is what waits.)
        # No autograd on the side stream: both regularisers' kernels compute their gradients with the value (`last_grads`), and the
        # engine's stream bookkeeping around an autograd call put a wait for THIS stream's newest kernel in front of them.
        side.wait_event(decoded)
        reg, l2_grads, mt_grads = {}, None, None
        det = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in use.items()}
        with torch.cuda.stream(side):
            if self.mesh_terms is not None:
                # in front of the k-NN preparation: three launches whose gradients (`last_grads`, buffers the module owns) join the
                # photometric ones in step 2 of the staged backward
                reg.update(self.mesh_terms(det))
                mt_grads = (self.mesh_terms.last_grads, torch.cuda.Event())
                mt_grads[1].record(side)
            if self.l2_norm is not None:
                # in front of the k-NN query on this stream: the appearance decoder's backward needs the opacity term
                reg["l2"] = self._l2(det)
                l2_grads = (dict(self.l2_norm.last_grads), torch.cuda.Event())
                l2_grads[1].record(side)
            edge = self.gaussian_connect.prepare({"xyz_canon": det["xyz_canon"], "scales": det["scales"]})
            side.wait_event(rendered)
            try:
                self.gaussian_connect.finish()
            except BaseException:
                self.gaussian_connect.abort()
                raise
            g_edge = self.gaussian_connect.last_grads["scales"]
            if self.gaussian_connect_w != 1.0:
                edge, g_edge = self.gaussian_connect_w * edge, self.gaussian_connect_w * g_edge
            reg["gaussian_connect_loss"] = edge
            if use["scales"].requires_grad:
                inject["scales"] = g_edge                    # reaches the decoders' backward through the _Inject node
            reg_root = edge.reshape(())
            inject["ready"] = torch.cuda.Event()
            inject["ready"].record(side)
            flush_triplane_prepare(side)                # (same stream, behind the query: executed in this order)
        loss_dict.update(reg)
        extras["loss_roots"] = (photo_root, reg_root)
        extras["staged"] = (attrs, use, inject, l2_grads)
        extras["staged_mesh_terms"] = mt_grads

    def _finish_joined(self, loss_dict, reg, regularisers, side):
        """The one-root tail of ``forward``: the regularisers joined (or, without a side stream, run here), -> the loss."""
        if side is not None:
            self.join_regularisers(reg)                          # join before the loss terms meet
        else:
            regularisers()
        loss = _sum_terms(loss_dict)
        for v in reg.values():
            loss = loss + v.reshape(())
        loss_dict.update(reg)
        loss_dict["loss"] = loss
        return loss

    def join_regularisers(self, loss_dict=None):
        """Make the current stream wait for the regularisers' side stream (a ``defer_regulariser_join`` forward leaves it
        unjoined), so that the regulariser losses can be read before ``backward``."""
        if self._side is not None:
            cur = torch.cuda.current_stream(self._side.device)
            cur.wait_stream(self._side)
            for v in (loss_dict or {}).values():
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(cur)

    def backward(self, loss_dict, extras):
        """Backward pass of a ``defer_regulariser_join`` forward, staged by hand (module docstring); then the streams join and
        ``loss_dict["loss"]`` = the sum of the terms.  (A forward that returned a loss: ``loss.backward()`` as usual.)"""
        try:
            return self._backward_staged(loss_dict, extras)
        except BaseException:
            reset_deferred()                                # (closures with raw gradient pointers must not outlive the pass)
            raise

    def _backward_staged(self, loss_dict, extras):
        photo_root, reg_root = extras["loss_roots"]
        attrs, use, inject, l2_grads = extras["staged"]
        one = getattr(self, "_one", None)
        if one is None or one.device != photo_root.device:
            from .photo_loss import register_unit_scalar
            one = self._one = register_unit_scalar(torch.ones((), dtype=photo_root.dtype, device=photo_root.device))     # (not a fill launch per root and step)
        dev = photo_root.device
        cur, side = torch.cuda.current_stream(dev), self._side
        names = [k for k, v in use.items() if torch.is_tensor(v) and v.requires_grad]
        leaves = [use[k] for k in names]
        m2d = extras.get("viewspace_points")
        pose_in = extras.get("pose_inputs", [])
        # 1. the photometric gradients of the decoded attributes: loss, composite, LBS -- on this stream, issued first
        got = torch.autograd.grad([photo_root], leaves + pose_in + ([m2d] if m2d is not None else []), [one], allow_unused=True)
        if m2d is not None:
            m2d.grad = got[-1]                                   # (what add_densification_stats reads: the densifier's statistic)
        g = dict(zip(names, got))
        pose_roots = [(t, x) for t, x in zip(pose_in, got[len(leaves):len(leaves) + len(pose_in)]) if x is not None]
        # 2. L2Norm's gradients (computed with its value, in front of the k-NN query on the side stream): ONE addition for the
        #    attributes that have both.  The k-NN regulariser's gradient (scales) is already in `inject`: it reaches the decoders'
        #    backward through the _Inject node, i.e. AFTER the appearance decoder's backward has been issued
        if l2_grads is not None:
            cur.wait_event(l2_grads[1])
            both_a, both_b = [], []
            for k, gr in l2_grads[0].items():
                if gr is None or k not in g:                     # (None: an attribute `l2_keys` leaves out -- no term, no gradient)
                    continue
                gr.record_stream(cur)
                if g[k] is None:
                    g[k] = gr
                else:
                    both_a.append(g[k]); both_b.append(gr)
            # (not torch._foreach_add_: its 64 k-element chunks make ten workgroups of the two 150 k-row attributes -- 19 us alone on the
            #  chip, 92 beside the k-NN query of the side stream; an add per tensor is 5 us.  The step itself did not get shorter
            #  for it -- 1.867-1.875 ms either way, same box: its length is the work of BOTH queues, LAB 6.8)
            for x, y in zip(both_a, both_b):
                x.add_(y)
        #    the mesh terms' gradients, next to them; the colour gradient goes into the DC rows of the photometric `shs` gradient in
        #    place (no [N,16,3] temporary)
        mt_grads = extras.get("staged_mesh_terms")
        if mt_grads is not None:
            cur.wait_event(mt_grads[1])
            for k in ("xyz_canon", "scales"):
                if k in g:
                    g[k] = mt_grads[0][k].clone() if g[k] is None else g[k].add_(mt_grads[0][k])
            if "shs" in g:
                if g["shs"] is None:
                    g["shs"] = torch.zeros_like(use["shs"])
                (g["shs"][:, 0] if g["shs"].dim() == 3 else g["shs"]).add_(mt_grads[0]["shs_dc"])
        # 3. the decoders' backward: appearance decoder first (its nodes are the youngest), then the _Inject node waits for the side stream
        #    (behind them the learned pose's dL/dA and dL/dtransl, if any: the oldest node of the step, one launch, reached last)
        roots = [(attrs[k], g[k]) for k in names if g.get(k) is not None] + pose_roots
        torch.autograd.backward([r for r, _ in roots], [x for _, x in roots])
        cur.wait_stream(side)
        for v in list(loss_dict.values()) + [reg_root]:
            v.record_stream(cur)
        total = photo_root.detach() + reg_root.detach()
        if l2_grads is not None:
            total = total + loss_dict["l2"].reshape(())
        if mt_grads is not None:
            for k in self.mesh_terms.KEYS:
                total = total + loss_dict[k].reshape(())
        loss_dict["loss"] = total
        return loss_dict["loss"]
