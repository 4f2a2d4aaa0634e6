"""The per-iteration bookkeeping of ``GaussianTrainer.train`` around ``AvatarStep`` -- what changes BETWEEN steps, and with it the
number of Gaussians every pre-sized piece of the hot path was built for:

    Adam step over the anchors, tri-plane and decoders                      gs_trainer.py:240-262
    densification statistics (screen-space gradient norm, visibility
    count, largest radius) after every backward                             gs_trainer.py:486-492, sings_hybrid.py:1013-1015
    ``oneupSHdegree`` every ``sh_interval`` steps                           gs_trainer.py:436-438
    densify (clone) + prune from the accumulated statistics,
    Adam moments carried over for the survivors                             gs_trainer.py:280-343, sings_hybrid.py:856-932, 968-1004
    densify by selective subdivision of the anchors' mesh                   gs_trainer.py:219-222, 515-521, sings_hybrid.py:1022-1150
    prune by edge collapse on the anchors' mesh                             gs_trainer.py:495-510, sings_hybrid.py:1153-1257

Two ways to change the set.  ``densify_and_prune`` follows the reference's ``vanilla`` strategy's clone + prune.
``densify_and_subdivide`` (a trainer built with ``mesh=MeshState``) is its ``hybrid`` strategy, the one every shipped configuration
sets: faces picked from the statistics are split 1-to-4 on the device (``sings_amd.topology``, csrc/sg_mesh.hip -- no trimesh, no
host copy of the mesh), the midpoints become new anchors with interpolated skinning weights, labels and scales; ``prune_and_simplify``
is the strategy's other half: transparent-and-small or big-and-dead vertices lose their longest edges by collapse, in one launch.
For the hot path what matters is THAT the set changes: P(t) != P(t-1).

A topology change (or a new SH degree) invalidates everything that was sized or captured for the old set:

    the captured HIP graph          ``CapturedStep.replay`` raises until ``AvatarTrainer`` has captured the step again
    the gradient arena              ``grad_arena.arena_sync`` raises for a stale registration; the trainer registers the new parameters
    the pair-capacity hint          re-measured with synchronous steps before the overflow check is deferred again
    Adam's moments, the statistics  ONE row map ``src`` per change (``_replace_set``): new row i takes its moments (``prune_and_simplify``: its
                                    statistics too) from old row ``src[i]`` or, at -1, starts at zero (``optim.take_rows``), as the reference does
    the mesh terms                  ``MeshTerms.reset``: the CSR of the new edges, built on the device; a holder of the old set refuses
    the frame-parallel collective   sized by the new flat buffer; the statistics are reduced (sum, sum, max) BEFORE the decision, so every
                                    rank takes the same one (``densify_decision`` is a pure function of the reduced statistics)

Nothing renders with stale sizes: the old anchors' parameter object is dropped, ``AvatarStep.topology_version`` moves on, and every holder
of an old version refuses.
"""
import os

import torch

from . import checkpoint as _ckpt
from . import overflow
from . import topology as _topo
from .avatar_init import initial_attributes
from .grad_arena import arena_sync, set_gradient_arena
from .optim import FusedAdam, take_rows
from .step_inputs import StepInputs, preserved
from .train_step import capture_step


def densify_decision(xyz_gradient_accum, denom, scales, opacity, max_grad, scale_threshold, min_opacity, big_scale):
    """-> (clone_mask [N], prune_mask [N + clones]) -- a PURE function of its arguments (every rank that holds the same reduced
    statistics and the same decoded attributes takes the same decision).

    clone   sings_hybrid.py:968-983  ``norm(grads) >= max_grad`` and ``max(scales) <= scale_threshold`` with grads = accum / denom, NaN -> 0
            (:987-988); the clones are appended behind the existing points (``densification_postfix``)
    prune   sings_hybrid.py:1000-1004 on the EXTENDED set: ``opacity < min_opacity`` or ``max(scales) > big_scale`` (``0.1 * extent``).  The
            reference's screen-size term reads ``max_radii2D`` AFTER ``densification_postfix`` has zeroed it (:930-932): it never
            fires, and is left out here."""
    grads = xyz_gradient_accum / denom
    grads = torch.where(torch.isnan(grads), torch.zeros_like(grads), grads)
    smax = scales.reshape(scales.shape[0], -1).max(dim=1).values
    clone = (torch.norm(grads, dim=-1) >= max_grad) & (smax <= scale_threshold)
    op = torch.cat([opacity.reshape(-1), opacity.reshape(-1)[clone]])
    sm = torch.cat([smax, smax[clone]])
    prune = (op < min_opacity) | (sm > big_scale)
    return clone, prune


class DecoderSchedule:
    """When the two decoders learn: the reference's ``opt_geo_from`` / ``opt_geo_until`` / ``opt_app_from`` / ``opt_app_until``
    (config.py:148-151; every shipped configuration: from 1 000, until 14 000 / 15 000).  ``flags(t) -> (opt_geo, opt_app)`` is
    gs_trainer.py:225-226 as written::

        opt_geo = False if t_iter < opt_geo_from and t_iter < opt_geo_until else True

    i.e. a decoder is frozen while ``t < from_ and t < until``.  ``until`` never freezes anything again: past ``from_`` the flag
    is True for good, and ``until`` only matters where it lies BEFORE ``from_`` (the decoder then thaws at ``until``)."""

    def __init__(self, opt_geo_from=1000, opt_geo_until=14000, opt_app_from=1000, opt_app_until=15000):
        self.opt_geo_from, self.opt_geo_until = int(opt_geo_from), int(opt_geo_until)
        self.opt_app_from, self.opt_app_until = int(opt_app_from), int(opt_app_until)

    def flags(self, t):
        return (not (t < self.opt_geo_from and t < self.opt_geo_until), not (t < self.opt_app_from and t < self.opt_app_until))


class CapturedStep:
    """A HIP graph of one training step, valid for ONE topology version of its ``AvatarStep``: ``replay`` refuses (RuntimeError) once
    the set of Gaussians or the SH degree has changed -- the graph holds the old tensors' addresses and the old sizes."""

    def __init__(self, module, fn, warmup=3, device=None):
        self.module, self.version = module, module.topology_version
        self.graph, self.outputs = capture_step(fn, warmup=warmup, device=device)

    def replay(self):
        if self.module.topology_version != self.version:
            raise RuntimeError(f"CapturedStep: captured for topology version {self.version}, the module is at "
                               f"{self.module.topology_version} (densify / prune / SH degree): capture the step again")
        self.graph.replay()
        return self.outputs


class AvatarTrainer:
    """``step(A, gt_rgb, mask)`` = one optimisation step on one posed frame (or a chunk [K,J,4,4]); ``densify_and_prune()`` /
    ``oneup_sh_degree()`` between steps.  ``use_graph``: the step (zero_grad, forward, backward) replays from a HIP graph that is
    captured again after every topology change; Adam and the statistics run outside it.  ``fp``: a ``sings_amd.dp.FrameParallel``
    -- parameter gradients live in one flat arena buffer and are all-reduced, the statistics are reduced before a decision.

    The optional parts: what each is, what it needs, where INTEGRATION.md describes it.  With any of them left at None nothing changes.
    A part's inputs reach the body through ``self.inputs`` (``step_inputs.StepInputs``); its device state that a run which is not a
    step changes is named by its ``live_tensors()`` and put back behind a capture's warm-up runs ("Trainer components").

    ``optimizer``         ``"torch"`` (``torch.optim.Adam``, outside the graph) or ``"fused"`` (``sings_amd.optim.FusedAdam``: one launch,
                          inside the body and so inside a captured step unless ``fp``); ``lr_schedules``: ``{group name:
                          fn(iteration)}``, applied to the optimiser's groups before every step.  §9.
    ``poses``             a ``sings_amd.pose.PoseTable`` -- the reference's ``optim_pose`` (sings_hybrid.py:142-150, 761-765): its learnable
                          tables join the optimiser as the groups of ``POSE_GROUPS``, ``lrs`` must name each; ``step_frames`` reads
                          ``A`` and ``transl`` from the tables.  §10.
    ``mesh``              a ``sings_amd.topology.MeshState`` over the anchors: what ``densify_and_subdivide`` and ``prune_and_simplify``
                          need and keep up to date.  §11, §12.
    ``mesh_terms``        a ``sings_amd.mesh_terms.MeshTerms`` -- the four mesh terms of gs_trainer.py:366-399, ``reset`` whenever the set
                          changes, ``set_iteration`` before every step.  Needs ``mesh=``.  §15.
    ``lpips_sampler``     a ``sings_amd.patch_sampler.DevicePatchSampler`` -- the step draws its own LPIPS patch corners from its mask, on
                          the device, inside a captured step.  Needs the module's LPIPS term with the sampler's patch size;
                          ``lpips_origins=`` is then refused.  §8.
    ``decoder_schedule``  a ``DecoderSchedule`` -- before every step the flags of ``self.iteration`` go to the module, the optimiser's
                          active groups, the arena; a change drops the captured graph.  §17.
    ``frames``            a ``sings_amd.frame_feed.FrameFeed`` -- ``step_next()`` takes nothing from outside: the body draws the next K
                          frames and the background colour.  Needs ``poses=`` with one row per frame of the store.  §18.
    ``set_density_schedule(schedule)``  a ``sings_amd.density.HybridDensitySchedule`` -- gated statistics, the L2 term's keys, the SH
                          degree and both changes of the set after the optimiser step, recorded in ``density_log``; ``run(n_steps)``
                          is ``step_next()`` that many times.  Needs ``mesh=``.  §19.
    ``set_outputs(outputs)``  a ``sings_amd.run_outputs.RunOutputs`` -- the run's pictures, turntable and splat file on the reference's
                          intervals, written behind the optimiser step and in front of the density schedule's changes.  §21.
    ``state_dict()`` / ``load_state_dict(sd, strict=True)`` / ``save_checkpoint(path)`` / ``load_checkpoint(path)``  the whole run, every
                          part above included, in the reference's ``SinGS.state_dict()`` layout plus one key; ``run_until(num_steps,
                          save_every, save_dir)`` saves on the reference's rule.  Host work between steps.  §20."""

    POSE_GROUPS = ("global_orient", "body_pose", "transl")

    def __init__(self, module, settings_fn, bg_color, lrs, smpl_scale=None, transl=None, use_graph=False, fp=None,
                 sh_degree=0, max_sh_degree=3, betas=(0.9, 0.999), eps=1e-15, optimizer="torch", lr_schedules=None, poses=None,
                 mesh=None, mesh_terms=None, lpips_sampler=None, decoder_schedule=None, frames=None):
        self.decoder_schedule = decoder_schedule
        # set_density_schedule(): the schedule, the statistics' gate (int32 [1] on the device), the word it holds, what was done
        self.density_schedule, self._gate, self._gate_value, self.density_log = None, None, None, []
        if frames is not None:
            if poses is None:
                raise ValueError("AvatarTrainer: frames= needs poses=PoseTable(...) (the drawn frames' rows of the pose tables)")
            if frames.store.F != int(poses.global_orient.shape[0]):
                raise ValueError(f"AvatarTrainer: the frame store holds {frames.store.F} frames, the pose tables "
                                 f"{int(poses.global_orient.shape[0])} rows")
            same = lambda t: (torch.is_tensor(t) and t.data_ptr() == frames.bg.data_ptr() and t.dtype == frames.bg.dtype
                              and tuple(t.shape) == tuple(frames.bg.shape))
            if frames.random_bg and not (same(bg_color) and same(getattr(settings_fn(int(sh_degree)), "bg", None))):
                raise ValueError("AvatarTrainer: with random_bg the feed's bg tensor must be both bg_color and the bg of the settings "
                                 "settings_fn returns (the render and the loss composite onto the same colour)")
        self.frames = frames
        # what step_next adopts of the feed: the SAME objects every call (one frame: [0] views, the step is handed [3,H,W] and [H,W])
        self._feed_views = None if frames is None else (frames.gt[0], frames.mask[0]) if frames.K == 1 else (frames.gt, frames.mask)
        if lpips_sampler is not None:
            if getattr(module, "lpips", None) is None or not module.lpips_w > 0.0:
                raise ValueError("AvatarTrainer: lpips_sampler needs the module's LPIPS term (AvatarStep(lpips=..., lpips_w > 0))")
            if lpips_sampler.patch_size != module.lpips_patch_size:
                raise ValueError(f"AvatarTrainer: lpips_sampler draws corners for patches of {lpips_sampler.patch_size}, the module "
                                 f"crops patches of {module.lpips_patch_size}")
        self.lpips_sampler = lpips_sampler
        if mesh_terms is not None and mesh is None:
            raise ValueError("AvatarTrainer: mesh_terms needs mesh=MeshState(...) (the edges and labels the terms are built from)")
        self.mesh_terms, self._mesh_verts, self._mesh_normals = mesh_terms, None, None
        if mesh_terms is not None:
            module.mesh_terms = mesh_terms
        if mesh is not None and mesh.num_verts != int(module.xyz.shape[0]):
            raise ValueError(f"AvatarTrainer: the mesh has {mesh.num_verts} vertices, the module {int(module.xyz.shape[0])} Gaussians")
        self.mesh, self.last_subdivision, self.last_simplification = mesh, None, None
        learnable = self._pose_params(poses)
        for what, names in (("lrs", lrs), ("lr_schedules", lr_schedules or {})):
            extra = [n for n in self.POSE_GROUPS if n in names and n not in learnable]
            if extra:
                raise ValueError(f"AvatarTrainer: {what} for pose groups {extra} " +
                                 ("need poses=PoseTable(...)" if poses is None else "that the PoseTable does not learn "
                                  "(learn_pose / learn_transl)"))
        missing = [n for n in learnable if n not in lrs]
        if missing:
            raise ValueError(f"AvatarTrainer: lrs has no entry for the pose groups {missing}")
        self.poses = poses
        self.m, self.settings_fn, self.bg = module, settings_fn, bg_color
        self.smpl_scale, self.transl, self.use_graph, self.fp = smpl_scale, transl, bool(use_graph), fp
        self.sh_degree, self.max_sh_degree = int(sh_degree), int(max_sh_degree)
        self.lrs, self.betas, self.eps = dict(lrs), betas, eps
        self.dev = module.xyz.device
        if optimizer not in ("torch", "fused"):
            raise ValueError(f"AvatarTrainer: optimizer must be 'torch' or 'fused', got {optimizer!r}")
        self.fused = optimizer == "fused"
        self.lr_schedules = dict(lr_schedules or {})
        unknown = set(self.lr_schedules) - set(self.lrs)
        if unknown:
            raise ValueError(f"AvatarTrainer: lr_schedules for unknown groups {sorted(unknown)}")
        if self.fused:
            self.opt = FusedAdam(self._groups(), betas=betas, eps=eps)        # (bound to the arena by _rebuild)
        else:
            self.opt = torch.optim.Adam(self._groups(), betas=betas, eps=eps)
        self.captured = self.flat = self.views = None
        # set_outputs(): the run's pictures (sings_amd.run_outputs.RunOutputs) and, kept for them only, the step's raw render
        self.outputs, self.last_render = None, None
        self.iteration = 0
        self.inputs = StepInputs()
        self._rebuild()

    @classmethod
    def _pose_params(cls, poses):
        """{group name: parameter} of the tables ``poses`` learns ({} without poses)."""
        if poses is None:
            return {}
        return {n: getattr(poses, n) for n in cls.POSE_GROUPS
                if isinstance(getattr(poses, n), torch.nn.Parameter) and getattr(poses, n).requires_grad}

    # ---- pieces sized by the set of Gaussians
    def _groups(self):
        m = self.m
        groups = [{"params": [m.xyz], "lr": self.lrs["xyz"], "name": "xyz"},
                  {"params": list(m.triplane.parameters()), "lr": self.lrs["triplane"], "name": "triplane"},
                  {"params": list(m.geometry_dec.parameters()), "lr": self.lrs["geometry"], "name": "geometry"},
                  {"params": list(m.appearance_dec.parameters()), "lr": self.lrs["appearance"], "name": "appearance"}]
        # the pose tables (sized by the frames, not by the Gaussians): behind the others, one group each
        return groups + [{"params": [p], "lr": self.lrs[n], "name": n} for n, p in self._pose_params(self.poses).items()]

    def _rebuild(self):
        """(Re)build what depends on the number of Gaussians / the SH degree: raster settings, statistics, arena, capacity hint, graph."""
        m = self.m
        self.rs = self.settings_fn(self.sh_degree)
        self.params = [p for g in self.opt.param_groups for p in g["params"]]
        m.enable_densification_stats()
        self._drop_graph()
        if self.fp is not None or self.fused:
            n = sum(p.numel() for p in self.params)
            self.flat = torch.zeros(n, dtype=torch.float32, device=self.dev)
            self.views = set_gradient_arena(self.params, self.flat)
        if self.fused:
            self.opt.bind_arena(self.flat, self.views)
        if self.mesh_terms is not None:
            self._reset_mesh_terms()
        if self.dev.type == "cuda":
            overflow.set_overflow_check("sync")                  # the next steps size the pair capacity for the new set
            overflow.reset_overflow_state()
        self._sizing = 2 if self.use_graph else 0

    def _reset_mesh_terms(self):
        """The mesh terms for the current mesh: the vertices the last topology call produced (the anchors before the first), their normals."""
        verts = self.m.xyz.detach() if self._mesh_verts is None else self._mesh_verts
        if self.mesh.num_verts != int(verts.shape[0]):
            raise RuntimeError(f"AvatarTrainer: the mesh has {self.mesh.num_verts} vertices, the new set {int(verts.shape[0])} Gaussians: "
                               "with mesh_terms the set changes through densify_and_subdivide / prune_and_simplify only")
        normals, self._mesh_verts, self._mesh_normals = self._mesh_normals, None, None
        if normals is None:                                      # (given: a loaded checkpoint's, the ones its terms were reset with)
            with torch.no_grad():
                normals = initial_attributes(verts.contiguous(), self.mesh.faces, self.mesh.edges)["normals"]
        self.mesh_terms.reset(self.mesh, normals, verts)

    def active_groups(self):
        """Names of the optimiser groups that learn under the module's current ``opt_geo`` / ``opt_app``."""
        m = self.m
        frozen = {"geometry": not m.opt_geo, "appearance": not m.opt_app, "triplane": not (m.opt_geo or m.opt_app)}
        return [g["name"] for g in self.opt.param_groups if not frozen.get(g["name"], False)]

    def _apply_decoder_schedule(self):
        """The flags of this iteration; on a change: the module, the optimiser's active groups, the captured graph, the arena."""
        m = self.m
        flags = self.decoder_schedule.flags(self.iteration)
        if flags == (m.opt_geo, m.opt_app):
            return
        m.set_trainable(*flags)
        self._drop_graph()
        active = set(self.active_groups())
        if self.fused:
            self.opt.set_active(active)
        view = {} if self.flat is None else {id(p): v for p, v in zip(self.params, self.views)}
        with torch.no_grad():
            for g in self.opt.param_groups:
                for p in (g["params"] if g["name"] not in active else ()):
                    if view:
                        view[id(p)].zero_()                      # (a slot nothing writes any more: zeros, not the last gradients)
                    p.grad = None                                # (a frozen parameter carries no gradient into the next step)

    def set_density_schedule(self, schedule):
        """Attach (or, with None, detach) a ``sings_amd.density.HybridDensitySchedule``: INTEGRATION.md §19 says what the steps do with
        it.  The gate is allocated here and handed to the module; the captured graph is dropped either way (the statistics' launch
        and the L2 term's key list are part of it)."""
        if schedule is not None and self.mesh is None:
            raise ValueError("AvatarTrainer.set_density_schedule needs mesh=MeshState(...) (prune_and_simplify / densify_and_subdivide "
                             "work on the anchors' mesh)")
        self.density_schedule = schedule
        if schedule is None:
            self._gate = self._gate_value = None
            self.m.l2_keys = ("xyz_offsets", "scales", "opacity")
        elif self._gate is None:
            self._gate, self._gate_value = torch.zeros(1, dtype=torch.int32, device=self.dev), 0
        self.m.stats_gate = self._gate
        self._drop_graph()

    def set_outputs(self, outputs):
        """Attach (or, with None, detach) a ``sings_amd.run_outputs.RunOutputs``: behind the optimiser step of iteration ``t`` -- and in front
        of the density schedule's SH degree and changes of the set, the reference's order (gs_trainer.py:271-274, :457-458) -- the run
        calls ``outputs.after_step(self, t)``.  With outputs the body keeps a reference to the step's raw render (the tensor a replayed
        graph rewrites), so the graph is dropped when outputs come or go; without them a step does what it did.  INTEGRATION.md §21."""
        if (outputs is None) != (self.outputs is None):
            self._drop_graph()
        self.outputs = outputs
        if outputs is None:
            self.last_render = None

    def _apply_density_schedule_before(self):
        """In front of step ``self.iteration``: the gate's word (a stream-ordered fill, only when it changes) and the L2 term's keys."""
        sch, t = self.density_schedule, self.iteration
        word = int(sch.decides_at(t))
        if word != self._gate_value:
            self._gate.fill_(word)
            self._gate_value = word
        keys = tuple(sch.l2_keys(t))
        if keys != tuple(self.m.l2_keys):
            self.m.l2_keys = keys
            self._drop_graph()

    def _apply_density_schedule_after(self, t):
        """Behind the optimiser step of iteration ``t``: gs_trainer.py:271-274 (``_periodic_check``'s SH degree, then ``_adjust_density``)."""
        sch = self.density_schedule
        if sch.sh_up(t):
            self.oneup_sh_degree()
        for mode in sch.actions(t):
            if mode == "prune":
                _, _, n_old, n_new = self.prune_and_simplify(**sch.prune_kwargs())
                skipped = self.last_simplification["skipped"]
            else:
                _, _, n_old, n_new = self.densify_and_subdivide(**sch.densify_kwargs())
                skipped = None
            self.density_log.append({"t": t, "mode": mode, "n_old": n_old, "n_new": n_new, "skipped": skipped})

    def run(self, n_steps):
        """``step_next()`` ``n_steps`` times -> the list of the steps' loss dicts (copies: a replayed graph reuses its output tensors)."""
        if self.frames is None:
            raise RuntimeError("AvatarTrainer.run needs frames=FrameFeed(...)")
        return [{k: v.clone() for k, v in self.step_next().items()} for _ in range(int(n_steps))]

    def run_until(self, num_steps, save_every=None, save_dir=None):
        """``step_next()`` for the iterations ``self.iteration .. num_steps`` (the reference's ``range(init_iter, num_steps + 1)``) -> the
        list of the steps' loss dicts.  With ``save_every`` and ``save_dir``: behind the step of iteration ``t`` the run is saved as
        ``human_{t:06d}.pth`` when ``t % save_every == 0 or t == num_steps`` (gs_trainer.py:426-428); the file resumes at ``t + 1``."""
        if self.frames is None:
            raise RuntimeError("AvatarTrainer.run_until needs frames=FrameFeed(...)")
        if (save_every is None) != (save_dir is None) or (save_every is not None and int(save_every) < 1):
            raise ValueError("AvatarTrainer.run_until: save_every (>= 1) and save_dir go together")
        out = []
        while self.iteration <= int(num_steps):
            t = self.iteration
            out.append({k: v.clone() for k, v in self.step_next().items()})
            if save_every is not None and (t % int(save_every) == 0 or t == int(num_steps)):
                self.save_checkpoint(os.path.join(save_dir, f"human_{t:06d}.pth"))
        return out

    # ---- checkpoint / resume (sings_amd.checkpoint): host work between steps, nothing a step executes
    def state_dict(self, spatial_lr_scale=None, betas=None):
        """The whole run as one dict: the reference's ``SinGS.state_dict()`` layout plus the key ``"sings_amd"``
        (``checkpoint.trainer_state_dict``).  ``spatial_lr_scale`` / ``betas``: the caller's, passed through."""
        return _ckpt.trainer_state_dict(self, spatial_lr_scale=spatial_lr_scale, betas=betas)

    def load_state_dict(self, sd, strict=True):
        """Make this trainer -- built the usual way, with the same optional parts -- the saved one; -> a report.  Everything is validated
        before anything changes: a refusal (ValueError naming the entry) leaves the trainer as it was.  ``strict=False``: a part only
        the file or only the trainer has is skipped and named in the report.  A dict without ``"sings_amd"`` (the reference's
        ``save_ckpt``): ``checkpoint.load_reference``."""
        return _ckpt.load_trainer_state_dict(self, sd, strict=strict)

    def save_checkpoint(self, path, spatial_lr_scale=None, betas=None):
        """``state_dict()`` into ``path``: written to a temporary file beside it, then ``os.replace``."""
        _ckpt.atomic_save(self.state_dict(spatial_lr_scale=spatial_lr_scale, betas=betas), path)

    def load_checkpoint(self, path, strict=True):
        """``load_state_dict`` of a file of ``save_checkpoint`` (read with ``torch.load(..., weights_only=True)``)."""
        return self.load_state_dict(_ckpt.load_file(path), strict=strict)

    def _body(self):
        for p in self.params:
            p.grad = None
        inp = self.inputs
        if inp.source == "feed":                                 # this step's frames and background: two launches, no host read
            self.frames.draw()
        A, transl = inp.A, self.transl
        if inp.source != "A":                                    # the frames' rows of the pose tables: ONE launch, index on the device
            A, transl = self.poses(inp.idx)
            if inp.single:
                A, transl = A[0], transl[0]
        origins = inp.lp_origins
        if self.lpips_sampler is not None:                       # this step's corners, drawn from its mask: two launches, no host read
            frames = A.dim() == 4
            origins = self.lpips_sampler.origins(inp.mask, frames=int(A.shape[0]) if frames else None)
            if not frames:
                origins = origins.reshape(-1, 2)
        loss, ld, ex = self.m(A, self.rs, inp.gt, inp.mask, self.bg, smpl_scale=self.smpl_scale, transl=transl,
                              lpips_origins=origins, lpips_bg=inp.lp_bg)
        if loss is None:
            self.m.backward(ld, ex)
        else:
            loss.backward()
        self.m.add_densification_stats(ex)
        if self.outputs is not None:
            self.last_render = ex["render_raw"].detach()         # (the training picture shows the step's own image)
        if self.fused and self.fp is None:
            self.opt.apply()                                     # (the Adam launch: part of the body, and so of a captured step)
        return {k: v.detach().reshape(()).clone() for k, v in ld.items()}

    def _drop_graph(self):
        """The captured step no longer matches what a step would run: the next graph step captures again."""
        self.captured = None

    def _live_tensors(self):
        """The device state a run of ``_body`` changes besides its outputs, stated by each component the trainer has (their
        ``live_tensors`` say why).  The gate: nothing in the body writes it; put back with the statistics it gates."""
        live = list(self.m.stats_tensors()) + ([] if self._gate is None else [self._gate])
        if self.lpips_sampler is not None:
            live += self.lpips_sampler.live_tensors()
        if self.frames is not None:
            live += self.frames.live_tensors()
        if self.fused and self.fp is None:                       # (the Adam launch is part of the body)
            live += self.opt.live_tensors()
        return live

    def _capture(self):
        overflow.set_deferred_overflow_check(True, capacity_pairs=overflow.capacity_pairs(self.dev))
        # (the capture's warm-up runs execute the body without being steps)
        with preserved(self._live_tensors(), lists=[self.opt.steps] if self.fused else ()):
            self.captured = CapturedStep(self.m, self._body, warmup=2, device=self.dev)
        overflow.check_deferred_overflow(self.dev)

    def step(self, A, gt_rgb, mask, lpips_origins=None, lpips_bg=None):
        """``lpips_origins`` / ``lpips_bg``: the step's LPIPS patch corners and random background (``AvatarStep.forward``), copied
        in like the frame's inputs, so that a replayed graph reads this step's patches."""
        return self._step("A", A, None, gt_rgb, mask, lpips_origins, lpips_bg)

    def step_frames(self, frame_idx, gt_rgb, mask, lpips_origins=None, lpips_bg=None):
        """One step on the frame(s) ``frame_idx`` of the pose tables: an int (one frame, the reference's step) or K indices (a
        sequence or an integer tensor: a chunk [K,J,4,4]).  The index is copied into a static int32 device tensor like the other inputs
        of the step, and the body reads ``A`` and the ``transl`` rows from ``poses`` there: a graph captured at one index replays at
        any other.  (The trainer's constant ``transl`` is not used: the table's rows are.)"""
        if self.poses is None:
            raise RuntimeError("AvatarTrainer.step_frames needs poses=PoseTable(...)")
        single = not torch.is_tensor(frame_idx) and not isinstance(frame_idx, (list, tuple))
        idx = torch.as_tensor([frame_idx] if single else frame_idx).reshape(-1)
        if idx.dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool) or idx.numel() < 1:
            raise ValueError("AvatarTrainer.step_frames: frame_idx must be an int or K >= 1 integer indices")
        if not idx.is_cuda:                                      # (indices that are already on the device are not read here)
            F = int(self.poses.global_orient.shape[0])
            if int(idx.min()) < 0 or int(idx.max()) >= F:
                raise IndexError(f"AvatarTrainer.step_frames: frame index outside the table's {F} rows")
        return self._step("idx", idx.to(self.dev, torch.int32), single, gt_rgb, mask, lpips_origins, lpips_bg)

    def _step(self, source, pose, single, gt_rgb, mask, lpips_origins, lpips_bg):
        if self.lpips_sampler is not None and lpips_origins is not None:
            raise ValueError("AvatarTrainer: the trainer draws the patch corners itself (lpips_sampler=): lpips_origins= cannot be passed too")
        on_dev = lambda v: None if v is None else torch.as_tensor(v).to(self.dev)
        lp_origins = on_dev(lpips_origins)
        if lp_origins is not None:
            lp_origins = lp_origins.to(torch.int32)
        # (the step reads A, or the tables' rows at idx: not both)
        if self.inputs.bind(source, single, gt=gt_rgb, mask=mask, lp_origins=lp_origins, lp_bg=on_dev(lpips_bg), **{source: pose}):
            self._drop_graph()
        return self._run()

    def step_next(self, lpips_bg=None):
        """One step on the next frame(s) of ``frames`` (a ``FrameFeed``): nothing is copied in -- the body draws the frames itself, and
        the static inputs ARE the feed's tensors.  ``lpips_bg``: as in ``step``."""
        if self.frames is None:
            raise RuntimeError("AvatarTrainer.step_next needs frames=FrameFeed(...)")
        fd, (gt, mask) = self.frames, self._feed_views
        if self.inputs.bind("feed", fd.K == 1, adopted=dict(idx=fd.idx, gt=gt, mask=mask),
                            lp_bg=None if lpips_bg is None else torch.as_tensor(lpips_bg).to(self.dev)):
            self._drop_graph()
        return self._run()

    def _run(self):
        """The step on the static inputs: schedules, the body (eager or replayed), the reduction, the optimiser."""
        if self.decoder_schedule is not None:
            self._apply_decoder_schedule()
        if self.density_schedule is not None:
            self._apply_density_schedule_before()
        for g in self.opt.param_groups:
            if g["name"] in self.lr_schedules:
                g["lr"] = self.lr_schedules[g["name"]](self.iteration)
        if self.mesh_terms is not None:
            self.mesh_terms.set_iteration(self.iteration)        # (device weights: a captured step replays with this iteration's)
        if self.fused:
            self.opt.advance()                                   # host half: this step's rows are on their way before the body runs
        if self.use_graph and self._sizing == 0:
            if self.captured is None:
                self._capture()
            ld = self.captured.replay()
        else:
            ld = self._body()                                    # eager (and the synchronous sizing steps in front of a capture)
            self._sizing = max(0, self._sizing - 1)
        if self.fp is not None:
            arena_sync(self.params, self.views, True)
            self.fp.all_reduce_grads(self.flat)
            arena_sync(self.params, self.views, False)
            if self.fused:
                self.opt.apply(sync=False)                       # (the arena holds the reduced gradients)
        if not self.fused:
            self.opt.step()
        if self.outputs is not None:                             # (before the SH degree and the set change: the reference's order)
            self.outputs.after_step(self, self.iteration)
        if self.density_schedule is not None:
            if self._gate_value:                                 # (a change of the set drops the graph whose outputs these may be)
                ld = {k: v.clone() for k, v in ld.items()}
            self._apply_density_schedule_after(self.iteration)
        self.iteration += 1
        return ld

    # ---- between steps
    def oneup_sh_degree(self):
        """gs_trainer.py:436-438.  The degree is a field of the raster settings: a captured step must be captured again."""
        if self.sh_degree < self.max_sh_degree:
            self.sh_degree += 1
            self.m.topology_version += 1
            self.rs = self.settings_fn(self.sh_degree)
            self._drop_graph()

    def _reduce_stats(self):
        """With ``fp``: the statistics summed / maximised over the ranks, in place, so that every rank takes the same decision."""
        if self.fp is not None:
            self.fp.reduce_densification_stats(*self.m.stats_tensors())

    def _scales_canon(self, attrs):
        """human_gs_out['scales_canon']: the decoded scales, times smpl_scale when the step has one (sings_hybrid.py:411-413, 455)."""
        return attrs["scales"] if self.smpl_scale is None else attrs["scales"] * self.smpl_scale.reshape(1, -1)

    def _reset_opacity(self):
        if not getattr(self.m.appearance_dec, "fixed_opacity", False):
            self.m.appearance_dec.reset_opacity(self.m.triplane(self.m.xyz))

    @torch.no_grad()
    def _replace_set(self, new_xyz, new_lbs_weights, src, scaling_multiplier=None, keep_stats=False, then=None):
        """The ONE place that replaces the set of Gaussians.  ``src`` (int64 [N_new]) is the row map: new row i carries on from old row
        ``src[i]``, or is new where ``src[i] == -1``.  Adam's moments go through ``take_rows`` (cat_tensors_to_optimizer /
        _prune_optimizer: kept rows bit for bit, zeros for the new ones, the step counts stay); with ``keep_stats`` the statistics too,
        otherwise they start at zero.  ``then()``: the caller's work on the new set (opacity reset) before the rebuild."""
        m = self.m
        group = next(g for g in self.opt.param_groups if g["name"] == "xyz")
        old = group["params"][0]
        state = None if self.fused else self.opt.state.pop(old, None)
        stats = [take_rows(t, src) for t in m.stats_tensors()] if keep_stats else None
        m.set_topology(new_xyz, new_lbs_weights, scaling_multiplier=scaling_multiplier)
        if self.fused:
            self.opt.reindex_rows(old, m.xyz, src)
        elif state:                                              # (torch creates a parameter's state at its first step)
            for k in ("exp_avg", "exp_avg_sq"):
                state[k] = take_rows(state[k], src)
            self.opt.state[m.xyz] = state
        group["params"][0] = m.xyz
        if then is not None:
            then()
        self._rebuild()
        if keep_stats:                                           # (set_topology and the rebuild start the statistics at zero)
            m.set_stats(stats)

    def _appended(self, n_old, n_new):                           # the row map of n_new new rows behind n_old kept ones
        return torch.cat([torch.arange(n_old, device=self.dev), torch.full((n_new,), -1, dtype=torch.int64, device=self.dev)])

    def densify_and_prune(self, max_grad, scale_threshold, min_opacity, big_scale, decision=None):
        """Clone + prune from the accumulated (and, with ``fp``, reduced) statistics; -> (clone_mask, prune_mask, N_old, N_new).
        ``decision``: a (clone_mask, prune_mask) pair to apply instead (tests drive a reference with the decision of the run)."""
        m = self.m
        self._reduce_stats()
        with torch.no_grad():
            if decision is None:
                attrs = m.decode()
                decision = densify_decision(m.xyz_gradient_accum, m.denom, attrs["scales"], attrs["opacity"], max_grad, scale_threshold,
                                            min_opacity, big_scale)
            clone, prune = decision
            n_old, keep = int(m.xyz.shape[0]), ~prune
            extended = lambda t: torch.cat([t, t[clone]])[keep].clone()       # (densification_postfix, then prune_points)
            self._replace_set(extended(m.xyz.detach()), extended(m.lbs_weights), self._appended(n_old, int(clone.sum()))[keep])
        return clone, prune, n_old, int(m.xyz.shape[0])

    def densify_and_subdivide(self, grad_threshold, scale_threshold, max_screen_size=None, max_n_gs=None, exclude=(6, 7), decision=None):
        """``SinGS.densify_and_subdivide`` (sings_hybrid.py:1022-1150) from the accumulated (and, with ``fp``, reduced) statistics; ->
        (selected_pts_mask, selected_faces_idx, N_old, N_new).  ``decision``: a (selected_pts_mask, selected_faces_idx) pair to apply
        instead of ``topology.subdivide_decision`` (whose docstring names the reference's quirks that are kept).

        The selected faces of ``mesh`` are split 1-to-4; their edge midpoints (of ``xyz_canon`` = anchor + offset) are appended to the
        anchors with the endpoints' mean skinning weights, the smaller endpoint's label and -- through ``scaling_multiplier``, which
        becomes per-Gaussian [N,1] -- the endpoints' mean scale, each clipped to 0.008 first; a selected old row is rescaled to the mean
        scale of all points.  Zero Adam moments for the new rows, the old rows' kept; opacity reset on the new set.  The reference also
        interpolates ``shs`` and never reads the result: not computed.  ``self.mesh`` then holds the new faces, labels, level ids and the
        unique edges of the new faces; ``self.last_subdivision`` what the call interpolated (``interpolated_scales`` of the new rows)."""
        if self.mesh is None:
            raise RuntimeError("AvatarTrainer.densify_and_subdivide needs mesh=MeshState(...)")
        m, mesh = self.m, self.mesh
        self._reduce_stats()
        with torch.no_grad():
            attrs = m.decode()
            scales_canon = self._scales_canon(attrs)
            if decision is None:
                decision = _topo.subdivide_decision(m.xyz_gradient_accum, m.denom, scales_canon, m.max_radii2D, mesh.vertex_label,
                                                    mesh.faces, grad_threshold, scale_threshold, max_screen_size=max_screen_size,
                                                    max_n_gs=max_n_gs, exclude=exclude)
            selected, faces_idx = (t.to(self.dev) for t in decision)
            sub_vertices, sub_faces, attr = _topo.subdivide_meshes(
                attrs["xyz_canon"], mesh.faces, faces_idx, {"vertex_label": mesh.vertex_label, "lbs_weights": m.lbs_weights,
                                                            "scales": torch.clip(scales_canon[:, :1].mean(-1), max=0.008)})
            n_old, n_new = int(m.xyz.shape[0]), int(sub_vertices.shape[0])
            # new multipliers: selected old rows to the mean scale, ones for the new rows (:1127-1131)
            sm = torch.cat([_topo.rescaled_multiplier(m.scaling_multiplier, scales_canon, selected),
                            torch.ones((n_new - n_old, 1), dtype=torch.float32, device=self.dev)])
            interpolated = attr["scales"][n_old:]

            def post_process():                                  # (:1136-1147) on the new set, before the rebuild
                self._reset_opacity()
                sm[n_old:] *= (interpolated / m.decode()["scales"][n_old:].mean(-1)).unsqueeze(1)     # decoded mean scale := interpolated

            mesh.replace(sub_faces, attr["vertex_label"])
            self._mesh_verts = sub_vertices if self.mesh_terms is not None else None
            self._replace_set(torch.cat([m.xyz.detach(), sub_vertices[n_old:]]), attr["lbs_weights"],
                              self._appended(n_old, n_new - n_old), scaling_multiplier=sm, then=post_process)
            self.last_subdivision = {"interpolated_scales": interpolated, "n_old": n_old}
        return selected, faces_idx, n_old, n_new

    def prune_and_simplify(self, opacity_threshold, scale_threshold, dead_grad=0.0005, large_scale=0.01, prune_max_n_gs_once=5000,
                           min_n_gs=None, exclude=(6, 7), decision=None):
        """``SinGS.prune_and_simplify`` (sings_hybrid.py:1153-1257) from the accumulated (and, with ``fp``, reduced) statistics; ->
        (vert_mask, prune_mask, N_old, N_new).  ``decision``: a (vert_mask, selected_edges) pair to apply instead of
        ``topology.simplify_decision`` (whose docstring names the reference's quirks that are kept).

        The selected edges of ``mesh`` are collapsed (``topology.collapse_edges`` at the reference's rate 0.5, on ``xyz_canon`` = anchor +
        offset); the vertices no face is left on are pruned.  The survivors keep their rows of the anchors, the skinning weights, a
        per-Gaussian ``scaling_multiplier`` and both Adam moments, bit for bit -- and, unlike after clone + prune, their accumulated
        statistics (``prune_points`` masks them, sings_hybrid.py:887-890; with ``fp`` each rank keeps its OWN sums, the reduced ones
        only take the decision).  Then ``mesh.prune``, the opacity reset on the new set, the rebuild.

        A skip (``simplify_decision``'s reasons, or a ``decision`` without edges) changes nothing -- no parameter, no statistic, not
        ``topology_version``, not a captured graph -- and returns ``prune_mask`` all false.  ``self.last_simplification`` records the reason,
        or the counts of the call."""
        if self.mesh is None:
            raise RuntimeError("AvatarTrainer.prune_and_simplify needs mesh=MeshState(...)")
        m, mesh = self.m, self.mesh
        own = [t.clone() for t in m.stats_tensors()] if self.fp is not None else None
        self._reduce_stats()
        with torch.no_grad():
            attrs = m.decode()
            n_old = int(m.xyz.shape[0])
            if decision is None:
                vert_mask, edges, reason = _topo.simplify_decision(
                    m.xyz_gradient_accum, m.denom, attrs["opacity"], self._scales_canon(attrs), mesh.vertex_label, mesh.faces,
                    opacity_threshold, scale_threshold, dead_grad=dead_grad, large_scale=large_scale,
                    prune_max_n_gs_once=prune_max_n_gs_once, min_n_gs=min_n_gs, exclude=exclude)
            else:
                vert_mask, edges = (t.to(self.dev) for t in decision)
                reason = None if int(edges.shape[0]) else "no_edges"
            result = None if reason else _topo.collapse_edges(attrs["xyz_canon"], m.lbs_weights, edges, mesh.faces, return_collapses=True)
            if own is not None:                                      # (the decision is taken: back to this rank's own sums)
                for dst, t in zip(m.stats_tensors(), own):
                    dst.copy_(t)
            if result is None:
                self.last_simplification = {"skipped": reason, "selected_edges": int(edges.shape[0])}
                return vert_mask, torch.zeros(n_old, dtype=torch.bool, device=self.dev), n_old, n_old
            _, new_faces, _, prune, collapses = result
            keep = ~prune
            sm = m.scaling_multiplier
            per_gaussian = torch.is_tensor(sm) and sm.dim() > 0 and sm.shape[0] == n_old and n_old != 1
            mesh.prune(new_faces, keep)
            self._mesh_verts = result[0] if self.mesh_terms is not None else None
            self._replace_set(m.xyz.detach()[keep], m.lbs_weights[keep], torch.arange(n_old, device=self.dev)[keep],
                              scaling_multiplier=sm[keep].clone() if per_gaussian else None, keep_stats=True, then=self._reset_opacity)
            n_new = int(m.xyz.shape[0])
            self.last_simplification = {"skipped": None, "selected_edges": int(edges.shape[0]), "collapses": collapses, "n_old": n_old,
                                        "n_new": n_new}
        return vert_mask, prune, n_old, n_new
