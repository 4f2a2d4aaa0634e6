"""What a training run leaves in its log directory every ``viz_interval`` / ``progress_save_interval`` iterations (gs_trainer.py:438-454),
as an opt-in component of ``AvatarTrainer`` (``trainer.set_outputs(RunOutputs(...))``):

    trigger     file                                     content
    viz         train/{t:06d}.png                        the step's own ground truth on its background beside the step's own clamped
                                                         render (:443-449: truncated bytes, plain concatenation)
    viz         canon/{idx:05d}.png                      the ``canon_nframes`` turntable frames (``canonical.render_canonical``)
    viz         meshes/human_pcd_{t:06d}_splat.ply       ``export.save_ply`` of the decoded set, when ``save_ply``
    progress    train_progress/{t:06d}.png               the progress sheet (``canonical.progress_sheet``)
    progress    train_{video_name}.avi                   with ``progress_video``: the same sheets as Motion-JPEG at 10 frames a second
                                                         (``_end_training``, gs_trainer.py:461-466), closed by ``finish()``

Every picture becomes bytes on the device (``sheets.image_sheets``) and crosses to the host once.  The progress video is encoded on the
device too (``video.JpegEncoder``) and is off by default; the sheets stay on disk beside it (the reference deletes them).  The
``device_png`` (off by default) encodes the pictures themselves on the device (``png.PngEncoder``) and writes the file bytes directly.  The
reference's ellipsoid meshes and the text label on the progress sheet are not written.  The component keeps nothing a resumed run needs: it adds
nothing to a checkpoint.
"""
import os

import torch

from . import canonical as _canon
from .sheets import image_sheets


def validation_grids(gt, pred, mask=None):
    """The reference's per-frame log images ``make_grid([gt, image], nrow=2, pad_value=1)`` (gs_trainer.py:588-591) of K frames in one
    launch: ``gt``, ``pred`` [K,3,H,W] fp32 on the GPU -> uint8 [K, H+4, 2W+6, 3], quantised as ``save_image`` does; sheet k is
    ``validate.comparison_grid(gt[k], pred[k])`` in bytes.  ``mask`` [K,H,W]: both images of frame k are multiplied by row k first (the
    ``zju`` branch, :580-582)."""
    return image_sheets(gt, pred, tiles_per_sheet=2, nrow=2, padding=2, pad_value=1.0, quant="round", mask=mask)


def _write_png(path, array):
    from PIL import Image
    Image.fromarray(array).save(path)


class RunOutputs:
    """``after_step(trainer, t)`` behind the optimiser step of iteration ``t`` writes what ``due(t)`` names (the module docstring's
    table).  ``A_static``: A_cano2pose [J,4,4] of the canonical pose (``canonical.static_A``); ``bg_color``: the background of the
    canonical renders; ``progress_interval`` None: no progress sheets (``save_progress_images`` off).  ``write(path, uint8 array)``:
    the writer of the pictures, PNG through PIL by default; the directories are made here.  ``progress_video`` (an attribute, like the
    sizes: off by default, set it before the first step): every progress sheet is also appended to ``train_<video_name>.avi`` at JPEG
    quality ``video_quality``; call ``finish()`` at the end of the run.  ``device_png`` (an attribute too, off by default): the
    ``train/``, ``canon/`` and ``train_progress/`` pictures are encoded to PNG on the device (``png.PngEncoder``, the turntable
    ``frames_per_launch`` frames per call) and the file bytes written under a temporary name, then renamed; ``write`` is then used for
    nothing.  The files decode to the same pixels either way."""

    def __init__(self, logdir, A_static, bg_color, viz_interval, progress_interval=None, canon_nframes=60, save_ply=True, write=None):
        if int(viz_interval) < 1 or (progress_interval is not None and int(progress_interval) < 1):
            raise ValueError("RunOutputs: viz_interval and progress_interval must be >= 1")
        if write is None:
            try:
                import PIL.Image  # noqa: F401
            except ImportError as e:
                raise RuntimeError("RunOutputs: writing PNG files needs PIL; pass write=fn(path, uint8 array) to write them otherwise") from e
            write = _write_png
        self.logdir, self.A_static, self.bg_color = str(logdir), A_static, bg_color
        self.viz_interval = int(viz_interval)
        self.progress_interval = None if progress_interval is None else int(progress_interval)
        self.canon_nframes, self.save_ply, self.write = int(canon_nframes), bool(save_ply), write
        self.canon_size, self.progress_size, self.frames_per_launch = 512, 256, 8       # gs_trainer.py:767
        self.progress_video, self.video_name, self.video_quality = False, "progress", 90
        self._video = self._video_encoder = None
        self.device_png = False
        self._png_encoders = {}

    def due(self, t):
        """The outputs of iteration ``t``, a subset of {"viz", "progress"}: gs_trainer.py:439 and :453 as written."""
        out = set()
        if t % self.viz_interval == 0:
            out.add("viz")
        if self.progress_interval is not None and t % self.progress_interval == 0:
            out.add("progress")
        return out

    def _put(self, rel, array):
        """``array``: uint8 on the GPU (copied here) or the numpy array of a copy the caller made."""
        path = os.path.join(self.logdir, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        self.write(path, array.cpu().numpy() if torch.is_tensor(array) else array)

    def _put_png(self, rels, u8):
        """``device_png``: ``u8`` uint8 [k,H,W,3] on the GPU -> the k files ``rels``, encoded in one call (one encoder per (W, H, K))."""
        from .frame_out import new_encoder
        from .png import write_atomic
        k, H, W = (int(n) for n in u8.shape[:3])
        K = max(k, self.frames_per_launch if k > 1 else 1)
        if (W, H, K) not in self._png_encoders:                  # (kept for the run: the pictures alternate between three sizes)
            self._png_encoders[W, H, K] = new_encoder("png", W, H, K, u8.device)
        for rel, data in zip(rels, self._png_encoders[W, H, K].encode_to_host(u8.contiguous())):
            path = os.path.join(self.logdir, rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            write_atomic(path, data)

    def _picture(self, rel, u8):
        """One picture, uint8 [H,W,3] on the GPU, to ``rel``."""
        if self.device_png:
            self._put_png([rel], u8[None])
        else:
            self._put(rel, u8)

    @staticmethod
    def training_picture(gt, mask, bg, render_raw):
        """uint8 [H, 2W, 3] on the GPU: ``gt * mask + bg * (1 - mask)`` (loss.py:55) beside the clamped render, truncated to bytes."""
        if gt.dim() == 4:                                        # (a chunk of K frames: the picture shows its first)
            gt, mask, render_raw = gt[0], mask[0] if mask.dim() == 3 else mask, render_raw[0]
        composite = gt * mask + bg[:, None, None] * (1.0 - mask)
        return image_sheets(composite, render_raw, tiles_per_sheet=2, nrow=2, padding=0, quant="trunc")[0]

    @torch.no_grad()
    def after_step(self, trainer, t):
        due = self.due(t)
        if not due:
            return
        m = trainer.m
        attrs = m.decode()
        canon = {"xyz_canon": attrs["xyz_canon"], "rotmat_canon": attrs["rot6d_canon"], "scales": attrs["scales"],
                 "opacity": attrs["opacity"], "shs": attrs["shs"], "lbs_weights": m.lbs_weights, "active_sh_degree": trainer.sh_degree}
        if "viz" in due:
            if trainer.last_render is None:
                raise RuntimeError("RunOutputs: the trainer has kept no render of this step (set_outputs before the step)")
            inp = trainer.inputs
            self._picture(f"train/{t:06d}.png", self.training_picture(inp.gt, inp.mask, trainer.bg, trainer.last_render))
            for i0, u8 in _canon.render_canonical_chunks(canon, self.A_static, self.bg_color, nframes=self.canon_nframes,
                                                         img_size=self.canon_size, frames_per_launch=self.frames_per_launch):
                if self.device_png:
                    self._put_png([f"canon/{i0 + j:05d}.png" for j in range(int(u8.shape[0]))], u8)
                    continue
                for j, frame in enumerate(u8.cpu().numpy()):     # (one copy per launch)
                    self._put(f"canon/{i0 + j:05d}.png", frame)
            if self.save_ply:
                self._save_ply(trainer, attrs, os.path.join(self.logdir, "meshes", f"human_pcd_{t:06d}_splat.ply"))
        if "progress" in due:
            sheet = _canon.progress_sheet(canon, self.A_static, self.bg_color, img_size=self.progress_size)
            self._picture(f"train_progress/{t:06d}.png", sheet)
            if self.progress_video:
                self._append_video(sheet)

    video_path = property(lambda self: os.path.join(self.logdir, f"train_{self.video_name}.avi"))

    def _append_video(self, sheet):
        """``sheet``: uint8 [Hs,Ws,3] on the GPU -> one more frame of the progress video (opened at the first sheet)."""
        from .frame_out import new_encoder
        from .video import MjpegWriter
        Hs, Ws = int(sheet.shape[0]), int(sheet.shape[1])
        if self._video is None:
            os.makedirs(self.logdir, exist_ok=True)
            self._video_encoder = new_encoder("jpeg", Ws, Hs, 1, sheet.device, self.video_quality)
            self._video = MjpegWriter(self.video_path, Ws, Hs, 10)                 # fps=10: gs_trainer.py:465
        self._video.write(self._video_encoder.encode_to_host(sheet[None].contiguous())[0])

    def finish(self):
        """Closes the progress video (the file appears under its name here); nothing to do without ``progress_video``."""
        if self._video is not None:
            self._video.close()
            self._video = self._video_encoder = None

    def _save_ply(self, trainer, attrs, path):
        from . import rotations as R
        from .export import save_ply
        n, dev = int(attrs["xyz_canon"].shape[0]), attrs["xyz_canon"].device
        rot6d = attrs["rot6d_canon"]
        rotq = torch.zeros(n, 4, device=dev) if rot6d is None else R.matrix_to_quaternion(R.rotation_6d_to_matrix(rot6d))
        save_ply({"xyz_canon": attrs["xyz_canon"], "shs": attrs["shs"], "opacity": attrs["opacity"],
                  "scales_canon": trainer._scales_canon(attrs), "rotq_canon": rotq}, path)
