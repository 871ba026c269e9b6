"""The monocular depth-consistency and depth-smoothness prior losses of the reference's default configuration (mono_loss.py
DepthConsistencyLoss / DepthSmoothLoss, criterions.py:13-17,99-105,170-183, tile.py:923-948) on the HIP kernels of csrc/mono.hip.

Per training step, on the batch's rays with valid = fore_valid | bg_valid and rendered depth p = pred_depth:
    L_depth  = sum_views sum_rays m (h0_v p + h1_v - t)^2 / sum m, (h0_v, h1_v) = the least-squares scale / shift of p onto the
               monocular depth t over view v's valid rays (0 when the view's system is singular);
    L_smooth = mean over the valid 2x2 patches of 0.25 sum_edges |normalize(mean n) . normalize(edge)|, the edges of the patch's
               back-projected points K^-1 (x, y, 1) p; a patch is valid when its four rays are and their monocular normals agree
               (n_r . mean n > 0.9);
    L        = w_depth(step) L_depth + w_smooth(step) L_smooth,  w(step) = w 0.1^((step - start) / 30000) for start < step < end.
The gradient w.r.t. p is added to the rendered depth's column of the training step's grad_out before the backward, so under
pose_grads the terms reach the poses through the existing ray gradients.

Differences from the reference, all deliberate:
  * With no valid patch the smoothness term contributes 0 with a zero gradient; the reference's torch.mean of an empty tensor is
    NaN, which reaches the total loss and every gradient.
  * The per-view moments are accumulated and the 2x2 system solved in float64: for ill-conditioned views (depths varying by a
    few per cent) this gives the exact-arithmetic answer, not the reference's float32 cancellation.
  * The gradient through (h0, h1) is taken as its analytic value, 0 (h minimises the same quadratic); float64 autograd through
    the reference's solve agrees to rounding (tests/test_gpu_mono.py).
  * Views are grouped by locs[:, 0], not by reshaping the batch to [num_camera, -1]: any ray order works.
Maps stay on the device as float32; the raw terms of the last step are kept as device tensors (no host synchronisation).
"""
import torch

from . import render
from ._capi import check, dev_ptr, lib, stream

_f32 = torch.float32
DECAY_STEPS = 30000   # criterions.py:13-17


def weight_decay(weight, step):
    """criterions.depth_weight_decay_func / smooth_weight_decay_func."""
    return weight * (0.1 ** (step / DECAY_STEPS))


class MonoLoss:
    """mono_loss.DepthConsistencyLoss + DepthSmoothLoss with criterions' two LossItems for the fused training step.

    ks [N,3,3] intrinsics; mono_depths [N,H,W] and mono_normals [N,H,W,3] (train_data.mono_depths / mono_normals; None = that term
    off); weight_depth / weight_smooth = WEIGHT_DEPTH_LOSS / WEIGHT_DEPTH_SMOOTH_LOSS; depth_start / smooth_start =
    DEPTH_LOSS_START / DEPTH_SMOOTH_LOSS_START; end_step = TRAINING.TOTAL_STEP (None = no end)."""

    def __init__(self, ks, mono_depths=None, mono_normals=None, weight_depth=0.01, weight_smooth=0.001, depth_start=0,
                 smooth_start=0, end_step=None):
        if mono_depths is None and mono_normals is None:
            raise ValueError("MonoLoss: needs mono_depths [N,H,W] or mono_normals [N,H,W,3]")
        if ks.dim() != 3 or tuple(ks.shape[1:]) != (3, 3):
            raise ValueError(f"MonoLoss: ks must be [N,3,3], got {tuple(ks.shape)}")
        N = ks.shape[0]
        ref = mono_depths if mono_depths is not None else mono_normals
        if ref.dim() < 3 or ref.shape[0] != N:
            raise ValueError(f"MonoLoss: maps must be [N={N},H,W(,3)], got {tuple(ref.shape)}")
        self.N, self.H, self.W = N, ref.shape[1], ref.shape[2]
        if mono_depths is not None and tuple(mono_depths.shape) != (N, self.H, self.W):
            raise ValueError(f"MonoLoss: mono_depths must be [N,H,W] = {(N, self.H, self.W)}, got {tuple(mono_depths.shape)}")
        if mono_normals is not None and tuple(mono_normals.shape) != (N, self.H, self.W, 3):
            raise ValueError(f"MonoLoss: mono_normals must be [N,H,W,3] = {(N, self.H, self.W, 3)}, got {tuple(mono_normals.shape)}")
        self.device = ref.device
        self.mono_depths = None if mono_depths is None else mono_depths.detach().to(self.device, _f32).contiguous()
        self.mono_normals = None if mono_normals is None else mono_normals.detach().to(self.device, _f32).contiguous()
        # K^-1 once, in float64 (the reference inverts ks every step)
        self.kinv = torch.linalg.inv(ks.detach().to(torch.float64).cpu()).reshape(N, 9).to(self.device, _f32).contiguous()
        self.weight_depth, self.weight_smooth = float(weight_depth), float(weight_smooth)
        self.depth_start, self.smooth_start = int(depth_start), int(smooth_start)
        self.end_step = end_step
        self.last_depth_loss = None    # raw L_depth of the last step that computed the term ([] device tensor)
        self.last_smooth_loss = None   # raw L_smooth

    # ---- schedule (LossItem.__call__: added for start < step < end, weight decayed from start) -------------------------------
    def _scale(self, weight, start, step):
        if weight == 0.0 or step <= start or (self.end_step is not None and step >= self.end_step):
            return 0.0
        return weight_decay(weight, step - start)

    def scale_depth(self, step):
        return 0.0 if self.mono_depths is None else self._scale(self.weight_depth, self.depth_start, step)

    def scale_smooth(self, step):
        return 0.0 if self.mono_normals is None else self._scale(self.weight_smooth, self.smooth_start, step)

    def active(self, step):
        """Whether either term is added at this step."""
        return self.scale_depth(step) != 0.0 or self.scale_smooth(step) != 0.0

    # ---- one step ------------------------------------------------------------------------------------------------------------
    def loss_grad(self, locs, depth, valid, w_depth, w_smooth):
        """-> (loss [3]: weighted total, raw L_depth, raw L_smooth; dL/d(depth) [B]) at the given weights (0 = term off)."""
        B = depth.shape[0]
        if depth.dim() != 1:
            raise ValueError(f"MonoLoss: depth must be [B], got {tuple(depth.shape)}")
        if tuple(locs.shape) != (B, 3):
            raise ValueError(f"MonoLoss: locs must be [B={B},3] (view, px, py), got {tuple(locs.shape)}")
        if valid is not None and tuple(valid.shape) != (B,):
            raise ValueError(f"MonoLoss: valid must be [B={B}], got {tuple(valid.shape)}")
        if w_smooth != 0.0 and B % 4:
            raise ValueError(f"MonoLoss: the smoothness term needs whole 2x2 patches, B={B} is not a multiple of 4")
        dev = depth.device
        depth = depth.detach().contiguous()          # (held here: the kernels read them after the pointers are taken)
        locs = locs.to(torch.int32).contiguous()
        loss = torch.empty(3, dtype=_f32, device=dev)
        grad = torch.empty(B, dtype=_f32, device=dev)
        n = lib().scanerf_mono_scratch_floats(B, self.N)
        scratch = torch.empty(n, dtype=_f32, device=dev)
        check(lib().scanerf_mono_loss_grad(
            dev_ptr(depth, _f32, "depth"), dev_ptr(valid, (torch.bool, torch.uint8), "valid", allow_none=True),
            dev_ptr(locs, torch.int32, "locs"),
            dev_ptr(self.mono_depths, _f32, "mono_depths", allow_none=True),
            dev_ptr(self.mono_normals, _f32, "mono_normals", allow_none=True), dev_ptr(self.kinv, _f32, "kinv"),
            self.N, self.H, self.W, B, float(w_depth), float(w_smooth), dev_ptr(loss, _f32, "loss"), dev_ptr(grad, _f32, "grad_depth"),
            dev_ptr(scratch, _f32, "scratch"), n, stream()), "mono_loss_grad")
        return loss, grad

    def __call__(self, step, locs, depth, valid=None):
        """-> None (no monocular term at this step) or (loss [1] weighted, dL/d(depth) [B]).  locs [B,3] int32 (view, px, py);
        depth [B] the rendered (merged) depth; valid [B] bool / uint8 or None (all)."""
        self.last_depth_loss = self.last_smooth_loss = None
        wd, ws = self.scale_depth(step), self.scale_smooth(step)
        if wd == 0.0 and ws == 0.0:
            return None
        if valid is not None:
            valid = valid.contiguous()
        loss, grad = self.loss_grad(locs, depth, valid, wd, ws)
        if wd != 0.0:
            self.last_depth_loss = loss[1]
        if ws != 0.0:
            self.last_smooth_loss = loss[2]
        return loss[0:1], grad

    # ---- hooks of tile_model's training steps: add the term's gradient to the photometric one --------------------------------
    def fused_term(self, step, locs, out, valid, grad_out):
        """Foreground-only step: grad_out[:, DEPTH] += dL/d(depth).  -> None or loss [1]."""
        r = self(step, locs, out[:, render.DEPTH].contiguous(), valid)
        if r is None:
            return None
        grad_out[:, render.DEPTH] += r[1]
        return r[0]

    def fgbg_term(self, step, locs, out_fg, out_bg, valid_fg, valid_bg, grad_fg, grad_bg):
        """Foreground + T_left * background step (tile.py:675-677: pred_depth = d_fg + T_left d_bg, valid = fore_valid | bg_valid):
        the foreground's depth column gets g, its T_left column g d_bg, the background's depth column T_left g.  -> None or loss [1]."""
        T = out_fg[:, render.T_LEFT]
        d_bg = out_bg[:, render.DEPTH]
        depth = (out_fg[:, render.DEPTH] + T * d_bg).contiguous()
        valid = None if valid_fg is None and valid_bg is None else (
            valid_bg if valid_fg is None else valid_fg if valid_bg is None else valid_fg.bool() | valid_bg.bool())
        r = self(step, locs, depth, valid)
        if r is None:
            return None
        g = r[1]
        grad_fg[:, render.DEPTH] += g
        grad_fg[:, render.T_LEFT] += g * d_bg
        grad_bg[:, render.DEPTH] += T * g
        return r[0]
