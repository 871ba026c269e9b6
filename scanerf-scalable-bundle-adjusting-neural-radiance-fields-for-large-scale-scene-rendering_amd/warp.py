"""The multi-view warp loss of the reference's default configuration (warp_loss.py:147-660 WarpLoss, criterions.py:19-21,92-97)
on the HIP kernels of csrc/warp.hip.

Per training step, on the rays the photometric term counts: p = rays_o + depth * rays_d is projected into the K <= 10 neighbour
views of lowest view cost (view_selection_kernel.cu:19-72), the colour those views saw there is fetched bilinearly, and
    L = w(step) * mean over B x K of score * mean_c((clamp(diffuse + specular, 0, 1) - neighbour colour)^2)
with score = visibility (a no-grad render of the neighbour rays with the tile's own renderer) x the neighbours' and the ray's
diffuse scores.  The gradient reaches depth, diffuse and specular, the rays, and the neighbour cameras' rts -- the multi-view
signal that refines the poses of views other than the one that owns a ray.

Differences from the reference, both deliberate:
  * K = min(top_k, number of cameras): torch.topk(k=10) raises when a tile sees fewer than 10 cameras.
  * dL/drts is summed in a fixed order, not with float atomics: the same inputs give bit-identical gradients.
Images and occlusion masks stay on the device; the only host synchronisation is the count of valid slots that the visibility
render's compaction needs.
"""
import torch

from ._capi import check, dev_ptr, lib, stream

_f32 = torch.float32
# out_ray columns (render.py) of the per-ray quantities the warp term reads: depth, diffuse (3), specular (3)
Q_COLS = (3, 5, 6, 7, 8, 9, 10)
T_LEFT_COL = 4


def warp_weight_warming(weight, step):
    """criterions.py:19-21: the weight ramps linearly over the first 10 000 steps."""
    return weight * max(min(step / 10000, 1.0), 0.0)


def ray_quantities(out_ray):
    """[B,16] render output -> [B,7] (depth, diffuse, specular), the kernels' ray_q."""
    return out_ray[:, list(Q_COLS)].contiguous()


class WarpLoss:
    """warp_loss.WarpLoss for the fused training step.

    cameras: an object with ks [N,3,3] and get_rts() -> [N,3,4] world-to-camera (cameras.CameraSet); images [N,H,W,3] f32 on the
    device (the training images, colours in [0, 1]); occlusions [N,H,W] bool (None = all true, tile.py:251,373); voxel_size =
    max(tile_size / finest resolution) (warp_loss.py:149); alpha / gamma = LOSS.ALPHA / LOSS.GAMMA; weight = WEIGHT_WARP_LOSS,
    start_step = WARP_LOSS_START, warming = WARP_WARPING (criterions.py:92-97, LossItem.__call__)."""

    VALID_COST = 0.176   # warp_loss.py:408

    def __init__(self, cameras, images, occlusions=None, voxel_size=None, alpha=10.0, gamma=20.0, top_k=10, weight=1.0,
                 start_step=0, warming=True):
        if voxel_size is None:
            raise ValueError("WarpLoss: voxel_size is required (max(tile_size / finest_resolution), warp_loss.py:149)")
        N = cameras.ks.shape[0]
        if images.dim() != 4 or images.shape[0] != N or images.shape[3] != 3:
            raise ValueError(f"WarpLoss: images must be [N={N},H,W,3], got {tuple(images.shape)}")
        self.cameras = cameras
        self.images = images.contiguous()
        self.N, self.H, self.W = N, images.shape[1], images.shape[2]
        if occlusions is not None:
            if tuple(occlusions.shape) != (N, self.H, self.W):
                raise ValueError(f"WarpLoss: occlusions must be [N,H,W] = {(N, self.H, self.W)}, got {tuple(occlusions.shape)}")
            occlusions = occlusions.to(torch.bool).contiguous()
        self.occlusions = occlusions
        self._ks = cameras.ks.detach().to(_f32).reshape(N, 9).contiguous()
        self.K = min(int(top_k), N)
        if not 1 <= self.K <= lib().scanerf_warp_max_neighbors():
            raise ValueError(f"WarpLoss: top_k={top_k} out of range")
        self.voxel_size, self.alpha, self.gamma = float(voxel_size), float(alpha), float(gamma)
        self.weight, self.start_step, self.warming = float(weight), int(start_step), bool(warming)
        self.last_loss = None       # weighted warp loss of the last step that computed it ([1] device tensor)
        self.last_grad_rts = None   # its dL/drts [N,3,4]

    # ---- schedule (LossItem.__call__: added only after start_step, weight warmed from there) -------------------------------
    def scale(self, step):
        if step <= self.start_step:
            return 0.0
        return warp_weight_warming(self.weight, step - self.start_step) if self.warming else self.weight

    def _cams(self, rts):
        """(ks [N,9], rts [N,12]) for the kernels; rts None = the cameras' current poses (get_rts evaluates the se(3) series in
        ~100 small torch launches: __call__ does it once per step and passes the result on)."""
        rts = (self.cameras.get_rts() if rts is None else rts).detach().reshape(self.N, 12).contiguous()
        return self._ks, rts

    # ---- the three kernels ---------------------------------------------------------------------------------------------------
    def select(self, rays_o, rays_d, q, ray_valid=None, rts=None):
        """-> nei_views [B,K] int32, nei_cost [B,K], nei_valid [B,K] bool (warp_loss.py:390-413, no [N,B] cost matrix)."""
        ks, rts = self._cams(rts)
        B, K, dev = rays_o.shape[0], self.K, rays_o.device
        views = torch.empty((B, K), dtype=torch.int32, device=dev)
        cost = torch.empty((B, K), dtype=_f32, device=dev)
        valid = torch.empty((B, K), dtype=torch.bool, device=dev)
        check(lib().scanerf_warp_select_views(
            dev_ptr(rays_o, _f32, "rays_o"), dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(q, _f32, "ray_q"),
            dev_ptr(ray_valid, (torch.bool, torch.uint8), "ray_valid", allow_none=True), dev_ptr(ks, _f32, "ks"),
            dev_ptr(rts, _f32, "rts"), self.N, self.H, self.W, K, B, dev_ptr(views, torch.int32, "nei_views"),
            dev_ptr(cost, _f32, "nei_cost"), dev_ptr(valid, torch.bool, "nei_valid"), stream()), "warp_select_views")
        return views, cost, valid

    def project(self, rays_o, rays_d, q, views, valid, rts=None):
        """-> dict grid [B,K,2], proj_depth [B,K], nei_origin / nei_direction [B,K,3], color [B,K,3], valid [B,K] bool (occlusion
        applied) -- proj2neighbor_forward + sample_neighbor_color (warp_loss.py:415-521)."""
        ks, rts = self._cams(rts)
        B, K, dev = rays_o.shape[0], views.shape[1], rays_o.device
        e = lambda *s: torch.empty((B, K) + s, dtype=_f32, device=dev)
        r = {"grid": e(2), "proj_depth": e(), "nei_origin": e(3), "nei_direction": e(3), "color": e(3),
             "valid": torch.empty((B, K), dtype=torch.bool, device=dev), "views": views}
        check(lib().scanerf_warp_project(
            dev_ptr(rays_o, _f32, "rays_o"), dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(q, _f32, "ray_q"), dev_ptr(ks, _f32, "ks"),
            dev_ptr(rts, _f32, "rts"), dev_ptr(views, torch.int32, "nei_views"), dev_ptr(valid, torch.bool, "nei_valid_in"),
            dev_ptr(self.images, _f32, "images"), dev_ptr(self.occlusions, torch.bool, "occlusions", allow_none=True),
            self.N, self.H, self.W, K, B, dev_ptr(r["grid"], _f32, "grid"), dev_ptr(r["proj_depth"], _f32, "proj_depth"),
            dev_ptr(r["nei_origin"], _f32, "nei_origin"), dev_ptr(r["nei_direction"], _f32, "nei_direction"),
            dev_ptr(r["color"], _f32, "nei_color"), dev_ptr(r["valid"], torch.bool, "nei_valid"), stream()), "warp_project")
        return r

    def loss_grad(self, rays_o, rays_d, q, ray_valid, proj, score, scale, rts=None):
        """-> loss [1], dL/d(ray_q) [B,7], dL/d(rays_o), dL/d(rays_d) [B,3], dL/drts [N,3,4] for given scores [B,K]."""
        ks, rts = self._cams(rts)
        B, K, dev = rays_o.shape[0], proj["views"].shape[1], rays_o.device
        loss = torch.empty(1, dtype=_f32, device=dev)
        gq = torch.empty((B, 7), dtype=_f32, device=dev)
        g_o, g_d = torch.empty((B, 3), dtype=_f32, device=dev), torch.empty((B, 3), dtype=_f32, device=dev)
        g_rts = torch.empty((self.N, 3, 4), dtype=_f32, device=dev)
        n = lib().scanerf_warp_scratch_floats(B, K, self.N)
        scratch = torch.empty(n, dtype=_f32, device=dev)
        score = score.to(_f32).contiguous()
        check(lib().scanerf_warp_loss_grad(
            dev_ptr(rays_o, _f32, "rays_o"), dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(q, _f32, "ray_q"),
            dev_ptr(ray_valid, (torch.bool, torch.uint8), "ray_valid", allow_none=True), dev_ptr(ks, _f32, "ks"),
            dev_ptr(rts, _f32, "rts"), dev_ptr(proj["views"], torch.int32, "nei_views"), dev_ptr(proj["valid"], torch.bool, "nei_valid"),
            dev_ptr(proj["grid"], _f32, "grid"), dev_ptr(proj["color"], _f32, "nei_color"), dev_ptr(score, _f32, "score"),
            dev_ptr(self.images, _f32, "images"), self.N, self.H, self.W, K, B, float(scale), dev_ptr(loss, _f32, "loss"),
            dev_ptr(gq, _f32, "grad_q"), dev_ptr(g_o, _f32, "grad_o"), dev_ptr(g_d, _f32, "grad_d"), dev_ptr(g_rts, _f32, "grad_rts"),
            dev_ptr(scratch, _f32, "scratch"), n, stream()), "warp_loss_grad")
        return loss, gq, g_o, g_d, g_rts

    # ---- scores (no grad): compute_visibility + soft_vis / soft_diffuse (warp_loss.py:222-229, :355-378, :640-650) -------------
    @torch.no_grad()
    def scores(self, q, proj, render_fn):
        """render_fn(rays_o [M,3], rays_d [M,3]) -> (depth [M], specular [M,3]): the tile's renderer, no grad.  -> score [B,K]."""
        valid = proj["valid"]
        score = torch.zeros(valid.shape, dtype=_f32, device=valid.device)
        sel = valid.reshape(-1).nonzero()[:, 0]          # the one host synchronisation: the number of valid slots
        if sel.numel():
            o = proj["nei_origin"].reshape(-1, 3)[sel].contiguous()
            d = proj["nei_direction"].reshape(-1, 3)[sel].contiguous()
            depth, spec = render_fn(o, d)
            vis = torch.exp(-self.alpha * (depth.reshape(-1) - proj["proj_depth"].reshape(-1)[sel]).abs() / self.voxel_size)
            nei_diffuse = torch.exp(-self.gamma * spec.mean(-1))
            score.view(-1)[sel] = vis * nei_diffuse
        ref_diffuse = torch.exp(-self.gamma * q[:, 4:7].mean(-1, keepdim=True))
        return score * ref_diffuse

    # ---- one step ----------------------------------------------------------------------------------------------------------
    def __call__(self, step, rays_o, rays_d, q, ray_valid, render_fn, rts=None):
        """-> None (no warp term at this step) or (loss [1] weighted, dL/d(ray_q) [B,7], dL/d(rays_o), dL/d(rays_d), dL/drts
        [N,3,4]).  q = [depth, diffuse, specular] [B,7] of the merged prediction; ray_valid [B] bool or None (all)."""
        self.last_loss = self.last_grad_rts = None
        scale = self.scale(step)
        if scale == 0.0 or rays_o.shape[0] == 0:
            return None
        q = q.detach().contiguous()
        with torch.no_grad():
            rts = self._cams(rts)[1]
            views, _, valid = self.select(rays_o, rays_d, q, ray_valid, rts)
            proj = self.project(rays_o, rays_d, q, views, valid, rts)
            score = self.scores(q, proj, render_fn)
            r = self.loss_grad(rays_o, rays_d, q, ray_valid, proj, score, scale, rts)
        self.last_loss, self.last_grad_rts = r[0], r[4]
        return r

    # ---- hooks of tile_model's training steps: add the term's gradients to the photometric ones ------------------------------
    def fused_term(self, step, rays_o, rays_d, out, ray_valid, grad_out, render_fn):
        """Foreground-only step: grad_out [B,16] += the warp gradient in the depth / diffuse / specular columns.
        -> None or (loss, dL/d(rays_o), dL/d(rays_d))."""
        r = self(step, rays_o, rays_d, ray_quantities(out), ray_valid, render_fn)
        if r is None:
            return None
        grad_out[:, list(Q_COLS)] += r[1]
        return r[0], r[2], r[3]

    def fgbg_term(self, step, rays_o, rays_d, out_fg, out_bg, valid_fg, valid_bg, grad_fg, grad_bg, render_fn):
        """Foreground + T_left * background step (tile.py:675-689: q = q_fg + T_left q_bg): the foreground columns get g, its T_left
        column g . q_bg, the background columns T_left g; rays valid in one branch only as photometric_loss_grad_fgbg treats them
        (the invalid branch holds zeros and T_left = 1).  -> None or (loss, dL/d(rays_o), dL/d(rays_d))."""
        T = out_fg[:, T_LEFT_COL:T_LEFT_COL + 1]
        q_bg = ray_quantities(out_bg)
        q = ray_quantities(out_fg) + T * q_bg
        valid = None if valid_fg is None and valid_bg is None else (
            valid_bg if valid_fg is None else valid_fg if valid_bg is None else valid_fg | valid_bg)
        r = self(step, rays_o, rays_d, q, valid, render_fn)
        if r is None:
            return None
        g = r[1]
        grad_fg[:, list(Q_COLS)] += g
        grad_fg[:, T_LEFT_COL] += (g * q_bg).sum(-1)
        grad_bg[:, list(Q_COLS)] += T * g
        return r[0], r[2], r[3]
