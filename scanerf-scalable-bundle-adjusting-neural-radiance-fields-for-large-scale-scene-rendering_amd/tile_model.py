"""Per-tile model and training step: the build's counterpart of the slice of tile.py /
hashgrid/__init__.py that turns the hot-path kernels into a training iteration
(tile.py:639-692 render_rays, :880-1015 train_one_step; hashgrid/__init__.py:413-596).

Two execution paths over the same parameters:

  * "ops":   the reference's own structure -- HIP sampler + HIP hash encoder behind the
             binding-surface names, decoder and compositing in torch (autograd), dense torch
             gradient of the table, fused sparse Adam kernel on the table;
  * "fused": one HIP launch for render forward and one for backward (render.py).

Scope is the foreground branch on synthetic rays; data loading, pose refinement and pruning schedules belong to the
trainer.  The warp and monocular loss terms join the fused steps through their hooks (warp.WarpLoss,
mono.MonoLoss: warp=, mono= / locs=).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _capi, network, render
from .cuda import adam_step_cuda, sample_points_grid
from .hashgrid import HashEmbeddingBG, level_resolutions
from .network import sh3
# the branch pass, its timer sections and the table-gradient routes live with the kernels' wrappers
from .render import (_TABLE_ROUTES, AUTOGRAD, FGBG_GRADIENTS, FGBG_STEP, MLP_FLOPS_PER_SAMPLE, POINTS_ADAM, POINTS_TABLE,  # noqa: F401
                     RAYS_ADAM, RECORDS_ADAM, RECORDS_TABLE, SINGLE, _Branch, _sec)

def composite_weights(sigma, dists, rays_d, infinity):
    """Alpha compositing weights of hashgrid/__init__.py:344-360 in torch: delta = dists * |d| (last sample 1e10 for a background
    ray), alpha = 1 - exp(-sigma delta), T_i = prod_{j<i} (1 - alpha_j + 1e-6), w = alpha T -> (w [B,S], T_left [B] = the
    transmittance BEFORE the last sample, the reference's quirk)."""
    delta = dists * rays_d.norm(dim=-1, keepdim=True)
    if infinity:
        delta = torch.cat([delta[:, :-1], torch.full_like(delta[:, :1], 1e10)], 1)
    alpha = 1.0 - torch.exp(-sigma * delta)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-6], 1), 1)[:, :-1]
    return alpha * T, T[:, -1]


@torch.no_grad()
def inverse_z_samples(rays_o, rays_d, box_center, box_half, num_sample, invalid_underground, floor_y=None):
    """Background samples in inverse depth beyond the HashGrid's 2x box (hashgrid/__init__.py:287-337): far = the ray's exit from
    the box (HIP ray_aabb_intersection; 0.1 for rays that miss it), z = 1 / ((1 - t) / (far + 1e-6) + t / 1e6) for t = linspace(0, 1, S),
    dists = differences with 1e-6 last; valid = not leaving through the floor y = floor_y (within 1e-4) when invalid_underground."""
    from .cuda import ray_aabb_intersection
    B, dev = rays_o.shape[0], rays_o.device
    bounds = torch.full((B, 2), -1.0, device=dev)
    ray_aabb_intersection(rays_o.contiguous(), rays_d.contiguous(), box_center.contiguous(), box_half.contiguous(), bounds)
    if invalid_underground:
        exit_y = rays_o[:, 1] + bounds[:, 1] * rays_d[:, 1]
        valid = ~(torch.abs(exit_y - floor_y) < 0.0001)
    else:
        valid = torch.ones(B, dtype=torch.bool, device=dev)
    far = torch.where(torch.any(bounds == -1, dim=-1, keepdim=True), torch.full_like(bounds[:, 1:], 0.1), bounds[:, 1:])
    t = torch.linspace(0.0, 1.0, steps=num_sample, device=dev)[None, :]
    z = (1.0 / (1.0 / (far + 1e-6) * (1.0 - t) + 1.0 / 1e6 * t)).contiguous()
    d = torch.cat([z[:, 1:] - z[:, :-1], torch.full((B, 1), 1e-6, device=dev)], -1).contiguous()
    return z, d, valid


@torch.no_grad()
def mesh_background_samples(fmesh, rays_o, rays_d, num_sample, bbox_size):
    """Background samples of BG_MODE "BS" (hashgrid/__init__.py:296-303): fmesh.background_sampling (fastmesh.FastMesh: between
    the ray's exit from the box fmesh.set() was given and the mesh behind it) with sample_range = max(bbox_size) / 10, bbox_size the
    HashGrid's (2x) box as host floats; dists = forward differences with 1e-6 last; valid = the ray has a background."""
    z, valid = fmesh.background_sampling(rays_o, rays_d, num_sample, max(bbox_size) / 10)
    d = torch.cat([z[:, 1:] - z[:, :-1], torch.full((z.shape[0], 1), 1e-6, device=z.device)], -1).contiguous()
    return z, d, valid


def _bg_samples(model, rays_o, rays_d, S_bg, invalid_underground, bg_mode, fmesh):
    if bg_mode == "IZ":
        return model.inverse_z_sampling(rays_o, rays_d, S_bg, invalid_underground)
    if bg_mode != "BS":
        raise ValueError(f"scanerf: bg_mode must be 'IZ' or 'BS', got {bg_mode!r}")
    if fmesh is None:
        raise ValueError("scanerf: bg_mode='BS' needs fmesh (fastmesh.FastMesh)")
    return mesh_background_samples(fmesh, rays_o, rays_d, S_bg, model.bbox_size.tolist())


class Decoder(nn.Module):
    """sigma / diffuse / tint / SH-conditioned specular decoder of the reference's ShallowMLP (network.py:151-190).
    The parameters ARE the render-time blob (rendering.py:101-112: per layer [bias, W^T]), one flat tensor: the fused
    kernels read it as it is, their gradient is its .grad, and the optimiser steps one tensor instead of sixteen
    (Adam is element-wise, so the update is the same).  Per-layer views carry the reference's parameter names."""

    def __init__(self, seed=0, in_channel=32):
        super().__init__()
        self.in_channel = in_channel  # 2 features per level: 32 in the reference, 16 for BASELINE configs[0] (ops path only)
        self.layers = network.layers(in_channel)
        self.params = nn.Parameter(network.xavier_blob(seed, in_channel=in_channel))
        self._views = {}

    def _view(self, name, kind):
        """weight [out,in] / bias [out] of a layer as a (differentiable) view of the blob"""
        k = 0
        for n, o, i in self.layers:
            if n == name:
                return self.params[k:k + o] if kind == "bias" else self.params[k + o:k + o + i * o].reshape(i, o).t()
            k += o + i * o
        raise KeyError(name)

    def __getattr__(self, attr):  # e.g. sigma_layer_mlp_0_bias -> view (the names tile.py's optimiser groups use)
        for n, _, _ in network.LAYERS:
            for kind in ("weight", "bias"):
                if attr == n.replace(".", "_") + "_" + kind:
                    return self._view(n, kind)
        return super().__getattr__(attr)

    def ref_state_dict(self):
        return {f"{n}.{k}": self._view(n, k) for n, _, _ in network.LAYERS for k in ("weight", "bias")}

    def load_ref_state_dict(self, sd):
        with torch.no_grad():
            self.params.copy_(network.blob_from_state_dict(sd, self.in_channel).to(self.params.device))

    def blob(self):
        return self.params

    def _lin(self, name, x):
        return F.linear(x, self._view(name, "weight"), self._view(name, "bias"))

    def forward(self, feats, dirs, weight_feature):
        act = lambda u: torch.exp(u * u * -50.0)
        v = dirs / (dirs.norm(2, dim=-1, keepdim=True) + 1e-8)
        H = self._lin("Spatial_MLP.mlp.2", act(self._lin("Spatial_MLP.mlp.0", feats * weight_feature)))
        sigma = F.softplus(self._lin("sigma_layer.mlp.0", H[..., :32]))
        tint = torch.sigmoid(self._lin("tint_layer.mlp.0", H[..., :32]))
        dif = torch.sigmoid(self._lin("diffuse_layer.mlp.0", H[..., :32]))
        h = act(self._lin("Directional_MLP.mlp.0", torch.cat([H[..., 32:], sh3(v)], -1)))
        h = act(self._lin("Directional_MLP.mlp.2", h))
        spec = torch.sigmoid(self._lin("Directional_MLP.mlp.4", h))
        return sigma, dif, spec, tint


class TileModel(nn.Module):
    """Geometry + parameters of one tile (hashgrid/__init__.py:33-92 with model_path == ""):
    `corner`/`size` describe the tile; the hash grid covers the 2x box around it."""

    def __init__(self, corner, size, device, log2_T=19, grid_resolution=(32, 2048), sampler_log2dim=4, seed=0,
                 table_dtype=torch.float32, n_levels=16, fp16_moments=False):
        """fp16_moments (opt-in; tables of >= 2^22 entries behind the t16s backward only): the table's Adam moments are kept in
        half precision and updated as adam_step_cuda_fp16 does (cuda/adam_kernel.cu:98-144) -- NOT what the reference's live code
        runs (torch.optim.Adam with fp32 state, tile.py:301), hence never the default."""
        super().__init__()
        self.fp16_moments = bool(fp16_moments)
        self.n_levels = n_levels  # the reference hard-codes 16; other counts run on the "ops" path only (configs[0]: 8)
        corner = torch.as_tensor(corner, dtype=torch.float32)
        size = torch.as_tensor(size, dtype=torch.float32)
        self.device = device
        self.bbox_center = corner + size / 2.0
        self.bbox_size = size * 2
        self.min_bbox = self.bbox_center - self.bbox_size / 2.0
        fin = (self.bbox_size / self.bbox_size.min() * grid_resolution[1]).int()
        base = (self.bbox_size / self.bbox_size.min() * grid_resolution[0]).int()
        self.resolution = level_resolutions(base, fin, n_levels).to(device).contiguous()
        g = torch.Generator().manual_seed(seed)
        T = 2 ** log2_T
        std = math.sqrt(2.0 / (T * 2 + n_levels * 2))  # xavier_normal_ on [L,T,2] (PyHashGridBG.py:72-73)
        self.features = nn.Parameter((torch.randn(n_levels, T, 2, generator=g) * std).to(device))
        self.table_dtype = table_dtype
        self.decoder = Decoder(seed, 2 * n_levels).to(device)
        self.log2dim = (sampler_log2dim - torch.log2(self.bbox_size.max() / self.bbox_size).int()).int().to(device)
        self.occupied_grid = torch.ones(tuple(int(2 ** k) for k in self.log2dim), dtype=torch.bool, device=device)
        self._occ_full = True  # set_occupancy() keeps it in step with the grid
        self.occ_corner = (self.min_bbox + self.bbox_size / 4.0).to(device).contiguous()
        self.occ_size = (self.bbox_size / 2.0).to(device).contiguous()
        self._min_dev = self.min_bbox.to(device)
        self._size_dev = self.bbox_size.to(device)
        self._center_dev = self.bbox_center.to(device).contiguous()
        self._half_dev = (self.bbox_size / 2.0).to(device).contiguous()
        self.packed = render.PackedDecoder(device)
        # fused sparse Adam state for the table (cuda/adam_kernel.cu semantics)
        self.exp_avg = torch.zeros_like(self.features, dtype=torch.float16 if self.fp16_moments else torch.float32)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.adam_step = 0
        self._half_table = None       # f16 / bf16 gather copy of the table (configs[2]); kept in step by the Adam epilogue
        self._overflow_grad = None    # zero table for the fused scatter's workspace-overflow path (never filled per step)
        # (the stream each of the two was filled on, and the streams already ordered behind it: _capi.ordered_after)
        self._half_table_from = self._overflow_grad_from = None

    def gather_table(self):
        """The table the fused kernels gather from: the fp32 master, or its resident half-precision copy (half the gather
        bytes, fp32 accumulate).  The copy is converted ONCE; after that the accumulate's Adam epilogue rewrites exactly the
        entries it moves (train_step_fused), so there is no per-step full-table conversion."""
        if self.table_dtype == torch.float32:
            return self.features
        if self._half_table is None or self._half_table.dtype != self.table_dtype:
            self._half_table = self.features.detach().to(self.table_dtype).contiguous()
            self._half_table_from = (torch.cuda.current_stream(self._half_table.device), set()) if self._half_table.is_cuda else None
        elif self._half_table_from is not None:   # (converted under another stream: this one waits for it, once)
            _capi.ordered_after(*self._half_table_from)
        return self._half_table

    def invalidate_gather_table(self):
        """Call after writing the fp32 master any other way than through train_step_fused (loading a checkpoint, ...)."""
        self._half_table = None

    def overflow_grad(self):
        if self._overflow_grad is None:
            self._overflow_grad = torch.zeros_like(self.features)
            self._overflow_grad_from = (torch.cuda.current_stream(self._overflow_grad.device), set()) if self._overflow_grad.is_cuda else None
        elif self._overflow_grad_from is not None:   # (zero-filled under another stream: this one waits for it, once)
            _capi.ordered_after(*self._overflow_grad_from)
        return self._overflow_grad

    def set_occupancy(self, grid):
        """Replace the sampler's occupancy grid (pruning: hashgrid/__init__.py:138-225)."""
        if tuple(grid.shape) != tuple(self.occupied_grid.shape):
            raise ValueError(f"occupancy grid must be {tuple(self.occupied_grid.shape)}, got {tuple(grid.shape)}")
        self.occupied_grid = grid.to(self.device, torch.bool).contiguous()
        self._occ_full = bool(self.occupied_grid.all())

    def weight_feature(self, global_step):
        """Coarse-to-fine mask on the device, cached: it is constant once global_step >= 10 000."""
        key = min(int(global_step), 10000)
        # (built by small kernels on the current stream: one 32-float copy per stream that asks, so that no stream reads a mask
        # another one has not finished writing)
        st = torch.cuda.current_stream(self.device).cuda_stream if str(self.device).startswith("cuda") else 0
        hit = self.__dict__.setdefault("_wf_by_stream", {}).get(st)
        if hit is None or hit[0] != key:
            hit = self._wf_by_stream[st] = (key, network.weight_feature(global_step, self.device))
        return hit[1]

    # ---- sampling (no grad: hashgrid/__init__.py:278-285) -------------------------------
    @torch.no_grad()
    def sample(self, rays_o, rays_d, S):
        z = torch.full((rays_o.shape[0], S), -1.0, device=self.device)
        d = torch.full((rays_o.shape[0], S), -1.0, device=self.device)
        sample_points_grid(rays_o, rays_d, z, d, self.occ_corner, self.occ_size, self.occupied_grid, self.log2dim)
        return z, d

    # ---- "ops" path: binding-surface kernels + torch decoder / compositing --------------
    def render_fore_ops(self, rays_o, rays_d, S, global_step, train=True):
        z, dist = self.sample(rays_o, rays_d, S)
        valid = torch.all(z != -1, dim=-1)
        o, d, z, dist = rays_o[valid], rays_d[valid], z[valid], dist[valid]
        B = o.shape[0]
        pts = o[:, None, :] + z[..., None] * d[:, None, :]
        x = (pts.reshape(-1, 3) - self._min_dev) / self._size_dev * 4.0 - 2.0
        feats = HashEmbeddingBG(x.contiguous(), self.features, self.resolution).reshape(B, S, 2 * self.n_levels)
        wf = network.weight_feature(global_step, self.device)[:2 * self.n_levels]
        if self.n_levels == 16 and getattr(self, "hip_decoder", True):
            # the decoder as ONE HIP op each way (csrc/decoder.hip) on the encoder's rows and the per-sample directions -- the two
            # halves of the reference's concatenated input (hashgrid/__init__.py:547), never concatenated (round 6) -- and the
            # compositing as one op each way (csrc/composite.hip) instead of cal_integrate_weight + accumulate x 4 in torch
            from . import decoder_op
            sigma, dif, spec, tint = decoder_op.decoder_apply_parts(feats.reshape(-1, 32), d[:, None, :].expand(B, S, 3).reshape(-1, 3),
                                                                    self.decoder.blob(), wf)
            if S <= render.COMPOSITE_BACKWARD_MAX_S:
                out_ray, w2 = render.composite_rays(sigma, dif, spec, tint, z, dist, d, False)
                out = {"valid": valid, "depth": out_ray[:, render.DEPTH], "diffuse": out_ray[:, render.DIFFUSE],
                       "specular": out_ray[:, render.SPECULAR], "T_left": out_ray[:, render.T_LEFT], "weights": w2, "rgb": out_ray[:, render.RGB]}
                if train:
                    out["l2_reg_specular"] = out_ray[:, render.W_SPEC2].sum() / (3.0 * B)   # = (w.detach() * spec ** 2).sum(1).mean() of the torch form below
                return out
            # (longer rays than the compositing op's adjoint takes: the torch compositing below, as hashgrid/grid.py does)
            sigma, dif, spec, tint = sigma.reshape(B, S, 1), dif.reshape(B, S, 3), spec.reshape(B, S, 3), tint.reshape(B, S, 3)
        else:   # other level counts (BASELINE configs[0]: 8), or hip_decoder = False: the torch graph
            sigma, dif, spec, tint = self.decoder(feats, d[:, None, :].expand(B, S, 3), wf)
        w2, T_left = composite_weights(sigma[..., 0], dist, d, False)
        w = w2[..., None]
        out = {"valid": valid, "depth": (w[..., 0] * z).sum(1), "diffuse": (w * dif).sum(1),
               "specular": (w * tint * spec).sum(1), "T_left": T_left, "weights": w[..., 0]}
        out["rgb"] = torch.clamp(out["diffuse"] + out["specular"], 0, 1)
        if train:
            out["l2_reg_specular"] = (w.detach() * spec ** 2).sum(1).mean()
        return out

    # ---- "fused" path -----------------------------------------------------------------------
    @torch.no_grad()
    def render_fore_fused(self, rays_o, rays_d, S, global_step):
        z, dist = self.sample(rays_o, rays_d, S)
        valid = torch.all(z != -1, dim=-1)
        self.packed.pack(self.decoder.blob(), network.weight_feature(global_step, self.device), (network.skip_levels(global_step) if LEVEL_SKIP else 0))
        table = self.gather_table()
        out, w = render.render_forward(rays_o, rays_d, z, dist, table, self.resolution, self.packed,
                                       self.min_bbox.tolist(), self.bbox_size.tolist(), render.FORE, False,
                                       ray_valid=valid)
        return out, w, valid

    # ---- background branch: inverse-depth sampling beyond the 2x box (hashgrid/__init__.py:306-337) ----
    @torch.no_grad()
    def inverse_z_sampling(self, rays_o, rays_d, S, invalid_underground=False):
        """hashgrid/__init__.py:306-337 (see inverse_z_samples)."""
        return inverse_z_samples(rays_o, rays_d, self._center_dev, self._half_dev, S, invalid_underground,
                                 floor_y=(self._center_dev - self._size_dev / 4.0)[1])

    @torch.no_grad()
    def render_rays_fused(self, rays_o, rays_d, S_fg, S_bg, global_step, invalid_underground=False, occlusion_mask=None,
                          bg_mode="IZ", fmesh=None):
        """tile.py:639-692 on the fused kernels: foreground (occupancy-sampled, contract_fore) and
        background (inverse-z, contract_bg, infinity) renders, merged with the foreground's T_left.
        occlusion_mask [B,1] bool (tile.py:655,661): both branches' valid sets are ANDed with it
        (hashgrid/__init__.py:420-421,479-480); a masked ray renders as zeros with T_left = 1, as every invalid ray.
        bg_mode "BS" with fmesh (fastmesh.FastMesh): the background is sampled between the box exit and the mesh behind it
        (mesh_background_samples) instead of in inverse depth; nothing else changes."""
        self.packed.pack(self.decoder.blob(), network.weight_feature(global_step, self.device), (network.skip_levels(global_step) if LEVEL_SKIP else 0))
        table = self.gather_table()
        box = (self.min_bbox.tolist(), self.bbox_size.tolist())
        z, dist = self.sample(rays_o, rays_d, S_fg)
        vf = torch.all(z != -1, dim=-1)
        if occlusion_mask is not None:
            vf = vf & occlusion_mask[..., 0]
        fg, wfg = render.render_forward(rays_o, rays_d, z, dist, table, self.resolution, self.packed, *box, render.FORE,
                                        False, ray_valid=vf)
        zb, db, vb = _bg_samples(self, rays_o, rays_d, S_bg, invalid_underground, bg_mode, fmesh)
        if occlusion_mask is not None:
            vb = vb & occlusion_mask[..., 0]
        bg, wbg = render.render_forward(rays_o, rays_d, zb, db, table, self.resolution, self.packed, *box, render.BG,
                                        True, ray_valid=vb)
        T = fg[:, render.T_LEFT, None]
        return {"fore_valid": vf, "bg_valid": vb, "T_left": T,
                "pred_color": fg[:, render.RGB] + T * bg[:, render.RGB],
                "pred_depth": fg[:, render.DEPTH, None] + T * bg[:, render.DEPTH, None],
                "pred_specular": fg[:, render.SPECULAR] + T * bg[:, render.SPECULAR],
                "pred_diffuse": fg[:, render.DIFFUSE] + T * bg[:, render.DIFFUSE],
                "fg": fg, "bg": bg, "fg_weights": wfg, "bg_weights": wbg, "fg_z_vals": z, "fg_dists": dist}

    # ---- surface normals and whole views (tile.py:695-756) ----------------------------------------------------------------------
    def _ray_normals(self, rays_o, rays_d, z, dist, valid):
        """sum_i w_i n_i [B,3] of sampled rays, zeros where `valid` (may be None) is off: one fused launch (csrc/normals.hip) on
        gather_table(), no coarse-to-fine mask (hashgrid/__init__.py:368-392 applies none)."""
        if self.n_levels != 16:
            raise RuntimeError("scanerf: the fused normals need 16 levels (the reference hard-codes them)")
        ones = torch.ones(32, dtype=torch.float32, device=self.device)
        out, _ = render.render_normals(rays_o.contiguous(), rays_d.contiguous(), z.contiguous(), dist.contiguous(), self.gather_table().detach(),
                                       self.resolution, self.decoder.blob().detach(), ones, self.min_bbox.tolist(), self.bbox_size.tolist(),
                                       False, ray_valid=valid)
        return out[:, :3]

    @torch.no_grad()
    def render_normals(self, rays_o, rays_d, S):
        """tile.py:695-712: the composited surface normals of the rays the foreground sampler serves, in their order, mapped to
        [0,1] as (sum_i w_i n_i + 1) / 2; None when it serves none.  (Valid = every sample placed, this package's fore_valid rule;
        the sampler fills a ray's row completely or not at all.)"""
        z, dist = self.sample(rays_o, rays_d, S)
        valid = torch.all(z != -1, dim=-1)
        if not bool(valid.any()):
            return None
        return (self._ray_normals(rays_o[valid], rays_d[valid], z[valid], dist[valid], None) + 1.0) / 2.0

    @torch.no_grad()
    def render_image_rays(self, rays_o, rays_d, S_fg, S_bg, global_step, occlusion_mask=None, batch_size=2 ** 14, normals=True,
                          invalid_underground=False, bg_mode="IZ", fmesh=None):
        """tile.py:724-756: a whole view in chunks of batch_size rays through render_rays_fused -> the reference's eight maps
        {"rgb", "fore_depth", "depth", "diffuse", "specular", "fore", "normal", "tint"} ([N,3], depths [N,1]).  "normal": what the
        reference's commented-out lines (:740,751) would fill -- render_normals' values on the fore-valid rays, zeros elsewhere
        (the chunk's own foreground samples and valid set go to the kernel, which writes zeros for the other rays: no second
        sampler launch, no compaction); normals=False leaves it black, as the reference ships it."""
        N = rays_o.shape[0]
        z3 = lambda: torch.zeros((N, 3), dtype=torch.float32, device=rays_o.device)
        z1 = lambda: torch.zeros((N, 1), dtype=torch.float32, device=rays_o.device)
        img = {"rgb": z3(), "fore_depth": z1(), "depth": z1(), "diffuse": z3(), "specular": z3(), "fore": z3(), "normal": z3(), "tint": z3()}
        for i in range(0, N, batch_size):
            o, d = rays_o[i:i + batch_size].contiguous(), rays_d[i:i + batch_size].contiguous()
            occ = None if occlusion_mask is None else occlusion_mask[i:i + batch_size]
            sl = slice(i, i + o.shape[0])
            out = self.render_rays_fused(o, d, S_fg, S_bg, global_step, invalid_underground=invalid_underground, occlusion_mask=occ,
                                         bg_mode=bg_mode, fmesh=fmesh)
            fg, vf = out["fg"], out["fore_valid"]
            img["rgb"][sl], img["depth"][sl] = out["pred_color"], out["pred_depth"]
            # (an invalid ray's foreground row is zeros: the masked scatters of tile.py:747-752 are these copies)
            img["fore_depth"][sl], img["fore"][sl], img["tint"][sl] = fg[:, render.DEPTH, None], fg[:, render.RGB], fg[:, render.TINT]
            img["diffuse"][sl], img["specular"][sl] = fg[:, render.DIFFUSE], fg[:, render.SPECULAR]
            if normals:
                n = self._ray_normals(o, d, out["fg_z_vals"], out["fg_dists"], vf)
                img["normal"][sl] = (n + 1.0) / 2.0 * vf[:, None]
        return img

    # ---- geometry out: the density's level set as a triangle mesh (the reference has none) ------------------------
    @torch.no_grad()
    def extract_mesh(self, n, level, global_step=None, normals=True, route="fused", min_faces=0, min_extent=0, keep_largest=None,
                     cameras=None, min_views=0, view_bias=None, view_far=None):
        """Surface nets over the tile box on a lattice of n = (nx, ny, nz) cells (an int: that many along the longest side, the others
        by the box's aspect), inside = sigma > level -> meshing.Mesh (world-space vertices, faces, cells, lattice, normals).
        global_step: the coarse-to-fine mask of that step; None = no mask, as the normals and the renderer read the table.
        min_faces / min_extent / keep_largest: meshing.filter_mesh's keep rule, applied before the normals are evaluated.
        cameras = (ks, c2ws, H, W) with min_views >= 1: the parts no camera saw go before that (meshing.cull_unseen)."""
        from . import meshing
        if self.n_levels != 16:
            raise RuntimeError("scanerf: the mesh extraction needs 16 levels (the reference hard-codes them)")
        if isinstance(n, int):
            n = meshing.cells_per_axis(self.occ_size, n)
        wf = torch.ones(32, dtype=torch.float32, device=self.device) if global_step is None else self.weight_feature(global_step)
        return meshing.extract_mesh(self.gather_table().detach(), self.resolution, self.decoder.blob().detach().contiguous(), wf,
                                    self.occupied_grid, self.log2dim, self.occ_corner, self.occ_size, n, level, normals=normals, route=route,
                                    min_faces=min_faces, min_extent=min_extent, keep_largest=keep_largest,
                                    cameras=cameras, min_views=min_views, view_bias=view_bias, view_far=view_far)

    # ---- optimiser on the table: fused sparse Adam (only touched entries move) --------------
    @torch.no_grad()
    def table_adam(self, lr, betas=(0.9, 0.99), eps=1e-15):
        g = self.features.grad
        K = self.features.numel() // 8
        adam_step_cuda(self.features.data.view(K, 8), g.view(K, 8), self.exp_avg.view(K, 8),
                       self.exp_avg_sq.view(K, 8), lr, betas[0], betas[1], eps, self.adam_step)
        self.adam_step += 1
        self._half_table = None  # (the fused path's epilogue keeps it in step instead: train_step_fused)


def sphere_shell_occupancy(model, radius, thickness):
    """Synthetic sampler occupancy: cells of the tile's sampling grid whose centre lies within
    thickness/2 of a sphere of `radius` around the tile centre -> bool grid shaped like model.occupied_grid."""
    dims = [int(2 ** k) for k in model.log2dim.tolist()]
    corner, size = model.occ_corner.cpu(), model.occ_size.cpu()
    axes = [corner[a] + (torch.arange(dims[a]) + 0.5) * (size[a] / dims[a]) - model.bbox_center[a] for a in range(3)]
    r = torch.sqrt(axes[0][:, None, None] ** 2 + axes[1][None, :, None] ** 2 + axes[2][None, None, :] ** 2)
    return (torch.abs(r - radius) <= thickness / 2.0).to(model.device).contiguous()


class KernelTimer:
    """HIP-event timing of named sections on torch's current stream (the stream every scanerf
    kernel is launched on).  bench.py uses it for the live per-kernel durations behind
    `roofline`; alg_bytes = algorithmic bytes of ONE launch of that section."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.events = {}
        self.bytes = {}
        self.flops = {}
        self.count = 0

    class _Section:
        def __init__(self, timer, name, alg_bytes, alg_flops=0):
            self.t, self.name, self.alg, self.flp = timer, name, alg_bytes, alg_flops

        def __enter__(self):
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

        def __exit__(self, *exc):
            self.e1.record()
            self.t.events.setdefault(self.name, []).append((self.e0, self.e1))
            self.t.bytes[self.name] = self.alg
            self.t.flops[self.name] = self.flp
            self.t.count += 1

    def section(self, name, alg_bytes=0, alg_flops=0):
        return KernelTimer._Section(self, name, alg_bytes, alg_flops)

    def summary(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) / len(v) for k, v in self.events.items()}

    def dominant(self, *_):
        """(name, avg ms, algorithmic bytes, algorithmic flops) of the section with the largest time."""
        s = self.summary()
        cand = {k: v for k, v in s.items() if self.bytes.get(k, 0) > 0} or s   # (sections without a byte count: time only)
        if not cand:
            return None, 0.0, 0, 0
        name = max(cand, key=cand.get)
        return name, cand[name], self.bytes[name], self.flops.get(name, 0)


def train_step_ops(model, dec_opt, rays_o, rays_d, target, S, global_step, table_lr=1e-2, timer=None):
    """One iteration of tile.py:880-1015 on the foreground branch: MSE + 0.01*l2_reg_specular
    (criterions.py:142-144, tile.py:999), decoder by torch Adam, table by the fused sparse Adam."""
    import sys
    _enc = sys.modules[__package__ + ".hashgrid.PyHashGridBG"]  # the module (the package re-exports the class)
    _enc.TIMER = timer
    model.features.grad = None
    dec_opt.zero_grad(set_to_none=True)
    with _sec(timer, "forward_total"):
        out = model.render_fore_ops(rays_o, rays_d, S, global_step, train=True)
        loss = F.mse_loss(out["rgb"], target[out["valid"]]) + 0.01 * out["l2_reg_specular"]
    with _sec(timer, "backward_total"):
        loss.backward()
    with _sec(timer, "sparse_adam", model.features.numel() * 32):
        model.table_adam(table_lr)
    dec_opt.step()
    _enc.TIMER = None
    return loss.detach()


# Route switches of the fused steps (module attributes; tests and A/B timings flip them, nothing reads the environment):
LARGE_T_ROUTE = "dfeat"     # tables above 2^21 entries: "dfeat" = stand-alone scatter from the backward's dfeat (default), "fused" = the
                            # backward's own records + the split pass
FORWARD_PLAN = True         # the forward launch counts the backward's record ranges (no separate plan launch)
LEVEL_SKIP = True           # levels whose coarse-to-fine weight is exactly zero are left out of gathers and records (same results)
JSTASH = True               # pose gradients: the forward stashes the encoder's position Jacobians for the backward


def table_grad_route(entry, T, B, S, arith, half_table=False, fused_adam=True, fused_scatter=None):
    """render.table_grad_route under this module's LARGE_T_ROUTE (only the steps' rows read it)."""
    return render.table_grad_route(entry, T, B, S, arith, half_table, fused_adam, fused_scatter, LARGE_T_ROUTE)


def _forward_plans(B, S, T):
    """The forward launch can reserve the t16 backward's record ranges itself (its hash indices are the plan's): no separate
    plan launch (0.25 ms at configs[1])."""
    return (render.backward_arith(True, False) in render._capi.T16_FAMILY and render.forward_plan_supported(B, S, T)
            and FORWARD_PLAN)


def _branch(model, *args, **kwargs):
    """render._Branch on the model's grid, decoder and 2x box; point gradients read the fp32 master."""
    return _Branch(model.resolution, model.packed, model.decoder.blob(), (model.min_bbox.tolist(), model.bbox_size.tolist()), *args,
                   master=model.features, box_dev=(model._min_dev, model._size_dev), **kwargs)


def _table_grad_adam(model, route, compact, rays_o, rays_d, branches, lr, timer):
    """The routes that end in the fused sparse Adam (no gradient table, no zero-fill, no dense optimiser scan): ONE step over
    the feature gradients of every branch."""
    B, S = rays_o.shape[0], sum(b.S for b in branches)
    over = model.overflow_grad()   # (the workspace-overflow path's zero table, never filled per step)
    adam = (model.features.data, model.exp_avg, model.exp_avg_sq, lr, 0.9, 0.99, 1e-15, model.adam_step)
    if route == RECORDS_ADAM:
        with _sec(timer, "table_grad_accumulate_adam", B * S * 16 * 64 + model.features.numel() * 28):
            if len(branches) == 1:
                render.scatter_accumulate_adam(branches[0].ws, *adam, B, S, half_table=model._half_table, overflow_grad=over,
                                               arith=branches[0].arith)
            else:
                fg, bg = branches
                render.scatter_accumulate_adam2(fg.ws, fg.S, bg.ws, bg.S, *adam, B, half_table=model._half_table,
                                                overflow_grad=over, arith=fg.arith)
    elif route == RAYS_ADAM:   # (the stand-alone scatter places the samples itself: rays + depths)
        with _sec(timer, "table_grad_scatter_adam", B * S * 16 * (8 + 16 * 8)):
            render.scatter_table_grad_adam_rays(rays_o, rays_d, [(b.z, b.dfeat, b.valid, b.box[2]) for b in branches],
                                                *branches[0].box[:2], model.resolution, *adam, overflow_grad=over,
                                                fp16_moments=model.fp16_moments)
    else:
        if len(branches) == 1:
            pts, dfeat = branches[0].points(), branches[0].dfeat
        else:
            pts, dfeat = torch.cat([b.points() for b in branches], 0), torch.cat([b.dfeat for b in branches], 1).contiguous()
        with _sec(timer, "table_grad_scatter_adam", B * S * 16 * (8 + 16 * 8)):
            render.scatter_table_grad_adam(pts, dfeat, model.resolution, *adam, half_table=model._half_table, overflow_grad=over,
                                           compact_records=compact)
    model.adam_step += 1


def train_step_fused(model, dec_opt, rays_o, rays_d, target, S, global_step, table_lr=1e-2, timer=None,
                     pose_grads=False, fused_scatter=None, compact_rays=None, dec_step=True, fused_adam=True, warp=None,
                     mono=None, locs=None):
    """The same iteration as train_step_ops on the fused kernels: one launch for the render forward,
    one for its adjoint, the atomic-free binned scatter for the table gradient, fused sparse Adam.
    fused_adam (default): the sparse Adam on the table runs in the accumulate's epilogue (no gradient table, model.features.grad
    is NOT set); False keeps accumulate -> model.features.grad -> adam_step_cuda (the binding-surface op).
    fused_scatter: True / False forces the backward's own records on / off (default: table_grad_route).
    pose_grads=True also returns dL/d(rays_o), dL/d(rays_d) (feed them to the pose graph:
    torch.autograd.backward([rays_o, rays_d], [g_o, g_d]) -- camera_utils.py:65-84 in the reference).
    warp (warp.WarpLoss, default None): the multi-view warp term joins the loss; its gradient is added to grad_out before the
    backward (and to the ray gradients with pose_grads), its dL/drts is left in warp.last_grad_rts.
    mono (mono.MonoLoss, default None) with locs [B,3] int32 (view, px, py) of the rays: the monocular depth / smoothness terms
    join the loss after the warp term; their depth gradient is added to grad_out before the backward.  The terms need the
    uncompacted batch (2x2 patches, per-view groups): mono turns valid-ray compaction off at the steps where a term is added
    (compact_rays=True with mono raises)."""
    _check_mono(mono, locs)
    if mono is not None and compact_rays:
        raise ValueError("train_step_fused: compact_rays=True cannot be combined with mono (the terms need the uncompacted batch)")
    B = rays_o.shape[0]
    dev = model.device
    with torch.no_grad():
        with _sec(timer, "sample_points_grid", B * (24 + 2 * 4 * S)):
            z, dist = model.sample(rays_o, rays_d, S)
        valid = render.ray_valid(z)  # all(z != -1) per ray (hashgrid/__init__.py:419)
        if compact_rays is None:  # a fully occupied sampler grid cannot produce invalid rays from inside the tile
            compact_rays = (not getattr(model, "_occ_full", False) and not pose_grads
                            and not (mono is not None and mono.active(global_step)))
        if compact_rays:
            # valid-ray compaction (hashgrid/__init__.py:419-421: the reference renders rays_o[valid] only) in one HIP launch
            # (csrc/compact.hip: wave ballot + popcount prefix sums): the fused backward runs its waves in lock step, so an
            # invalid ray costs as much as a valid one there
            with _sec(timer, "compact_rays", B * (36 + 8 * S)):
                n, co, cd, ct, cz, cdist = render.compact_rays(valid, rays_o, rays_d, target, z, dist)
            if n < B:
                rays_o, rays_d, target, z, dist = co, cd, ct, cz, cdist
                B = n
                valid = None
            if B == 0:
                return torch.zeros((), device=dev)
        model.packed.pack(model.decoder.blob(), model.weight_feature(global_step), (network.skip_levels(global_step) if LEVEL_SKIP else 0))
        # gather table: the fp32 master itself, or its resident bf16/f16 copy (configs[2]: half the gather bytes, fp32 accumulate)
        table = model.gather_table()
        T = model.features.shape[1]
        (route,), compact = table_grad_route(SINGLE, T, B, [S], render.backward_arith(True, pose_grads),
                                             model._half_table is not None, fused_adam, fused_scatter)
        br = _branch(model, rays_o, rays_d, z, dist, valid, render.FORE, False, route, compact, timer)
        plan = br.records and _forward_plans(B, S, T)
        out = br.forward(table, plan, jstash=plan and pose_grads and table.dtype == torch.float32 and JSTASH)
    # loss and dL/d(out_ray) in two launches (the torch graph for it was ~60 tiny kernels with host-bound gaps)
    loss, grad_out = render.photometric_loss_grad(out, target, valid, 0.01)
    wterm = None
    if warp is not None:
        with _sec(timer, "warp_loss"):
            wterm = warp.fused_term(global_step, rays_o, rays_d, out, valid, grad_out,
                                    lambda o, d: _visibility_render_fore(model, o, d, S, global_step))
    mterm = None
    if mono is not None:
        with _sec(timer, "mono_loss"):
            mterm = mono.fused_term(global_step, locs, out, valid, grad_out)
    with torch.no_grad():
        gtab = model.overflow_grad() if fused_adam else torch.zeros_like(model.features)
        gblob = torch.zeros(network.PARAMSIZE, device=dev)
        g = br.backward(grad_out, model.weight_feature(global_step), gblob, gtab, pose_grads)
        if g is not None and wterm is not None:
            g = (g[0] + wterm[1], g[1] + wterm[2])
        if fused_adam:
            _table_grad_adam(model, route, compact, rays_o, rays_d, [br], table_lr, timer)
        else:
            model.features.grad = gtab
            with _sec(timer, "sparse_adam", model.features.numel() * 28):
                model.table_adam(table_lr)
        model.decoder.params.grad = gblob
        if dec_step:  # False: the caller steps the optimiser itself (it holds more parameter groups: camera poses)
            dec_opt.step()
    if wterm is not None:
        loss = loss + wterm[0]
    if mterm is not None:
        loss = loss + mterm
    return (loss[0], *g) if pose_grads else loss[0]


def _check_mono(mono, locs):
    if mono is not None and locs is None:
        raise ValueError("scanerf: mono needs locs [B,3] int32 (view, px, py) of the batch's rays")


# ---- the warp term's visibility render (warp_loss.py:355-378: the tile's renderer on the neighbour rays, no grad) ---------------
# Fresh sample / output buffers and no plan workspace: the training forward's stashes (xstash, tile_T, jstash, record workspace),
# which the backward still reads, are left alone.  The decoder re-pack writes what the training step packed (same blob, same mask).
@torch.no_grad()
def _visibility_render_fore(model, rays_o, rays_d, S, global_step):
    out, _, _ = model.render_fore_fused(rays_o, rays_d, S, global_step)
    return out[:, render.DEPTH], out[:, render.SPECULAR]


@torch.no_grad()
def _visibility_render_fgbg(model, rays_o, rays_d, S_fg, S_bg, global_step, invalid_underground):
    r = model.render_rays_fused(rays_o, rays_d, S_fg, S_bg, global_step, invalid_underground)
    return r["pred_depth"][:, 0], r["pred_specular"]


def _fgbg_pass(model, rays_o, rays_d, target, S_fg, S_bg, global_step, invalid_underground, timer, pose_grads, warp, routes,
               compact, mono=None, locs=None, bg_mode="IZ", fmesh=None, occlusion_mask=None):
    """Both branches of a tile's render on `routes` (table_grad_route): forward, the merged loss (+ the warp, then the monocular
    terms), backward
    -> (loss [1], (fg, bg) _Branch, grad_blob, gradient table or None, (g_o, g_d) or None).  On the records + adam2 route the
    steps' timer sections, gather_table(), the forward's record plans and the background's own record workspace; elsewhere
    fgbg_gradients' reference: the fp32 master, only the backward timed."""
    B = rays_o.shape[0]
    dev = model.device
    T = model.features.shape[1]
    fused = routes[0] == RECORDS_ADAM
    if pose_grads and not fused and render.backward_arith(True, True) not in render._capi.T16_FAMILY:
        raise RuntimeError("scanerf: fgbg pose gradients need the t16 backward (render.set_arith)")
    with torch.no_grad():
        model.packed.pack(model.decoder.blob(), model.weight_feature(global_step), (network.skip_levels(global_step) if LEVEL_SKIP else 0))
        table = model.gather_table() if fused else model.features
        with _sec(timer if fused else None, "sample_points_grid", B * (24 + 2 * 4 * S_fg)):
            z, dist = model.sample(rays_o, rays_d, S_fg)
        vf = render.ray_valid(z) if fused else torch.all(z != -1, dim=-1)
        zb, db, vb = _bg_samples(model, rays_o, rays_d, S_bg, invalid_underground, bg_mode, fmesh)
        if occlusion_mask is not None:   # as render_rays_fused: both branches' valid sets
            vf &= occlusion_mask[..., 0].to(vf.dtype)   # (in place: render.ray_valid's flags keep their padded buffer)
            vb = vb & occlusion_mask[..., 0]
        ws_bg = None
        if fused:   # the background branch's own record workspace (both plans live until the one accumulate)
            need_bg = render.lib().scanerf_render_scatter_workspace_bytes(B, S_bg, T)
            if getattr(model, "_ws_bg", None) is None or model._ws_bg.numel() < need_bg:
                model._ws_bg = torch.empty(need_bg, dtype=torch.uint8, device=dev)
            ws_bg = model._ws_bg
        branches = (_branch(model, rays_o, rays_d, z, dist, vf, render.FORE, False, routes[0], compact, timer, fused),
                    _branch(model, rays_o, rays_d, zb, db, vb, render.BG, True, routes[1], compact, timer, fused, ws_bg))
        for b in branches:
            b.forward(table, plan=fused and _forward_plans(B, b.S, T), jstash=pose_grads)
    # merge and loss on the per-ray outputs (tile.py:666-690; criterions.py:142-144; tile.py:999), two HIP launches
    loss, gfg, gbg = render.photometric_loss_grad_fgbg(branches[0].out, branches[1].out, target, vf, vb, 0.01)
    wterm = None
    if warp is not None:
        with _sec(timer, "warp_loss"):
            wterm = warp.fgbg_term(global_step, rays_o, rays_d, branches[0].out, branches[1].out, vf, vb, gfg, gbg,
                                   lambda o, d: _visibility_render_fgbg(model, o, d, S_fg, S_bg, global_step, invalid_underground))
    mterm = None
    if mono is not None:
        with _sec(timer, "mono_loss"):
            mterm = mono.fgbg_term(global_step, locs, branches[0].out, branches[1].out, vf, vb, gfg, gbg)
    with torch.no_grad():
        gtab = torch.zeros_like(model.features) if routes[0] in _TABLE_ROUTES else None
        gblob = torch.zeros(network.PARAMSIZE, device=dev)
        if fused:
            gtab = model.overflow_grad()
        g = None
        for b, grad_out in zip(branches, (gfg, gbg)):
            gb = b.backward(grad_out, model.weight_feature(global_step), gblob, gtab, pose_grads)
            if gb is not None:
                g = gb if g is None else (g[0] + gb[0], g[1] + gb[1])
        if g is not None and wterm is not None:
            g = (g[0] + wterm[1], g[1] + wterm[2])
    if wterm is not None:
        loss = loss + wterm[0]
    if mterm is not None:
        loss = loss + mterm
    return loss, branches, gblob, gtab, g


def fgbg_gradients(model, rays_o, rays_d, target, S_fg, S_bg, global_step, invalid_underground=False, timer=None,
                   pose_grads=False, warp=None, mono=None, locs=None, bg_mode="IZ", fmesh=None, occlusion_mask=None):
    """Loss and parameter gradients of the complete per-tile render of tile.py:639-692 / :880-1015: foreground
    (occupancy-sampled, contract_fore) + T_left * background (inverse-z, contract_bg, infinity), MSE on the merged colour
    over all rays + 0.01 * (l2_reg_specular of both branches) -- two fused forward/backward pairs over the same table and
    decoder, each branch's table gradient into ONE gradient table.  Returns (loss, grad_table [16,T,2], grad_blob [13994])
    (+ dL/d(rays_o), dL/d(rays_d) with pose_grads: t16 backward on the fp32 table, any table size).
    warp: as in train_step_fused, on the merged prediction (warp.WarpLoss.fgbg_term).
    mono, locs: as in train_step_fused, on the merged depth d_fg + T_left d_bg (mono.MonoLoss.fgbg_term).
    bg_mode, fmesh, occlusion_mask: as in train_step_fgbg."""
    _check_mono(mono, locs)
    routes, compact = table_grad_route(FGBG_GRADIENTS, model.features.shape[1], rays_o.shape[0], [S_fg, S_bg],
                                       render.backward_arith())
    loss, _, gblob, gtab, g = _fgbg_pass(model, rays_o, rays_d, target, S_fg, S_bg, global_step, invalid_underground, timer,
                                         pose_grads, warp, routes, compact, mono, locs, bg_mode, fmesh, occlusion_mask)
    return (loss[0].detach(), gtab, gblob, *g) if pose_grads else (loss[0].detach(), gtab, gblob)


def train_step_fgbg(model, dec_opt, rays_o, rays_d, target, S_fg, S_bg, global_step, table_lr=1e-2,
                    invalid_underground=False, timer=None, pose_grads=False, dec_step=True, warp=None, mono=None, locs=None,
                    bg_mode="IZ", fmesh=None, occlusion_mask=None):
    """One complete training iteration of a tile (tile.py:880-1015: foreground + T_left * background, tile.py:639-692) on the
    fused kernels: both branches' forward, ONE loss launch pair for the merged prediction, both branches' backward emitting
    their scatter records, and ONE accumulate + sparse Adam over both record sets (the two gradients meet in one Adam step).
    Above 2^21 entries the two branches' dfeat go through ONE stand-alone scatter ending in the sparse Adam instead, and where
    neither applies through gradient tables + adam_step_cuda (table_grad_route).
    pose_grads=True (fp32 tables, t16 backward): also returns dL/d(rays_o), dL/d(rays_d) of the merged prediction -- the sum of
    the two branches' ray gradients, each formed inside its backward launch from the forward's position Jacobians
    (-> (loss, g_o, g_d)); dec_step=False: the caller steps the decoder's optimiser (it holds the camera parameters too).
    warp (warp.WarpLoss, default None): the multi-view warp term on the merged prediction, chained to both branches before their
    backward (see train_step_fused).
    mono (mono.MonoLoss, default None) with locs [B,3] int32: the monocular terms on the merged depth, after the warp term.
    bg_mode "BS" with fmesh (fastmesh.FastMesh): the background branch samples between the box exit and the mesh behind it
    (BG_MODE "BS", hashgrid/__init__.py:296-303) instead of in inverse depth; nothing else changes.  occlusion_mask [B,1] bool:
    ANDed into both branches' valid sets, as in render_rays_fused.  With the defaults the step is what it was without them."""
    _check_mono(mono, locs)
    routes, compact = table_grad_route(FGBG_STEP, model.features.shape[1], rays_o.shape[0], [S_fg, S_bg],
                                       render.backward_arith(), model._half_table is not None)
    if pose_grads and model.gather_table().dtype != torch.float32:
        raise RuntimeError("scanerf: train_step_fgbg(pose_grads=True) gathers from the fp32 table")
    loss, branches, gblob, gtab, g = _fgbg_pass(model, rays_o, rays_d, target, S_fg, S_bg, global_step, invalid_underground,
                                                timer, pose_grads, warp, routes, compact, mono, locs, bg_mode, fmesh,
                                                occlusion_mask)
    with torch.no_grad():
        if routes[0] in _TABLE_ROUTES:
            model.features.grad = gtab
            model.table_adam(table_lr)
        else:
            _table_grad_adam(model, routes[0], compact, rays_o, rays_d, branches, table_lr, timer)
        model.decoder.params.grad = gblob
        if dec_step:
            dec_opt.step()
    return (loss[0], *g) if pose_grads else loss[0]
