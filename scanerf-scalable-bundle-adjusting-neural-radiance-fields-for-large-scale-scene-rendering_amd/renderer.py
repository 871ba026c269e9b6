"""Multi-tile novel-view renderer: the build's counterpart of RenderingHashGrid's render path
(rendering.py:93-174 parse_blocks, :286-544 render_rays_base) on the HIP render-time ops, plus the
tile export / load formats it consumes (hashgrid/__init__.py:248-257 feature.npz, tile.py:516-529).

Per view: compute_ray_forward -> ray_block_intersection -> argsort(near) -> per tracing step
{sample_points -> prepare_points -> pts_inference -> accumulate_color} -> update_outgoing_bidx ->
per blended background {inverse_z_sampling -> bg_pts_inference_v2 -> accumulate_color} -> merge.
With normals=True each tracing step also runs pts_normals -> accumulate_normal (no reference counterpart: include/scanerf_hip.h).
"""
import os

import numpy as np
import torch

from . import network
from .cuda import compute_ray_forward
from .hashgrid.lib import HASHGRID as _HG
from .hashgrid import (accumulate_color, accumulate_normal, bg_pts_inference_v2, inverse_z_sampling, prepare_points,
                       process_occupied_grid, SKIP_UNSAMPLED, pts_inference, pts_inference_tracing, pts_normals, ray_block_intersection,
                       sample_points, sort_tracing_blocks, tracing_fusable, update_outgoing_bidx)


def write_feature_npz(path, features, occupied_grid, min_bbox, bbox_size, log2dim, resolution):
    """`feature.npz` as HashGrid.export writes it (hashgrid/__init__.py:248-257): fp16 table, occupancy, the 2x box, the sampler's
    log2dim, the level resolutions -- in that key order (golden G12 compares with a file written by the reference's own writer)."""
    cpu = lambda t: t.detach().cpu().numpy()
    np.savez(os.path.join(path, "feature.npz"), features=cpu(features).astype(np.float16), occupied_grid=cpu(occupied_grid),
             block_corner=cpu(min_bbox), block_size=cpu(bbox_size), grid_log2dim=cpu(log2dim), resolution=cpu(resolution))


def export_tile(path, model):
    """feature.npz (fp16 table, occupancy, 2x-box corner/size, log2dim, resolution) + decoder.pth
    (state dict with the reference's ShallowMLP key names)."""
    os.makedirs(path, exist_ok=True)
    write_feature_npz(path, model.features, model.occupied_grid, model.min_bbox, model.bbox_size, model.log2dim, model.resolution)
    torch.save({k: v.detach().cpu() for k, v in model.decoder.ref_state_dict().items()}, os.path.join(path, "decoder.pth"))


def load_tile(path):
    f = np.load(os.path.join(path, "feature.npz"))
    sd = torch.load(os.path.join(path, "decoder.pth"), map_location="cpu")
    return {"features": f["features"], "occupied_grid": f["occupied_grid"], "block_corner": f["block_corner"],
            "block_size": f["block_size"], "grid_log2dim": f["grid_log2dim"], "resolution": f["resolution"],
            "blob": network.blob_from_state_dict(sd).numpy()}


def render_box(block_corner, block_size):
    """feature.npz stores the 2x HashGrid box (hashgrid/__init__.py:50,254-255); the renderer traces the inner tile box:
    corner + size / 4, size / 2 (rendering.py:164-165)."""
    return block_corner + block_size / 4.0, block_size / 2.0


class _Rays:
    """The rays of a tracing pass, one row per ray.  Constants of the batch: rays_o, rays_d, inter (ray_block_intersection's [n,nb,2])
    and tracing_blocks (each ray's tile order).  STATE, which a pass updates in place: tracing_idx, z_start, transp, dif, spec, depth
    and normal (None unless asked for)."""
    STATE = ("tracing_idx", "z_start", "transp", "dif", "spec", "depth", "normal")
    FIELDS = ("rays_o", "rays_d", "inter", "tracing_blocks") + STATE

    def __init__(self, **fields):
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    def take(self, idx):
        """the sub-batch of the rays `idx`: every field gathered and contiguous"""
        return _Rays(**{k: t if t is None else t[idx].contiguous() for k, t in vars(self).items()})

    def put_back(self, idx, sub):
        """the state of `sub` = take(idx) written to its rows (an index listed twice receives equal values twice)"""
        for k in self.STATE:
            if getattr(self, k) is not None:
                getattr(self, k)[idx] = getattr(sub, k)


def _work_buffers(sm, n, S, normals, dev):
    """(pd, ps, pa, pn): per-sample diffuse, specular, opacity and -- with normals, else None -- normal of n rays x S samples in the
    layout sm, uninitialised (the inference ops write them)"""
    new = lambda c: torch.empty(_HG.sample_shape(sm, n, S, c), device=dev)
    return new(3), new(3), new(1), new(3) if normals else None


class TileSetRenderer:
    def __init__(self, device, tiles):
        """tiles: dicts as returned by load_tile (block_corner / block_size describe the 2x HashGrid box;
        the renderer works on the inner tile box: rendering.py:164-165)."""
        self.device = device
        # route switches (A/B timing, tests): slot lists derived inside the inference kernel (pts_inference_tracing) instead of
        # prepare_points + pts_inference; a tracing pass runs on the running rays alone when fewer than this many tenths run
        self.fuse_slots = True
        self.compact_below_tenths = 9
        self.skip_zero_transmittance_background = True   # exact: see _behind_background
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device).contiguous()
        self.feature_tables = t(np.stack([x["features"] for x in tiles]), torch.float16)
        self.params = t(np.stack([x["blob"] for x in tiles]), torch.float32)
        # the decoders' MFMA images are packed ONCE, here, and owned by this renderer (not looked up per call in a cache
        # keyed on an address the allocator may hand to the next renderer's blobs)
        from .hashgrid.lib.HASHGRID import PackedDecoders
        self.packed = PackedDecoders(self.params)
        self.resolution = t(np.stack([x["resolution"] for x in tiles]), torch.int32)
        self.grid_log2dim = t(np.stack([x["grid_log2dim"] for x in tiles]), torch.int32)
        grids = [np.asarray(x["occupied_grid"]).reshape(-1) for x in tiles]
        self.grid_starts = t(np.cumsum([0] + [g.size for g in grids[:-1]]), torch.int64)
        self.occupied_grid = t(np.concatenate(grids), torch.bool)
        corner = t(np.stack([x["block_corner"] for x in tiles]), torch.float32)
        size = t(np.stack([x["block_size"] for x in tiles]), torch.float32)
        self.block_corner, self.block_size = (x.contiguous() for x in render_box(corner, size))
        # sampling grid: each tile's occupancy dilated into the tiles it overlaps (rendering.py:168-173)
        self.fake_occupied_grid = self.occupied_grid.clone()
        for i in range(len(tiles)):
            process_occupied_grid(i, int(torch.prod(2 ** self.grid_log2dim[i]).cpu()), self.block_corner, self.block_size,
                                  self.occupied_grid, self.grid_starts, self.grid_log2dim, self.fake_occupied_grid)

    def compute_rays(self, H, W, K, c2w):
        """Pixel-centre rays of one view (rendering.py:272-284) through the HIP ray kernel."""
        dev = self.device
        j, i = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        locs = torch.stack([torch.zeros_like(i), i, j], -1).reshape(-1, 3).int().contiguous()
        o = torch.empty(H * W, 3, device=dev)
        d = torch.empty(H * W, 3, device=dev)
        compute_ray_forward(o, d, torch.as_tensor(K, dtype=torch.float32, device=dev).reshape(1, 9).contiguous(),
                            torch.as_tensor(c2w, dtype=torch.float32, device=dev)[:3, :4].reshape(1, 12).contiguous(), locs)
        return o, d

    @torch.no_grad()
    def render_rays(self, rays_o, rays_d, num_sample=128, num_bg_sample=128, sample_range=1e6, layout=2,
                    skip_saturated_background=False, normals=False):
        """-> (diffuse [B,3], specular [B,3], depth [B,1], transparency [B,1]); normals=True adds a fifth tensor, normal [B,3]: the
        tiles' density normals blended per sample as the colours are and accumulated with the foreground's transmittance (raw vector
        in world coordinates, foreground only, not normalised; the display mapping (n + 1) / 2 stays with the caller).  The four
        colour outputs are the same bits either way.
        skip_saturated_background: False (default) = the reference's behaviour, every ray gets its blended background
        (rendering.py:534-536); True = rays whose foreground transmittance is <= 1e-5 (the threshold at which rendering.py:356
        stops tracing them) get none: colour changes by <= 1e-5, but the returned DEPTH loses transparency * bg_depth, which can
        reach ~1e-5 * sample_range = 10 units (tests/test_gpu_render_time.py bounds both).
        layout of the per-sample work arrays between the ops (same ops, same arithmetic per sample; scanerf_hip.h
        `sample_major`): 0 = the reference's [B,S]; 2 (default) = [B/32,S,32]: a wave of the inference kernel holds ONE depth
        index of 32 neighbouring rays -- neighbouring pixels share their cells down to the fine levels, so the table gathers of
        a wave fall on a few lines instead of 32 per level -- and walks along those rays; 1 = [S,B] (measured slower: every
        CU on the same depth slab)."""
        n_rays = rays_o.shape[0]
        rays, sm, fused, n_hit, max_tracing = self._set_up(rays_o, rays_d, max(num_sample, num_bg_sample), layout, normals)
        B = rays.transp.shape[0]
        work = _work_buffers(sm, B, num_sample, normals, self.device)   # full size: every full-size pass reuses them
        self._trace(rays, n_hit, max_tracing, work, num_sample=num_sample, sm=sm, fused=fused)
        if num_bg_sample != num_sample:   # (else the background reuses the full-size colour buffers)
            del work
            work = _work_buffers(sm, B, num_bg_sample, False, self.device)
        out = self._behind_background(rays, work, num_bg_sample=num_bg_sample, sample_range=sample_range, sm=sm,
                                      skip_saturated=skip_saturated_background)
        return tuple(t[:n_rays] for t in out) if B != n_rays else out

    def _set_up(self, rays_o, rays_d, max_sample, layout, normals):
        """-> (rays, sm, fused, n_hit, max_tracing): the batch as _Rays in its initial state, padded to a multiple of 32 where the layout
        sm that will be used needs it; whether the inference kernel derives the slot lists (pts_inference_tracing); the number of tiles
        each ray's path meets [B,1] and the view's maximum of it."""
        dev, nb = self.device, self.block_corner.shape[0]
        sm = int(layout)
        # the single-pass comparison kernel (HASHGRID.INFER_ARITH = "f32"; also what > 64 tiles or >= 2^31 samples fall back to)
        # reads the reference's [B,S] arrays only
        single_pass = _HG.INFER_ARITH == "f32" or nb > 64 or (rays_o.shape[0] + 31) * max_sample >= 2 ** 31
        if single_pass:
            sm = 0
        if sm == 2 and rays_o.shape[0] % 32:  # pad with copies of the last ray
            pad = 32 - rays_o.shape[0] % 32
            rays_o = torch.cat([rays_o, rays_o[-1:].expand(pad, 3)]).contiguous()
            rays_d = torch.cat([rays_d, rays_d[-1:].expand(pad, 3)]).contiguous()
        B = rays_o.shape[0]
        inter = torch.full((B, nb, 2), 1e7, device=dev)
        ray_block_intersection(rays_o, rays_d, self.block_corner, self.block_size, inter)
        tracing_blocks = sort_tracing_blocks(inter)   # = torch.argsort(inter[..., 0], dim=-1, stable=True)
        max_tracing = int(torch.mean((inter != 1e7).float(), dim=-1).sum(dim=-1).max().cpu())
        zeros = lambda c, dtype=torch.float32: torch.zeros(B, c, dtype=dtype, device=dev)
        rays = _Rays(rays_o=rays_o, rays_d=rays_d, inter=inter, tracing_blocks=tracing_blocks, tracing_idx=zeros(1, torch.int32),
                     z_start=zeros(1), transp=torch.ones(B, 1, device=dev), dif=zeros(3), spec=zeros(3), depth=zeros(1),
                     normal=zeros(3) if normals else None)
        # tiles each ray's path meets (the sorted list ends at the first miss): a ray whose tracing index has reached its own count has
        # nothing left to sample -- sample_points leaves it at once (`bound.x == kInf`), so dropping it from `running` (the
        # reference's mask compares with the view's maximum, rendering.py:356) changes no value and lets the later passes run on
        # the few rays that do cross a second tile
        n_hit = (inter[..., 0] != 1e7).sum(dim=-1, keepdim=True).to(torch.int32).clamp_(max=max_tracing)
        return rays, sm, tracing_fusable(nb) and not single_pass and self.fuse_slots, n_hit, max_tracing

    def _fg_pass(self, rays, running, work, *, num_sample, sm, fused):
        """One tracing pass (rendering.py:356-420) over `rays`, whose state it updates in place.  running: [n] bool, the rays that get
        slot lists; work: _work_buffers of as many rays."""
        r, dev = rays, self.device
        pd, ps, pa, pn = work
        shape = lambda *tail: _HG.sample_shape(sm, r.transp.shape[0], num_sample, *tail)
        boxes = (self.block_corner, self.block_size)
        scene = (self.resolution, self.occupied_grid, self.grid_starts, self.grid_log2dim, *boxes)
        z = torch.full(shape(), -1.0, device=dev)
        dd = torch.full(shape(), -1.0, device=dev)
        sample_points(r.rays_o, r.rays_d, *boxes, self.fake_occupied_grid, self.grid_starts, self.grid_log2dim, r.tracing_blocks,
                      r.inter, r.tracing_idx, r.z_start, z, dd, sample_major=sm)
        if r.normal is not None or not fused:   # the normals read slot lists, on either colour route (which stays what it would have been)
            bi = torch.full(shape(4), -1, dtype=torch.int16, device=dev)
            prepare_points(z, running, r.inter, bi, sample_major=sm)
        if r.normal is not None:
            pts_normals(r.rays_o, r.rays_d, z, dd, bi, self.feature_tables, self.params, *scene, pn, sample_major=sm)
        # fused: no slot lists for the colours, the inference kernel derives them; rays that got no sample in this pass (first depth
        # -1) are neither written by it nor read by the accumulations
        flags = sm | SKIP_UNSAMPLED if fused else sm
        if fused:
            pts_inference_tracing(r.rays_o, r.rays_d, z, dd, running, r.inter, self.feature_tables, self.packed, *scene, pd, ps, pa,
                                  sample_major=flags)
        else:
            pts_inference(r.rays_o, r.rays_d, z, dd, bi, self.feature_tables, self.packed, *scene, pd, ps, pa, sample_major=sm)
        if r.normal is not None:   # (before accumulate_color, which advances the transparency both read)
            accumulate_normal(pn, pa, r.transp, z, r.normal, sample_major=flags)
        accumulate_color(pd, ps, pa, r.transp, z, r.dif, r.spec, r.depth, sample_major=flags)

    def _trace(self, rays, n_hit, max_tracing, work, *, num_sample, sm, fused):
        """The tracing loop: passes over the tiles along each ray until no ray runs.  work: the full-size _work_buffers."""
        B, how = rays.transp.shape[0], dict(num_sample=num_sample, sm=sm, fused=fused)
        for _ in range(max_tracing):
            running = ((rays.tracing_idx < n_hit) & (rays.transp > 1e-5))[:, 0].contiguous()
            n_run = int(running.sum())
            if n_run == 0:
                break
            if n_run * 10 > B * self.compact_below_tenths:   # (compaction costs ~0.1 ms of gathers)
                self._fg_pass(rays, running, work, **how)
                continue
            # Not every ray runs (rays that miss every tile; later passes: most have left the tiles or are saturated): the pass runs
            # on the running rays alone -- every op is per ray, so each running ray gets the values the full-size pass gives it; the
            # others' colours are untouched either way, and their tracing state (which the full-size pass advances) is never read
            # again: a ray that stopped stays stopped (the full-size pass costs its fills, slot lists and accumulation for every ray:
            # ~4 ms at 1920x1080 for nothing)
            idx = running.nonzero()[:, 0]
            if sm == 2 and n_run % 32:   # (the padding repeats the last running ray)
                idx = torch.cat([idx, idx[-1:].expand(32 - n_run % 32)])
            n = idx.shape[0]
            sub = rays.take(idx)
            self._fg_pass(sub, torch.ones(n, dtype=torch.bool, device=self.device),
                          _work_buffers(sm, n, num_sample, rays.normal is not None, self.device), **how)
            rays.put_back(idx, sub)

    def _behind_background(self, rays, work, *, num_bg_sample, sample_range, sm, skip_saturated):
        """The blended backgrounds of each ray's exit tile(s) (rendering.py:421-536), composed behind the traced foreground
        -> render_rays' outputs for the whole (padded) batch.  work: _work_buffers of B rays x num_bg_sample samples."""
        r, dev, B = rays, self.device, rays.transp.shape[0]
        pd, ps, pa, _ = work
        zeros = lambda c: torch.zeros(B, c, device=dev)
        bg_b = torch.full((B, 4), -1, dtype=torch.int16, device=dev)
        bg_w = zeros(4)
        update_outgoing_bidx(r.rays_o, r.rays_d, self.block_corner, self.block_size, r.tracing_blocks, r.inter, bg_b, bg_w, 0.12, False)
        bg_w = bg_w / torch.sum(bg_w, dim=-1, keepdim=True)
        # rays whose foreground transmittance is EXACTLY zero (an opacity rounded to 1.0 on the way: hard surfaces) get no background:
        # it would be multiplied by that zero -- `dif + 0 * bgd` is `dif` bit for bit, colour and depth alike -- so nothing changes
        # but the decoder work of their 128 background samples (exact, unlike skip_saturated_background below)
        if self.skip_zero_transmittance_background:
            bg_b[(r.transp == 0)[:, 0]] = -1
        if skip_saturated:
            # rays the foreground has saturated get no background: it would enter the pixel with weight <= 1e-5 -- 400x below
            # one 8-bit step -- and on an opaque scene it is most of the frame's decoder work
            bg_b[(r.transp <= 1e-5)[:, 0]] = -1
        n_blend = int((bg_w > 0).sum(dim=-1).max().cpu())
        bgd, bgs, bgz = zeros(3), zeros(3), zeros(1)
        for i in range(n_blend):
            zb = torch.full(_HG.sample_shape(sm, B, num_bg_sample), -1.0, device=dev)
            inverse_z_sampling(r.inter, bg_b[:, i].contiguous(), zb, sample_range, sample_major=sm)
            # (bg_pts_inference_v2 writes every sample: zeros where the ray has no background tile at this blend step)
            bg_pts_inference_v2(r.rays_o, r.rays_d, zb, bg_b, i, self.block_corner, self.block_size, self.resolution,
                                self.feature_tables, self.packed, pd, ps, pa, sample_major=sm)
            t1, td, ts, tz = torch.ones(B, 1, device=dev), zeros(3), zeros(3), zeros(1)
            accumulate_color(pd, ps, pa, t1, zb, td, ts, tz, sample_major=sm)
            w = torch.nan_to_num(bg_w[:, i:i + 1])  # rays with no exit tile: 0/0 in the reference's normalisation
            bgd += td * w
            bgs += ts * w
            bgz += tz * w
        out = (r.dif + r.transp * bgd, r.spec + r.transp * bgs, r.depth + r.transp * bgz, r.transp)
        return out if r.normal is None else out + (r.normal,)

    def render(self, H, W, K, c2w, **kw):
        """One view -> (diffuse [H,W,3], specular [H,W,3], depth [H,W,1], transparency [H,W,1]), and with normals=True the normal map
        [H,W,3] (render_rays)."""
        o, d = self.compute_rays(H, W, K, c2w)
        dif, spec, depth, transp, *nm = self.render_rays(o, d, **kw)
        return (dif.reshape(H, W, 3), spec.reshape(H, W, 3), depth.reshape(H, W, 1), transp.reshape(H, W, 1),
                *(x.reshape(H, W, 3) for x in nm))

    def scene_box(self):
        """(corner, size), 3 floats each: the bounding box of the tiles' render boxes."""
        lo = self.block_corner.min(0).values.cpu().numpy().astype(np.float32)
        hi = (self.block_corner + self.block_size).max(0).values.cpu().numpy().astype(np.float32)
        return lo.tolist(), (hi - lo).tolist()

    @torch.no_grad()
    def extract_mesh(self, level, cells_per_axis=256, box=None, route="fused", normals=False, min_faces=0, min_extent=0,
                     keep_largest=None, report=None, cameras=None, min_views=0, view_bias=None, view_far=None, simplify=None,
                     colors=None, color_scale=1, **color_kw):
        """ONE mesh of the whole scene: the level set sigma == level of the density this renderer draws, the tiles' densities blended
        per point with the render-time weights (meshing.extract_scene_mesh).  box = (corner, size) of the world box
        the lattice covers (default: scene_box()), with cells_per_axis cells along its longest side.  normals=True: the vertex normals,
        the blended density's own gradient (meshing.scene_sigma_normals_points).  min_faces / min_extent /
        keep_largest: meshing.filter_mesh's keep rule (floaters and unused vertices go), applied before the normals
        are evaluated; report: a dict that receives the component count and the rows before and after.  cameras = (ks, c2ws, H, W)
        with min_views >= 1: the parts no camera saw go first (meshing.cull_unseen; view_bias: half a lattice spacing
        by default).  simplify=cell: meshing.simplify_mesh as the last step.  -> meshing.Mesh.
        colors="diffuse" | "rgb" (needs cameras): the FINAL vertices -- after the cull, the filter and simplify --
        are coloured by color_mesh from this scene's renders at the cameras (H // color_scale x W // color_scale; color_kw goes to
        color_mesh).  -> (mesh, rgb [V,3] f32), the mesh the one of the call without colours.  None: the Mesh alone, as before."""
        from . import meshing
        if colors not in (None, "diffuse", "rgb"):
            raise RuntimeError(f"scanerf: colors must be None, 'diffuse' or 'rgb', got {colors!r}")
        if colors is None and (color_kw or color_scale != 1):
            raise RuntimeError(f"scanerf: extract_mesh: {sorted(color_kw) or 'color_scale'} only mean something with colors=")
        if colors is not None and (cameras is None or len(cameras) != 4):
            raise RuntimeError("scanerf: extract_mesh(colors=...) needs cameras=(ks, c2ws, H, W)")
        corner, size = self.scene_box() if box is None else box
        size = [float(v) for v in size]
        paint = None
        if colors is not None:
            paint = lambda mesh, bias: self.color_mesh(mesh, cameras, which=colors, scale=color_scale, bias=bias,
                                                       **dict({"far": float("inf") if view_far is None else float(view_far)}, **color_kw))[0]
            return meshing.extract_scene_mesh(self.feature_tables, self.resolution, self.params, self.block_corner, self.block_size,
                                              self.occupied_grid, self.grid_starts, self.grid_log2dim, corner, size,
                                              meshing.cells_per_axis(size, cells_per_axis), level, route=route, normals=normals,
                                              min_faces=min_faces, min_extent=min_extent, keep_largest=keep_largest, report=report,
                                              cameras=cameras, min_views=min_views, view_bias=view_bias, view_far=view_far,
                                              simplify=simplify, colors=paint)
        return meshing.extract_scene_mesh(self.feature_tables, self.resolution, self.params, self.block_corner, self.block_size,
                                          self.occupied_grid, self.grid_starts, self.grid_log2dim, corner, size,
                                          meshing.cells_per_axis(size, cells_per_axis), level, route=route, normals=normals,
                                          min_faces=min_faces, min_extent=min_extent, keep_largest=keep_largest, report=report,
                                          cameras=cameras, min_views=min_views, view_bias=view_bias, view_far=view_far, simplify=simplify)

    @torch.no_grad()
    def evaluate_mesh(self, gt, level, cells_per_axis=256, n_samples=200000, thresholds=(0.05,), max_dist=float("inf"), seed=0,
                      log2dim=6, return_distances=False, normals=False, **extract):
        """The geometric score of this scene's mesh against `gt` ((vertices, faces) or a PLY path, e.g. the dataset's scan):
        extract_mesh(level, cells_per_axis, **extract) -- box, route and the filter rules min_faces / min_extent / keep_largest
        included -- then evaluation.compare_meshes(extracted, gt, ...).  -> its dict (pred = the extracted mesh).
        normals=True adds compare_meshes' "normal_consistency" (face normals of both meshes; it is not passed to the extraction)."""
        from . import evaluation
        evaluation._flag(normals, "normals")
        mesh = self.extract_mesh(level, cells_per_axis, **extract)
        return evaluation.compare_meshes((mesh.vertices, mesh.faces), gt, n_samples, thresholds, max_dist=max_dist, seed=seed,
                                         log2dim=log2dim, return_distances=return_distances, device=mesh.vertices.device,
                                         normals=normals)

    @torch.no_grad()
    def color_mesh(self, mesh, cameras, which="diffuse", scale=1, max_transparency=0.5, views_per_batch=8, min_cos=0.0, bias=None,
                   normals="mesh", far=float("inf"), fill=(0.5, 0.5, 0.5), log2dim=6, route="fused", report=None, **render_kw):
        """Vertex colours for any mesh of this scene from the field's own renders: cameras = (ks, c2ws, H, W) are
        rendered exactly as fuse_mesh / score_mesh render them (H // scale x W // scale, K scaled, render_kw to render;
        which="diffuse": clamp(diffuse), "rgb": clamp(diffuse + specular)), views_per_batch at a time, and each batch is projected
        onto the vertices while it is held (meshing.ViewColors: the mesh occludes itself, bilinear samples, cosine weights with the
        mesh's normals).  mesh: a meshing.Mesh or anything with .vertices / .faces on this device.  bias: how far towards the eye a
        segment starts, so that a vertex's own faces do not hide it: None takes half the mean edge length (meshing.default_edge_bias);
        extract_mesh passes the extractors' view_bias (half a lattice spacing by default).  far: the cameras' range.
        -> (rgb [V,3] f32, valid [V] bool); report receives count_histogram and invalid."""
        from . import fusion, meshing
        if which not in ("diffuse", "rgb"):
            raise RuntimeError(f"scanerf: which must be 'diffuse' or 'rgb', got {which!r}")
        if cameras is None or len(cameras) != 4:
            raise RuntimeError("scanerf: color_mesh needs cameras=(ks, c2ws, H, W)")
        ks, c2ws, H, W = cameras
        scale = fusion._positive_int(scale, "scale")
        vpb = fusion._views_per_batch(views_per_batch)
        H, W = fusion._positive_int(H, "H"), fusion._positive_int(W, "W")
        h, w = H // scale, W // scale
        if h < 1 or w < 1:
            raise RuntimeError(f"scanerf: H={H} W={W} leave no pixel at scale={scale}")
        if not 0.0 <= float(max_transparency) <= 1.0:
            raise RuntimeError(f"scanerf: max_transparency must lie in [0, 1], got {max_transparency!r}")
        ks = fusion.scale_cameras(ks, scale)
        c2ws = torch.as_tensor(c2ws).to(torch.float32)
        if c2ws.dim() != 3 or c2ws.shape[0] != ks.shape[0] or c2ws.shape[1] < 3 or c2ws.shape[2] != 4:
            raise RuntimeError(f"scanerf: c2ws must be [C,3,4] (or [C,4,4]) with C={ks.shape[0]}, got {tuple(c2ws.shape)}")
        if bias is None:
            bias = meshing.default_edge_bias(mesh)
        blend = meshing.ViewColors(mesh, float(bias), normals, 0.0, far, min_cos, fill, log2dim, route)
        if not blend.empty:
            for i, _, images, _ in self._scene_batches(ks, c2ws, h, w, vpb, which, float(max_transparency), render_kw):
                blend.add(images, ks[i:i + vpb], c2ws[i:i + vpb])
        return blend.result(report)

    def _scene_batches(self, ks, c2ws, h, w, vpb, colors, max_transparency, render_kw, normals=False):
        """The scene rendered at cameras ks / c2ws (already scaled) at h x w, vpb at a time -> an iterator of (first index, depth maps
        [B,h,w] masked by fusion.mask_depth, images [B,h,w,3] (fusion.clamped_image; None without colors), normal maps [B,h,w,3] or
        None): what fuse_mesh integrates and score_mesh compares with."""
        from . import fusion
        kw = dict(render_kw, normals=True) if normals else render_kw
        for i in range(0, int(ks.shape[0]), vpb):
            maps, images, nmaps = [], [], []
            for c in range(i, min(i + vpb, int(ks.shape[0]))):
                diffuse, specular, depth, transp, *nm = self.render(h, w, ks[c], c2ws[c], **kw)
                maps.append(fusion.mask_depth(depth[..., 0], transp[..., 0], max_transparency))
                if colors is not None:
                    images.append(fusion.clamped_image(diffuse, specular if colors == "rgb" else None))
                if normals:
                    nmaps.append(nm[0])
            yield (i, torch.stack(maps).contiguous(), torch.stack(images).contiguous() if colors is not None else None,
                   torch.stack(nmaps).contiguous() if normals else None)

    @torch.no_grad()
    def score_mesh(self, mesh, cameras, colors=None, which="diffuse", scale=1, max_transparency=0.5, views_per_batch=8, normals=False,
                   log2dim=6, max_depth_diff=None, **render_kw):
        """Does the mesh, seen from the capture's cameras, look like what the field renders there?  cameras = (ks,
        c2ws, H, W); every camera is rendered exactly as fuse_mesh renders it (H // scale x W // scale, K scaled, the depth masked at
        max_transparency, render_kw to render) and the mesh -- (vertices, faces), a PLY path or a meshing.Mesh -- is rendered at the same
        cameras (evaluation.render_mesh), views_per_batch at a time.  colors: the mesh's vertex colours [V,3] in 0..1 (fuse_mesh's
        second return): compared with the scene's clamp(diffuse) (which="diffuse") or clamp(diffuse + specular) ("rgb").
        normals=True: the mesh's normal map (its vertex normals, or its face normals) against the scene's.
        -> evaluation.compare_renders' dict (pred = the mesh, target = the scene)."""
        from . import evaluation, fusion
        if which not in ("diffuse", "rgb"):
            raise RuntimeError(f"scanerf: which must be 'diffuse' or 'rgb', got {which!r}")
        if not isinstance(normals, bool):
            raise RuntimeError(f"scanerf: normals must be True or False, got {normals!r}")
        if cameras is None or len(cameras) != 4:
            raise RuntimeError("scanerf: score_mesh needs cameras=(ks, c2ws, H, W)")
        ks, c2ws, H, W = cameras
        scale = fusion._positive_int(scale, "scale")
        vpb = fusion._views_per_batch(views_per_batch)
        H, W = fusion._positive_int(H, "H"), fusion._positive_int(W, "W")
        h, w = H // scale, W // scale
        if h < 1 or w < 1:
            raise RuntimeError(f"scanerf: H={H} W={W} leave no pixel at scale={scale}")
        if not 0.0 <= float(max_transparency) <= 1.0:
            raise RuntimeError(f"scanerf: max_transparency must lie in [0, 1], got {max_transparency!r}")
        ks = fusion.scale_cameras(ks, scale)
        c2ws = torch.as_tensor(c2ws).to(torch.float32)
        if c2ws.dim() != 3 or c2ws.shape[0] != ks.shape[0] or c2ws.shape[1] < 3 or c2ws.shape[2] != 4:
            raise RuntimeError(f"scanerf: c2ws must be [C,3,4] (or [C,4,4]) with C={ks.shape[0]}, got {tuple(c2ws.shape)}")
        acc = evaluation.RenderScore(max_depth_diff)
        preds = evaluation.render_mesh(mesh, (ks, c2ws, h, w), colors=colors, normals=normals, log2dim=log2dim, views_per_batch=vpb,
                                       device=self.device)
        scene = self._scene_batches(ks, c2ws, h, w, vpb, which if colors is not None else None, float(max_transparency), render_kw,
                                    normals=normals)
        for (i, pred), (j, maps, images, nmaps) in zip(preds, scene):
            target = {"depth": maps}
            if images is not None:
                target["color"] = images
            if nmaps is not None:
                target["normal"] = nmaps
            acc.add(pred, target)
        return acc.result()

    @torch.no_grad()
    def fuse_mesh(self, cameras, cells_per_axis=256, box=None, trunc=None, max_transparency=0.5, scale=1, views_per_batch=8,
                  min_weight=1, min_faces=0, min_extent=0, keep_largest=None, report=None, colors=None, normals=False, simplify=None,
                  score=False, **render_kw):
        """ONE mesh of what the cameras saw (fusion.py): cameras = (ks [C,3,3], c2ws [C,3,4], H, W), typically the
        capture's.  Each camera is rendered at H // scale x W // scale (K scaled as fusion.scale_cameras does; render_kw goes to
        render), its depth set to 0 where the transparency exceeds max_transparency or the depth is not finite (fusion.mask_depth),
        and the maps are fused views_per_batch at a time (never more of them are held) into a TSDF volume over box = (corner, size)
        (default: scene_box()) with cells_per_axis cells along its longest side; trunc: 4 x the largest spacing by default.  Then
        TSDFVolume.extract: the zero set, the support cull, filter_mesh's rules.  -> meshing.Mesh (no normals).
        colors: "diffuse" also fuses clamp(diffuse, 0, 1) of the same renders (the view-independent part: the
        sensible colour of a mesh), "rgb" clamp(diffuse + specular, 0, 1) (the image shown everywhere else), batched with the depth
        maps; -> (mesh, rgb [V,3] f32), the mesh the one of the call without colours.  None: no colour, the Mesh alone.
        normals=True: the Mesh carries the volume's gradient normals (TSDFVolume.vertex_normals).
        simplify=cell: TSDFVolume.extract's last step, meshing.simplify_mesh on the world grid of that cell.
        score=True (needs a `report` dict): the finished mesh is rendered at the same cameras, with the fused colours
        when there are any, and compared with the renders it was fused from (evaluation.compare_renders, views_per_batch at a time);
        the dict goes to report["render_score"].  The scene is rendered once: the masked depth maps and images of all cameras are
        kept until then.  What is returned does not change."""
        from . import fusion, meshing
        meshing._simplify_rule(simplify)
        if not isinstance(score, bool):
            raise RuntimeError(f"scanerf: score must be True or False, got {score!r}")
        if score and not isinstance(report, dict):
            raise RuntimeError("scanerf: fuse_mesh(score=True) writes report['render_score']: pass report={}")
        if not isinstance(normals, bool):
            raise RuntimeError(f"scanerf: normals must be True or False, got {normals!r}")
        if colors not in (None, "diffuse", "rgb"):
            raise RuntimeError(f"scanerf: colors must be None, 'diffuse' or 'rgb', got {colors!r}")
        if cameras is None or len(cameras) != 4:
            raise RuntimeError("scanerf: fuse_mesh needs cameras=(ks, c2ws, H, W)")
        ks, c2ws, H, W = cameras
        scale = fusion._positive_int(scale, "scale")
        vpb = fusion._views_per_batch(views_per_batch)
        H, W = fusion._positive_int(H, "H"), fusion._positive_int(W, "W")
        h, w = H // scale, W // scale
        if h < 1 or w < 1:
            raise RuntimeError(f"scanerf: H={H} W={W} leave no pixel at scale={scale}")
        if not 0.0 <= float(max_transparency) <= 1.0:
            raise RuntimeError(f"scanerf: max_transparency must lie in [0, 1], got {max_transparency!r}")
        fusion._min_weight(min_weight)
        meshing._rules(min_faces, min_extent, keep_largest, True)
        ks = fusion.scale_cameras(ks, scale)
        c2ws = torch.as_tensor(c2ws).to(torch.float32)
        if c2ws.dim() != 3 or c2ws.shape[0] != ks.shape[0] or c2ws.shape[1] < 3 or c2ws.shape[2] != 4:
            raise RuntimeError(f"scanerf: c2ws must be [C,3,4] (or [C,4,4]) with C={ks.shape[0]}, got {tuple(c2ws.shape)}")
        corner, size = self.scene_box() if box is None else box
        size = [float(v) for v in size]
        n = meshing.cells_per_axis(size, cells_per_axis)
        spacing = fusion.lattice_spacing(size, n)
        vol = fusion.TSDFVolume([float(v) for v in corner], spacing, n, fusion.default_trunc(spacing) if trunc is None else trunc,
                                self.device, color=colors is not None)
        kept = []
        for i, maps, images, _ in self._scene_batches(ks, c2ws, h, w, vpb, colors, float(max_transparency), render_kw):
            vol.integrate(maps, ks[i:i + vpb], c2ws[i:i + vpb], colors=images)
            if score:
                kept.append((i, maps, images))
        if score:
            from . import evaluation
            out = vol.extract(min_weight, min_faces, min_extent, keep_largest, report, colors=colors is not None, normals=normals,
                              simplify=simplify)
            mesh, rgb = out if colors is not None else (out, None)
            acc = evaluation.RenderScore()
            if mesh.faces.shape[0]:
                batches = evaluation.render_mesh(mesh, (ks, c2ws, h, w), colors=rgb, normals=False, views_per_batch=vpb)
                for (i, pred), (j, maps, images) in zip(batches, kept):
                    acc.add(pred, {"depth": maps} if images is None else {"depth": maps, "color": images})
            report["render_score"] = acc.result()
            return out
        return vol.extract(min_weight, min_faces, min_extent, keep_largest, report, colors=colors is not None, normals=normals,
                           simplify=simplify)
