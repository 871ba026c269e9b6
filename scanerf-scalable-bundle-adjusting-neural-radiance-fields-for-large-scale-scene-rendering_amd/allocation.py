"""Tile allocation from mesh depth: the reference's preprocess/build_tiles.py, which turns a mesh and a camera log into
tiles/tile_info.txt and tiles/training_views.txt -- the two files every training entry point starts from.

  tile_grid        candidate tile corners over the mesh bounds                       build_tiles.py:98-114
  view_coverage    per (tile, camera) the number of quarter-resolution pixels whose ray enters the tile before it meets the
                   mesh: ONE fused launch of csrc/coverage.hip for all cameras       build_tiles.py:129-156 (a loop over cameras:
                   torch rays, a [B,K,2] bounds tensor, a depth pass, a reduction)
  coverage_ratio   counts -> the reference's occupied ratio                          build_tiles.py:155
  select_tiles     which tiles stay and which views train each                       build_tiles.py:160-222
  allocate_tiles   the three above on a mesh
  write_allocation the two files, through formats                                    build_tiles.py:203-237
  read_ignore_log  DATADIR/ignore.log                                                build_tiles.py:78-91
The debug dumps (camera.obj, tiles.obj) are not written.  view_coverage has no CPU path: CPU tensors raise.
"""
import os

import numpy as np
import torch

from . import formats
from ._capi import check, dev_ptr, lib, stream
from .fastmesh import FastMesh, _require_gpu

_f32, _i32, _i64 = torch.float32, torch.int32, torch.int64


def boxes_per_pass():
    """Boxes the coverage kernel counts per pass over a chunk of pixels (its on-chip capacity); larger K takes several passes."""
    return int(lib().scanerf_view_coverage_boxes_per_pass())


def _cameras(ks, c2ws, device=None):
    """-> Ks [C,9], C2Ws [C,12] float32, contiguous (on `device` when given)."""
    ks, c2ws = torch.as_tensor(ks), torch.as_tensor(c2ws)
    if device is not None:
        ks, c2ws = ks.to(device), c2ws.to(device)
    if ks.dim() != 3 or tuple(ks.shape[1:]) != (3, 3):
        raise RuntimeError(f"scanerf: ks must be [C,3,3], got {tuple(ks.shape)}")
    if c2ws.dim() != 3 or c2ws.shape[0] != ks.shape[0] or c2ws.shape[1] < 3 or c2ws.shape[2] != 4:
        raise RuntimeError(f"scanerf: c2ws must be [C,3,4] (or [C,4,4]) with C={ks.shape[0]}, got {tuple(c2ws.shape)}")
    return ks.to(_f32).reshape(-1, 9).contiguous(), c2ws[:, :3, :].to(_f32).reshape(-1, 12).contiguous()


def view_coverage(fmesh, ks, c2ws, H, W, box_centers, box_sizes, scale=4):
    """counts int32 [K, C]: for box k (centre, FULL side lengths) and camera c, the pixels of the H // scale x W // scale
    frame whose ray meets the box with near_k < depth.  Rays: the reference's get_rays_torch_v2 on K / scale (no pixel-centre
    offset, directions not normalised); depth: fmesh.first_hit, 0 (sky) -> 1e5; near: ray_aabb_intersection_v2's.  One launch
    for all cameras; integer counts, bit-reproducible.  GPU only."""
    for t, name in ((ks, "ks"), (c2ws, "c2ws"), (box_centers, "box_centers"), (box_sizes, "box_sizes")):
        _require_gpu(t, name)
    k9, c12 = _cameras(ks, c2ws)
    centers = box_centers.detach().to(_f32).reshape(-1, 3).contiguous()
    sizes = box_sizes.detach().to(_f32).expand_as(centers).contiguous()
    C, K = k9.shape[0], centers.shape[0]
    counts = torch.zeros(K, C, dtype=_i32, device=k9.device)
    pre = fmesh.tris is not None
    check(lib().scanerf_view_coverage(
        dev_ptr(k9, _f32, "ks"), dev_ptr(c12, _f32, "c2ws"), C, int(H), int(W), int(scale), dev_ptr(centers, _f32, "box_centers"),
        dev_ptr(sizes, _f32, "box_sizes"), K, dev_ptr(fmesh.vertices, _f32, "vertices"), dev_ptr(fmesh.faces, _i32, "faces"),
        dev_ptr(fmesh.tris, _f32, "tris") if pre else None, dev_ptr(fmesh.bitmask, _i64, "bitmask"),
        dev_ptr(fmesh.rank, _i32, "rank"), dev_ptr(fmesh.start_num, _i32, "start_num"),
        dev_ptr(fmesh.cell_faces, _i32, "cell_faces"), dev_ptr(fmesh.scene_info, _f32, "scene_info"), fmesh.log2dim,
        dev_ptr(counts, _i32, "counts"), stream()), "view_coverage")
    return counts


def coverage_ratio(counts, H, W, scale):
    """The reference's occupied ratio, its quirk kept: the FULL-resolution denominator H * W goes with the count over the
    truncated (H // scale) x (W // scale) frame (build_tiles.py:155)."""
    return counts.float() / (H * W) * (scale ** 2)


def tile_grid(scene_bound, tile_size, overlap_ratio, offset, max_dim_tile):
    """scene_bound [6] (min corner, max corner) -> corners [K,3] float32 of the candidate tiles and their number per axis.
    The grid starts at min + offset; per axis min(ceil((max - (min + offset)) / tile_size), max_dim_tile) tiles, stepping
    (1 - overlap_ratio) * tile_size; tile k = (x, y, z) with z fastest."""
    bound = torch.as_tensor(scene_bound, dtype=_f32).cpu().reshape(6)
    size = torch.as_tensor(tile_size, dtype=_f32).cpu().reshape(3)
    mn = bound[:3] + torch.as_tensor(offset, dtype=_f32).cpu().reshape(3)
    side = torch.ceil((bound[3:] - mn) / size).int()
    side = [min(int(side[a]), int(max_dim_tile[a])) for a in range(3)]
    xs, ys, zs = torch.meshgrid(torch.arange(side[0]), torch.arange(side[1]), torch.arange(side[2]), indexing="ij")
    grid = torch.stack([xs, ys, zs], -1).reshape(-1, 3)
    return mn + grid * (1 - overlap_ratio) * size, side


def select_tiles(related, camera_centers, corners, tile_size, expect_num, min_num_image, scene_type, ignore=(), thresh=0.1):
    """Which candidate tiles stay and which views train each (build_tiles.py:160-222).

    related [K,C]: coverage ratios; camera_centers [C,3]; corners [K,3]; tile_size [3].
      * camera c is inside tile k when 0 <= (cam - corner) / size < 1 on every axis; tiles with no camera inside are set aside;
      * with fewer than expect_num tiles left, the set-aside tiles of smallest mean camera-to-centre distance are added; with
        more, the expect_num tiles of smallest such distance are kept; the kept ids are sorted;
      * score = related for scene_type "indoor", thresh * inside + related otherwise; ignored cameras score 0;
      * a tile's views are the cameras with score > thresh in descending score; a tile stays only with strictly more than
        min_num_image views; the tiles that stay are renumbered 0, 1, 2, ...
    Ties (the reference's torch.sort and argsort leave their order open) are broken by a STABLE sort: among equal scores the
    lower camera index comes first, among equal distances the lower tile id.
    -> {"tiles": candidate ids kept, "views": per kept tile the camera ids, "corners": [n,3] float32 of the kept tiles}."""
    related = torch.as_tensor(related).detach().to("cpu", _f32).clone()
    cams = torch.as_tensor(camera_centers).detach().to("cpu", _f32).reshape(-1, 3)
    corners = torch.as_tensor(corners).detach().to("cpu", _f32).reshape(-1, 3)
    size = torch.as_tensor(tile_size, dtype=_f32).cpu().reshape(3)
    if tuple(related.shape) != (corners.shape[0], cams.shape[0]):
        raise RuntimeError(f"scanerf: related must be [K,C] = [{corners.shape[0]},{cams.shape[0]}], got {tuple(related.shape)}")
    distance = torch.norm(cams[None] - (corners[:, None] + size / 2.0), dim=-1).mean(-1)
    cam_loc = (cams[None] - corners[:, None]) / size
    inside = torch.all((cam_loc >= 0) & (cam_loc < 1), dim=-1)
    aside = [k for k in range(corners.shape[0]) if not bool(inside[k].any())]
    valid = [k for k in range(corners.shape[0]) if k not in aside]
    nearest = lambda ids: [ids[i] for i in torch.argsort(distance[ids], descending=False, stable=True).tolist()]
    if len(valid) < expect_num:
        valid = valid + nearest(aside)[:expect_num - len(valid)]
    elif len(valid) > expect_num:
        valid = nearest(valid)[:expect_num]
    valid.sort()
    score = related if scene_type == "indoor" else thresh * inside + related
    ignore = [int(i) for i in ignore]
    if ignore:
        score[:, ignore] = 0
    scores, images = torch.sort(score, dim=1, descending=True, stable=True)
    tiles, views = [], []
    for k in valid:
        chosen = images[k][scores[k] > thresh].tolist()
        if len(chosen) > min_num_image:
            tiles.append(k)
            views.append(chosen)
    return {"tiles": tiles, "views": views, "corners": corners[tiles]}


def allocate_tiles(mesh, ks, c2ws, H, W, tile_size, overlap_ratio=0.2, offset=(0.0, 0.0, 0.0), expect_num=1, min_num_image=60,
                   max_dim_tile=(100000, 100000, 100000), scene_type="outdoor", ignore=(), scale=4, thresh=0.1, device=None):
    """mesh: a PLY path or a FastMesh; ks [C,3,3], c2ws [C,3,4] (arrays or tensors, any device); the keyword arguments are the
    reference's ALLOCATION keys (TILE_SIZE, OVERLAP_RATIO, OFFSET, EXPECT_NUM, MIN_NUM_IMAGE, MAX_DIM_TILE, SCENE_TYPE).
    -> select_tiles' result plus "tile_size" [3], "scene_type", "all_corners" [K,3], "counts" [K,C] int32 and "related" [K,C]."""
    fmesh = mesh if isinstance(mesh, FastMesh) else FastMesh(mesh, device=device)
    dev = fmesh.device
    size = torch.as_tensor(tile_size, dtype=_f32).cpu().reshape(3)
    corners, _ = tile_grid(fmesh.get_sceneinfo().cpu(), size, overlap_ratio, offset, max_dim_tile)
    ks, c2ws = torch.as_tensor(ks), torch.as_tensor(c2ws)
    centers = (corners + size / 2.0).to(dev)
    counts = view_coverage(fmesh, ks.to(dev), c2ws.to(dev), H, W, centers, size.to(dev)[None, :], scale).cpu()
    related = coverage_ratio(counts, H, W, scale)
    result = select_tiles(related, c2ws[:, :3, 3], corners, size, expect_num, min_num_image, scene_type, ignore, thresh)
    result.update(tile_size=size, scene_type=scene_type, all_corners=corners, counts=counts, related=related)
    return result


def write_allocation(tile_dir, result):
    """tile_dir/tile_info.txt and tile_dir/training_views.txt as the reference writes them: resolution pair 32 8192 for
    "outdoor" scenes and 32 4096 otherwise, flag 0."""
    os.makedirs(tile_dir, exist_ok=True)
    finest = 8192 if result["scene_type"] == "outdoor" else 4096
    formats.write_tile_info(os.path.join(tile_dir, "tile_info.txt"), np.asarray(result["corners"], np.float64).reshape(-1, 3),
                            np.asarray(result["tile_size"], np.float64), (32, finest))
    formats.write_training_views(os.path.join(tile_dir, "training_views.txt"), result["views"])


def read_ignore_log(path):
    """Camera ids to leave out of every tile's views; a missing file is no ids.  One id per line, or `first last` for the
    half-open range first .. last - 1; any other line is skipped (build_tiles.py:78-91)."""
    if not os.path.exists(path):
        return []
    ignore = []
    with open(path, "r") as f:
        for line in f:
            tok = line.strip().split(" ")
            if len(tok) == 1 and tok[0]:
                ignore.append(int(tok[0]))
            elif len(tok) == 2:
                ignore += list(range(int(tok[0]), int(tok[1])))
    return ignore
