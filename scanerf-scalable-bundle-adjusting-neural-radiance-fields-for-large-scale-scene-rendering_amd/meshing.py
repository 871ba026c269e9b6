"""Level-set mesh extraction (csrc/isosurface.hip): surface nets over a tile's density, or over a caller's value
lattice.  The reference has no mesh extraction; the definition is the comment of include/scanerf_hip.h.

    surface_nets(values, level, origin, spacing)        the dense op on a value array [nx+1, ny+1, nz+1]
    extract_mesh(features, ..., n, level)               the tile's density level set; route="fused" never stores the lattice,
                                                        route="dense" composes lattice points -> render.sigma_normals_points ->
                                                        liveness -> the dense op (the witness, and fine for small lattices)
    extract_scene_mesh(tables, ..., box, n, level)      ONE mesh of a tiled scene: the level set of the tiles' densities blended with
                                                        the multi-tile renderer's weights on a lattice over a world box
    scene_sigma_normals_points(points, tables, ...)     that blended density, its gradient (weight terms included) and the normal at
                                                        world points: the scene mesh's vertex normals
    mesh_components(faces, n_vertices, cells)           connected components: labels and the per-component table (csrc/mesh_components.hip;
                                                        DESIGN.md 4.17)
    filter_mesh(mesh, min_faces, min_extent, keep_largest)   drop floaters and unused vertices by component; the extractors take the
                                                        same three rules and filter before they evaluate normals
    vertex_views(mesh, ks, c2ws, H, W, bias)            how many cameras see each vertex, the mesh itself occluding (csrc/mesh_visibility.hip;
                                                        DESIGN.md 4.19)
    cull_unseen(mesh, ks, c2ws, H, W, min_views, bias)  drop the faces none of whose vertices min_views cameras saw; the extractors take
                                                        cameras / min_views / view_bias and cull before the component rule
    simplify_mesh(mesh, cell, origin, colors)           vertex clustering on a world grid: positions, normals and colours averaged per cell
                                                        (csrc/mesh_simplify.hip); the scene extractors take simplify=cell
    color_from_views(mesh, images, ks, c2ws, bias)      vertex colours for any mesh from posed images: project, sample, blend
                                                        (csrc/mesh_colors.hip); extract_scene_mesh takes colors=callable

All return a Mesh: vertices [V,3] f32 (world), faces [F,3] i32 (counter-clockwise seen from the outside), cells [V,3] i32 (the owning
cell of each vertex), lattice [V,3] f32 (the vertices in lattice coordinates) and, on request, normals [V,3] f32.  Two launches with
one host read of (V, F) between them; no CPU path."""
import collections
import ctypes

import numpy as np
import torch

from . import render
from ._capi import check, dev_ptr, lib, stream

Mesh = collections.namedtuple("Mesh", "vertices faces cells lattice normals")
ROUTES = ("fused", "dense")
_f32 = torch.float32


def _lattice_size(n):
    n = [int(v) for v in n]
    if len(n) != 3:
        raise RuntimeError(f"scanerf: n must hold 3 cell counts, got {n}")
    return n


def _scratch(device, n):
    nbytes = int(lib().scanerf_isosurface_scratch_bytes(*n))
    if nbytes == 0:
        raise RuntimeError(f"scanerf: lattice n={tuple(n)} is not supported (every n_k >= 1, fewer than 2^31 cells and points): "
                           + lib().scanerf_last_error().decode("utf-8", "replace"))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _totals(scratch):
    """The one host read: (V, F) as the count pass left them."""
    V, F = (int(v) for v in scratch[:16].view(torch.int64).tolist())
    if V >= 2 ** 31 // 3 or F >= 2 ** 31 // 3:
        raise RuntimeError(f"scanerf: the mesh has V={V} vertices and F={F} faces: too many for int32 indices")
    return V, F


def _outputs(device, V, F):
    return (torch.empty((V, 3), dtype=_f32, device=device), torch.empty((F, 3), dtype=torch.int32, device=device),
            torch.empty((V, 3), dtype=torch.int32, device=device), torch.empty((V, 3), dtype=_f32, device=device))


def _fused(device, n, count, emit, head, box=()):
    """The sequence every fused route runs: scratch, the count pass `count`, the one host read of (V, F), the outputs, the emit pass
    `emit` unless the mesh is empty.  count / emit: the exports' names behind "scanerf_"; head: the arguments both start with;
    box: what the emit pass takes behind them (the world placement, where the head does not hold it already).  -> Mesh."""
    scratch, nbytes = _scratch(device, n)
    check(getattr(lib(), "scanerf_" + count)(*head, scratch.data_ptr(), nbytes, stream()), count)
    V, F = _totals(scratch)
    vertices, faces, cells, lattice = _outputs(device, V, F)
    if V:
        check(getattr(lib(), "scanerf_" + emit)(*head, *box, scratch.data_ptr(), nbytes, vertices.data_ptr(), faces.data_ptr(),
                                                cells.data_ptr(), lattice.data_ptr(), V, F, stream()), emit)
    return Mesh(vertices, faces, cells, lattice, None)


def _host3(v, name):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    return render._host3(v, name)


def _f32_div(a, b):
    """a / b as one float32 division (what the kernels' host side forms), as a Python float."""
    return float(np.float32(a) / np.float32(b))


def surface_nets(values, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """The dense op: values [nx+1, ny+1, nz+1] f32 on the GPU, inside = values > level (level > 0), vertex = origin + L * spacing."""
    if not isinstance(values, torch.Tensor) or values.dim() != 3:
        raise RuntimeError("scanerf: values must be a [nx+1, ny+1, nz+1] tensor")
    p = dev_ptr(values, _f32, "values")
    n = [int(s) - 1 for s in values.shape]
    o, sp = _host3(origin, "origin"), _host3(spacing, "spacing")
    return _fused(values.device, n, "isosurface_count_dense", "isosurface_emit_dense", (p, *n, float(level)), (o, sp))


def lattice_positions(n, device):
    """Contracted positions [(nx+1)(ny+1)(nz+1), 3] of the lattice points, x fastest last: x = float(i) * (2 / n) - 1, two roundings."""
    axes = [torch.arange(n[k] + 1, device=device, dtype=_f32) * _f32_div(2.0, n[k]) - 1.0 for k in range(3)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).contiguous()


def live_points(n, occupied_grid):
    """[nx+1, ny+1, nz+1] bool: the lattice points that lie in the closed extent of an occupied sampler cell -- point i lies in cell c of
    an axis iff c n <= i G <= (c + 1) n, in integers."""
    occ = occupied_grid.to(_f32)
    for k in range(3):
        G = int(occupied_grid.shape[k])
        iG = torch.arange(n[k] + 1, device=occ.device, dtype=torch.int64)[:, None] * G
        c = torch.arange(G, device=occ.device, dtype=torch.int64)[None, :]
        member = ((c * n[k] <= iG) & (iG <= (c + 1) * n[k])).to(_f32)      # [n_k + 1, G_k]
        occ = torch.movedim(torch.tensordot(member, torch.movedim(occ, k, 0), dims=1), 0, k)
    return occ > 0


def _contracted(lattice, n):
    h = [_f32_div(2.0, n[k]) for k in range(3)]
    return (lattice * torch.tensor(h, dtype=_f32, device=lattice.device) - 1.0).contiguous()


def extract_mesh(features, resolutions, blob, weight_feature, occupied_grid, log2dim, occ_corner, occ_size, n, level, normals=False,
                 route="fused", min_faces=0, min_extent=0, keep_largest=None, report=None, cameras=None, min_views=0, view_bias=None,
                 view_far=None):
    """The level set sigma == level of a tile's density as a triangle mesh.  features [16,T,2] f32 / f16, resolutions [16,3], blob (the
    flat decoder blob), weight_feature [32], occupied_grid bool [2^log2dim], occ_corner / occ_size: the tile box (3 floats each),
    n: cells per axis of the lattice over it.  normals=True adds render.sigma_normals_points' normals at the vertices
    (axis_scale = 4 / (2 occ_size)).  min_faces / min_extent / keep_largest: filter_mesh's keep rule, applied BEFORE the normals are
    evaluated (they are computed at the kept vertices only); the defaults keep everything.  report: a dict that receives the
    component count and the rows before and after the filter.  cameras = (ks, c2ws, H, W) with min_views >= 1: cull_unseen on the raw
    mesh, BEFORE the component rule (so min_faces removes what the cull fragments); view_bias: half a lattice spacing by default;
    view_far: the cameras' range (None: no limit); report["cull"] receives cull_unseen's report."""
    if route not in ROUTES:
        raise RuntimeError(f"scanerf: route must be one of {ROUTES}, got {route!r}")
    _rules(min_faces, min_extent, keep_largest, True)
    _view_rule(cameras, min_views, view_bias, view_far)
    n = _lattice_size(n)
    T, mid = render._normals_common(features, resolutions, blob, weight_feature)
    occ = dev_ptr(occupied_grid, (torch.bool, torch.uint8), "occupied_grid")
    log2dim = [int(v) for v in (log2dim.tolist() if isinstance(log2dim, torch.Tensor) else log2dim)]
    if len(log2dim) != 3 or tuple(occupied_grid.shape) != tuple(2 ** k for k in log2dim):
        raise RuntimeError(f"scanerf: occupied_grid {tuple(occupied_grid.shape)} does not match log2dim {log2dim}")
    corner, size = _host3(occ_corner, "occ_corner"), _host3(occ_size, "occ_size")
    if not all(s > 0 for s in size):
        raise RuntimeError(f"scanerf: occ_size must be positive, got {list(size)}")
    if not float(level) > 0:
        raise RuntimeError(f"scanerf: level={level} must be > 0")
    device = features.device
    if route == "dense":
        sigma, _, _ = render.sigma_normals_points(lattice_positions(n, device), features, resolutions, blob, weight_feature)
        values = torch.where(live_points(n, occupied_grid).reshape(-1), sigma, torch.zeros_like(sigma)).reshape(n[0] + 1, n[1] + 1, n[2] + 1)
        step = [_f32_div(size[k], n[k]) for k in range(3)]
        mesh = surface_nets(values.contiguous(), level, list(corner), step)
    else:
        l2d = (ctypes.c_int32 * 3)(*log2dim)
        head = (*mid, T, occ, l2d, int(occupied_grid.numel()), *n, float(level))
        mesh = _fused(device, n, "isosurface_count", "isosurface_emit", head, (corner, size))
    mesh = _cull_extracted(mesh, cameras, min_views, view_bias, view_far, size, n, route, report)
    mesh = _filter(mesh, min_faces, min_extent, keep_largest, _COMPONENT_ROUTE[route], False, report)
    if normals:
        if mesh.vertices.shape[0]:
            _, _, nrm = render.sigma_normals_points(_contracted(mesh.lattice, n), features, resolutions, blob, weight_feature,
                                                    axis_scale=[_f32_div(4.0, 2.0 * s) for s in size])
        else:
            nrm = torch.empty((0, 3), dtype=_f32, device=device)
        mesh = mesh._replace(normals=nrm)
    return mesh


# ---- one mesh of a tiled scene: the level set of the tiles' blended density -----------------------------------
def _scene_field_dense(feature_tables, resolutions, blobs, corners, sizes, occupied_grid, grid_starts, log2dim, corner, size, n):
    """The witness of the fused scene route: the definition of include/scanerf_hip.h op by op.  World positions, membership, weights,
    cells and occupancy in numpy float32 on the host (IEEE by construction; every quantity but the weight is a product of per-axis
    terms), sigma_b from render.sigma_normals_points at the contributing points of each tile, the blend in ascending tile index.
    -> values [nx+1, ny+1, nz+1] f32 (numpy)."""
    f32 = np.float32
    device = feature_tables.device
    host = lambda t, dt: np.ascontiguousarray(t.detach().cpu().numpy()).astype(dt)
    cn, sz, occ = host(corners, f32), host(sizes, f32), host(occupied_grid, bool).reshape(-1)
    starts, l2d = host(grid_starts, np.int64), host(log2dim, np.int64)
    wp = [f32(corner[k]) + np.arange(n[k] + 1, dtype=f32) * (f32(size[k]) / f32(n[k])) for k in range(3)]
    assert all(a.dtype == f32 for a in wp)
    shape = tuple(m + 1 for m in n)
    num, W = np.zeros(shape, f32), np.zeros(shape, f32)
    ones = torch.ones(32, dtype=_f32, device=device)
    for b in range(cn.shape[0]):
        pt = [(wp[k] - cn[b, k]) / sz[b, k] for k in range(3)]
        inb = [(p >= 0) & (p <= 1) for p in pt]
        listed = inb[0][:, None, None] & inb[1][None, :, None] & inb[2][None, None, :]
        if not listed.any():
            continue
        dis = [(f32(0.5) - np.abs(p - f32(0.5))) * sz[b, k] for k, p in enumerate(pt)]
        dx, dz = dis[0][:, None], dis[2][None, :]
        w2 = np.where((dx != 0) & (dz != 0), dx * dz, np.where(dx != 0, dx, np.where(dz != 0, dz, f32(0)))).astype(f32)   # xz_weight
        w = np.broadcast_to(w2[:, None, :], shape)
        W = np.where(listed, W + w, W).astype(f32)
        loc = []
        for k in range(3):
            r = 1 << int(l2d[b, k])
            with np.errstate(invalid="ignore", over="ignore"):
                cc = (pt[k] * f32(r)).astype(f32)
            loc.append(np.clip(np.where(np.isfinite(cc), cc, 0).astype(np.int64), 0, r - 1))    # C (int): truncation, then the clamp
        off = (loc[0][:, None, None] << int(l2d[b, 1] + l2d[b, 2])) | (loc[1][None, :, None] << int(l2d[b, 2])) | loc[2][None, None, :]
        run = listed & occ[starts[b] + off]
        if not run.any():
            continue
        idx = np.argwhere(run)
        x = np.stack([(f32(2.0) * pt[k] - f32(1.0))[idx[:, k]] for k in range(3)], 1).astype(f32)
        sigma, _, _ = render.sigma_normals_points(torch.from_numpy(x).to(device), feature_tables[b], resolutions[b], blobs[b], ones)
        prod = (w[run] * sigma.cpu().numpy()).astype(f32)
        num[run] = num[run] + prod
    inv = np.where(W > 0, f32(1.0) / np.where(W > 0, W, f32(1.0)), f32(1.0)).astype(f32)
    return (num * inv).astype(f32)


def _scene_tile_args(feature_tables, resolutions, blobs, corners, sizes, occupied_grid, grid_starts, log2dim):
    """The checks of the tile arrays that every scene op makes, before any launch -> (the eight tile pointers of the exports:
    tables, blobs, resolution, occ, grid_starts, log2dim, corners, sizes; T; nb)."""
    tabs = dev_ptr(feature_tables, torch.float16, "feature_tables")
    if feature_tables.dim() != 4 or feature_tables.shape[1] != 16 or feature_tables.shape[3] != 2:
        raise RuntimeError(f"scanerf: feature_tables must be [nb,16,T,2], got {tuple(feature_tables.shape)}")
    nb, T = int(feature_tables.shape[0]), int(feature_tables.shape[2])
    if nb < 1:
        raise RuntimeError("scanerf: a scene mesh needs at least one tile")
    if T < 2 or T & (T - 1):
        raise RuntimeError(f"scanerf: the table size T={T} must be a power of two")
    from . import _capi
    ptrs = []
    for t, dt, name, shape in ((blobs, _f32, "blobs", (nb, _capi.PARAMSIZE)), (resolutions, torch.int32, "resolutions", (nb, 16, 3)),
                               (occupied_grid, (torch.bool, torch.uint8), "occupied_grid", None), (grid_starts, torch.int64, "grid_starts", (nb,)),
                               (log2dim, torch.int32, "log2dim", (nb, 3)), (corners, _f32, "corners", (nb, 3)), (sizes, _f32, "sizes", (nb, 3))):
        ptrs.append(dev_ptr(t, dt, name))
        if shape is not None and tuple(t.shape) != shape:
            raise RuntimeError(f"scanerf: {name} must be {list(shape)}, got {list(t.shape)}")
    return (tabs, *ptrs), T, nb


def extract_scene_mesh(feature_tables, resolutions, blobs, corners, sizes, occupied_grid, grid_starts, log2dim, box_corner, box_size, n,
                       level, route="fused", normals=False, min_faces=0, min_extent=0, keep_largest=None, report=None, cameras=None,
                       min_views=0, view_bias=None, view_far=None, simplify=None, colors=None):
    """One mesh of a tiled scene: the level set of the field the multi-tile renderer draws -- the tiles' densities blended per lattice
    point with the renderer's xz-distance weights -- on a lattice of n cells over the world box box_corner / box_size (the definition:
    include/scanerf_hip.h, scanerf_isosurface_count_tiles).  The tile arrays are TileSetRenderer's: feature_tables [nb,16,T,2] f16,
    resolutions [nb,16,3] i32, blobs [nb,13994], corners / sizes [nb,3] (render boxes), occupied_grid (the tiles' own grids,
    concatenated), grid_starts [nb] i64, log2dim [nb,3] i32.  -> Mesh; normals=True adds scene_sigma_normals_points' normals at the
    vertices (the gradient of the blended field itself), otherwise normals is None.  route="fused" never stores the
    lattice; route="dense" composes host geometry -> render.sigma_normals_points per tile -> blend -> surface_nets (the witness).
    min_faces / min_extent / keep_largest: filter_mesh's keep rule, applied BEFORE the normals are evaluated; the
    defaults keep everything.  report: a dict that receives the component count and the rows before and after the filter.
    cameras = (ks, c2ws, H, W) with min_views >= 1: cull_unseen on the raw mesh, BEFORE the component rule;
    view_bias: half a lattice spacing by default; view_far: the cameras' range (None: no limit).
    simplify=cell: simplify_mesh on the world grid of that cell as the LAST step, after the filter and the normals;
    the Mesh then has no cells / lattice; report["simplify"] receives its rows.
    colors=callable: called as colors(mesh, bias) on the FINAL mesh -- after the cull, the filter and simplify --
    with bias = view_bias or its default; it returns the vertex colours [V,3] (TileSetRenderer.extract_mesh passes its color_mesh:
    the scene's renders projected onto the vertices).  -> (Mesh, rgb).  None: the Mesh alone, exactly as without the argument."""
    _simplify_rule(simplify)
    if route not in ROUTES:
        raise RuntimeError(f"scanerf: route must be one of {ROUTES}, got {route!r}")
    _rules(min_faces, min_extent, keep_largest, True)
    _view_rule(cameras, min_views, view_bias, view_far)
    if colors is not None and not callable(colors):
        raise RuntimeError(f"scanerf: extract_scene_mesh colors must be None or a callable (mesh, bias) -> [V,3], got {colors!r}")
    n = _lattice_size(n)
    tiles = (feature_tables, resolutions, blobs, corners, sizes, occupied_grid, grid_starts, log2dim)
    head, T, nb = _scene_tile_args(*tiles)
    corner, size = _host3(box_corner, "box_corner"), _host3(box_size, "box_size")
    if not all(0 < s < float("inf") for s in size):
        raise RuntimeError(f"scanerf: box_size must be positive, got {list(size)}")
    if not float(level) > 0:
        raise RuntimeError(f"scanerf: level={level} must be > 0")
    device = feature_tables.device
    if route == "dense":
        values = _scene_field_dense(*tiles, corner, size, n)
        step = [_f32_div(size[k], n[k]) for k in range(3)]
        mesh = surface_nets(torch.from_numpy(values).to(device).contiguous(), level, list(corner), step)
    else:
        mesh = _fused(device, n, "isosurface_count_tiles", "isosurface_emit_tiles", (*head, T, nb, corner, size, *n, float(level)))
    mesh = _cull_extracted(mesh, cameras, min_views, view_bias, view_far, size, n, route, report)
    mesh = _filter(mesh, min_faces, min_extent, keep_largest, _COMPONENT_ROUTE[route], False, report)
    if normals:
        mesh = mesh._replace(normals=scene_sigma_normals_points(mesh.vertices, *tiles, route=route)[2])
    mesh = _simplified(mesh, simplify, None, report, _SIMPLIFY_ROUTE[route])
    if colors is None:
        return mesh
    return mesh, colors(mesh, default_view_bias(size, n) if view_bias is None else float(view_bias))


# ---- the blended density's gradient at world points (csrc/scene_normals.hip) -----------------------------------------
def _scene_normals_dense(points, feature_tables, resolutions, blobs, corners, sizes, occupied_grid, grid_starts, log2dim):
    """The witness of the fused op: the definition of include/scanerf_hip.h (scanerf_scene_sigma_normals_points) op by op.  Position,
    membership, weight, weight gradient, cell and occupancy in numpy float32 on the host, (sigma_b, grad sigma_b) from
    render.sigma_normals_points at the contributing points of each tile, the sums in numpy float32 in the definition's order.
    -> (sigma [N], grad [N,3], normal [N,3]) numpy f32."""
    f32 = np.float32
    device = feature_tables.device
    host = lambda t, dt: np.ascontiguousarray(t.detach().cpu().numpy()).astype(dt)
    p = host(points, f32)
    cn, sz, occ = host(corners, f32), host(sizes, f32), host(occupied_grid, bool).reshape(-1)
    starts, l2d = host(grid_starts, np.int64), host(log2dim, np.int64)
    N = p.shape[0]
    W, num = np.zeros(N, f32), np.zeros(N, f32)
    A, B, C = np.zeros((N, 3), f32), np.zeros((N, 3), f32), np.zeros((N, 3), f32)
    contributed = np.zeros(N, bool)
    ones = torch.ones(32, dtype=_f32, device=device)
    half, zero = f32(0.5), f32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(cn.shape[0]):
            pt = ((p - cn[b]) / sz[b]).astype(f32)
            listed = ((pt >= 0) & (pt <= 1)).all(1)
            if not listed.any():
                continue
            dis = ((half - np.abs(pt - half)) * sz[b]).astype(f32)
            dx, dz = dis[:, 0], dis[:, 2]
            side = np.where(pt < half, f32(1), np.where(pt > half, f32(-1), zero)).astype(f32)
            both, only_x, only_z = (dx != 0) & (dz != 0), (dx != 0) & ~(dz != 0), ~(dx != 0) & (dz != 0)
            w = np.where(both, dx * dz, np.where(only_x, dx, np.where(only_z, dz, zero))).astype(f32)             # xz_weight
            gw = np.zeros((N, 3), f32)
            gw[:, 0] = np.where(both, side[:, 0] * dz, np.where(only_x, side[:, 0], zero))
            gw[:, 2] = np.where(both, side[:, 2] * dx, np.where(only_z, side[:, 2], zero))
            W = np.where(listed, W + w, W).astype(f32)
            C = np.where(listed[:, None], C + gw, C).astype(f32)
            r = (1 << l2d[b]).astype(np.int64)
            cc = (pt * r.astype(f32)).astype(f32)
            loc = np.clip(np.where(np.isfinite(cc), cc, 0).astype(np.int64), 0, r - 1)                              # C (int), then the clamp
            off = (loc[:, 0] << int(l2d[b, 1] + l2d[b, 2])) | (loc[:, 1] << int(l2d[b, 2])) | loc[:, 2]
            run = listed & occ[starts[b] + off]
            if not run.any():
                continue
            x = (f32(2.0) * pt[run] - f32(1.0)).astype(f32)
            sigma, grad, _ = render.sigma_normals_points(torch.from_numpy(np.ascontiguousarray(x)).to(device), feature_tables[b],
                                                         resolutions[b], blobs[b], ones,
                                                         axis_scale=[_f32_div(2.0, sz[b, k]) for k in range(3)], want_grad=True)
            sigma, grad = sigma.cpu().numpy(), grad.cpu().numpy()
            num[run] = num[run] + (w[run] * sigma).astype(f32)
            A[run] = A[run] + (w[run, None] * grad).astype(f32)
            B[run] = B[run] + (sigma[:, None] * gw[run]).astype(f32)
            contributed |= run
        inv = np.where(W > 0, f32(1.0) / np.where(W > 0, W, f32(1.0)), f32(1.0)).astype(f32)
        v = (num * inv).astype(f32)
        g = (((A + B) - v[:, None] * C) * inv[:, None]).astype(f32)
        q = g * g
        nrm = (g * (f32(-1.0) / (np.sqrt((q[:, 0] + q[:, 1]) + q[:, 2]) + f32(1e-8)))[:, None]).astype(f32)
    keep = contributed
    return (np.where(keep, v, zero).astype(f32), np.where(keep[:, None], g, zero).astype(f32),
            np.where(keep[:, None], nrm, zero).astype(f32))


def scene_sigma_normals_points(points, feature_tables, resolutions, blobs, corners, sizes, occupied_grid, grid_starts, log2dim,
                               want_grad=False, route="fused"):
    """The blended density of a tiled scene, its gradient and the normal at world points [N,3] f32 (any order; the definition:
    include/scanerf_hip.h, scanerf_scene_sigma_normals_points): the field extract_scene_mesh cuts, v = sum_b w_b sigma_b / W, and the
    gradient of exactly that function, the blend weights' gradients included.  The tile arrays are extract_scene_mesh's.
    -> (sigma [N], grad [N,3] or None, normal [N,3] = -grad / (|grad| + 1e-8)); zeros where no tile contributes.  route="fused": one
    launch, no per-tile index arrays; route="dense": host geometry -> render.sigma_normals_points per tile -> the sums (the witness)."""
    if route not in ROUTES:
        raise RuntimeError(f"scanerf: route must be one of {ROUTES}, got {route!r}")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("scanerf: points must be a [N,3] tensor")
    tiles = (feature_tables, resolutions, blobs, corners, sizes, occupied_grid, grid_starts, log2dim)
    head, T, nb = _scene_tile_args(*tiles)
    p = dev_ptr(points, _f32, "points")
    device, N = points.device, int(points.shape[0])
    if N == 0:   # (an empty tensor has no address to hand over)
        empty = torch.empty((0, 3), dtype=_f32, device=device)
        return torch.empty((0,), dtype=_f32, device=device), (empty.clone() if want_grad else None), empty
    if route == "dense":
        sigma, grad, normal = (torch.from_numpy(a).to(device) for a in _scene_normals_dense(points, *tiles))
        return sigma, (grad if want_grad else None), normal
    sigma = torch.empty((N,), dtype=_f32, device=device)
    normal = torch.empty((N, 3), dtype=_f32, device=device)
    grad = torch.empty((N, 3), dtype=_f32, device=device) if want_grad else None
    check(lib().scanerf_scene_sigma_normals_points(p, *head, T, nb, sigma.data_ptr(), grad.data_ptr() if want_grad else None,
                                                   normal.data_ptr(), N, stream()), "scene_sigma_normals_points")
    return sigma, grad, normal


# ---- connected components and the filter by component (csrc/mesh_components.hip) -----------------------------------
Components = collections.namedtuple("Components", "labels label n_vertices n_faces cell_min cell_max")
COMPONENT_ROUTES = ("fused", "composed")
_COMPONENT_ROUTE = {"fused": "fused", "dense": "composed"}      # the extractors' witness route composes the filter too
_i32 = torch.int32


def _rules(min_faces, min_extent, keep_largest, have_cells):
    """The keep rule's values, checked -> (min_faces, min_extent, keep_largest or None, any rule active?)."""
    for name, v in (("min_faces", min_faces), ("min_extent", min_extent), ("keep_largest", keep_largest)):
        if v is None and name == "keep_largest":
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise RuntimeError(f"scanerf: {name} must be a non-negative integer, got {v!r}")
    if min_extent > 0 and not have_cells:
        raise RuntimeError("scanerf: min_extent needs the vertices' cells (Mesh.cells); there are none")
    active = min_faces > 0 or min_extent > 0 or keep_largest is not None
    return int(min_faces), int(min_extent), None if keep_largest is None else int(keep_largest), active


def _component_args(faces, n_vertices, cells, route, check_range):
    """The checks every component op makes before any launch -> (V, F).  check_range: the public functions' one device reduction
    with one host read for the face indices; the extractors' own outputs skip it."""
    if route not in COMPONENT_ROUTES:
        raise RuntimeError(f"scanerf: route must be one of {COMPONENT_ROUTES}, got {route!r}")
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, (int, np.integer)) or not 0 <= n_vertices < 2 ** 31 // 3:
        raise RuntimeError(f"scanerf: n_vertices must be an integer in [0, 2^31 / 3), got {n_vertices!r}")
    V = int(n_vertices)
    dev_ptr(faces, _i32, "faces")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f"scanerf: faces must be [F,3], got {tuple(faces.shape)}")
    F = int(faces.shape[0])
    if F >= 2 ** 31 // 3:
        raise RuntimeError(f"scanerf: F={F} faces are too many for int32 indices")
    if cells is not None:
        dev_ptr(cells, _i32, "cells")
        if tuple(cells.shape) != (V, 3) or cells.device != faces.device:
            raise RuntimeError(f"scanerf: cells must be [{V},3] on {faces.device}, got {tuple(cells.shape)} on {cells.device}")
    if F and V == 0:
        raise RuntimeError(f"scanerf: {F} faces with no vertices")
    if check_range and F:
        lo, hi = torch.stack(torch.aminmax(faces)).tolist()
        if lo < 0 or hi >= V:
            raise RuntimeError(f"scanerf: face indices run from {lo} to {hi}, outside [0, {V})")
    return V, F


def _labels_composed(faces, V):
    """The witness: rounds of scatter_reduce(amin) over the edges (both directions) plus labels = labels[labels], to a fixed point
    (one host read per round).  An edge (s, d) lowers the label of d's LABEL to s's label (hooking the tree, not the vertex: a chain
    takes a few dozen rounds, not its length); the jump carries it to the vertices.  A label only decreases, names a vertex of its
    own component and is <= every vertex that carries it.  At the fixed point lab[lab] == lab and lab[lab[d]] <= lab[s] for both
    directions of every edge, so a label is constant over every edge: it is the component's smallest index.  -> labels [V] int64."""
    lab = torch.arange(V, dtype=torch.int64, device=faces.device)
    if faces.shape[0] == 0:
        return lab
    f = faces.to(torch.int64)
    src, dst = f[:, [0, 1, 0, 2, 1, 2]].reshape(-1), f[:, [1, 0, 2, 0, 2, 1]].reshape(-1)
    while True:
        new = lab.scatter_reduce(0, lab[dst], lab[src], "amin", include_self=True)
        new = new[new]
        if torch.equal(new, lab):
            return lab
        lab = new


def _table_composed(faces, cells, lab):
    """The table by bincount / scatter_reduce, rows in ascending label order -> (label, n_vertices, n_faces, cell_min, cell_max)."""
    V = lab.shape[0]
    roots = torch.nonzero(lab == torch.arange(V, dtype=torch.int64, device=lab.device)).reshape(-1)
    nv = torch.bincount(lab, minlength=V)[roots]
    nf = torch.bincount(lab[faces[:, 0].to(torch.int64)], minlength=V)[roots] if faces.shape[0] else torch.zeros_like(nv)
    cmin = cmax = None
    if cells is not None:
        idx = lab[:, None].expand(V, 3)
        big = torch.iinfo(torch.int32)
        cmin = torch.full((V, 3), big.max, dtype=_i32, device=lab.device).scatter_reduce(0, idx, cells, "amin")[roots]
        cmax = torch.full((V, 3), big.min, dtype=_i32, device=lab.device).scatter_reduce(0, idx, cells, "amax")[roots]
    return roots.to(_i32), nv.to(_i32), nf.to(_i32), cmin, cmax


def _components_scratch(device, V, F):
    nbytes = int(lib().scanerf_mesh_components_scratch_bytes(V, F))
    if nbytes == 0:
        raise RuntimeError(f"scanerf: a mesh of V={V} vertices and F={F} faces is not supported: "
                           + lib().scanerf_last_error().decode("utf-8", "replace"))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _components(faces, V, F, cells, route):
    """-> (Components with the table in rank order, order [C] i64: the library's row (ascending label) of every rank, state: the
    fused route's (scratch, nbytes) for the filter or None).  V >= 1."""
    device = faces.device
    if route == "composed":
        lab = _labels_composed(faces, V)
        rows, state = _table_composed(faces, cells, lab), None
        labels = lab.to(_i32)
    else:
        scratch, nbytes = _components_scratch(device, V, F)
        labels = torch.empty((V,), dtype=_i32, device=device)
        check(lib().scanerf_mesh_components_label(faces.data_ptr(), V, F, labels.data_ptr(), scratch.data_ptr(), nbytes, stream()),
              "mesh_components_label")
        C = int(scratch[:8].view(torch.int64).item())      # the one host read: the number of components
        new = lambda *shape: torch.empty(shape, dtype=_i32, device=device)
        rows = (new(C), new(C), new(C), new(C, 3) if cells is not None else None, new(C, 3) if cells is not None else None)
        ptr = lambda t: None if t is None else t.data_ptr()
        check(lib().scanerf_mesh_components_table(faces.data_ptr(), ptr(cells), labels.data_ptr(), V, F, scratch.data_ptr(), nbytes, C,
                                                  *(ptr(t) for t in rows), stream()), "mesh_components_table")
        state = (scratch, nbytes)
    label, nf = rows[0], rows[2]
    # rank: n_faces descending, ties by label ascending -- one int64 key per row (labels are distinct: no two keys are equal)
    order = torch.argsort(((2 ** 31 - 1 - nf.to(torch.int64)) << 32) | label.to(torch.int64))
    return Components(labels, *(None if t is None else t[order].contiguous() for t in rows)), order, state


def _empty_components(device, with_cells):
    e = lambda *shape: torch.empty(shape, dtype=_i32, device=device)
    return Components(e(0), e(0), e(0), e(0), e(0, 3) if with_cells else None, e(0, 3) if with_cells else None)


def mesh_components(faces, n_vertices, cells=None, route="fused"):
    """The connected components of a mesh (the definition: include/scanerf_hip.h, scanerf_mesh_components_label): faces [F,3] i32
    over n_vertices vertices, optionally their cells [V,3] i32 (Mesh.cells).  -> Components(labels [V] i32: the smallest vertex index
    of each vertex's component; label, n_vertices, n_faces [C] i32 and, with cells, cell_min, cell_max [C,3] i32: one row per
    component, ordered by n_faces descending, ties by label ascending -- the row number is the component's rank).  route="fused":
    a lock-free union-find and aggregated integer sums on the GPU, one host read (C); route="composed": torch label propagation,
    bincount and scatter_reduce (the witness; a host read per round).  Both give the same bits."""
    V, F = _component_args(faces, n_vertices, cells, route, True)
    if V == 0:
        return _empty_components(faces.device, cells is not None)
    return _components(faces, V, F, cells, route)[0]


def _keep_ranked(comps, min_faces, min_extent, keep_largest):
    """The keep rule on the table in rank order -> [C] bool."""
    keep = comps.n_faces >= min_faces
    if min_extent > 0:
        keep &= (comps.cell_max - comps.cell_min + 1).max(1).values >= min_extent
    if keep_largest is not None:
        keep &= torch.arange(keep.shape[0], device=keep.device) < keep_largest
    return keep


def _filter(mesh, min_faces, min_extent, keep_largest, route, check_range, report=None):
    """filter_mesh behind its checks of the rule.  report: a dict that receives the component count and the rows before and after."""
    arrays = {"vertices": (mesh.vertices, _f32), "cells": (mesh.cells, _i32), "lattice": (mesh.lattice, _f32), "normals": (mesh.normals, _f32)}
    if not isinstance(mesh.vertices, torch.Tensor) or mesh.vertices.dim() != 2 or mesh.vertices.shape[1] != 3:
        raise RuntimeError("scanerf: mesh.vertices must be a [V,3] tensor")
    Vn = int(mesh.vertices.shape[0])
    for name, (t, dt) in arrays.items():
        if t is None and name != "vertices":
            continue
        dev_ptr(t, dt, name)
        if tuple(t.shape) != (Vn, 3) or t.device != mesh.vertices.device:
            raise RuntimeError(f"scanerf: mesh.{name} must be [{Vn},3] on {mesh.vertices.device}, got {tuple(t.shape)} on {t.device}")
    min_faces, min_extent, keep_largest, active = _rules(min_faces, min_extent, keep_largest, mesh.cells is not None)
    V, F = _component_args(mesh.faces, Vn, mesh.cells, route, check_range and (active or report is not None))
    if mesh.faces.device != mesh.vertices.device:
        raise RuntimeError(f"scanerf: mesh.faces lives on {mesh.faces.device}, the vertices on {mesh.vertices.device}")
    if report is not None:
        report.update(components=0, kept_components=0, vertices=(V, V), faces=(F, F))
    if V == 0 or not (active or report is not None):
        return mesh
    comps, order, state = _components(mesh.faces, V, F, mesh.cells, route)
    C = int(comps.label.shape[0])
    if report is not None:
        report.update(components=C, kept_components=C)
    if not active:
        return mesh            # the default rule keeps everything: the input, bit for bit
    device = mesh.vertices.device
    ranked = _keep_ranked(comps, min_faces, min_extent, keep_largest)
    present = [(k, t) for k, (t, _) in arrays.items() if t is not None]
    if route == "composed":
        kept = torch.zeros(V, dtype=torch.bool, device=device)
        kept[comps.label[ranked].to(torch.int64)] = True
        kv = kept[comps.labels.to(torch.int64)]
        kf = kv[mesh.faces[:, 0].to(torch.int64)] if F else torch.zeros(0, dtype=torch.bool, device=device)
        new_index = torch.cumsum(kv, 0) - 1
        out = {k: t[kv].contiguous() for k, t in present}
        out["faces"] = new_index[mesh.faces[kf].to(torch.int64)].to(_i32).reshape(-1, 3).contiguous()
    else:
        scratch, nbytes = state
        keep = torch.empty(C, dtype=torch.uint8, device=device)
        keep[order] = ranked.to(torch.uint8)       # the library's row order: ascending label
        head = (mesh.faces.data_ptr(), comps.labels.data_ptr(), keep.data_ptr(), V, F, C, scratch.data_ptr(), nbytes)
        check(lib().scanerf_mesh_filter_count(*head, stream()), "mesh_filter_count")
        Vk, Fk = (int(v) for v in scratch[8:24].view(torch.int64).tolist())      # the one host read: (V', F')
        out = {k: torch.empty((Vk, 3), dtype=t.dtype, device=device) for k, t in present}
        out["faces"] = torch.empty((Fk, 3), dtype=_i32, device=device)
        if Vk:
            src = {k: None for k in arrays}
            src.update({k: t.data_ptr() for k, t in present})
            dst = {k: (out[k].data_ptr() if k in out else None) for k in arrays}
            check(lib().scanerf_mesh_filter_emit(*head, src["vertices"], src["cells"], src["lattice"], src["normals"], dst["vertices"],
                                                 out["faces"].data_ptr() if Fk else None, dst["cells"], dst["lattice"], dst["normals"],
                                                 Vk, Fk, stream()), "mesh_filter_emit")
    if report is not None:
        report.update(kept_components=int(ranked.sum()), vertices=(V, int(out["vertices"].shape[0])), faces=(F, int(out["faces"].shape[0])))
    return Mesh(out["vertices"], out["faces"], out.get("cells"), out.get("lattice"), out.get("normals"))


def filter_mesh(mesh, min_faces=0, min_extent=0, keep_largest=None, route="fused"):
    """Drop components of a Mesh (floaters, unused vertices) by the keep rule of include/scanerf_hip.h: a component stays iff
    n_faces >= min_faces and extent >= min_extent (extent: the largest side of its box of cells, in cells) and (keep_largest is None
    or rank < keep_largest), the rank by n_faces descending, ties by label ascending.  The defaults keep everything and return the
    input.  min_faces=1 alone removes exactly the vertices no face uses.  Kept vertices and faces stay in their order, the faces'
    indices are remapped, cells / lattice / normals (where the mesh has them) are gathered row for row.  -> Mesh."""
    return _filter(mesh, min_faces, min_extent, keep_largest, route, True)


# ---- which cameras see the mesh, and the cull by it (csrc/mesh_visibility.hip) ---------------------------------------
VIEW_ROUTES = ("fused", "composed")
_VIEW_ROUTE = {"fused": "fused", "dense": "composed"}      # the extractors' witness route composes the visibility too


def _min_views(min_views):
    if isinstance(min_views, bool) or not isinstance(min_views, (int, np.integer)) or min_views < 0:
        raise RuntimeError(f"scanerf: min_views must be a non-negative integer, got {min_views!r}")
    return int(min_views)


def _view_rule(cameras, min_views, view_bias, view_far):
    """The extractors' view arguments, checked before any launch."""
    if _min_views(min_views) > 0 and (cameras is None or len(cameras) != 4):
        raise RuntimeError("scanerf: min_views >= 1 needs cameras=(ks, c2ws, H, W)")
    if view_bias is not None and not 0.0 < float(view_bias) < float("inf"):
        raise RuntimeError(f"scanerf: view_bias must be > 0 and finite, got {view_bias!r}")
    if view_far is not None and not float(view_far) > 0.0:
        raise RuntimeError(f"scanerf: view_far must be > 0, got {view_far!r}")


def default_view_bias(size, n):
    """Half a lattice spacing (the smallest axis): a surface-nets vertex lies within its cell, its faces within one spacing of it."""
    return 0.5 * min(_f32_div(size[k], n[k]) for k in range(3))


def _cull_extracted(mesh, cameras, min_views, view_bias, view_far, size, n, route, report):
    if cameras is None or min_views == 0:
        return mesh
    ks, c2ws, H, W = cameras
    sub = {} if report is not None else None
    mesh = cull_unseen(mesh, ks, c2ws, H, W, min_views=min_views, bias=default_view_bias(size, n) if view_bias is None else float(view_bias),
                       far=float("inf") if view_far is None else float(view_far), route=_VIEW_ROUTE[route], report=sub)
    if report is not None:
        report["cull"] = sub
    return mesh


def vertex_views(mesh, ks, c2ws, H, W, bias, near=0.0, far=float("inf"), want_mask=False, route="fused", log2dim=6):
    """For every vertex of `mesh` the number of cameras that see it, the mesh itself being the occluder: the tracer is built on the
    mesh (FastMesh.from_arrays, log2dim) and FastMesh.point_views queries its vertices.  -> (views [V] i32, mask [V, ceil(C/32)] i32 or
    None).  bias: how far towards the eye a segment starts, so that the vertex's own faces do not hide it (about half an edge)."""
    if route not in VIEW_ROUTES:
        raise RuntimeError(f"scanerf: route must be one of {VIEW_ROUTES}, got {route!r}")
    from .allocation import _cameras
    from .fastmesh import FastMesh
    dev_ptr(mesh.vertices, _f32, "vertices")
    dev_ptr(mesh.faces, _i32, "faces")
    device = mesh.vertices.device
    V = int(mesh.vertices.shape[0])
    if V == 0 or mesh.faces.shape[0] == 0:      # nothing to build a tracer on (and nothing the cull would keep)
        C = _cameras(ks, c2ws)[0].shape[0]
        return (torch.zeros(V, dtype=_i32, device=device),
                torch.zeros((V, (C + 31) // 32), dtype=_i32, device=device) if want_mask else None)
    fm = FastMesh.from_arrays(mesh.vertices, mesh.faces, device, log2dim=log2dim)
    return fm.point_views(mesh.vertices, ks, c2ws, H, W, bias, near=near, far=far, want_mask=want_mask, route=route)


def cull_by_views(mesh, views, min_views=1, report=None):
    """The cull rule on given per-vertex view counts [V] (any integer dtype, the mesh's device): a face stays iff at least one of its
    three vertices has views >= min_views, a vertex stays iff a kept face uses it.  Kept rows stay in their order, the faces' indices
    are remapped, cells / lattice / normals (where the mesh has them) are gathered row for row: filter_mesh's contract with a per-face
    rule.  min_views=0 returns the input object.  report: receives vertices / faces (before, after) and views_histogram (entry k: the
    vertices seen by exactly k cameras).  torch ops (mask, cumsum, gather): it is not the hot path."""
    min_views = _min_views(min_views)
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    if not isinstance(views, torch.Tensor) or views.dtype.is_floating_point or tuple(views.shape) != (V,) or views.device != mesh.vertices.device:
        raise RuntimeError(f"scanerf: views must be an integer tensor [{V}] on {mesh.vertices.device}")
    if report is not None:
        report.update(vertices=(V, V), faces=(F, F), views_histogram=torch.bincount(views.to(torch.int64)).tolist() if V else [])
    if min_views == 0:
        return mesh
    f = mesh.faces.to(torch.int64)
    kf = (views >= min_views)[f].any(1) if F else torch.zeros(0, dtype=torch.bool, device=f.device)
    kv = torch.zeros(V, dtype=torch.bool, device=f.device)
    kv[f[kf].reshape(-1)] = True
    new_index = torch.cumsum(kv, 0) - 1
    gather = lambda t: None if t is None else t[kv].contiguous()
    out = Mesh(gather(mesh.vertices), new_index[f[kf]].to(_i32).reshape(-1, 3).contiguous(), gather(mesh.cells), gather(mesh.lattice),
               gather(mesh.normals))
    if report is not None:
        report.update(vertices=(V, int(out.vertices.shape[0])), faces=(F, int(out.faces.shape[0])))
    return out


def cull_unseen(mesh, ks, c2ws, H, W, min_views=1, bias=None, near=0.0, far=float("inf"), log2dim=6, route="fused", report=None):
    """Drop the parts of a Mesh that fewer than min_views cameras saw (inner shells, undersides, the far side of the capture's border):
    vertex_views on the mesh itself, then cull_by_views.  bias is required (the extractors pass half a lattice spacing).
    min_views=0 returns the input object (the views are computed only for a report)."""
    min_views = _min_views(min_views)
    if route not in VIEW_ROUTES:
        raise RuntimeError(f"scanerf: route must be one of {VIEW_ROUTES}, got {route!r}")
    if bias is None:
        raise RuntimeError("scanerf: cull_unseen needs bias (about half an edge of the mesh)")
    if min_views == 0 and report is None:
        return mesh
    views, _ = vertex_views(mesh, ks, c2ws, H, W, bias, near=near, far=far, route=route, log2dim=log2dim)
    return cull_by_views(mesh, views, min_views, report)


# ---- simplification by vertex clustering (csrc/mesh_simplify.hip) ----------------------------------------------------
SIMPLIFY_ROUTES = ("fused", "composed")
_CELL_LIMIT = 2 ** 20


def _simplify_cell(cell):
    """The cluster cell's side, checked -> the float32 value as a Python float."""
    if isinstance(cell, bool) or not isinstance(cell, (int, float, np.integer, np.floating)):
        raise RuntimeError(f"scanerf: cell must be a number, got {cell!r}")
    with np.errstate(over="ignore"):
        h = float(np.float32(cell))
    if not 0.0 < h < float("inf"):
        raise RuntimeError(f"scanerf: cell must be positive and finite in float32, got {cell!r}")
    return h


def _simplify_args(mesh, cell, origin, colors, route):
    """The checks simplify_mesh makes before any library call -> (V, F, h, origin as 3 floats)."""
    if route not in SIMPLIFY_ROUTES:
        raise RuntimeError(f"scanerf: route must be one of {SIMPLIFY_ROUTES}, got {route!r}")
    h = _simplify_cell(cell)
    o = [float(np.float32(v)) for v in _host3(origin, "origin")]
    if not all(np.isfinite(o)):
        raise RuntimeError(f"scanerf: origin must be finite, got {list(o)}")
    dev_ptr(mesh.vertices, _f32, "vertices")
    if mesh.vertices.dim() != 2 or mesh.vertices.shape[1] != 3:
        raise RuntimeError(f"scanerf: mesh.vertices must be [V,3], got {tuple(mesh.vertices.shape)}")
    Vn = int(mesh.vertices.shape[0])
    for name, t in (("normals", mesh.normals), ("colors", colors)):
        if t is None:
            continue
        dev_ptr(t, _f32, name)
        if tuple(t.shape) != (Vn, 3) or t.device != mesh.vertices.device:
            raise RuntimeError(f"scanerf: {name} must be [{Vn},3] on {mesh.vertices.device}, got {tuple(t.shape)} on {t.device}")
    V, F = _component_args(mesh.faces, Vn, None, "fused", True)
    if mesh.faces.device != mesh.vertices.device:
        raise RuntimeError(f"scanerf: mesh.faces lives on {mesh.faces.device}, the vertices on {mesh.vertices.device}")
    if V > 2 ** 29:
        raise RuntimeError(f"scanerf: V={V} vertices are more than simplify_mesh takes (2^29)")
    return V, F, h, o


def _fixed(a):
    """t of the definition: rint(clamp(a, -32767, 32767) * 65536) as int64."""
    return torch.round(torch.clamp(a, -32767.0, 32767.0) * 65536.0).to(torch.int64)


def _rounded_mean(S, n):
    """M = floor((2 S + n) / (2 n)) on int64."""
    return torch.div(2 * S + n, 2 * n, rounding_mode="floor")


def _simplify_key(vertices, o, h):
    """-> (k [V,3] f32, q [V,3] i64, good [V] bool by the coordinates): the key's four float32 operations, one torch op each."""
    # (h as a device tensor: torch divides by a host scalar by multiplying with its reciprocal, which is another rounding)
    u = (vertices - torch.tensor(o, dtype=_f32, device=vertices.device)) / torch.tensor([h], dtype=_f32, device=vertices.device)
    k = torch.floor(u)
    f = u - k
    good = (torch.isfinite(vertices) & (k.abs() < float(_CELL_LIMIT))).all(1)
    q = torch.where(good[:, None], f * 65536.0, torch.zeros_like(f)).to(torch.int64)
    return k, q, good


def _simplify_composed(mesh, colors, V, F, h, o):
    """The witness: the definition of include/scanerf_mesh_tools_hip.h in torch ops -> (vertices, faces, normals, colors, counts)."""
    device = mesh.vertices.device
    k, q, good = _simplify_key(mesh.vertices, o, h)
    for t in (mesh.normals, colors):
        if t is not None:
            good &= torch.isfinite(t).all(1)
    n_bad = int((~good).sum())
    if n_bad:
        raise RuntimeError(f"scanerf: simplify_mesh: {n_bad} bad vertices (not finite, or more than 2^20 cells from the origin)")
    index = torch.arange(V, dtype=torch.int64, device=device)
    cells, member = torch.unique(k.to(torch.int64), dim=0, return_inverse=True)
    first = torch.full((cells.shape[0],), V, dtype=torch.int64, device=device).scatter_reduce(0, member, index, "amin")
    label = first[member]
    root = label == index
    row = (torch.cumsum(root, 0) - 1)[label]
    roots = index[root]
    Vk = int(roots.shape[0])
    counts = torch.zeros(Vk, dtype=torch.int64, device=device).index_add_(0, row, torch.ones_like(row))
    single = (counts == 1)[:, None]
    n = counts[:, None]

    def mean(t):
        return _rounded_mean(torch.zeros((Vk, 3), dtype=torch.int64, device=device).index_add_(0, row, t), n).to(_f32) * 2.0 ** -16

    o_t = torch.tensor(o, dtype=_f32, device=device)
    out_v = torch.where(single, mesh.vertices[roots], o_t + (k[roots] + mean(q)) * h)
    out_n = out_c = None
    if mesh.normals is not None:
        m = mean(_fixed(mesh.normals))
        length = torch.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]) + 1e-8
        out_n = torch.where(single, mesh.normals[roots], m / length[:, None]).contiguous()
    if colors is not None:
        out_c = torch.where(single, colors[roots], mean(_fixed(colors))).contiguous()
    rf = row[mesh.faces.to(torch.int64)].reshape(-1, 3)
    keep = (rf[:, 0] != rf[:, 1]) & (rf[:, 0] != rf[:, 2]) & (rf[:, 1] != rf[:, 2])
    return out_v.contiguous(), rf[keep].to(_i32).contiguous(), out_n, out_c, counts


def _simplify_fused(mesh, colors, V, F, h, o):
    from ._capi import tool
    device = mesh.vertices.device
    nbytes = ctypes.c_size_t(0)
    check(tool("scanerf_mesh_simplify_scratch_bytes")(V, F, ctypes.addressof(nbytes)), "mesh_simplify_scratch_bytes")
    nbytes = int(nbytes.value)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
    ptr = lambda t: None if t is None else t.data_ptr()
    host_o = (ctypes.c_float * 3)(*o)
    head = (mesh.vertices.data_ptr(), mesh.faces.data_ptr() if F else None, ptr(mesh.normals), ptr(colors), V, F,
            ctypes.addressof(host_o), h, scratch.data_ptr(), nbytes)
    check(tool("scanerf_mesh_simplify_cluster")(*head, stream()), "mesh_simplify_cluster")
    Vk, Fk, n_bad = (int(v) for v in scratch[:24].view(torch.int64).tolist())      # the one host read
    if n_bad:
        raise RuntimeError(f"scanerf: simplify_mesh: {n_bad} bad vertices (not finite, or more than 2^20 cells from the origin)")
    new = lambda rows, dt, on=True: torch.empty((rows, 3), dtype=dt, device=device) if on else None
    out_v, out_f = new(Vk, _f32), new(Fk, _i32)
    out_n, out_c = new(Vk, _f32, mesh.normals is not None), new(Vk, _f32, colors is not None)
    sums = torch.empty((Vk, 9), dtype=torch.int64, device=device)
    counts = torch.empty((Vk,), dtype=_i32, device=device)
    check(tool("scanerf_mesh_simplify_emit")(*head, sums.data_ptr(), counts.data_ptr(), out_v.data_ptr(), out_f.data_ptr() if Fk else None,
                                             ptr(out_n), ptr(out_c), Vk, Fk, stream()), "mesh_simplify_emit")
    return out_v, out_f, out_n, out_c, counts


def simplify_mesh(mesh, cell, origin=(0.0, 0.0, 0.0), colors=None, route="fused", report=None):
    """Simplify a Mesh by vertex clustering (the definition: include/scanerf_mesh_tools_hip.h, scanerf_mesh_simplify_cluster): the
    vertices in one cell of the world grid of cubic cells of side `cell` at `origin` become one vertex at their (fixed-point) mean,
    with the mean normal (renormalised) and, with colors [V,3] f32, the mean colour; faces are re-indexed, those that lose a corner
    disappear, the rest keep their order and winding.  Output vertices follow the input's order (a cluster stands where its first
    member stood); a cluster of one member is that member, bit for bit.  -> Mesh with cells=None, lattice=None and normals iff the
    input has them, or (Mesh, colors) when colors are given.  route="fused": a lock-free table and integer atomics on the GPU, one
    host read of (V', F', n_bad); route="composed": torch.unique / scatter_reduce / index_add_ / cumsum (the witness).  Both give
    the same bits.  A vertex that is not finite, has a non-finite attribute or lies 2^20 cells or more from the origin is an error.
    report: a dict that receives clusters, largest_cluster and vertices / faces as (before, after)."""
    V, F, h, o = _simplify_args(mesh, cell, origin, colors, route)
    device = mesh.vertices.device
    if V == 0:
        e = lambda dt, on=True: torch.empty((0, 3), dtype=dt, device=device) if on else None
        out = (e(_f32), e(_i32), e(_f32, mesh.normals is not None), e(_f32, colors is not None), None)
    else:
        out = (_simplify_composed if route == "composed" else _simplify_fused)(mesh, colors, V, F, h, o)
    if report is not None:
        report.update(clusters=int(out[0].shape[0]), largest_cluster=int(out[4].max()) if V else 0,
                      vertices=(V, int(out[0].shape[0])), faces=(F, int(out[1].shape[0])))
    simplified = Mesh(out[0], out[1], None, None, out[2])
    return simplified if colors is None else (simplified, out[3])


_SIMPLIFY_ROUTE = {"fused": "fused", "dense": "composed"}      # the extractors' witness route composes the simplification too


def _simplify_rule(simplify):
    """The extractors' simplify argument, checked before any launch."""
    if simplify is not None:
        _simplify_cell(simplify)


def _simplified(mesh, simplify, colors, report, route="fused"):
    """The extractors' last step: simplify=None leaves the mesh (and the colours) as they are."""
    if simplify is None:
        return mesh if colors is None else (mesh, colors)
    sub = {} if report is not None else None
    out = simplify_mesh(mesh, simplify, colors=colors, route=route, report=sub)
    if report is not None:
        report["simplify"] = sub
    return out


def cells_per_axis(occ_size, longest):
    """Lattice for a box: `longest` cells along its longest side, the other sides by the box's aspect (at least 1)."""
    size = [float(v) for v in (occ_size.detach().cpu().tolist() if isinstance(occ_size, torch.Tensor) else occ_size)]
    return [max(1, int(round(int(longest) * s / max(size)))) for s in size]


# ---- vertex colours from posed images (csrc/mesh_colors.hip) ----------------------------------------------------------
COLOR_ROUTES = ("fused", "composed")
DEFAULT_FILL = (0.5, 0.5, 0.5)


def _fill(fill):
    try:
        out = [float(v) for v in fill]
    except (TypeError, ValueError):
        out = []
    if len(out) != 3 or not all(abs(v) < float("inf") for v in out):
        raise RuntimeError(f"scanerf: fill must be three finite numbers, got {fill!r}")
    return out


def resolve_colors(acc, fill=DEFAULT_FILL):
    """The sums of FastMesh.project_colors -> (colors [N,3] f32, valid [N] bool): acc[:, :3] / Wt where Wt > 0 (some camera
    contributed), else `fill`.  One launch; include/scanerf_mesh_tools_hip.h is the definition."""
    from ._capi import tool
    fill = _fill(fill)
    if not isinstance(acc, torch.Tensor) or acc.dtype != _f32 or acc.dim() != 2 or acc.shape[1] != 4:
        raise RuntimeError(f"scanerf: acc must be [N,4] float32, got {tuple(acc.shape) if isinstance(acc, torch.Tensor) else type(acc).__name__}")
    N = int(acc.shape[0])
    ptr = dev_ptr(acc, _f32, "acc")
    colors = torch.empty(N, 3, dtype=_f32, device=acc.device)
    valid = torch.empty(N, dtype=torch.uint8, device=acc.device)
    if N:
        check(tool("scanerf_mesh_resolve_colors")(ptr, N, (ctypes.c_float * 3)(*fill), dev_ptr(colors, _f32, "colors"),
                                                  dev_ptr(valid, torch.uint8, "valid"), stream()), "mesh_resolve_colors")
    return colors, valid.to(torch.bool)


def _views_per_batch(views_per_batch):
    if isinstance(views_per_batch, bool) or not isinstance(views_per_batch, (int, np.integer)) or views_per_batch < 1:
        raise RuntimeError(f"scanerf: views_per_batch must be a positive integer, got {views_per_batch!r}")
    return int(views_per_batch)


def _color_rule(min_cos, fill, route):
    """color_from_views' scalar arguments, checked before any launch."""
    if route not in COLOR_ROUTES:
        raise RuntimeError(f"scanerf: route must be one of {COLOR_ROUTES}, got {route!r}")
    if not 0.0 <= float(min_cos) < 1.0:
        raise RuntimeError(f"scanerf: min_cos must lie in [0, 1), got {min_cos!r}")
    return float(min_cos), _fill(fill)


def default_edge_bias(mesh):
    """Half the mean edge length of the mesh's faces: the bias of a mesh that comes without its lattice (one host read)."""
    if mesh.faces.shape[0] == 0:
        return 1.0
    v = mesh.vertices[mesh.faces.to(torch.int64)]
    edges = torch.stack([v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]], 1)
    mean = float(torch.linalg.norm(edges, dim=-1).mean())
    if not 0.0 < mean < float("inf"):
        raise RuntimeError(f"scanerf: the mesh's mean edge length is {mean}: pass bias")
    return 0.5 * mean


class ViewColors:
    """The running blend of one mesh's vertex colours: the tracer is built once on the mesh, add(images, ks, c2ws) projects a batch
    of cameras into the sums (consecutive batches give the bits of one call), result() divides.  What color_from_views and
    TileSetRenderer.color_mesh feed batch by batch."""

    def __init__(self, mesh, bias, normals="mesh", near=0.0, far=float("inf"), min_cos=0.0, fill=DEFAULT_FILL, log2dim=6, route="fused"):
        from .fastmesh import FastMesh
        self.min_cos, self.fill = _color_rule(min_cos, fill, route)
        self.route, self.bias, self.near, self.far = route, bias, near, far
        if isinstance(normals, str):
            if normals != "mesh":
                raise RuntimeError(f"scanerf: normals must be 'mesh', None or a [V,3] tensor, got {normals!r}")
            normals = getattr(mesh, "normals", None)
        dev_ptr(mesh.vertices, _f32, "vertices")
        dev_ptr(mesh.faces, _i32, "faces")
        self.points = mesh.vertices
        V, device = int(mesh.vertices.shape[0]), mesh.vertices.device
        if normals is not None and (not isinstance(normals, torch.Tensor) or tuple(normals.shape) != (V, 3) or normals.dtype != _f32):
            raise RuntimeError(f"scanerf: normals must be [{V},3] float32")
        self.normals = None if normals is None else normals.contiguous()
        self.empty = V == 0 or mesh.faces.shape[0] == 0      # nothing to build a tracer on: every vertex keeps `fill`
        self.fm = None if self.empty else FastMesh.from_arrays(mesh.vertices, mesh.faces, device, log2dim=log2dim)
        self.acc = torch.zeros(V, 4, dtype=_f32, device=device)
        self.count = torch.zeros(V, dtype=_i32, device=device)

    def add(self, images, ks, c2ws):
        if self.empty:
            return
        images = torch.as_tensor(images)
        if images.dtype == torch.uint8:
            # (a one-element tensor, not a Python number: torch multiplies by the reciprocal of a scalar divisor on the GPU)
            images = images.to(self.points.device).to(_f32) / torch.full((1,), 255.0, dtype=_f32, device=self.points.device)
        images = images.to(self.points.device, _f32).contiguous()
        self.fm.project_colors(self.points, images, ks, c2ws, self.bias, normals=self.normals, near=self.near, far=self.far,
                               min_cos=self.min_cos, acc=self.acc, count=self.count, route=self.route)

    def result(self, report=None):
        V = int(self.points.shape[0])
        if V == 0:
            colors, valid = torch.empty(0, 3, dtype=_f32, device=self.points.device), torch.empty(0, dtype=torch.bool, device=self.points.device)
        elif self.empty:
            colors = torch.tensor(self.fill, dtype=_f32, device=self.points.device).repeat(V, 1)
            valid = torch.zeros(V, dtype=torch.bool, device=self.points.device)
        else:
            colors, valid = resolve_colors(self.acc, self.fill)
        if report is not None:
            report.update(count_histogram=torch.bincount(self.count.to(torch.int64)).tolist() if V else [],
                          invalid=int((~valid).sum()) if V else 0)
        return colors, valid


def color_from_views(mesh, images, ks, c2ws, bias, normals="mesh", near=0.0, far=float("inf"), min_cos=0.0, views_per_batch=8,
                     fill=DEFAULT_FILL, log2dim=6, route="fused", report=None):
    """Vertex colours for ANY mesh from posed images: every vertex is projected into every camera, the cameras that
    see it (vertex_views' rule, the mesh itself occluding; bias as there) are sampled bilinearly and blended, weighted by the cosine
    between the vertex normal and the direction to the eye.  -> (colors [V,3] f32, valid [V] bool); a vertex nobody contributed to
    gets `fill` and valid False.
    images: [C,H,W,3] (array or tensor on any device; uint8 is read as 0..255 -> 0..1), moved views_per_batch at a time, or a
    callable (i0, i1) -> [i1-i0,H,W,3].  normals: "mesh" = mesh.normals when present, else no weighting; None = no weighting; a
    [V,3] tensor.  min_cos drops grazing views.  report: a dict that receives count_histogram (entry k: the vertices k cameras
    contributed to) and invalid.  The tracer is built once; V == 0 or F == 0 returns without a launch."""
    vpb = _views_per_batch(views_per_batch)
    from .allocation import _cameras
    ks, c2ws = torch.as_tensor(ks), torch.as_tensor(c2ws)
    C = int(_cameras(ks, c2ws)[0].shape[0])
    if not callable(images) and (getattr(images, "ndim", 0) != 4 or images.shape[0] != C or images.shape[3] != 3):
        raise RuntimeError(f"scanerf: images must be [C,H,W,3] with C={C}, or a callable (i0, i1) -> [i1-i0,H,W,3]")
    blend = ViewColors(mesh, bias, normals, near, far, min_cos, fill, log2dim, route)
    if not blend.empty:
        for i in range(0, C, vpb):
            j = min(i + vpb, C)
            batch = images(i, j) if callable(images) else images[i:j]
            if tuple(batch.shape[:1]) != (j - i,) or batch.ndim != 4 or batch.shape[3] != 3:
                raise RuntimeError(f"scanerf: images({i}, {j}) must be [{j - i},H,W,3], got {tuple(batch.shape)}")
            blend.add(np.array(batch) if isinstance(batch, np.ndarray) else batch,      # (a copy: a memory-mapped file is read here)
                      ks[i:j], c2ws[i:j])
    return blend.result(report)
