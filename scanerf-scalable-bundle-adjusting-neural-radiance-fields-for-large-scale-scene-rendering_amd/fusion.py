"""Depth-map fusion (csrc/tsdf.hip): mesh what the cameras saw instead of the density's level set.  Depth maps
rendered (or traced) at the capture's cameras are fused into a truncated signed distance volume, and the volume's zero set is cut by
the dense surface-nets op.  The reference has no counterpart; the definition is the comment of include/scanerf_mesh_tools_hip.h.

    TSDFVolume(origin, spacing, n, trunc, device)     owns acc [P,2] = (S, Wt) per lattice point, zeros
        .integrate(depths, ks, c2ws, near, far)       every lattice point against every camera, one launch; route="composed" is the
                                                      witness: one eager float32 torch op per operation of the definition, no skip
        .values(min_weight)                           the value lattice in [0, 1] (inside > 0.5) and which points were observed
        .extract(min_weight, ...)                     surface_nets at 0.5 -> cell_support -> support_cull -> filter_mesh's rules
    support_cull(mesh, support)                       a face stays iff all three vertices have support 8
    fuse_depth_maps(depths, ks, c2ws, box, n, ...)    the above in one call, the cameras fed in batches
    mask_depth / scale_cameras                        what TileSetRenderer.fuse_mesh does to its renders and cameras

Depth is z-depth (compute_ray_forward's rays have camera-z component 1, so TileSetRenderer.render's and FastMesh.render_depth's
depth is); 0 marks a pixel without depth.  No CPU path."""
import math

import numpy as np
import torch

from . import meshing
from ._capi import check, dev_ptr, stream, tool

ROUTES = ("fused", "composed")
_f32, _i32 = torch.float32, torch.int32


def _positive_int(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise RuntimeError(f"scanerf: {name} must be a positive integer, got {v!r}")
    return int(v)


def _min_weight(min_weight):
    if isinstance(min_weight, bool) or not isinstance(min_weight, (int, float, np.integer, np.floating)) or not min_weight >= 1:
        raise RuntimeError(f"scanerf: min_weight must be a number >= 1, got {min_weight!r}")
    return float(min_weight)


def _range(near, far):
    near, far = float(near), float(far)
    if not near >= 0.0:
        raise RuntimeError(f"scanerf: near must be >= 0, got {near}")
    if not far > near:
        raise RuntimeError(f"scanerf: far must be > near={near} (inf for no limit), got {far}")
    return near, far


def _depth_maps(depths, ks, c2ws, device):
    """The checks of a batch of depth maps and its cameras -> (depths [C,H,W] f32, Ks [C,9], C2Ws [C,12], C, H, W)."""
    from .allocation import _cameras
    if not isinstance(depths, torch.Tensor) or depths.dtype != _f32 or depths.dim() != 3:
        raise RuntimeError("scanerf: depths must be a [C,H,W] float32 tensor"
                           + (f", got {tuple(depths.shape)} {depths.dtype}" if isinstance(depths, torch.Tensor) else ""))
    C, H, W = (int(s) for s in depths.shape)
    if H < 1 or W < 1:
        raise RuntimeError(f"scanerf: depths {tuple(depths.shape)}: an image has at least one pixel")
    k9, c12 = _cameras(ks, c2ws, device)
    if k9.shape[0] != C:
        raise RuntimeError(f"scanerf: {C} depth maps but {k9.shape[0]} cameras")
    return depths.detach().contiguous(), k9, c12, C, H, W


class TSDFVolume:
    def __init__(self, origin, spacing, n, trunc, device):
        """A lattice of n = (nx, ny, nz) cells, point (i, j, k) at origin + float(index) * spacing (the dense surface-nets op's vertex
        placement, so its vertices and these points share a frame); trunc: the truncation distance in world units."""
        self.n = [int(v) for v in meshing._lattice_size(n)]
        self.origin, self.spacing = meshing._host3(origin, "origin"), meshing._host3(spacing, "spacing")
        if not all(v >= 1 for v in self.n):
            raise RuntimeError(f"scanerf: every n_k must be >= 1, got {self.n}")
        self.points = (self.n[0] + 1) * (self.n[1] + 1) * (self.n[2] + 1)
        if self.points >= 2 ** 31:
            raise RuntimeError(f"scanerf: n={tuple(self.n)} has {self.points} lattice points: 2^31 or more")
        if not all(0.0 < v < math.inf for v in self.spacing):
            raise RuntimeError(f"scanerf: spacing must be positive and finite, got {list(self.spacing)}")
        if not all(math.isfinite(v) for v in self.origin):
            raise RuntimeError(f"scanerf: origin must be finite, got {list(self.origin)}")
        self.trunc = float(trunc)
        if not 0.0 < self.trunc < math.inf:
            raise RuntimeError(f"scanerf: trunc must be > 0 and finite, got {trunc!r}")
        self.device = torch.device(device)
        self.acc = torch.zeros((self.points, 2), dtype=_f32, device=self.device)

    @property
    def shape(self):
        return tuple(v + 1 for v in self.n)

    # ---- integration ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def integrate(self, depths, ks, c2ws, near=0.0, far=math.inf, route="fused", counters=None):
        """Add the cameras' observations to acc, camera by camera in their order: depths [C,H,W] f32 z-depth on the GPU, ks [C,3,3],
        c2ws [C,3,4] (arrays or tensors).  A pixel counts iff its depth is finite and near < depth <= far (0 marks "no depth").
        The sums start from what acc holds: feeding the cameras in batches gives the bits of one call.  counters: a zeroed
        [3] int64 GPU tensor that receives (pairs evaluated, (block, camera) pairs skipped, updates): the measurement entry."""
        if route not in ROUTES:
            raise RuntimeError(f"scanerf: route must be one of {ROUTES}, got {route!r}")
        near, far = _range(near, far)
        d, k9, c12, C, H, W = _depth_maps(depths, ks, c2ws, self.device)
        acc = dev_ptr(self.acc, _f32, "acc")
        dp = dev_ptr(d, _f32, "depths")
        if d.device != self.acc.device:
            raise RuntimeError(f"scanerf: depths live on {d.device}, the volume on {self.acc.device}")
        if C == 0:      # (an empty tensor has no address to hand over)
            return self
        if route == "composed":
            if counters is not None:
                raise RuntimeError("scanerf: counters belong to the fused route")
            self._integrate_composed(d, k9, c12, H, W, near, far)
            return self
        head = (dp, k9.data_ptr(), c12.data_ptr(), C, H, W, self.origin, self.spacing, *self.n, self.trunc, near, far, acc)
        if counters is None:
            check(tool("scanerf_tsdf_integrate")(*head, stream()), "tsdf_integrate")
        else:
            if tuple(counters.shape) != (3,):
                raise RuntimeError("scanerf: counters must be a [3] int64 tensor")
            check(tool("scanerf_tsdf_integrate_counted")(*head, dev_ptr(counters, torch.int64, "counters"), stream()),
                  "tsdf_integrate_counted")
        return self

    def lattice_points(self):
        """World positions [P,3] f32 of the lattice points, z fastest: origin + float(index) * spacing, two roundings."""
        dev = self.acc.device
        scalar = lambda v: torch.tensor(v, dtype=_f32, device=dev)
        axes = [scalar(self.origin[k]) + torch.arange(self.n[k] + 1, device=dev, dtype=_f32) * scalar(self.spacing[k]) for k in range(3)]
        return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).contiguous()

    def _integrate_composed(self, depths, k9, c12, H, W, near, far):
        """The witness: the definition of include/scanerf_mesh_tools_hip.h, every operation one eager float32 torch op, one camera at a
        time, every point against every camera (no skip)."""
        dev = self.acc.device
        scalar = lambda v: torch.tensor(v, dtype=_f32, device=dev)
        near, far, trunc, Hf, Wf, one = scalar(near), scalar(far), scalar(self.trunc), scalar(float(H)), scalar(float(W)), scalar(1.0)
        P = self.lattice_points()
        S, Wt = self.acc[:, 0].clone(), self.acc[:, 1].clone()
        for c in range(k9.shape[0]):
            K, T = k9[c], c12[c]
            w0, w1, w2 = P[:, 0] - T[3], P[:, 1] - T[7], P[:, 2] - T[11]
            xc = (w0 * T[0] + w1 * T[4]) + w2 * T[8]
            yc = (w0 * T[1] + w1 * T[5]) + w2 * T[9]
            zc = (w0 * T[2] + w1 * T[6]) + w2 * T[10]
            u = K[0] * (xc / zc) + K[2]
            v = K[4] * (yc / zc) + K[5]
            inview = (zc > near) & (u >= 0) & (u < Wf) & (v >= 0) & (v < Hf)
            idx = torch.nonzero(inview).reshape(-1)
            if idx.shape[0] == 0:
                continue
            px, py = u[idx].to(torch.int64), v[idx].to(torch.int64)      # truncation, as (int)
            D = depths[c][py, px]
            sdf = D - zc[idx]
            observed = torch.isfinite(D) & (D > near) & (D <= far) & (sdf >= -trunc)
            at = idx[observed]
            term = torch.minimum(one, sdf[observed] / trunc)
            S[at] = S[at] + term
            Wt[at] = Wt[at] + one
        self.acc[:, 0] = S
        self.acc[:, 1] = Wt

    # ---- the value lattice and the mesh ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def values(self, min_weight=1):
        """-> (values [nx+1, ny+1, nz+1] f32, observed [nx+1, ny+1, nz+1] bool): observed = Wt >= min_weight,
        values = 0.5 - 0.5 (S / Wt) where observed, else 0: in [0, 1], inside iff above 0.5, an unobserved point is outside."""
        min_weight = _min_weight(min_weight)
        acc = dev_ptr(self.acc, _f32, "acc")
        values = torch.empty(self.shape, dtype=_f32, device=self.acc.device)
        observed = torch.empty(self.shape, dtype=torch.uint8, device=self.acc.device)
        check(tool("scanerf_tsdf_values")(acc, self.points, min_weight, values.data_ptr(), observed.data_ptr(), stream()), "tsdf_values")
        return values, observed.view(torch.bool)

    @torch.no_grad()
    def cell_support(self, observed, cells):
        """cells [V,3] i32 (Mesh.cells) -> support [V] i32: how many of the 8 corners of each cell are observed."""
        obs = dev_ptr(observed, (torch.bool, torch.uint8), "observed")
        if tuple(observed.shape) != self.shape:
            raise RuntimeError(f"scanerf: observed must be {list(self.shape)}, got {list(observed.shape)}")
        cp = dev_ptr(cells, _i32, "cells")
        if cells.dim() != 2 or cells.shape[1] != 3:
            raise RuntimeError(f"scanerf: cells must be [V,3], got {tuple(cells.shape)}")
        V = int(cells.shape[0])
        support = torch.empty((V,), dtype=_i32, device=cells.device)
        if V:
            check(tool("scanerf_tsdf_cell_support")(obs, *self.n, cp, V, support.data_ptr(), stream()), "tsdf_cell_support")
        return support

    @torch.no_grad()
    def extract(self, min_weight=1, min_faces=0, min_extent=0, keep_largest=None, report=None):
        """The fused surface: surface_nets(values, 0.5) -> cell_support -> support_cull -> filter_mesh's three rules.  -> meshing.Mesh
        (no normals).  report: a dict that receives support_cull's rows under "support" and the component filter's."""
        min_weight = _min_weight(min_weight)
        meshing._rules(min_faces, min_extent, keep_largest, True)
        values, observed = self.values(min_weight)
        mesh = meshing.surface_nets(values, 0.5, list(self.origin), list(self.spacing))
        sub = {} if report is not None else None
        mesh = support_cull(mesh, self.cell_support(observed, mesh.cells), sub)
        if report is not None:
            report["support"] = sub
        return meshing._filter(mesh, min_faces, min_extent, keep_largest, "fused", False, report)


def support_cull(mesh, support, report=None):
    """Drop what is not surrounded by observation: a face stays iff all three of its vertices have support 8 (every corner of the
    vertex's cell was observed), a vertex stays iff a kept face uses it.  Otherwise cull_by_views' contract: kept rows stay in their
    order, the faces' indices are remapped, cells / lattice / normals (where the mesh has them) are gathered row for row.  It removes
    the spurious sheet between "inside, observed" and "deeper than trunc, never observed", and the ragged rims at frustum borders.
    report: receives vertices / faces (before, after) and support_histogram (entry k: the vertices with support k).  torch ops."""
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    if not isinstance(support, torch.Tensor) or support.dtype.is_floating_point or tuple(support.shape) != (V,) or support.device != mesh.vertices.device:
        raise RuntimeError(f"scanerf: support must be an integer tensor [{V}] on {mesh.vertices.device}")
    f = mesh.faces.to(torch.int64)
    kf = (support == 8)[f].all(1) if F else torch.zeros(0, dtype=torch.bool, device=f.device)
    kv = torch.zeros(V, dtype=torch.bool, device=f.device)
    kv[f[kf].reshape(-1)] = True
    new_index = torch.cumsum(kv, 0) - 1
    gather = lambda t: None if t is None else t[kv].contiguous()
    out = meshing.Mesh(gather(mesh.vertices), new_index[f[kf]].to(_i32).reshape(-1, 3).contiguous(), gather(mesh.cells),
                       gather(mesh.lattice), gather(mesh.normals))
    if report is not None:
        report.update(vertices=(V, int(out.vertices.shape[0])), faces=(F, int(out.faces.shape[0])),
                      support_histogram=torch.bincount(support.to(torch.int64), minlength=9).tolist() if V else [0] * 9)
    return out


def default_trunc(spacing):
    """4 x the largest lattice spacing: a stated default (a few cells on either side of the surface), not a measurement."""
    return 4.0 * max(float(v) for v in spacing)


def lattice_spacing(box_size, n):
    """The spacing of n cells over a box: one float32 division per axis, as the extractors place their lattices."""
    return [meshing._f32_div(box_size[k], n[k]) for k in range(3)]


def _views_per_batch(v):
    return _positive_int(v, "views_per_batch")


def fuse_depth_maps(depths, ks, c2ws, box_corner, box_size, n, trunc=None, views_per_batch=8, near=0.0, far=math.inf, min_weight=1,
                    min_faces=0, min_extent=0, keep_largest=None, report=None):
    """Depth maps [C,H,W] f32 (z-depth, 0 = no depth) of the cameras ks / c2ws -> the Mesh of what they saw, on a lattice of n cells
    over the world box box_corner / box_size.  trunc: default_trunc of the spacing.  The cameras are integrated views_per_batch at a
    time (the same bits for every batch size).  The rest: TSDFVolume.extract."""
    vpb = _views_per_batch(views_per_batch)
    n = meshing._lattice_size(n)
    corner, size = meshing._host3(box_corner, "box_corner"), meshing._host3(box_size, "box_size")
    if not all(0.0 < s < math.inf for s in size):
        raise RuntimeError(f"scanerf: box_size must be positive and finite, got {list(size)}")
    if not all(v >= 1 for v in n):
        raise RuntimeError(f"scanerf: every n_k must be >= 1, got {n}")
    spacing = lattice_spacing(size, n)
    _min_weight(min_weight)
    meshing._rules(min_faces, min_extent, keep_largest, True)
    near, far = _range(near, far)
    if not isinstance(depths, torch.Tensor) or depths.dim() != 3:
        raise RuntimeError("scanerf: depths must be a [C,H,W] float32 tensor")
    vol = TSDFVolume(list(corner), spacing, n, default_trunc(spacing) if trunc is None else trunc, depths.device)
    ks, c2ws = torch.as_tensor(ks), torch.as_tensor(c2ws)
    for i in range(0, int(depths.shape[0]), vpb):
        vol.integrate(depths[i:i + vpb], ks[i:i + vpb], c2ws[i:i + vpb], near=near, far=far)
    return vol.extract(min_weight, min_faces, min_extent, keep_largest, report)


# ---- what TileSetRenderer.fuse_mesh does to its cameras and renders ---------------------------------------------------------------
def scale_cameras(ks, scale):
    """ks [C,3,3] for the H // scale x W // scale frame: fx, fy, cx, cy each divided by scale in float32, as csrc/coverage.hip does."""
    scale = _positive_int(scale, "scale")
    ks = torch.as_tensor(ks).to(_f32).clone()
    if ks.dim() != 3 or tuple(ks.shape[1:]) != (3, 3):
        raise RuntimeError(f"scanerf: ks must be [C,3,3], got {tuple(ks.shape)}")
    s = torch.tensor(float(scale), dtype=_f32, device=ks.device)
    for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)):
        ks[:, r, c] = ks[:, r, c] / s
    return ks


def mask_depth(depth, transparency, max_transparency):
    """A rendered depth map with 0 (no depth) where the ray kept more than max_transparency of its transmittance (it stopped at
    nothing: sky, gaps) or the depth is not finite."""
    bad = (transparency > max_transparency) | ~torch.isfinite(depth)
    return torch.where(bad, torch.zeros_like(depth), depth)

