"""Depth-map fusion (csrc/tsdf.hip): mesh what the cameras saw instead of the density's level set.  Depth maps
rendered (or traced) at the capture's cameras are fused into a truncated signed distance volume, and the volume's zero set is cut by
the dense surface-nets op.  The reference has no counterpart; the definition is the comment of include/scanerf_mesh_tools_hip.h.

    TSDFVolume(origin, spacing, n, trunc, device)     owns acc [P,2] = (S, Wt) per lattice point, zeros
        .integrate(depths, ks, c2ws, near, far)       every lattice point against every camera, one launch; route="composed" is the
                                                      witness: one eager float32 torch op per operation of the definition, no skip
        .values(min_weight)                           the value lattice in [0, 1] (inside > 0.5) and which points were observed
        .extract(min_weight, ...)                     surface_nets at 0.5 -> cell_support -> support_cull -> filter_mesh's rules
    TSDFVolume(..., color=True)                       also owns cacc [P,4] = (R, G, B, Wc): integrate(..., colors=)
                                                      sums the images' pixels in the same launch, vertex_colors(mesh) reads them
                                                      back at a mesh's vertices, extract(colors=True) -> (mesh, rgb)
    TSDFVolume.vertex_normals(mesh)                   the volume's own gradient at a mesh's vertices: (normal, grad);
                                                      extract(normals=True) sets Mesh.normals on the FINAL mesh; route="composed" is
                                                      the witness, one eager float32 torch op per operation of the definition
    support_cull(mesh, support)                       a face stays iff all three vertices have support 8
    fuse_depth_maps(depths, ks, c2ws, box, n, ...)    the above in one call, the cameras fed in batches; colors= [C,H,W,3] -> (mesh, rgb)
    mask_depth / scale_cameras / clamped_image        what TileSetRenderer.fuse_mesh does to its renders and cameras

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


def _color_maps(colors, depths):
    """The checks of a batch of images against its depth maps -> colors [C,H,W,3] f32, contiguous."""
    want = (*depths.shape, 3)
    if not isinstance(colors, torch.Tensor) or colors.dtype != _f32 or tuple(colors.shape) != want:
        raise RuntimeError(f"scanerf: colors must be a {list(want)} float32 tensor (the depth maps' cameras and pixels)"
                           + (f", got {tuple(colors.shape)} {colors.dtype}" if isinstance(colors, torch.Tensor) else ""))
    if colors.device != depths.device:
        raise RuntimeError(f"scanerf: colors live on {colors.device}, depths on {depths.device}")
    return colors.detach().contiguous()


def _fill(fill):
    if isinstance(fill, bool) or not isinstance(fill, (int, float, np.integer, np.floating)) or not math.isfinite(fill):
        raise RuntimeError(f"scanerf: fill must be a finite number, got {fill!r}")
    return float(fill)


class TSDFVolume:
    def __init__(self, origin, spacing, n, trunc, device, color=False):
        """A lattice of n = (nx, ny, nz) cells, point (i, j, k) at origin + float(index) * spacing (the dense surface-nets op's vertex
        placement, so its vertices and these points share a frame); trunc: the truncation distance in world units.  color=True: the
        volume also sums colours, in cacc [P,4] = (R, G, B, Wc) zeros: 16 bytes per lattice point beside acc's 8 (0.87 GB at a
        512 x 205 x 512 lattice); integrate then needs colors=."""
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
        if not isinstance(color, (bool, np.bool_)):
            raise RuntimeError(f"scanerf: color must be True or False, got {color!r}")
        self.acc = torch.zeros((self.points, 2), dtype=_f32, device=self.device)
        self.cacc = torch.zeros((self.points, 4), dtype=_f32, device=self.device) if color else None

    @property
    def shape(self):
        return tuple(v + 1 for v in self.n)

    # ---- integration ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def integrate(self, depths, ks, c2ws, near=0.0, far=math.inf, route="fused", counters=None, colors=None):
        """Add the cameras' observations to acc, camera by camera in their order: depths [C,H,W] f32 z-depth on the GPU, ks [C,3,3],
        c2ws [C,3,4] (arrays or tensors).  A pixel counts iff its depth is finite and near < depth <= far (0 marks "no depth").
        The sums start from what acc holds: feeding the cameras in batches gives the bits of one call.  counters: a zeroed
        [3] int64 GPU tensor that receives (pairs evaluated, (block, camera) pairs skipped, updates): the measurement entry.
        A volume with colour needs colors [C,H,W,3] f32 (any other volume refuses them): an observed pair with sdf <= trunc and a
        finite pixel adds the pixel, unclamped, to cacc (R, G, B) and 1 to Wc, in the same launch; acc gets the same bits either way;
        counters is then [4], the fourth the coloured pairs."""
        if route not in ROUTES:
            raise RuntimeError(f"scanerf: route must be one of {ROUTES}, got {route!r}")
        near, far = _range(near, far)
        d, k9, c12, C, H, W = _depth_maps(depths, ks, c2ws, self.device)
        if (colors is None) != (self.cacc is None):
            raise RuntimeError("scanerf: a volume with colour (color=True) needs colors=, a volume without takes none")
        col = None if colors is None else _color_maps(colors, d)
        acc = dev_ptr(self.acc, _f32, "acc")
        dp = dev_ptr(d, _f32, "depths")
        if d.device != self.acc.device:
            raise RuntimeError(f"scanerf: depths live on {d.device}, the volume on {self.acc.device}")
        if C == 0:      # (an empty tensor has no address to hand over)
            return self
        if route == "composed":
            if counters is not None:
                raise RuntimeError("scanerf: counters belong to the fused route")
            self._integrate_composed(d, k9, c12, H, W, near, far, col)
            return self
        if col is not None:
            head = (dp, dev_ptr(col, _f32, "colors"), k9.data_ptr(), c12.data_ptr(), C, H, W, self.origin, self.spacing, *self.n,
                    self.trunc, near, far, acc, dev_ptr(self.cacc, _f32, "cacc"))
            if counters is None:
                check(tool("scanerf_tsdf_integrate_color")(*head, stream()), "tsdf_integrate_color")
            else:
                if tuple(counters.shape) != (4,):
                    raise RuntimeError("scanerf: counters must be a [4] int64 tensor (a volume with colour)")
                check(tool("scanerf_tsdf_integrate_color_counted")(*head, dev_ptr(counters, torch.int64, "counters"), stream()),
                      "tsdf_integrate_color_counted")
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

    def _integrate_composed(self, depths, k9, c12, H, W, near, far, colors=None):
        """The witness: the definition of include/scanerf_mesh_tools_hip.h, every operation one eager float32 torch op, one camera at a
        time, every point against every camera (no skip); with colors, the colour rule beside it."""
        dev = self.acc.device
        scalar = lambda v: torch.tensor(v, dtype=_f32, device=dev)
        near, far, trunc, Hf, Wf, one = scalar(near), scalar(far), scalar(self.trunc), scalar(float(H)), scalar(float(W)), scalar(1.0)
        P = self.lattice_points()
        S, Wt = self.acc[:, 0].clone(), self.acc[:, 1].clone()
        RGB, Wc = (self.cacc[:, :3].clone(), self.cacc[:, 3].clone()) if colors is not None else (None, None)
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
            if colors is not None:
                pix = colors[c][py[observed], px[observed]]
                coloured = (sdf[observed] <= trunc) & torch.isfinite(pix).all(1)
                ct = at[coloured]
                RGB[ct] = RGB[ct] + pix[coloured]
                Wc[ct] = Wc[ct] + one
        self.acc[:, 0] = S
        self.acc[:, 1] = Wt
        if colors is not None:
            self.cacc[:, :3] = RGB
            self.cacc[:, 3] = Wc

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
    def vertex_colors(self, mesh, fill=0.5):
        """The colours of a mesh's vertices (a volume with colour; the mesh from this volume's lattice, with cells and lattice) ->
        (rgb [V,3] f32, weight [V] f32): the sums and Wc of the eight corners of each vertex's cell interpolated trilinearly at
        mesh.lattice, then rgb = sums / weight.  A vertex with weight 0 (no corner of its cell was coloured) gets `fill` in all
        three channels.  The values are the means of what was integrated: unclamped images give unclamped colours."""
        fill = _fill(fill)
        if self.cacc is None:
            raise RuntimeError("scanerf: vertex_colors needs a volume with colour (color=True)")
        if getattr(mesh, "cells", None) is None or getattr(mesh, "lattice", None) is None:
            raise RuntimeError("scanerf: vertex_colors needs mesh.cells and mesh.lattice (a mesh of this volume's lattice)")
        cacc = dev_ptr(self.cacc, _f32, "cacc")
        cp, lp = dev_ptr(mesh.cells, _i32, "cells"), dev_ptr(mesh.lattice, _f32, "lattice")
        V = int(mesh.cells.shape[0])
        if mesh.cells.dim() != 2 or mesh.cells.shape[1] != 3 or tuple(mesh.lattice.shape) != (V, 3):
            raise RuntimeError(f"scanerf: cells and lattice must be [V,3], got {tuple(mesh.cells.shape)} and {tuple(mesh.lattice.shape)}")
        if mesh.cells.device != self.cacc.device or mesh.lattice.device != self.cacc.device:
            raise RuntimeError(f"scanerf: the mesh lives on {mesh.cells.device}, the volume on {self.cacc.device}")
        rgb = torch.empty((V, 3), dtype=_f32, device=self.cacc.device)
        weight = torch.empty((V,), dtype=_f32, device=self.cacc.device)
        if V:
            check(tool("scanerf_tsdf_vertex_colors")(cacc, *self.n, cp, lp, V, rgb.data_ptr(), weight.data_ptr(), stream()),
                  "tsdf_vertex_colors")
            rgb[weight == 0] = fill
        return rgb, weight

    def _normals_inputs(self, mesh, values, observed):
        """The checks of vertex_normals that need no device -> V."""
        if getattr(mesh, "cells", None) is None or getattr(mesh, "lattice", None) is None:
            raise RuntimeError("scanerf: vertex_normals needs mesh.cells and mesh.lattice (a mesh of this volume's lattice)")
        if (values is None) != (observed is None):
            raise RuntimeError("scanerf: vertex_normals takes values and observed together (what TSDFVolume.values returned), or neither")
        for t, name in ((mesh.cells, "cells"), (mesh.lattice, "lattice"), (values, "values"), (observed, "observed")):
            if t is not None and not isinstance(t, torch.Tensor):
                raise RuntimeError(f"scanerf: {name} must be a torch.Tensor, got {type(t).__name__}")
        V = int(mesh.cells.shape[0]) if mesh.cells.dim() else -1
        if mesh.cells.dim() != 2 or mesh.cells.shape[1] != 3 or tuple(mesh.lattice.shape) != (V, 3):
            raise RuntimeError(f"scanerf: cells and lattice must be [V,3], got {tuple(mesh.cells.shape)} and {tuple(mesh.lattice.shape)}")
        if values is not None and (tuple(values.shape) != self.shape or tuple(observed.shape) != self.shape):
            raise RuntimeError(f"scanerf: values and observed must be {list(self.shape)}, got {list(values.shape)} and {list(observed.shape)}")
        return V

    @torch.no_grad()
    def vertex_normals(self, mesh, min_weight=1, values=None, observed=None, route="fused"):
        """The normals of a mesh's vertices from the volume's own gradient (the mesh from this volume's lattice, with
        cells and lattice) -> (normal [V,3] f32, grad [V,3] f32).  Per lattice point and axis the difference of the observed
        neighbours' values (central where both exist, one-sided where one does, 0 where none), interpolated trilinearly over the
        eight corners of the vertex's cell at mesh.lattice: grad; normal = -grad / (|grad| + 1e-8), pointing out of the surface as the
        faces are wound.  A vertex whose cell has an unobserved corner (or lies outside the lattice) gets zeros: after the support
        cull no vertex is of this kind.  values / observed: what self.values(min_weight) returned, when the caller holds them
        (min_weight is then not used).  route="composed" is the witness: one eager float32 torch op per operation."""
        if route not in ROUTES:
            raise RuntimeError(f"scanerf: route must be one of {ROUTES}, got {route!r}")
        min_weight = _min_weight(min_weight)
        V = self._normals_inputs(mesh, values, observed)
        cp, lp = dev_ptr(mesh.cells, _i32, "cells"), dev_ptr(mesh.lattice, _f32, "lattice")
        if mesh.cells.device != self.acc.device or mesh.lattice.device != self.acc.device:
            raise RuntimeError(f"scanerf: the mesh lives on {mesh.cells.device}, the volume on {self.acc.device}")
        if values is None:
            values, observed = self.values(min_weight)
        vp, op = dev_ptr(values, _f32, "values"), dev_ptr(observed, (torch.bool, torch.uint8), "observed")
        if values.device != self.acc.device or observed.device != self.acc.device:
            raise RuntimeError(f"scanerf: values live on {values.device}, observed on {observed.device}, the volume on {self.acc.device}")
        if route == "composed":
            return self._vertex_normals_composed(values, observed, mesh.cells, mesh.lattice)
        normal = torch.empty((V, 3), dtype=_f32, device=self.acc.device)
        grad = torch.empty((V, 3), dtype=_f32, device=self.acc.device)
        if V:
            check(tool("scanerf_tsdf_vertex_normals")(vp, op, *self.n, self.spacing, cp, lp, V, normal.data_ptr(), grad.data_ptr(),
                                                      stream()), "tsdf_vertex_normals")
        return normal, grad

    def _vertex_normals_composed(self, values, observed, cells, lattice):
        """The witness: the definition of include/scanerf_mesh_tools_hip.h with all four branches of the lattice gradient, every
        operation one eager float32 torch op, the gathers through index arithmetic."""
        dev = self.acc.device
        scalar = lambda v: torch.tensor(v, dtype=_f32, device=dev)
        V = int(cells.shape[0])
        val, obs = values.reshape(-1), observed.reshape(-1).view(torch.uint8) != 0
        n = torch.tensor(self.n, dtype=torch.int64, device=dev)
        stride = ((self.n[1] + 1) * (self.n[2] + 1), self.n[2] + 1, 1)
        cell = cells.to(torch.int64)
        inside = ((cell >= 0) & (cell < n)).all(1)
        c = torch.where(inside[:, None], cell, torch.zeros_like(cell))
        zero, one = scalar(0.0), scalar(1.0)
        t = torch.minimum(torch.maximum(lattice - cell.to(_f32), zero), one)
        t = torch.where(torch.isnan(t), zero, t)                       # fmaxf(NaN, 0) = 0
        w = torch.stack([one - t, t], -1)                              # [V,3,2]
        corner = [(d >> 2, (d >> 1) & 1, d & 1) for d in range(8)]
        idx = [[c[:, k] + o[k] for k in range(3)] for o in corner]
        row = lambda i: (i[0] * stride[0] + i[1] * stride[1]) + i[2]
        ok = inside.clone()
        for i in idx:
            ok &= obs[row(i)]
        G = []
        for a in range(3):
            h = scalar(self.spacing[a])
            h2 = h + h
            acc = None
            for d, i in enumerate(idx):
                q = row(i)
                in_p, in_m = i[a] + 1 <= n[a], i[a] - 1 >= 0
                qp, qm = torch.where(in_p, q + stride[a], q), torch.where(in_m, q - stride[a], q)
                has_p, has_m = in_p & obs[qp], in_m & obs[qm]
                vq, vp, vm = val[q], val[qp], val[qm]
                g = torch.where(has_p & has_m, (vp - vm) / h2,
                                torch.where(has_p, (vp - vq) / h, torch.where(has_m, (vq - vm) / h, torch.zeros_like(vq))))
                wd = (w[:, 0, corner[d][0]] * w[:, 1, corner[d][1]]) * w[:, 2, corner[d][2]]
                acc = wd * g if acc is None else acc + wd * g
            G.append(acc)
        G = torch.stack(G, 1) if V else torch.zeros((0, 3), dtype=_f32, device=dev)
        length = torch.sqrt((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2])
        normal = (-G) / (length + scalar(1e-8))[:, None]
        none = torch.zeros_like(G)
        return torch.where(ok[:, None], normal, none).contiguous(), torch.where(ok[:, None], G, none).contiguous()

    @torch.no_grad()
    def extract(self, min_weight=1, min_faces=0, min_extent=0, keep_largest=None, report=None, colors=False, normals=False,
                simplify=None):
        """The fused surface: surface_nets(values, 0.5) -> cell_support -> support_cull -> filter_mesh's three rules.  -> meshing.Mesh
        (no normals unless asked for).  report: a dict that receives support_cull's rows under "support" and the component filter's.
        colors=True (a volume with colour): -> (mesh, rgb [V,3] f32), vertex_colors on the FINAL mesh, after the support cull and the
        component filter; report["color"] receives the number of vertices no camera coloured (they hold vertex_colors' fill).
        normals=True: the returned Mesh has normals = vertex_normals on the FINAL mesh, from the values / observed
        this call already holds; report["normals"] receives the number of vertices with a zero normal.
        simplify=cell: meshing.simplify_mesh on the world grid of that cell as the LAST step, the normals and colours
        averaged with the vertices; the Mesh then has no cells / lattice; report["simplify"] receives its rows.  None: nothing."""
        meshing._simplify_rule(simplify)
        if not isinstance(colors, (bool, np.bool_)):
            raise RuntimeError(f"scanerf: colors must be True or False, got {colors!r}")
        if not isinstance(normals, (bool, np.bool_)):
            raise RuntimeError(f"scanerf: normals must be True or False, got {normals!r}")
        if colors and self.cacc is None:
            raise RuntimeError("scanerf: extract(colors=True) needs a volume with colour (color=True)")
        min_weight = _min_weight(min_weight)
        meshing._rules(min_faces, min_extent, keep_largest, True)
        values, observed = self.values(min_weight)
        mesh = meshing.surface_nets(values, 0.5, list(self.origin), list(self.spacing))
        sub = {} if report is not None else None
        mesh = support_cull(mesh, self.cell_support(observed, mesh.cells), sub)
        if report is not None:
            report["support"] = sub
        mesh = meshing._filter(mesh, min_faces, min_extent, keep_largest, "fused", False, report)
        if normals:
            normal, _ = self.vertex_normals(mesh, min_weight, values, observed)
            mesh = meshing.Mesh(mesh.vertices, mesh.faces, mesh.cells, mesh.lattice, normal)
            if report is not None:
                report["normals"] = int((normal == 0).all(1).sum())
        if not colors:
            return meshing._simplified(mesh, simplify, None, report)
        rgb, weight = self.vertex_colors(mesh)
        if report is not None:
            report["color"] = int((weight == 0).sum())
        return meshing._simplified(mesh, simplify, rgb, report)


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
                    min_faces=0, min_extent=0, keep_largest=None, report=None, colors=None, normals=False, simplify=None):
    """Depth maps [C,H,W] f32 (z-depth, 0 = no depth) of the cameras ks / c2ws -> the Mesh of what they saw, on a lattice of n cells
    over the world box box_corner / box_size.  trunc: default_trunc of the spacing.  The cameras are integrated views_per_batch at a
    time (the same bits for every batch size).  The rest: TSDFVolume.extract.  colors [C,H,W,3] f32 (the cameras' images, values in
    [0, 1] for a PLY): -> (mesh, rgb [V,3] f32), the mesh the one of the call without colours.  normals=True: the Mesh carries
    TSDFVolume.vertex_normals.  simplify=cell: TSDFVolume.extract's last step."""
    meshing._simplify_rule(simplify)
    vpb = _views_per_batch(views_per_batch)
    if not isinstance(normals, (bool, np.bool_)):
        raise RuntimeError(f"scanerf: normals must be True or False, got {normals!r}")
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
    if colors is not None and (not isinstance(colors, torch.Tensor) or colors.dim() != 4 or colors.shape[0] != depths.shape[0]):
        raise RuntimeError("scanerf: colors must be a [C,H,W,3] float32 tensor, one image per depth map")
    vol = TSDFVolume(list(corner), spacing, n, default_trunc(spacing) if trunc is None else trunc, depths.device, color=colors is not None)
    ks, c2ws = torch.as_tensor(ks), torch.as_tensor(c2ws)
    for i in range(0, int(depths.shape[0]), vpb):
        vol.integrate(depths[i:i + vpb], ks[i:i + vpb], c2ws[i:i + vpb], near=near, far=far,
                      colors=None if colors is None else colors[i:i + vpb])
    return vol.extract(min_weight, min_faces, min_extent, keep_largest, report, colors=colors is not None, normals=bool(normals),
                       simplify=simplify)


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



def clamped_image(diffuse, specular=None):
    """The image fuse_mesh integrates: clamp(diffuse, 0, 1) (colors="diffuse") or clamp(diffuse + specular, 0, 1) (colors="rgb"), one
    float32 addition and one clamp per channel.  A NaN stays a NaN: the integration leaves such a pixel out."""
    image = diffuse if specular is None else diffuse + specular
    return torch.clamp(image.to(_f32), 0.0, 1.0)
