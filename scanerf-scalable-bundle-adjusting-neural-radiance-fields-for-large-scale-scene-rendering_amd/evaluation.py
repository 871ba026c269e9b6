"""Geometric evaluation of a mesh against another: sample both surfaces, ask for every sample the exact distance to
the other mesh (FastMesh.closest_point, csrc/mesh_distance.hip -- the hot step), and reduce: accuracy (pred -> gt), completeness
(gt -> pred), chamfer distance, precision / recall / F-score at distance thresholds, and on request normal consistency (DESIGN.md 4.22:
the dot product of the sampled face's and the nearest face's unit normals).  The reference scores images only
(postprocess/evaluation.py: PSNR / SSIM, here TileTrainer.validate); it has no geometric score.
The image-space score: render_mesh draws a mesh with its vertex colours and normals at the capture's cameras
(FastMesh.render_views, csrc/mesh_render.hip) and compare_renders sets those images against the field's renders there: coverage, depth
error, PSNR over the jointly covered pixels, normal angle.

sample_surface and the reductions are torch ops: they touch each sample once and are not a hot path (the query is)."""
import math

import torch

from . import formats

_f32, _f64, _i64 = torch.float32, torch.float64, torch.int64


def sample_surface(vertices, faces, n, seed):
    """n points on the surface, area-weighted and stratified -> (points [n,3] f32, face [n] i64), on the device of `vertices`.
    Sample i takes u_i = (i + xi_i) / n of the total area and the face whose interval of the float64 area prefix sum holds u_i
    (cum[f-1] <= u_i < cum[f]: a zero-area face has an empty interval and is never chosen), so every face gets its share of n
    within one sample either way; inside the face the point is uniform by the square-root map: s = sqrt(r1), barycentrics
    (1 - s, s (1 - r2), s r2).  (xi, r1, r2) are the columns of ONE torch.rand(n, 3, float64) from a CPU generator seeded with `seed`:
    the same seed gives the same bits on any device.  Built from torch ops; not a hot path."""
    v = torch.as_tensor(vertices)
    f = torch.as_tensor(faces).to(device=v.device, dtype=_i64)
    n = int(n)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"scanerf: sample_surface needs vertices [V,3] and faces [F,3], got {tuple(v.shape)} and {tuple(f.shape)}")
    if n < 0:
        raise ValueError(f"scanerf: sample_surface n={n}")
    tri = v.to(_f64)[f]                                    # [F,3,3]
    A, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cum = torch.cumsum(0.5 * torch.linalg.cross(ab, ac).norm(dim=1), 0)
    total = cum[-1] if cum.numel() else torch.zeros((), dtype=_f64)
    if not bool(total > 0) or not bool(torch.isfinite(total)):
        raise ValueError("scanerf: sample_surface: the mesh has no area")
    r = torch.rand(n, 3, dtype=_f64, generator=torch.Generator(device="cpu").manual_seed(int(seed))).to(v.device)
    u = (torch.arange(n, dtype=_f64, device=v.device) + r[:, 0]) / max(n, 1) * total
    u = torch.minimum(u, torch.nextafter(total, torch.zeros_like(total)))   # (a product rounded up to the total itself)
    idx = torch.searchsorted(cum, u, right=True)
    s = torch.sqrt(r[:, 1:2])
    pts = A[idx] + (s * (1.0 - r[:, 2:3])) * ab[idx] + (s * r[:, 2:3]) * ac[idx]
    return pts.to(_f32).contiguous(), idx


def _direction(d, thresholds):
    """d [n] distances, +inf = not found -> the figures of one direction (float64 reductions on d's device)."""
    d = d.to(_f64)
    n = d.numel()
    found = torch.isfinite(d)
    df = d[found]
    k = df.numel()
    nan = float("nan")
    return {"n": n, "not_found": float(n - k) / n if n else nan,
            "mean": float(df.mean()) if k else nan, "median": float(df.median()) if k else nan,
            "rms": float(df.square().mean().sqrt()) if k else nan,
            "within": {float(t): (float((d <= float(t)).sum()) / n if n else nan) for t in thresholds}}


def summarize(d_pred_to_gt, d_gt_to_pred, thresholds):
    """The scores from the two distance arrays (+inf = nothing within max_dist).  mean / median (the lower of two middle values) /
    rms run over the points found; not_found and the threshold shares over ALL points of the direction.  precision[t] = share of
    pred samples within t of gt, recall[t] = share of gt samples within t of pred, fscore = their harmonic mean (0 when both are 0);
    chamfer = the mean of the two means."""
    a, b = _direction(d_pred_to_gt, thresholds), _direction(d_gt_to_pred, thresholds)
    ts = [float(t) for t in thresholds]
    pr, rc = {t: a["within"][t] for t in ts}, {t: b["within"][t] for t in ts}
    fs = {t: (2.0 * pr[t] * rc[t] / (pr[t] + rc[t]) if pr[t] + rc[t] > 0 else 0.0) for t in ts}
    return {"pred_to_gt": a, "gt_to_pred": b, "precision": pr, "recall": rc, "fscore": fs, "chamfer": 0.5 * (a["mean"] + b["mean"])}


def _flag(v, name):
    if not isinstance(v, bool):
        raise ValueError(f"scanerf: {name} must be True or False, got {v!r}")
    return v


def face_normals(vertices, faces):
    """-> (unit [F,3] f64, has_area [F] bool): cross(b - a, c - a) of each face in float64 from the float32 vertices, normalised;
    a face with zero (or non-finite) area has has_area False and the normal 0."""
    v = torch.as_tensor(vertices).to(_f32).to(_f64)
    tri = v[torch.as_tensor(faces).to(device=v.device, dtype=_i64)]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = n.norm(dim=1)
    ok = torch.isfinite(length) & (length > 0)
    return torch.where(ok[:, None], n / torch.where(ok, length, torch.ones_like(length))[:, None], torch.zeros_like(n)), ok


def _consistency(dist, sample_face, nearest_face, sample_normals, sample_area, nearest_normals, nearest_area):
    """One direction of normal_consistency: dist [n] (+inf = not found), sample_face [n] (rows of sample_normals: the mesh the
    samples were drawn on), nearest_face [n] (rows of nearest_normals: the other mesh; any value where not found).  A sample counts
    iff its distance is finite and both faces have area; c = n_sample . n_nearest.  -> mean, mean_abs, skipped (the share of the n
    samples left out; NaN figures when none counts).  Torch ops on the arrays' device; no GPU needed."""
    n = int(dist.numel())
    found = torch.isfinite(dist.to(_f64))
    sf = sample_face.to(_i64)
    nf = torch.where(found, nearest_face.to(_i64), torch.zeros_like(sf)).clamp_(0, max(int(nearest_normals.shape[0]) - 1, 0))
    if nearest_normals.shape[0] == 0 or sample_normals.shape[0] == 0:
        use = torch.zeros_like(found)
    else:
        use = found & sample_area[sf] & nearest_area[nf]
    c = (sample_normals[sf[use]] * nearest_normals[nf[use]]).sum(1)
    k = int(c.numel())
    nan = float("nan")
    return {"mean": float(c.mean()) if k else nan, "mean_abs": float(c.abs().mean()) if k else nan,
            "skipped": float(n - k) / n if n else nan}


def normal_consistency(pred, gt, pred_to_gt, gt_to_pred):
    """The orientation score beside the distances: pred, gt = (vertices, faces); pred_to_gt / gt_to_pred =
    (dist, sample_face, nearest_face) of the direction.  -> {"pred_to_gt", "gt_to_pred": _consistency's figures, "mean": the mean
    of the two directions' mean}.  1: the surfaces face the same way where they are close; -1: one of them is wound inside out;
    mean_abs ignores the winding."""
    pn, pa = face_normals(*pred)
    gn, ga = face_normals(*gt)
    a = _consistency(*pred_to_gt, pn, pa, gn, ga)
    b = _consistency(*gt_to_pred, gn, ga, pn, pa)
    return {"pred_to_gt": a, "gt_to_pred": b, "mean": 0.5 * (a["mean"] + b["mean"])}


def _mesh_arrays(mesh, device):
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, "__fspath__"):
        v, f = formats.read_ply(mesh)
        return torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    v, f = mesh
    return torch.as_tensor(v).to(device=device, dtype=_f32), torch.as_tensor(f).to(device=device, dtype=torch.int32)


@torch.no_grad()
def compare_meshes(pred, gt, n_samples, thresholds, max_dist=float("inf"), seed=0, log2dim=6, return_distances=False, device=None,
                   normals=False):
    """pred, gt: (vertices [V,3], faces [F,3]) or PLY paths.  n_samples points are drawn on each surface (sample_surface; seed for
    pred, seed + 1 for gt) and queried against the OTHER mesh's FastMesh (log2dim; exact nearest triangle, cut at max_dist).
    -> summarize()'s dict plus n_samples, thresholds and max_dist (None = no cut); with return_distances=True also "distances":
    per direction the sample points, their faces, the distances and the nearest faces of the other mesh (tensors on the device).
    normals=True adds "normal_consistency" (normal_consistency above): per direction the mean and mean absolute dot product of the
    sampled face's and the nearest face's unit normals over the samples that were found and whose two faces have area, the share
    skipped, and "mean" over the two directions.  Without it the dict is what it was, key for key."""
    _flag(normals, "normals")
    from .fastmesh import FastMesh
    if device is None:
        dv = [m[0].device for m in (pred, gt) if isinstance(m, (tuple, list)) and isinstance(m[0], torch.Tensor) and m[0].is_cuda]
        device = dv[0] if dv else torch.device("cuda", torch.cuda.current_device())
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise ValueError(f"scanerf: compare_meshes max_dist must be >= 0 (inf for no cut), got {max_dist}")
    if int(n_samples) < 1:
        raise ValueError(f"scanerf: compare_meshes n_samples={n_samples}")
    thresholds = [float(t) for t in thresholds]
    (pv, pf), (gv, gf) = _mesh_arrays(pred, device), _mesh_arrays(gt, device)
    ps, ps_face = sample_surface(pv, pf, n_samples, seed)
    gs, gs_face = sample_surface(gv, gf, n_samples, seed + 1)
    d_pg, f_pg, _ = FastMesh.from_arrays(gv, gf, device, log2dim).closest_point(ps, max_dist, want_closest=False)
    d_gp, f_gp, _ = FastMesh.from_arrays(pv, pf, device, log2dim).closest_point(gs, max_dist, want_closest=False)
    out = summarize(d_pg, d_gp, thresholds)
    out.update(n_samples=int(n_samples), thresholds=thresholds, max_dist=None if math.isinf(max_dist) else max_dist)
    if normals:
        out["normal_consistency"] = normal_consistency((pv, pf), (gv, gf), (d_pg, ps_face, f_pg), (d_gp, gs_face, f_gp))
    if return_distances:
        out["distances"] = {"pred_to_gt": {"points": ps, "sample_face": ps_face, "dist": d_pg, "face": f_pg},
                            "gt_to_pred": {"points": gs, "sample_face": gs_face, "dist": d_gp, "face": f_gp}}
    return out


def json_line(result):
    """compare_meshes' dict (without the distances) as one JSON line (threshold keys become strings)."""
    import json
    return json.dumps({k: v for k, v in result.items() if k != "distances"})


def save_distances(path, result):
    """The "distances" of compare_meshes(return_distances=True) as an .npz: <direction>_<points|sample_face|dist|face>."""
    import numpy as np
    np.savez(path, **{f"{d}_{k}": t.cpu().numpy() for d, arrs in result["distances"].items() for k, t in arrs.items()})


def add_score_arguments(ap, required):
    """The arguments tools/compare_meshes.py and the extraction commands' --compare share (argparse)."""
    ap.add_argument("--samples", type=int, default=None if required else 200000, required=required, metavar="N",
                    help="points drawn on each surface")
    ap.add_argument("--threshold", type=float, nargs="+", required=required, default=None, metavar="T",
                    help="distance thresholds of precision / recall / fscore (world units)")
    ap.add_argument("--max-dist", type=float, default=float("inf"), metavar="D", help="give up on a point beyond this distance")
    ap.add_argument("--log2dim", type=int, default=6, help="grid cells per axis of the query structure, as a power of two (4..7)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--normal-consistency", action="store_true",
                    help="also score orientation: the dot product of the sampled and the nearest face's unit normals (normal_consistency)")


def score_line(pred, gt, args, device, distances=None):
    """-> json_line(compare_meshes(pred, gt)) under `args` (add_score_arguments); distances: an .npz path for save_distances."""
    res = compare_meshes(pred, gt, args.samples, args.threshold, max_dist=args.max_dist, seed=args.seed, log2dim=args.log2dim,
                         return_distances=distances is not None, device=device,
                         normals=args.normal_consistency)
    if distances is not None:
        save_distances(distances, res)
    return json_line(res)


# ---- image-space score of a mesh: the mesh rendered at the capture's cameras against the field's renders there ----------
def _render_mesh_inputs(mesh, colors, normals, device):
    """-> vertices, faces, vertex normals or None, vertex colours or None, want_normals."""
    vn = None
    if hasattr(mesh, "_fields") and "vertices" in mesh._fields:          # meshing.Mesh
        vn = getattr(mesh, "normals", None)
        mesh = (mesh.vertices, mesh.faces)
    if device is None:
        device = mesh[0].device if isinstance(mesh, (tuple, list)) and isinstance(mesh[0], torch.Tensor) and mesh[0].is_cuda else \
            torch.device("cuda", torch.cuda.current_device())
    v, f = _mesh_arrays(mesh, device)
    if isinstance(normals, bool):
        vn = vn if normals else None
        want = normals
    elif normals is None:
        vn, want = None, False
    else:
        vn, want = normals, True
    as_rows = lambda a, name: None if a is None else _rows(a, v.shape[0], name, device)
    return v, f, as_rows(vn, "normals"), as_rows(colors, "colors"), want


def _rows(a, V, name, device):
    a = torch.as_tensor(a)
    if a.dim() != 2 or tuple(a.shape) != (V, 3) or not a.dtype.is_floating_point:
        raise RuntimeError(f"scanerf: {name} must be [V,3] floating point with V={V}, got {tuple(a.shape)} {a.dtype}")
    return a.to(device=device, dtype=_f32).contiguous()


@torch.no_grad()
def render_mesh(mesh, cameras, colors=None, normals=True, log2dim=6, views_per_batch=8, device=None, collect=False):
    """The mesh seen from cameras = (ks [C,3,3], c2ws [C,3,4], H, W) (FastMesh.render_views, csrc/mesh_render.hip -- the hot step).
    mesh: (vertices, faces), a PLY path or a meshing.Mesh; colors: vertex colours [V,3] in 0..1, or None; normals: True = a normal map
    from the Mesh's vertex normals (interpolated) or, where it has none, from the face normals; False / None = no normal map; an
    array [V,3] = those vertex normals.  The FastMesh is built once (log2dim); the cameras are rendered views_per_batch at a time.
    -> an iterator of (first view index, {"depth" [B,H,W], "face" [B,H,W], "normal" [B,H,W,3], "color" [B,H,W,3]}): one batch of
    images exists at a time.  collect=True: one dict with all C views instead."""
    from .fastmesh import FastMesh
    from .fusion import _views_per_batch
    vpb = _views_per_batch(views_per_batch)
    if cameras is None or len(cameras) != 4:
        raise RuntimeError("scanerf: render_mesh needs cameras=(ks, c2ws, H, W)")
    ks, c2ws, H, W = cameras
    v, f, vn, vc, want = _render_mesh_inputs(mesh, colors, normals, device)
    fm = FastMesh.from_arrays(v, f, v.device, log2dim)
    ks, c2ws = torch.as_tensor(ks), torch.as_tensor(c2ws)
    C = int(ks.shape[0])

    def batches():
        for i in range(0, C, vpb):
            yield i, fm.render_views(ks[i:i + vpb], c2ws[i:i + vpb], H, W, normals=vn, colors=vc, want_normals=want)
    if not collect:
        return batches()
    parts = [b for _, b in batches()]
    if not parts:
        return fm.render_views(ks, c2ws, H, W, normals=vn, colors=vc, want_normals=want)
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


class RenderScore:
    """compare_renders, fed batch by batch: add(pred, target) any number of times, then result().  It keeps per-view figures and
    float64 sums, never an image."""

    def __init__(self, max_depth_diff=None):
        if max_depth_diff is not None and not float(max_depth_diff) >= 0.0:
            raise ValueError(f"scanerf: max_depth_diff must be >= 0 or None, got {max_depth_diff!r}")
        self.max_depth_diff = None if max_depth_diff is None else float(max_depth_diff)
        self.views = []
        self.sums = None
        self.has_color = self.has_normal = None

    @staticmethod
    def _figures(s, has_color, has_normal):
        nan = float("nan")
        div = lambda a, b: a / b if b else nan
        out = {"coverage": div(s["joint"], s["either"]), "pred_only": div(s["pred_only"], s["either"]),
               "target_only": div(s["target_only"], s["either"]), "depth_abs_mean": div(s["abs"], s["joint"]),
               "depth_rmse": math.sqrt(s["sq"] / s["joint"]) if s["joint"] else nan}
        if has_color:
            out["psnr"] = 10.0 * math.log10(255.0 ** 2 / (s["color_sq"] / s["color_n"] + 1e-8)) if s["color_n"] else nan
        if has_normal:
            out["normal_deg_mean"] = div(s["angle"], s["angle_n"])
        return out

    def add(self, pred, target):
        dp, dt = torch.as_tensor(pred["depth"]), torch.as_tensor(target["depth"])
        if dp.dim() != 3 or dp.shape != dt.shape:
            raise RuntimeError(f"scanerf: compare_renders needs depth [C,H,W] on both sides, got {tuple(dp.shape)} and {tuple(dt.shape)}")
        dt = dt.to(dp.device)
        has_color = "color" in pred and "color" in target
        has_normal = "normal" in pred and "normal" in target
        if self.has_color is None:
            self.has_color, self.has_normal = has_color, has_normal
        elif (self.has_color, self.has_normal) != (has_color, has_normal):
            raise RuntimeError("scanerf: compare_renders: the batches do not carry the same maps")
        for name, on in (("color", has_color), ("normal", has_normal)):
            if on and (tuple(pred[name].shape) != tuple(dp.shape) + (3,) or tuple(target[name].shape) != tuple(dp.shape) + (3,)):
                raise RuntimeError(f"scanerf: compare_renders: {name} must be [C,H,W,3] on both sides")
        from . import metrics
        for c in range(dp.shape[0]):
            a, b = dp[c].to(_f64), dt[c].to(_f64)
            P, T = torch.isfinite(a) & (a > 0), torch.isfinite(b) & (b > 0)
            J = P & T
            diff = (a - b)[J]
            s = {"joint": int(J.sum()), "either": int((P | T).sum()), "pred_only": int((P & ~T).sum()),
                 "target_only": int((T & ~P).sum()), "abs": float(diff.abs().sum()), "sq": float(diff.square().sum()),
                 "color_sq": 0.0, "color_n": 0, "angle": 0.0, "angle_n": 0}
            S = J if self.max_depth_diff is None else J & ((a - b).abs() <= self.max_depth_diff)
            view_psnr = None
            if has_color:
                cp = pred["color"][c][S].to(_f32) * 255.0
                ct = target["color"][c].to(dp.device)[S].to(_f32) * 255.0
                s["color_n"] = int(cp.numel())
                s["color_sq"] = float((cp.to(_f64) - ct.to(_f64)).square().sum())
                view_psnr = metrics.psnr(cp, ct) if s["color_n"] else float("nan")
            if has_normal:
                np_, nt = pred["normal"][c][S].to(_f64), target["normal"][c].to(dp.device)[S].to(_f64)
                lp, lt = np_.norm(dim=1), nt.norm(dim=1)
                ok = (lp > 0) & (lt > 0) & torch.isfinite(lp) & torch.isfinite(lt)
                cos = ((np_[ok] / lp[ok, None]) * (nt[ok] / lt[ok, None])).sum(1).clamp(-1.0, 1.0)
                s["angle_n"] = int(ok.sum())
                s["angle"] = float(torch.rad2deg(torch.acos(cos)).sum())
            fig = self._figures(s, has_color, has_normal)
            if view_psnr is not None:
                fig["psnr"] = view_psnr
            self.views.append(fig)
            self.sums = dict(s) if self.sums is None else {k: self.sums[k] + s[k] for k in s}
        return self

    def result(self):
        zero = {k: 0 for k in ("joint", "either", "pred_only", "target_only", "abs", "sq", "color_sq", "color_n", "angle", "angle_n")}
        return {"n_views": len(self.views), "max_depth_diff": self.max_depth_diff, "per_view": list(self.views),
                "pooled": self._figures(self.sums or zero, bool(self.has_color), bool(self.has_normal))}


def compare_renders(pred, target, max_depth_diff=None):
    """Two sets of renders of the same cameras, pixel against pixel.  pred, target: {"depth": [C,H,W]} and optionally "color"
    [C,H,W,3] in 0..1 and "normal" [C,H,W,3] (any length; 0 = none), tensors or arrays.  A render COVERS a pixel iff its depth there
    is finite and > 0.  With P, T the covered sets, J = P and T (jointly covered), E = P or T, per view, in float64:
        coverage = |J| / |E|;  pred_only = |P - T| / |E|;  target_only = |T - P| / |E|       (the three add up to 1)
        depth_abs_mean = mean over J of |d_pred - d_target|;  depth_rmse = sqrt(mean over J of (d_pred - d_target)^2)
        psnr (only when both sides have "color") = metrics.psnr(255 pred, 255 target) over the pixels S:
            10 log10(255^2 / (mse + 1e-8)), mse the mean over the 3 |S| values
        normal_deg_mean (only when both sides have "normal") = the mean angle in degrees, acos of the clamped dot product of the two
            normalised normals, over the pixels of S where both normals are non-zero.
    S = J, or with max_depth_diff the pixels of J whose depths differ by at most that much: where the two renders show different
    surfaces (an occlusion the mesh lacks) the colours and normals are not comparable; the depth figures and the shares keep all of J.
    -> {"n_views", "max_depth_diff", "per_view": [one dict per view], "pooled": the same figures over the pixels of all views
    together (from float64 sums)}.  A figure over an empty set is nan.  Plain torch on the arrays' device; not a hot path."""
    return RenderScore(max_depth_diff).add(pred, target).result()


def render_score_line(score):
    """compare_renders' dict as one JSON line (nan stays NaN, as json writes it)."""
    import json
    return json.dumps(score)
