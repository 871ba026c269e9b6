"""Yardstick and case list of the colour fusion (csrc/tsdf.hip; test infrastructure, numpy only, no GPU import), written
from the comment of include/scanerf_mesh_tools_hip.h, not from the kernel.  It builds on tsdf_reference (the geometry's yardstick),
which it imports and does not change.

    integrate(case, dtype)          geometry AND colour in float64 (the reference) or float32 (the restatement: the kernel's and the
                                    composed torch route's IEEE operations, so equal bits are expected of all three)
    vertex_colors(cacc, ...)        the interpolation at mesh vertices, float64 or float32, with its bound
    reference_mesh(case)            the culled surface-nets mesh of the float32 acc (what fusion.TSDFVolume.extract returns)
    case(name)                      the four cases of tsdf_reference with colour maps; uniform(value) / camera_index() on sphere40

THE COLOUR RULE.  For camera c, in order, for a pair that tsdf_reference's rule calls OBSERVED: COLOURED iff sdf <= trunc and the
three channels of colors[c][py][px] are finite; then R += r, G += g, B += b, Wc += 1, the channels as they are (no clamp).

AMBIGUITY.  tsdf_reference's flags, and one more that mirrors its -trunc flag: a point is flagged when for some camera it is in view
with a valid pixel and |sdf - trunc| <= FLAG_WIDTH u (A_2 + |D| + trunc): the float32 sdf differs from the float64 one by at most
4 u A_2 + u |sdf|, so the band decision can differ only inside that width (64 is eight times it).

THE BOUND FOR THE COLOUR SUMS at a point whose decisions agree.  The pixels are float32 values in both precisions and nothing is
computed from them but the ordered sum, so the only rounding is the addition's: the computed partial sum s_k = fl(s_{k-1} + r_k)
differs from s_{k-1} + r_k by at most u |s_k|, hence |R32 - R64| <= u sum_k |s_k| to first order, k over the coloured cameras; times
(1 + 2^-10) for the higher orders (at most 70 terms: 70 u is far below 2^-10).  Wc is a count: equal.

THE BOUND FOR A VERTEX COLOUR (eight products, seven additions, one division; u = 2^-24, absolute errors, float64 taken as exact).
  t = fl(lattice - cell): <= u t;  1 - t: <= u t + u (1 - t) = u.  Every axis weight carries an ABSOLUTE error <= u (relative to a
    weight near 0 it is unbounded, which is why the analysis is absolute).
  w_d = (wx wy) wz: dw_d <= u (wy wz + wx wz + wx wy) + 2 u w_d   (the three weights' errors and the two products' roundings)
  num_k = sum_d w_d c_dk in ascending d: dnum_k <= sum_d (dw_d |c_dk| + u |w_d c_dk|) + u sum_{j=1..7} |partial_j|;  den likewise
  rgb_k = num_k / den:  |n'/d' - n/d| <= (dnum + |n/d| dden) / d' with d' >= den - dden, plus u |rgb_k| for the division.
  bound_k = ((dnum_k + |rgb_k| dden) / (den - dden) + u |rgb_k|) (1 + 2^-10); a vertex with den - dden <= den / 2 is not judged (its
  weight is itself rounding noise: none in the cases).  The weight's own bound is dden (1 + 2^-10)."""
import functools

import numpy as np

import surface_nets_reference as SN
import tsdf_reference as TR

U, FLAG_WIDTH, f32 = TR.U, TR.FLAG_WIDTH, np.float32
HIGHER = 1.0 + 2.0 ** -10


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def integrate(case, dtype=np.float64, acc=None, cacc=None, cameras=None, details=False):
    """The definition on `case` (a tsdf_reference case with "colors" [C,H,W,3] float32) for the cameras `cameras` (default: all, in
    order), starting from acc [P,2] and cacc [P,4] (default zeros).  -> {"acc", "cacc"}; float64 adds "ambiguous" [P] (the geometry's
    flags and the band flag) and "bound" [P,3] for the colour sums; details=True adds per-pair "observed", "coloured" [C,P] (row i:
    the i-th camera fed), "added" [C,P,3] and "pixel" [C,P] (py * W + px, -1 out of view)."""
    T = dtype
    P = TR.lattice_points(case["origin"], case["spacing"], case["n"]).astype(T)
    n_pts = P.shape[0]
    acc = np.zeros((n_pts, 2), T) if acc is None else np.asarray(acc).astype(T)
    cacc = np.zeros((n_pts, 4), T) if cacc is None else np.asarray(cacc).astype(T)
    S, Wt, RGB, Wc = acc[:, 0].copy(), acc[:, 1].copy(), cacc[:, :3].copy(), cacc[:, 3].copy()
    near, far, trunc = T(f32(case["near"])), T(f32(case["far"])), T(f32(case["trunc"]))
    H, W = case["depths"].shape[1:]
    assert case["colors"].shape == (*case["depths"].shape, 3) and case["colors"].dtype == f32
    Hf, Wf, one = T(H), T(W), T(1)
    cams = range(len(case["ks"])) if cameras is None else cameras
    band = np.zeros(n_pts, bool)
    bound = np.zeros((n_pts, 3))
    out = {k: [] for k in ("observed", "coloured", "added", "pixel")}
    with np.errstate(all="ignore"):
        for c in cams:
            K, M = case["ks"][c].reshape(9).astype(T), case["c2ws"][c].reshape(12).astype(T)
            fx, cx, fy, cy = K[0], K[2], K[4], K[5]
            w0, w1, w2 = P[:, 0] - M[3], P[:, 1] - M[7], P[:, 2] - M[11]
            xc = (w0 * M[0] + w1 * M[4]) + w2 * M[8]
            yc = (w0 * M[1] + w1 * M[5]) + w2 * M[9]
            zc = (w0 * M[2] + w1 * M[6]) + w2 * M[10]
            u = fx * (xc / zc) + cx
            v = fy * (yc / zc) + cy
            assert u.dtype == T and zc.dtype == T
            inview = (zc > near) & (u >= 0) & (u < Wf) & (v >= 0) & (v < Hf)
            px = np.where(inview, u, 0).astype(np.int64)      # truncation, as (int)
            py = np.where(inview, v, 0).astype(np.int64)
            D = case["depths"][c][py, px].astype(T)
            valid = np.isfinite(D) & (D > near) & (D <= far)
            sdf = D - zc
            observed = inview & valid & (sdf >= -trunc)
            term = np.minimum(one, sdf / trunc)
            S = np.where(observed, S + np.where(observed, term, T(0)), S).astype(T)
            Wt = np.where(observed, Wt + one, Wt).astype(T)
            pix = case["colors"][c][py, px].astype(T)                                   # [P,3]
            coloured = observed & (sdf <= trunc) & np.isfinite(pix).all(1)
            add = np.where(coloured[:, None], pix, T(0))
            RGB = np.where(coloured[:, None], RGB + add, RGB).astype(T)
            Wc = np.where(coloured, Wc + one, Wc).astype(T)
            if details:
                out["observed"].append(observed), out["coloured"].append(coloured), out["added"].append(add)
                out["pixel"].append(np.where(inview, py * W + px, -1))
            if T is np.float64:
                A2 = np.abs(w0 * M[2]) + np.abs(w1 * M[6]) + np.abs(w2 * M[10])
                band |= inview & valid & (np.abs(sdf - trunc) <= FLAG_WIDTH * U * (A2 + np.abs(D) + trunc))
                bound += np.where(coloured[:, None], np.abs(RGB) * U, 0.0)
    res = {"acc": np.stack([S, Wt], 1), "cacc": np.concatenate([RGB, Wc[:, None]], 1)}
    assert res["acc"].dtype == T and res["cacc"].dtype == T
    if T is np.float64:
        geometry = TR.integrate(case, np.float64, acc=acc, cameras=cameras)
        assert np.array_equal(geometry["acc"], res["acc"]), "the geometry restated here is not tsdf_reference's"
        res["band"] = band
        res["ambiguous"] = geometry["ambiguous"] | band
        res["bound"] = bound * HIGHER
    if details:
        res.update({k: np.stack(v) for k, v in out.items()})
    return res


def _rows(n, cells):
    """cells [V,3] -> (inside [V] bool, rows [V,8] of the cell's corners in cell_support's order; 0 where outside)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    ok = ((cells >= 0) & (cells < np.asarray(n))).all(1)
    c = np.where(ok[:, None], cells, 0)
    q = [((c[:, 0] + (d >> 2)) * (n[1] + 1) + (c[:, 1] + ((d >> 1) & 1))) * (n[2] + 1) + (c[:, 2] + (d & 1)) for d in range(8)]
    return ok, np.stack(q, 1)


def vertex_colors(cacc, n, cells, lattice, dtype=np.float64):
    """The header's scanerf_tsdf_vertex_colors on cacc [P,4] float32, cells [V,3] int, lattice [V,3] float32, every operation in
    `dtype`.  -> {"rgb" [V,3], "weight" [V]}; float64 adds "bound" [V,3], "weight_bound" [V] and "judged" [V] (see the module text)."""
    T = dtype
    cacc, lattice = np.asarray(cacc, f32).astype(T), np.asarray(lattice, f32).reshape(-1, 3).astype(T)
    ok, q = _rows(n, cells)
    cell = np.asarray(cells, np.int64).reshape(-1, 3).astype(T)
    with np.errstate(all="ignore"):
        t = np.fmin(np.fmax(lattice - cell, T(0)), T(1))           # fmaxf / fminf: a NaN becomes 0
        w = np.stack([T(1) - t, t], -1)                             # [V,3,2]
        assert w.dtype == T
        num = None
        dnum, partial = np.zeros((len(q), 4)), np.zeros((len(q), 4))
        for d in range(8):
            i, j, k = d >> 2, (d >> 1) & 1, d & 1
            wd = (w[:, 0, i] * w[:, 1, j]) * w[:, 2, k]
            prod = wd[:, None] * cacc[q[:, d]]
            num = prod if d == 0 else num + prod
            assert num.dtype == T
            if T is np.float64:
                dw = U * (w[:, 1, j] * w[:, 2, k] + w[:, 0, i] * w[:, 2, k] + w[:, 0, i] * w[:, 1, j]) + 2.0 * U * wd
                dnum += dw[:, None] * np.abs(cacc[q[:, d]]) + U * np.abs(prod)
                if d:
                    partial += np.abs(num)
        num = np.where(ok[:, None], num, T(0))
        den = num[:, 3]
        rgb = np.where((den > 0)[:, None], num[:, :3] / den[:, None], T(0)).astype(T)
    res = {"rgb": rgb, "weight": den}
    if T is np.float64:
        dnum = np.where(ok[:, None], dnum + U * partial, 0.0)
        dden = dnum[:, 3]
        lo = den - dden
        judged = (den <= 0) | (lo > 0.5 * den)
        with np.errstate(all="ignore"):
            b = ((dnum[:, :3] + np.abs(rgb) * dden[:, None]) / lo[:, None] + U * np.abs(rgb)) * HIGHER
        res["bound"] = np.where((den > 0)[:, None] & judged[:, None], b, 0.0)
        res["weight_bound"] = dden * HIGHER
        res["judged"] = judged
    return res


def reference_mesh(c, min_weight=1.0):
    """-> (raw, culled): surface_nets_reference at 0.5 on the values of the case's float32 acc, and tsdf_reference's support cull of it
    (every kept vertex has support 8): the mesh TSDFVolume.extract returns, cell for cell."""
    val, obs = TR.values(c["cref32"]["acc"], min_weight)
    shape = [m + 1 for m in c["n"]]
    raw = SN.surface_nets(val.reshape(shape), 0.5, c["origin"], c["spacing"], dtype=np.float64)
    return raw, TR.support_cull(raw, TR.cell_support(obs.reshape(shape), c["n"], raw.cells))


# ---- the colour maps -----------------------------------------------------------------------------------------------------------------
def radial_answer(points):
    """0.5 + 0.5 p / |p|: the colour of the sphere's surface point in direction p."""
    p = np.asarray(points, np.float64)
    return 0.5 + 0.5 * p / np.linalg.norm(p, axis=-1, keepdims=True)


def radial_colors(ks, c2ws, depths):
    """[C,H,W,3] float32: radial_answer at each pixel's hit point eye + depth * ray (pixel-centre ray, camera-z component 1), 0 on a
    miss; float64 arithmetic on the float32 cameras and depth maps, rounded once."""
    C, H, W = depths.shape
    out = np.zeros((C, H, W, 3), f32)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for c in range(C):
        K, M = ks[c].astype(np.float64), c2ws[c].astype(np.float64)
        dc = np.stack([(px + 0.5 - K[0, 2]) / K[0, 0], (py + 0.5 - K[1, 2]) / K[1, 1], np.ones_like(px, np.float64)], -1)
        hit = M[:, 3] + depths[c].astype(np.float64)[..., None] * (dc @ M[:, :3].T)
        miss = depths[c] <= 0
        with np.errstate(all="ignore"):
            out[c] = np.where(miss[..., None], 0.0, radial_answer(np.where(miss[..., None], 1.0, hit))).astype(f32)
    return out


def with_colors(base, colors, name=None):
    """A colour case: the tsdf_reference case `base` (shared arrays, treat as read-only) with the maps `colors`."""
    c = {k: base[k] for k in ("ks", "c2ws", "depths", "origin", "spacing", "n", "trunc", "near", "far")}
    c["name"] = name or base["name"]
    c["colors"] = np.ascontiguousarray(colors, f32)
    assert c["colors"].shape == (*c["depths"].shape, 3)
    return c


PLANTED = 6      # pixels of sphere40 that receive a non-finite channel


def _sphere(name):
    base = TR.case(name)
    colors = radial_colors(base["ks"], base["c2ws"], base["depths"])
    c = with_colors(base, colors)
    if name == "sphere40":
        # pixels the reference shows to be coloured (each by several lattice points) lose a channel: the finite rule then does work
        r = integrate(c, np.float64, details=True)
        cam, pt = np.nonzero(r["coloured"])
        pick = np.random.default_rng(40).choice(len(cam), PLANTED, replace=False)
        H, W = c["depths"].shape[1:]
        c["planted"] = []
        for i, (a, p) in enumerate(zip(cam[pick], pt[pick])):
            pix = int(r["pixel"][a, p])
            c["colors"][a, pix // W, pix % W, i % 3] = (np.nan, np.inf, -np.inf)[(i // 3 + i) % 3]
            c["planted"].append((int(a), pix // W, pix % W))
        c["coloured_before_planting"] = int(r["coloured"].sum())
    return c


def edges():
    """tsdf_reference.edges() with one more camera and colour maps whose values are exact binary fractions (every hand answer is
    exact in both precisions).  Camera c's map is ((c + 1) / 16, 0.5, 1 - (c + 1) / 16) but for the pixels set below.  Camera 9 sits
    at z = 0.8125 (zc = 0.1875 at z = 1) and holds 0.4375 + 2^-25: sdf = 0.25 + 2^-25, ONE ULP ABOVE +trunc.
    "color_rows": (camera, (i, j, k), observed, coloured, what was added), "color_points": ((i, j, k), the final (R, G, B, Wc))."""
    e = TR.edges()
    C = len(e["ks"]) + 1
    ks, c2ws = np.concatenate([e["ks"], e["ks"][:1]]), np.concatenate([e["c2ws"], e["c2ws"][:1]])
    depths = np.concatenate([e["depths"], np.zeros_like(e["depths"][:1])])
    c2ws[9, 2, 3] = 0.8125
    depths[9][:] = f32(0.4375) + f32(2.0 ** -25)
    assert float(depths[9, 0, 0]) - 0.1875 == 0.25 + 2.0 ** -25 and np.nextafter(f32(0.25), f32(1)) == f32(0.25 + 2.0 ** -25)
    base = lambda c: ((c + 1) / 16, 0.5, 1 - (c + 1) / 16)
    colors = np.zeros((C, 8, 8, 3), f32)
    for c in range(C):
        colors[c] = base(c)
    colors[0, 0, 0] = (-0.5, 1.5, 0.25)               # below 0 and above 1: summed as they are
    colors[7, 1, 0] = (np.nan, 0.5, 0.5)              # one channel not finite: the geometry is updated, the colour is not
    colors[7, 1, 1] = (0.25, 0.5, np.inf)
    colors[7, 1, 2] = (-np.inf, 0.0, 0.0)
    none = (0.0, 0.0, 0.0)
    rows = [
        (0, (0, 0, 0), True, True, (-0.5, 1.5, 0.25)),     # pixel (0, 0): unclamped
        (0, (1, 0, 0), True, True, base(0)),               # pixel 2
        (0, (0, 0, 1), True, True, (-0.5, 1.5, 0.25)),     # sdf = -trunc exactly: observed, in the band; x = y = 0: pixel (0, 0) again
        (0, (1, 0, 4), False, False, none),                # an odd column: no depth, no colour
        (1, (0, 0, 0), False, False, none),                # one ulp below -trunc: not observed
        (2, (0, 0, 0), True, True, base(2)),               # sdf = +trunc EXACTLY: coloured
        (2, (0, 0, 1), True, True, base(2)),               # sdf = 0
        (3, (0, 0, 1), True, True, base(3)),               # sdf = 0.125
        (4, (0, 0, 1), True, False, none),                 # sdf = 0.75: observed (term 1), free space: not coloured
        (5, (0, 0, 0), False, False, none),                # looking away
        (5, (2, 2, 2), False, False, none),
        (6, (0, 0, 0), False, False, none),                # the all-invalid map
        (7, (0, 1, 0), True, False, none),                 # NaN in R
        (7, (1, 1, 0), True, False, none),                 # +inf in B
        (7, (2, 1, 0), True, False, none),                 # -inf in R
        (7, (3, 1, 0), True, True, base(7)),               # the next pixel: finite
        (8, (0, 0, 0), True, False, none),                 # sdf = 7: free space
        (9, (0, 0, 0), True, False, none),                 # one ulp above +trunc: the geometry gets term 1, the colour nothing
    ]
    # (0, 0, 0) is coloured by camera 0, then by camera 2, by no other: the sums in that order
    points = [((0, 0, 0), (-0.5 + 3 / 16, 1.5 + 0.5, 0.25 + 13 / 16, 2.0))]
    case = TR._case("edges", ks, c2ws, depths, e["origin"], e["spacing"], e["n"], e["trunc"], e["near"], e["far"])
    case["colors"] = colors
    case["color_rows"], case["color_points"], case["geometry_rows"] = rows, points, e["rows"]
    return case


def _finish(c):
    c["cref64"] = integrate(c, np.float64)
    c["cref32"] = integrate(c, np.float32)
    c["judged"] = ~c["cref64"]["ambiguous"]
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """The colour case and its float64 / float32 results, computed once and shared (treat as read-only)."""
    return _finish(edges() if name == "edges" else _sphere(name))


CASES = TR.CASES
SPHERES = ("sphere6", "sphere40", "sphere70")
CONSTANT = (0.25, 0.5, 0.75)
# the radial known answer on the culled reference mesh: max over vertices of the largest channel error, and the
# margin for choices that move the culled mesh's vertex set (not for the kernel)
RADIAL_MAX = {"sphere6": 0.082, "sphere40": 0.031, "sphere70": 0.022}
RADIAL_MARGIN = 1.5


@functools.lru_cache(maxsize=None)
def uniform(kind):
    """sphere40 with every camera's map one colour (kind="constant": CONSTANT) or camera c's map (c, 0, 0) (kind="camera_index")."""
    base = TR.case("sphere40")
    colors = np.zeros((*base["depths"].shape, 3), f32)
    if kind == "constant":
        colors[:] = CONSTANT
    else:
        colors[..., 0] = np.arange(len(base["ks"]), dtype=f32)[:, None, None]
    return _finish(with_colors(base, colors, "sphere40_" + kind))
