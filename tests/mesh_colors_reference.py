"""Independent yardstick for the project-and-blend op (scanerf_amd.fastmesh.FastMesh.project_colors, csrc/mesh_colors.hip), numpy only,
written from the definition in include/scanerf_mesh_tools_hip.h and not from the kernel (a helper module, not a test).  It builds on
mesh_visibility_reference (MV), which decides SEEN for every (point, camera) pair, and adds the facing rule, the bilinear sample and
the blend:

  evaluate(case, float64)   the yardstick: MV's float64 brute force over every face decides seen; everything after it in float64;
  evaluate(case, float32)   the restatement: MV's float32 brute force decides seen; every operation after it in float32, operation by
                            operation in the definition's order, the sums in ascending camera order starting from acc / count (what
                            a correct float32 kernel computes where no pair is flagged).

FLAGS.  A pair is flagged when float32 may legitimately decide it the other way: MV's `ambiguous` (the segment grazes an edge or ends
at a face, the point lies at a border of the frustum), and, with min_cos > 0, |cosv - min_cos| < 1e-4 in float64.  With min_cos = 0 a
pair at the threshold has the weight 0: it moves `count`, and the rows are compared where the counts agree.  Bilinear sampling is
continuous across a change of taps and at the clamp, so the sample needs no flag.  A row is flagged when one of its pairs is.

THE BOUND (bound(r32, r64)).  For a row whose contributing cameras are the same in both evaluations, per channel k, with
u = 2^-24, D = the sum of the weights (float64), n = the contributing cameras:
    B_k = 2 * sum_c wt_c (|dpx_c| + |dpy_c|) S_ck / D  +  2 * (sum_c |dwt_c|) R_k / D  +  (2 n + 12) u M_k
  * dpx, dpy: the restatement's own pixel-coordinate error |px32 - px64|, |py32 - py64| (asserted < 1/2).  Inside one cell of the
    pixel grid the bilinear value has |d/dx|, |d/dy| <= the spread of the cell's four taps; a step shorter than a pixel stays in
    the cells next to the float64 position, so S_ck = max - min over the 4 x 4 taps around it (indices clamped) bounds the slope
    along the whole step.  The camera's value moves by at most (|dpx| + |dpy|) S, and the weighted mean by the weighted mean of that.
  * dwt: the restatement's own weight error |wt32 - wt64| (0 without normals).  d(mean)/d(wt_c) = (val_c - mean) / D, and
    |val_c - mean| <= R_k = max - min of the contributing cameras' values.
  * both first-order terms are doubled to cover their second-order remainders (the products of two such errors).
  * the rounding of the arithmetic itself: a sample is three lerps of four roundings each on values of magnitude <= M_k (the largest
    |tap| of the windows): <= 12 u M_k to first order; the blend is n products, n additions in the numerator, n in the
    denominator and one division: its relative error is <= (2 n) u to first order on a mean of magnitude <= M_k.
The bound is derived from the inputs and the two evaluations' coordinates and weights; it never looks at a kernel's output."""
import functools

import numpy as np

import fastmesh_reference as FR
import mesh_visibility_reference as MV
import tile_allocation_reference as TA

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
FLAG_COS = 1e-4
FILL = (0.5, 0.5, 0.5)
FLAGGED_ROWS_CAP = 0.10      # at most this share of a case's rows may hold a flagged pair (tests/test_mesh_colors_cpu.py)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def vertex_normals(V, F):
    """Area-weighted average of the adjacent faces' normals (cross(b - a, c - a), as wound) per vertex, unit, float32; a vertex
    without a face (or with cancelling ones) gets 0."""
    V64 = np.asarray(V, f32).astype(f64)
    n = np.cross(V64[F[:, 1]] - V64[F[:, 0]], V64[F[:, 2]] - V64[F[:, 0]])
    out = np.zeros_like(V64)
    for k in range(3):
        np.add.at(out, F[:, k], n)
    length = np.linalg.norm(out, axis=1)
    return np.where(length[:, None] > 0, out / np.where(length > 0, length, 1.0)[:, None], 0.0).astype(f32)


def smooth_images(C, H, W):
    """Analytic, smooth, in (0, 1), different per camera and channel: for the float64 judgement."""
    c, y, x, k = np.meshgrid(np.arange(C), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    return (0.5 + 0.4 * np.sin(0.13 * x + 0.07 * y + 1.1 * k + 0.5 * c) * np.cos(0.05 * x - 0.11 * y + 0.3 * c)).astype(f32)


def random_images(C, H, W, seed=11):
    """Independent uniform pixels: every tap and every weight matters to the bits."""
    return np.random.default_rng(seed).uniform(0.0, 1.0, (C, H, W, 3)).astype(f32)


def linear_images(C, H, W):
    """I[c, y, x, k] = a + b (x + 1/2) + g (y + 1/2), coefficients per camera and channel: the bilinear value at (px, py) is
    a + b px + g py wherever no index is clamped.  -> images, coefficients [C,3,3] (a, b, g)."""
    rng = np.random.default_rng(5)
    co = np.stack([rng.uniform(0.2, 0.4, (C, 3)), rng.uniform(-0.002, 0.002, (C, 3)), rng.uniform(-0.002, 0.002, (C, 3))], -1)
    y, x = np.arange(H)[None, :, None, None] + 0.5, np.arange(W)[None, None, :, None] + 0.5
    return (co[:, None, None, :, 0] + co[:, None, None, :, 1] * x + co[:, None, None, :, 2] * y).astype(f32), co


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def blend(points, normals, images, ks, c2ws, seen, min_cos=0.0, dtype=f64, acc=None, count=None):
    """The definition after SEEN, every operation in `dtype`.  seen [N,C] bool.  -> dict: acc [N,4], count [N] i32, contributed [N,C]
    bool, px, py, wt [N,C], val [N,C,3] (NaN where the pair is not seen), cosv [N,C]."""
    T = dtype
    pts = np.asarray(points, f32).reshape(-1, 3).astype(T)
    N, C = len(pts), len(ks)
    img = np.asarray(images, f32)
    H, W = img.shape[1:3]
    nrm = None if normals is None else np.asarray(normals, f32).reshape(-1, 3).astype(T)
    acc = np.zeros((N, 4), T) if acc is None else np.asarray(acc, f32).astype(T).copy()
    count = np.zeros(N, np.int32) if count is None else np.asarray(count, np.int32).copy()
    out = {k: np.full((N, C), np.nan, T) for k in ("px", "py", "wt", "cosv")}
    out["val"] = np.full((N, C, 3), np.nan, T)
    out["contributed"] = np.zeros((N, C), bool)
    half, one, mc = T(0.5), T(1.0), T(f32(min_cos))
    with np.errstate(all="ignore"):
        for c in range(C):
            K, M = np.asarray(ks[c], f32).astype(T).reshape(9), np.asarray(c2ws[c], f32)[:3].astype(T).reshape(12)
            E = np.array([M[3], M[7], M[11]], T)
            w = pts - E
            xc = (w[:, 0] * M[0] + w[:, 1] * M[4]) + w[:, 2] * M[8]
            yc = (w[:, 0] * M[1] + w[:, 1] * M[5]) + w[:, 2] * M[9]
            zc = (w[:, 0] * M[2] + w[:, 1] * M[6]) + w[:, 2] * M[10]
            length = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
            px, py = K[0] * (xc / zc) + K[2], K[4] * (yc / zc) + K[5]
            s = seen[:, c]
            if nrm is not None:
                nl = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
                q = (nrm[:, 0] * w[:, 0] + nrm[:, 1] * w[:, 1]) + nrm[:, 2] * w[:, 2]
                cosv = (-q) / (length * nl)
                faces = cosv > mc
                wt = cosv
            else:
                cosv = np.full(N, np.nan, T)
                faces, wt = np.ones(N, bool), np.ones(N, T)
            sx, sy = np.where(s, px, half), np.where(s, py, half)          # an unseen pair samples pixel 0: never used
            u, v = sx - half, sy - half
            x0f, y0f = np.floor(u), np.floor(v)
            ax, ay = u - x0f, v - y0f
            xi, yi = x0f.astype(np.int64), y0f.astype(np.int64)
            x0, x1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
            y0, y1 = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
            I = img[c]
            a, b, g, d = I[y0, x0], I[y0, x1], I[y1, x0], I[y1, x1]
            finite = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(g).all(1) & np.isfinite(d).all(1)
            a, b, g, d = (t.astype(T) for t in (a, b, g, d))
            ax, ay = ax[:, None], ay[:, None]
            top = (one - ax) * a + ax * b
            bot = (one - ax) * g + ax * d
            val = (one - ay) * top + ay * bot
            use = s & faces & finite
            wv = wt[:, None] * val
            acc[:, :3] = np.where(use[:, None], acc[:, :3] + wv, acc[:, :3])
            acc[:, 3] = np.where(use, acc[:, 3] + wt, acc[:, 3])
            count += use
            out["contributed"][:, c] = use
            out["px"][:, c], out["py"][:, c] = np.where(s, px, np.nan), np.where(s, py, np.nan)
            out["wt"][:, c], out["cosv"][:, c] = np.where(s, wt, np.nan), np.where(s, cosv, np.nan)
            out["val"][:, c] = np.where(s[:, None], val, np.nan)
    out.update(acc=acc, count=count)
    return out


def resolve(acc, fill=FILL, dtype=f32):
    """scanerf_mesh_resolve_colors in `dtype` -> (colors [N,3], valid [N] bool)."""
    acc = np.asarray(acc).astype(dtype)
    valid = acc[:, 3] > 0
    with np.errstate(all="ignore"):
        colors = np.where(valid[:, None], acc[:, :3] / acc[:, 3:4], np.asarray(fill, dtype)[None])
    return colors.astype(dtype), valid


@functools.lru_cache(maxsize=None)
def _seen32(name):
    c = CASES[name]()
    return MV.evaluate(c["points"], c["ks"], c["c2ws"], c["H"], c["W"], c["bias"], c["V"], c["F"], c["near"], c["far"], dtype=f32)["seen"]


def seen_of(case, dtype):
    """[N,C] bool: MV's float64 reference (recorded for the large cases) or its float32 restatement (computed once per case)."""
    if dtype == f64:
        return case["ref"]["seen"]
    if case["name"] in CASES:
        return _seen32(case["name"])
    return MV.evaluate(case["points"], case["ks"], case["c2ws"], case["H"], case["W"], case["bias"], case["V"], case["F"], case["near"],
                       case["far"], dtype=f32)["seen"]


def evaluate(case, dtype=f64, images="smooth", normals="case", cameras=None, acc=None, count=None, fill=FILL):
    """A case through the whole definition in `dtype`.  images: a key of the case ("smooth", "random") or an array [C,H,W,3];
    normals: "case" (the case's), None, or an array; cameras: the columns to take, in this order (default: all, ascending).
    -> blend()'s dict plus colors, valid (resolve in `dtype`) and, for float64, flagged [N,C] and flagged_rows [N]."""
    img = case[images] if isinstance(images, str) else images
    nrm = case["normals"] if isinstance(normals, str) else normals
    cols = np.arange(len(case["ks"])) if cameras is None else np.asarray(cameras, np.int64)
    seen = seen_of(case, dtype)[:, cols]
    out = blend(case["points"], nrm, np.asarray(img)[cols], case["ks"][cols], case["c2ws"][cols], seen, case["min_cos"], dtype, acc, count)
    out["colors"], out["valid"] = resolve(out["acc"], fill, dtype)
    out["seen"] = seen
    if dtype == f64:
        flagged = case["ref"]["ambiguous"][:, cols].copy()
        if nrm is not None and case["min_cos"] > 0:
            with np.errstate(invalid="ignore"):
                flagged |= seen & (np.abs(out["cosv"] - f64(f32(case["min_cos"]))) < FLAG_COS)
        out["flagged"], out["flagged_rows"] = flagged, flagged.any(1)
    return out


def _window(img, x, y):
    """The 4 x 4 taps around the float64 position (x, y) of one camera's image, indices clamped -> [n,16,3] float64."""
    H, W = img.shape[:2]
    xi, yi = np.floor(x - 0.5).astype(np.int64), np.floor(y - 0.5).astype(np.int64)
    xs = np.clip(xi[:, None] + np.arange(-1, 3)[None], 0, W - 1)
    ys = np.clip(yi[:, None] + np.arange(-1, 3)[None], 0, H - 1)
    return img[ys[:, :, None], xs[:, None, :]].reshape(len(x), 16, 3).astype(f64)


def bound(r32, r64, images):
    """The module text's B [N,3] for the float32 restatement r32 against the yardstick r64 on `images` [C,H,W,3]; +inf where the two
    disagree about the contributing cameras (such a row is not judged).  -> (B, judged [N] bool)."""
    img = np.asarray(images, f32)
    N, C = r64["contributed"].shape
    same = (r32["contributed"] == r64["contributed"]).all(1)
    coord, dw, D, M = np.zeros((N, 3)), np.zeros(N), np.zeros(N), np.zeros((N, 3))
    lo, hi = np.full((N, 3), np.inf), np.full((N, 3), -np.inf)
    with np.errstate(all="ignore"):
        for c in range(C):
            j = np.nonzero(r64["contributed"][:, c] & same)[0]
            if not len(j):
                continue
            dpx = np.abs(r32["px"][j, c].astype(f64) - r64["px"][j, c])
            dpy = np.abs(r32["py"][j, c].astype(f64) - r64["py"][j, c])
            assert (dpx < 0.5).all() and (dpy < 0.5).all(), "a float32 pixel coordinate is off by half a pixel"
            win = _window(img[c], r64["px"][j, c], r64["py"][j, c])
            S = win.max(1) - win.min(1)
            wt = r64["wt"][j, c]
            coord[j] += (wt * (dpx + dpy))[:, None] * S
            dw[j] += np.abs(r32["wt"][j, c].astype(f64) - wt)
            D[j] += wt
            M[j] = np.maximum(M[j], np.abs(win).max(1))
            lo[j], hi[j] = np.minimum(lo[j], r64["val"][j, c]), np.maximum(hi[j], r64["val"][j, c])
        n = r64["count"].astype(f64)
        R = np.where(np.isfinite(hi - lo), hi - lo, 0.0)
        B = 2.0 * coord / D[:, None] + 2.0 * (dw / D)[:, None] * R + ((2.0 * n + 12.0) * U)[:, None] * M
    judged = same & r64["valid"]
    return np.where(judged[:, None], B, np.inf), judged


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _with_images(case, normals, min_cos):
    C, H, W = len(case["ks"]), case["H"], case["W"]
    return dict(case, normals=None if normals is None else np.asarray(normals, f32), min_cos=min_cos, smooth=smooth_images(C, H, W),
                random=random_images(C, H, W))


@functools.lru_cache(maxsize=None)
def terrain():
    """MV.terrain() (2 497 vertices, 8 cameras at 102 x 134) with the terrain's vertex normals and min_cos = 0.2."""
    V, F = TA.mesh()
    return dict(_with_images(MV.terrain(), _upward(vertex_normals(V, F)), 0.2), name="terrain")


def _upward(n):
    """The height field's faces are wound one way and the boxes' another: the cases want normals on the cameras' side (z up)."""
    return np.where(n[:, 2:3] < 0, -n, n).astype(f32)


@functools.lru_cache(maxsize=None)
def nested(extra=False):
    """MV.nested(): normals pointing away from each shell's centre, min_cos = 0."""
    c = MV.nested(extra)
    n = vertex_normals(c["V"], c["F"])
    centre = np.where(np.arange(len(n))[:, None] < c["n_outer"], 0.0, np.array([0.13, -0.21, 0.07]))
    out = np.where(((c["V"] - centre) * n).sum(1, keepdims=True) < 0, -n, n)
    return dict(_with_images(c, out, 0.0), name="nested_extra" if extra else "nested")


@functools.lru_cache(maxsize=None)
def edges():
    """MV.edges(): free points, so hand-made normals: towards +x (both eyes lie there), one zero, one NaN; min_cos = 0."""
    c = MV.edges()
    n = np.tile(np.array([[1.0, 0.1, -0.05]], f32), (len(c["points"]), 1))
    n[3] = 0.0
    n[5, 1] = np.nan
    return _with_images(c, n, 0.0)


@functools.lru_cache(maxsize=None)
def many_cameras():
    """MV.many_cameras(): 300 terrain vertices against 65 cameras (a pass of the kernel and one more), min_cos = 0.1."""
    V, F = TA.mesh()
    return _with_images(MV.many_cameras(), _upward(vertex_normals(V, F))[::8][:MV.MANY_POINTS], 0.1)


PLATES_MIN_COS = 0.3


@functools.lru_cache(maxsize=None)
def plates():
    """Known answers, by hand.  Two plates |x|, |y| <= 1: the front one at z = 0, the rear one at z = -1.  Cameras 0 and 1 above
    (eyes (0, 0, 5) and (2, 0.5, 4.5)), camera 2 grazing (eye (6, 0, 0.5)): from the front plate's points its cosine is ~0.08, from
    the rear plate's ~0.24, both below min_cos = 0.3.  Points 0..3 lie on the front plate, 4..6 on the rear plate under it: hidden
    from cameras 0 and 1 by the front plate, seen by camera 2 alone (its line passes z = 0 at x > 3).  All normals are (0, 0, 1),
    but point 3's, which is 0.  Image c holds the constant CONSTANTS[c]."""
    V = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1]], f32)
    F = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    H, W = 17, 33
    cams = [FR.look_at(e, (0, 0, -0.5), H, W, 20.0) for e in ((0.0, 0.001, 5.0), (2.0, 0.5, 4.5), (6.0, 0.0, 0.5))]
    pts = np.array([(0.3, 0.2, 0), (-0.4, 0.1, 0), (0.1, -0.45, 0), (0.25, 0.3, 0), (0.3, 0.2, -1), (-0.2, 0.1, -1), (0.1, -0.3, -1)], f32)
    normals = np.tile(np.array([[0, 0, 1]], f32), (len(pts), 1))
    normals[3] = 0
    c = MV._case("plates", pts, np.stack([K for _, K in cams]), np.stack([m for m, _ in cams]), H, W, 0.05, V, F)
    c = _with_images(c, normals, PLATES_MIN_COS)
    c["constant"] = np.broadcast_to(CONSTANTS[:, None, None, :], (3, H, W, 3)).astype(f32).copy()
    c["eyes"] = np.array([(0.0, 0.001, 5.0), (2.0, 0.5, 4.5), (6.0, 0.0, 0.5)])
    return c


CONSTANTS = np.array([(0.2, 0.4, 0.6), (0.8, 0.1, 0.3), (0.5, 0.9, 0.7)], f32)
CASES = {"terrain": terrain, "nested": nested, "nested_extra": lambda: nested(True), "edges": edges, "many_cameras": many_cameras,
         "plates": plates}


@functools.lru_cache(maxsize=None)
def small(name, H, W):
    """small_images of a named case, computed once."""
    return small_images(CASES[name](), H, W)


SMALL_POINTS = 100      # the brute-force visibility reference of a small-image case is recomputed: a third of the points keeps it quick


def small_images(case, H, W):
    """The case seen through the same cameras at H x W pixels (K scaled per axis): images so small that a good share of the points
    project into the border half pixel, where the indices clamp.  The first SMALL_POINTS points; the visibility reference is recomputed
    (no record)."""
    sx, sy = W / case["W"], H / case["H"]
    ks = case["ks"].copy()
    ks[:, 0, :] *= f32(sx)
    ks[:, 1, :] *= f32(sy)
    c = MV._case(f"{case['name']}@{H}x{W}", case["points"][:SMALL_POINTS], ks, case["c2ws"], H, W, case["bias"], case["V"], case["F"], case["near"],
                 case["far"])
    return _with_images(c, None if case["normals"] is None else case["normals"][:SMALL_POINTS], case["min_cos"])


# ---- the round trip on the icosphere --------------------------------------------------------------------------------------------------
def icosphere(radius, levels):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [np.asarray(v, f64) / np.linalg.norm(v) for v in ((-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t),
                                                            (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1))]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = out
    return (radius * np.stack(V)).astype(f32), np.asarray(F, np.int32)


ROUND_TRIP_MIN_COS = 0.5


@functools.lru_cache(maxsize=None)
def round_trip():
    """A unit icosphere (162 vertices) with the vertex colours 0.5 + 0.5 * position, 14 cameras at distance 4 (near the 6 axes and
    the 8 diagonals: every vertex has one within 45 degrees of its normal), 48 x 48 pixels.  The case's images are NOT set here: they are a render of the coloured mesh (mesh_render_reference.render, or
    FastMesh.render_views on the GPU), projected back with min_cos = 0.5 and the vertex normals = the positions."""
    V, F = icosphere(1.0, 2)
    H = W = 48
    eyes = [(4, 0.1, 0.2), (-4, 0.2, -0.1), (0.1, 4, 0.3), (0.2, -4, -0.2), (0.15, 0.1, 4), (-0.1, 0.2, -4)]
    eyes += [(2.3 * x + 0.1, 2.3 * y - 0.05, 2.3 * z + 0.15) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
    cams = [FR.look_at(e, (0, 0, 0), H, W, 75.0) for e in eyes]
    c = MV._case("round_trip", V, np.stack([K for _, K in cams]), np.stack([m for m, _ in cams]), H, W, 0.02, V, F)
    colors = (0.5 + 0.5 * V).astype(f32)
    return dict(c, normals=V.copy(), min_cos=ROUND_TRIP_MIN_COS, colors=colors)


@functools.lru_cache(maxsize=None)
def round_trip_reference():
    """The pipeline in numpy: mesh_render_reference renders the coloured icosphere in float32 (the images a correct float32 renderer
    hands over), the new reference projects them back in float64 and in float32.  -> (images f32, r64, r32)."""
    import mesh_render_reference as RR
    c = round_trip()
    img = RR.render(c["ks"].reshape(-1, 9), c["c2ws"].reshape(-1, 12), c["H"], c["W"], c["V"], c["F"], colors=c["colors"], dtype=f32)["color"]
    img = np.asarray(img, f32)
    return img, evaluate(c, f64, images=img), evaluate(c, f32, images=img)
