"""Yardstick and case list of the depth-map fusion (csrc/tsdf.hip; test infrastructure, numpy only, no GPU import),
written from the comment of include/scanerf_mesh_tools_hip.h, not from the kernel.

    integrate(case, dtype)      the definition in float64 (the reference) or float32 (the restatement: the same IEEE operations as
                                the kernel and the composed torch route, so equal bits are expected of all three)
    values / cell_support / support_cull      the other three statements of the header, and the cull rule of fusion.support_cull
    ambiguity flags and the bound for S       below
    sphere(...) / edges()       the cases

The lattice points are the definition's float32 positions in BOTH dtypes (they are the op's input, two float32 roundings by definition);
what is judged is everything after them.

AMBIGUITY.  With u = 2^-24, A_k = sum_a |w_a| |R_ak| (the magnitude of the three products of xc, yc, zc) and FLAG_WIDTH = 64, a point
is flagged when for some camera, in float64,
  * |zc - near| <= FLAG_WIDTH u A_2, or
  * the point may be in view (zc > near - that width) and lies inside the image +- 1 px and u (or v) is within
    FLAG_WIDTH u M of an integer, M = (|fx| (A_0 + |q| A_2) / |zc| + |fx q| + |cx|) the magnitudes that enter u = fx q + cx, q = xc / zc, or
  * it is in view with a valid pixel and |sdf + trunc| <= FLAG_WIDTH u (A_2 + |D| + trunc).
A float32 decision can differ from the float64 one only inside these widths (the rounding of zc is <= 4 u A_2, of u <= ~8 u M,
of sdf <= 4 u A_2 + u |sdf|): 64 is eight times the largest.

THE BOUND FOR S at a point whose decisions agree (first order in u, times 1 + 2^-10 for the higher orders):
  w_a = fl(P_a - E_a), the products and the two additions: |d zc| <= 4 u A_2      (A_2 <= |w| |R_2|)
  sdf = fl(D - zc):        |d sdf| <= 4 u A_2 + u |sdf|
  r = fl(sdf / trunc):     |d r|   <= |d sdf| / trunc + u |r|;      term = min(1, r) moves by no more (min is 1-Lipschitz)
  S = the sequential sum:  each addition rounds by <= u |partial sum|
  bound = sum over the observed cameras of ((4 A_2 + |sdf|) / trunc + |r|) u  +  u sum_k |S_k|,   k = 1 .. Wt,
a function of |w| (through A_2), D (through sdf), trunc and Wt (the number of terms and partial sums); none of it is tuned."""
import functools

import numpy as np

U = 2.0 ** -24
FLAG_WIDTH = 64.0
CAP = 0.10          # the flags may leave out at most this share of a sphere case's lattice points
RADIUS = 0.8
BOX = (-1.1, 2.2)   # corner, side of [-1.1, 1.1]^3
TRUNC, NEAR, FAR = 0.25, 0.1, 1e5
f32 = np.float32


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def lattice_points(origin, spacing, n):
    """[P,3] float32, z fastest: origin_a + float(i_a) * spacing_a, two float32 roundings."""
    ax = [f32(origin[k]) + np.arange(n[k] + 1, dtype=f32) * f32(spacing[k]) for k in range(3)]
    assert all(a.dtype == f32 for a in ax)
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def integrate(case, dtype=np.float64, acc=None, cameras=None, details=False):
    """The definition on `case` for the cameras `cameras` (default: all, in order), starting from acc [P,2] (default zeros).
    -> {"acc" [P,2] dtype}; dtype float64 adds "ambiguous" [P] bool and "bound" [P]; details=True adds per-pair "inview", "observed",
    "term" [C,P]."""
    T = dtype
    P = lattice_points(case["origin"], case["spacing"], case["n"]).astype(T)
    n_pts = P.shape[0]
    acc = np.zeros((n_pts, 2), T) if acc is None else np.asarray(acc).astype(T)
    S, Wt = acc[:, 0].copy(), acc[:, 1].copy()
    near, far, trunc = T(f32(case["near"])), T(f32(case["far"])), T(f32(case["trunc"]))
    H, W = case["depths"].shape[1:]
    Hf, Wf, one = T(H), T(W), T(1)
    cams = range(len(case["ks"])) if cameras is None else cameras
    amb = np.zeros(n_pts, bool)
    bound_terms, bound_sums = np.zeros(n_pts), np.zeros(n_pts)
    out = {k: [] for k in ("inview", "observed", "term")}
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
            r = sdf / trunc
            term = np.minimum(one, r)
            S = np.where(observed, S + np.where(observed, term, T(0)), S).astype(T)
            Wt = np.where(observed, Wt + one, Wt).astype(T)
            if details:
                out["inview"].append(inview), out["observed"].append(observed), out["term"].append(np.where(observed, term, T(0)))
            if T is np.float64:
                A = [np.abs(w0 * M[k]) + np.abs(w1 * M[4 + k]) + np.abs(w2 * M[8 + k]) for k in range(3)]
                wz = FLAG_WIDTH * U * A[2]
                amb |= np.abs(zc - near) <= wz
                maybe = zc > near - wz
                inside = (u >= -1) & (u <= Wf + 1) & (v >= -1) & (v <= Hf + 1)
                for val, f, c0, Ak, q in ((u, fx, cx, A[0], xc / zc), (v, fy, cy, A[1], yc / zc)):
                    mag = np.abs(f) * (Ak + np.abs(q) * A[2]) / np.abs(zc) + np.abs(f * q) + np.abs(c0)
                    amb |= maybe & inside & (np.abs(val - np.rint(val)) <= FLAG_WIDTH * U * mag)
                amb |= inview & valid & (np.abs(sdf + trunc) <= FLAG_WIDTH * U * (A[2] + np.abs(D) + trunc))
                bound_terms += np.where(observed, ((4.0 * A[2] + np.abs(sdf)) / trunc + np.abs(r)) * U, 0.0)
                bound_sums += np.where(observed, np.abs(S) * U, 0.0)
    res = {"acc": np.stack([S, Wt], 1)}
    if T is np.float64:
        res["ambiguous"] = amb
        res["bound"] = (bound_terms + bound_sums) * (1.0 + 2.0 ** -10)
    if details:
        res.update({k: np.stack(v) for k, v in out.items()})
    return res


def values(acc, min_weight=1.0):
    """-> (values [P] float32, observed [P] bool): observed = Wt >= min_weight; values = observed ? 0.5 - 0.5 (S / Wt) : 0, float32."""
    acc = np.asarray(acc, f32)
    S, Wt = acc[:, 0], acc[:, 1]
    observed = Wt >= f32(min_weight)
    with np.errstate(all="ignore"):
        val = f32(0.5) - f32(0.5) * (S / Wt)
    return np.where(observed, val, f32(0)).astype(f32), observed


def cell_support(observed, n, cells):
    """observed [nx+1, ny+1, nz+1] bool, cells [V,3] -> [V] int32: the observed corners of each cell; 0 for a cell outside the lattice."""
    obs = np.asarray(observed).reshape([m + 1 for m in n]).astype(np.int32)
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    ok = ((cells >= 0) & (cells < np.asarray(n))).all(1)
    c = np.where(ok[:, None], cells, 0)
    s = sum(obs[c[:, 0] + (d >> 2), c[:, 1] + ((d >> 1) & 1), c[:, 2] + (d & 1)] for d in range(8))
    return np.where(ok, s, 0).astype(np.int32)


def support_cull(mesh, support):
    """The rule of fusion.support_cull on a surface_nets_reference.Mesh: a face stays iff all three vertices have support 8, a vertex
    iff a kept face uses it; order kept, indices remapped, cells / lattice gathered."""
    f = np.asarray(mesh.faces, np.int64).reshape(-1, 3)
    kf = (np.asarray(support) == 8)[f].all(1)
    kv = np.zeros(len(mesh.vertices), bool)
    kv[f[kf].reshape(-1)] = True
    new = np.cumsum(kv) - 1
    return type(mesh)(mesh.vertices[kv], new[f[kf]].astype(np.int32).reshape(-1, 3), mesh.cells[kv], mesh.lattice[kv])


# ---- the sphere cases ----------------------------------------------------------------------------------------------------------------
def _cameras(rng, C, H, W):
    ks, c2ws = np.zeros((C, 3, 3), f32), np.zeros((C, 3, 4), f32)
    for c in range(C):
        d = rng.normal(size=3)
        eye = d / np.linalg.norm(d) * rng.uniform(3.0, 3.6)
        t = rng.normal(size=3)
        target = t / np.linalg.norm(t) * rng.uniform(0.0, 0.1)
        z = (target - eye) / np.linalg.norm(target - eye)
        a = np.cross(z, [1.0, 0.0, 0.0] if abs(z[0]) < 0.9 else [0.0, 1.0, 0.0])
        a /= np.linalg.norm(a)
        b = np.cross(z, a)
        roll = rng.uniform(0.0, 2.0 * np.pi)
        x = np.cos(roll) * a + np.sin(roll) * b
        y = np.cross(z, x)                                   # x cross y = z: right-handed
        c2ws[c, :, 0], c2ws[c, :, 1], c2ws[c, :, 2], c2ws[c, :, 3] = x, y, z, eye
        f = 60.0 + rng.uniform(-2.0, 2.0)
        ks[c] = [[f, 0, W / 2 + rng.uniform(-0.5, 0.5)], [0, f, H / 2 + rng.uniform(-0.5, 0.5)], [0, 0, 1]]
    return ks, c2ws


def sphere_depth(ks, c2ws, H, W, radius=RADIUS):
    """[C,H,W] float32: the analytic z-depth of the origin-centred sphere along the pixel-centre rays (camera-z component 1), 0 on a
    miss.  float64 arithmetic on the float32 cameras."""
    out = np.zeros((len(ks), H, W), f32)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for c in range(len(ks)):
        K, M = ks[c].astype(np.float64), c2ws[c].astype(np.float64)
        dc = np.stack([(px + 0.5 - K[0, 2]) / K[0, 0], (py + 0.5 - K[1, 2]) / K[1, 1], np.ones_like(px, np.float64)], -1)
        d = dc @ M[:, :3].T
        o = M[:, 3]
        a, b, cc = (d * d).sum(-1), (d * o).sum(-1), (o * o).sum() - radius * radius
        disc = b * b - a * cc
        t = (-b - np.sqrt(np.where(disc > 0, disc, 0))) / a
        out[c] = np.where((disc > 0) & (t > 0), t, 0).astype(f32)
    return out


def _case(name, ks, c2ws, depths, origin, spacing, n, trunc, near, far):
    return {"name": name, "ks": np.ascontiguousarray(ks, f32), "c2ws": np.ascontiguousarray(c2ws, f32),
            "depths": np.ascontiguousarray(depths, f32), "origin": [float(f32(v)) for v in origin],
            "spacing": [float(f32(v)) for v in spacing], "n": [int(v) for v in n], "trunc": float(f32(trunc)),
            "near": float(f32(near)), "far": float(f32(far))}


def sphere(name, C, H, W, n, seed):
    rng = np.random.default_rng(seed)
    ks, c2ws = _cameras(rng, C, H, W)
    spacing = [f32(BOX[1]) / f32(m) for m in n]              # one float32 division per axis, as fusion.lattice_spacing
    return _case(name, ks, c2ws, sphere_depth(ks, c2ws, H, W), [BOX[0]] * 3, spacing, n, TRUNC, NEAR, FAR)


# name: (C, H, W, n, seed).  The seeds are chosen: the cap on the flags holds for every seed tried (0 .. 11: 4.4 - 5.9 % on the dense
# cases), but whether the culled surface of a dense case is CLOSED depends on the cameras drawn -- trunc = 0.25 is 1.8 to 3.2
# spacings here, a surface cell's inner corner lies up to 1.7 spacings deep, and one such corner that no camera observes within trunc
# leaves a hole: 6 of the seeds 0 .. 11 give a closed sphere40, 8 of them a closed sphere70 (chi 2 to 12 otherwise).
SPHERES = {"sphere6": (6, 48, 64, (32, 32, 32), 6), "sphere40": (40, 48, 64, (24, 20, 28), 40), "sphere70": (70, 30, 40, (16, 16, 16), 3)}


# ---- the hand-built case -------------------------------------------------------------------------------------------------------------
def edges():
    """Lattice origin (0, 0, 1), spacing 0.25, n = 4^3 (every coordinate exact); 8 x 8 maps; near = 0.125, far = 8, trunc = 0.25.
    Every camera sits on the z axis with R = I (camera 5: turned by pi about y) so that zc = z - E_z, u = fx x / zc + cx by hand.
    "rows": (camera, (i, j, k), in view, observed, term) worked out by hand."""
    C, H, W = 9, 8, 8
    ks = np.tile(np.array([[8, 0, 0], [0, 8, 0], [0, 0, 1]], f32), (C, 1, 1))
    c2ws = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32), (C, 1, 1))
    depths = np.zeros((C, H, W), f32)
    depths[0][:, 0::2] = 1.0                                  # camera 0: even pixel columns hold 1, odd ones nothing
    c2ws[1, 2, 3] = c2ws[2, 2, 3] = 0.5
    depths[1][:] = f32(0.25) - f32(2.0 ** -25)                # zc = 0.5 at z = 1: sdf = -(0.25 + 2^-25), one ulp below -trunc
    depths[2][:] = 0.75                                       # sdf = +0.25 = +trunc exactly at z = 1
    c2ws[3, 2, 3] = 0.875                                     # zc = 0.125 = near at z = 1
    depths[3][:] = 0.5
    c2ws[4, 2, 3] = 1.0                                       # the eye IS lattice point (0, 0, 0)
    depths[4][:] = 1.0
    c2ws[5, :, :3] = np.diag([-1.0, 1.0, -1.0])               # looking away: zc = -z
    depths[5][:] = 1.0
    # camera 6: every pixel invalid (zeros)
    ks[7, 0, 0] = ks[7, 1, 1] = 4.0                           # u = 4 x / z: pixel i at z = 1
    depths[7][:] = 1.0
    depths[7][0, :5] = [0.0, -1.0, np.inf, np.nan, 9.0]       # nothing, negative, +inf, NaN, beyond far
    ks[8, 0, 0] = ks[8, 1, 1] = 4.0
    depths[8][:] = 8.0                                        # == far: valid
    rows = [
        (0, (0, 0, 0), True, True, 0.0),       # the image corner u = v = 0
        (0, (1, 0, 0), True, True, 0.0),       # u = 2 exactly: pixel 2 (holds 1), not pixel 1 (holds nothing)
        (0, (2, 1, 0), True, True, 0.0),       # u = 4, v = 2
        (0, (4, 0, 0), False, False, 0.0),     # u = 8 = W: outside
        (0, (0, 4, 0), False, False, 0.0),     # v = 8 = H: outside
        (0, (0, 0, 1), True, True, -1.0),      # zc = 1.25: sdf = -0.25 = -trunc exactly: observed
        (0, (1, 0, 4), True, False, 0.0),      # z = 2, x = 0.25: u = 1: an odd column, no depth
        (1, (0, 0, 0), True, False, 0.0),      # one ulp below -trunc
        (2, (0, 0, 0), True, True, 1.0),       # sdf = +trunc exactly
        (2, (0, 0, 1), True, True, 0.0),       # zc = 0.75 = D
        (3, (0, 0, 0), False, False, 0.0),     # zc = near exactly: not in view (strict)
        (3, (0, 0, 1), True, True, 0.5),       # zc = 0.375, D = 0.5: sdf / trunc = 0.5
        (4, (0, 0, 0), False, False, 0.0),     # the point at the eye: zc = 0, u = NaN
        (4, (0, 0, 1), True, True, 1.0),       # zc = 0.25, D = 1: sdf = 0.75, clamped to 1
        (5, (0, 0, 0), False, False, 0.0),     # looking away
        (5, (2, 2, 2), False, False, 0.0),
        (6, (0, 0, 0), True, False, 0.0),      # the all-invalid map
        (7, (0, 0, 0), True, False, 0.0),      # pixel 0: 0
        (7, (1, 0, 0), True, False, 0.0),      # pixel 1: negative
        (7, (2, 0, 0), True, False, 0.0),      # pixel 2: +inf
        (7, (3, 0, 0), True, False, 0.0),      # pixel 3: NaN
        (7, (4, 0, 0), True, False, 0.0),      # pixel 4: beyond far
        (7, (0, 1, 0), True, True, 0.0),       # the next row: 1
        (8, (0, 0, 0), True, True, 1.0),       # D == far counts; sdf = 7 is clamped to 1
    ]
    case = _case("edges", ks, c2ws, depths, [0.0, 0.0, 1.0], [0.25] * 3, (4, 4, 4), 0.25, 0.125, 8.0)
    case["rows"] = rows
    return case


@functools.lru_cache(maxsize=None)
def case(name):
    """The case and its float64 / float32 results, computed once and shared (treat as read-only)."""
    c = edges() if name == "edges" else sphere(name, *SPHERES[name])
    c["ref64"] = integrate(c, np.float64)
    c["ref32"] = integrate(c, np.float32)
    c["judged"] = ~c["ref64"]["ambiguous"]
    return c


CASES = ("sphere6", "sphere40", "sphere70", "edges")


def point_index(n, ijk):
    return (ijk[0] * (n[1] + 1) + ijk[1]) * (n[2] + 1) + ijk[2]
