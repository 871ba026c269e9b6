"""Independent float64 yardstick for the mesh tracer (scanerf_amd.fastmesh, csrc/mesh.hip), numpy only, written from the
definitions and not from the kernels:

  nearest_hit   Moeller-Trumbore against EVERY face, no grid: smallest t > 0, else 0 (+ which rays are "grazing");
  first_enter   the registration rule in numpy, then per occupied cell the slab interval of the ray with the CELL and with the
                cell's box; among the cells the ray passes through whose box it hits, the one entered first answers.  No DDA;
  build_grid    the acceleration structure's arrays by plain loops;
  walk          a float64 DDA over that grid with the two first-hit rules: the carried candidate (what the product does) and the
                reference's early return at the first cell with any hit.
"""
import numpy as np


# ---- fixtures (generated, seed 7) -------------------------------------------------------------------------------------------------
_CUBE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], float)
_CUBE_FACES = [[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [1, 2, 6], [1, 6, 5],
               [0, 4, 7], [0, 7, 3]]


def terrain_fixture(seed=7, n=48, boxes=12):
    """48 x 48 height field over [-10,10]^2 plus 12 random boxes -> V [2497,3] f32, F [4752,3] i32, and three ray sets
    (o, d float32): 4 096 from above the terrain pointing down-ish, 2 048 from outside the grid (radius 25..40) aimed at the
    scene, 512 axis-aligned (two zero direction components)."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-10, 10, n + 1)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    Z = 0.8 * np.sin(0.6 * X) * np.cos(0.5 * Y) + 0.3 * rng.normal(size=X.shape) * 0.2
    V, F = [np.stack([X, Y, Z], -1).reshape(-1, 3)], []
    idx = lambda i, j: i * (n + 1) + j
    for i in range(n):
        for j in range(n):
            F += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    base = (n + 1) ** 2
    for _ in range(boxes):
        c = rng.uniform(-8, 8, 3)
        c[2] = rng.uniform(-0.5, 1)
        s = rng.uniform(0.5, 3, 3)
        V.append(_CUBE * s + c)
        F += [[a + base for a in f] for f in _CUBE_FACES]
        base += 8
    V = np.concatenate(V).astype(np.float32)
    F = np.array(F, np.int32)
    B = 4096
    o = np.stack([rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(1.5, 6, B)], -1).astype(np.float32)
    d = rng.normal(size=(B, 3))
    d[:, 2] -= 0.6
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = (o, d.astype(np.float32))
    B = 2048
    u = rng.normal(size=(B, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    oo = u * rng.uniform(25, 40, (B, 1))
    aim = np.stack([rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(-1, 2, B)], -1)
    dd = aim - oo
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    outside = (oo.astype(np.float32), dd.astype(np.float32))
    B = 512
    axis = rng.integers(0, 3, B)
    sign = rng.choice([-1.0, 1.0], B)
    da = np.zeros((B, 3))
    da[np.arange(B), axis] = sign
    oa = np.stack([rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(-1, 3, B)], -1)
    oa[np.arange(B), axis] = -sign * rng.uniform(0, 30, B)     # behind the scene along the axis: inside or outside the grid
    axial = (oa.astype(np.float32), da.astype(np.float32))
    return V, F, {"inside": inside, "outside": outside, "axial": axial}


def sloping_plane_fixture():
    """Two large triangles forming a SLOPING plane (their bounding box is the whole cube: registered in every cell, far from
    their surface) and a small box floating above it; rays from above aimed at the box.  -> V, F, (o, d), box top z."""
    P = np.array([[-10, -10, -4], [10, -10, -4], [10, 10, 4], [-10, 10, 4]], float)   # z = 0.4 y
    box = _CUBE * np.array([1.0, 1.0, 0.5]) + np.array([-0.5, -0.5, 2.0])            # top at z = 2.5, plane below it at z ~ 0
    V = np.concatenate([P, box]).astype(np.float32)
    F = np.array([[0, 1, 2], [0, 2, 3]] + [[a + 4 for a in f] for f in _CUBE_FACES], np.int32)
    rng = np.random.default_rng(11)
    B = 256
    o = np.stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(3.2, 3.9, B)], -1)
    aim = np.stack([rng.uniform(-0.4, 0.4, B), rng.uniform(-0.4, 0.4, B), np.full(B, 2.5)], -1)
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return V, F, (o.astype(np.float32), d.astype(np.float32)), 2.5


def look_at(eye, target, H, W, focal):
    """-> c2w [3,4] (columns: right, down, forward, eye), K [3,3] of a pinhole camera looking at `target` with z up."""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0, 0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]])
    return np.stack([right, down, fwd, eye], 1).astype(np.float32), K.astype(np.float32)


def camera_rays(c2w, K, H, W):
    """Rays of every pixel in row-major order, float32: d = R ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1), o = the eye."""
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    x = (px + 0.5 - K[0, 2]) / K[0, 0]
    y = (py + 0.5 - K[1, 2]) / K[1, 1]
    R = c2w[:, :3].astype(np.float64)
    d = x[..., None] * R[:, 0] + y[..., None] * R[:, 1] + R[:, 2]
    o = np.broadcast_to(c2w[:, 3].astype(np.float64), d.shape)
    return o.reshape(-1, 3).astype(np.float32), d.reshape(-1, 3).astype(np.float32)


def shell_fixture(half=12.0, n=8):
    """A closed cube shell [-half, half]^3, every side n x n quads (12 n^2 triangles): a mesh that surrounds a tile, so that every
    ray leaving the tile has a background."""
    ts = np.linspace(-half, half, n + 1)
    V, F = [], []
    for axis in range(3):
        for sgn in (-half, half):
            base = len(V)
            for a in ts:
                for b in ts:
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = sgn, a, b
                    V.append(p)
            for i in range(n):
                for j in range(n):
                    q = lambda u, v: base + u * (n + 1) + v
                    F += [[q(i, j), q(i + 1, j), q(i + 1, j + 1)], [q(i, j), q(i + 1, j + 1), q(i, j + 1)]]
    return np.array(V, np.float32), np.array(F, np.int32)


# ---- brute force --------------------------------------------------------------------------------------------------------------------
def _moller_trumbore(o, d, A, E1, E2):
    """o, d [b,1,3]; A, E1, E2 [1,F,3] float64 -> t, u, v, ok [b,F]."""
    p = np.cross(d, E2)
    det = (E1 * p).sum(-1)
    ok = np.abs(det) > 1e-12
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    tv = o - A
    u = (tv * p).sum(-1) * inv
    q = np.cross(tv, E1)
    v = (d * q).sum(-1) * inv
    t = (E2 * q).sum(-1) * inv
    return t, u, v, ok


def nearest_hit(o, d, V, F, chunk=256):
    """-> t64 [B] (0 = no hit) and grazing [B] bool: some face with 0 < t <= 1.001 t_hit + 1e-3 (any t > 0 for a miss) has
    a barycentric margin min(u, v, 1 - u - v) of absolute value below 1e-4: the ray passes that close to an edge, so
    float32 may decide the other way."""
    o, d, V = o.astype(np.float64), d.astype(np.float64), V.astype(np.float64)
    A, E1, E2 = V[F[:, 0]][None], (V[F[:, 1]] - V[F[:, 0]])[None], (V[F[:, 2]] - V[F[:, 0]])[None]
    best = np.zeros(len(o))
    grazing = np.zeros(len(o), bool)
    for s in range(0, len(o), chunk):
        t, u, v, ok = _moller_trumbore(o[s:s + chunk, None], d[s:s + chunk, None], A, E1, E2)
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)
        hit = ok & (m >= 0) & (t > 0)
        th = np.where(hit, t, np.inf).min(1)
        near = ok & (t > 0) & (t <= 1.001 * th[:, None] + 1e-3)
        grazing[s:s + chunk] = (near & (np.abs(m) < 1e-4)).any(1)
        best[s:s + chunk] = np.where(np.isfinite(th), th, 0.0)
    return best, grazing


# ---- the grid, by plain loops ---------------------------------------------------------------------------------------------------
def build_grid(V, F, log2dim):
    """The structure's arrays.  The registration arithmetic is float32, operation by operation as csrc/mesh.hip does it
    ((min - min_corner) / cell, truncated), so that a face lands in the same cells."""
    V = V.astype(np.float32)
    side = 1 << log2dim
    mn, mx = V.min(0), V.max(0)
    cell = np.float32((mx - mn).max() / np.float32(side))
    tri = V[F]                                     # [F,3,3]
    fmin, fmax = tri.min(1), tri.max(1)
    lo = np.clip(((fmin - mn) / cell).astype(np.int32), 0, side - 1)
    hi = np.clip(((fmax - mn) / cell).astype(np.int32), 0, side - 1)
    cells = {}
    for f in range(len(F)):
        for x in range(lo[f, 0], hi[f, 0] + 1):
            for y in range(lo[f, 1], hi[f, 1] + 1):
                for z in range(lo[f, 2], hi[f, 2] + 1):
                    cells.setdefault((x << (2 * log2dim)) | (y << log2dim) | z, []).append(f)
    order = sorted(cells)
    n_words = side ** 3 // 64
    bitmask = np.zeros(n_words, np.uint64)
    for n in order:
        bitmask[n >> 6] |= np.uint64(1) << np.uint64(n & 63)
    pop = np.array([bin(int(w)).count("1") for w in bitmask], np.int64)
    rank = (np.cumsum(pop) - pop).astype(np.uint32)
    start_num, cell_faces, cell_box = [], [], []
    for n in order:
        fs = cells[n]                               # ascending: faces were visited in order
        start_num.append((len(cell_faces), len(fs)))
        cell_faces += fs
        pts = V[F[fs]].reshape(-1, 3)
        cell_box.append(np.concatenate([pts.min(0), pts.max(0)]))
    return {"log2dim": log2dim, "side": side, "scene_info": np.concatenate([mn, [cell]]).astype(np.float32),
            "scene_bound": np.concatenate([mn, mx]).astype(np.float32), "cells": np.array(order, np.int64),
            "bitmask": bitmask, "rank": rank, "start_num": np.array(start_num, np.int32),
            "cell_faces": np.array(cell_faces, np.int32), "cell_box": np.array(cell_box, np.float32)}


def _slab(o, d, lo, hi):
    """Slab interval of rays o, d [...,3] with boxes lo, hi [...,3] (broadcast), clamped to [0, 1e5] -> t_in, t_out [N] (t_in > t_out: miss)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        a, b = (lo - o) * inv, (hi - o) * inv
    near, far = np.minimum(a, b), np.maximum(a, b)
    # a zero direction component: inside the slab -> (-inf, inf); outside -> an empty interval
    zero = d == 0
    inside = (o >= lo) & (o <= hi)
    near = np.where(zero, np.where(inside, -np.inf, np.inf), near)
    far = np.where(zero, np.where(inside, np.inf, -np.inf), far)
    t0, t1 = near.max(-1), far.min(-1)
    return np.maximum(t0, 0.0), np.minimum(t1, 1e5)


def first_enter(o, d, V, F, log2dim, grid=None):
    """-> [B] float64 by the definition: cells the ray passes through (t_in < t_out) whose cell_box it hits; the one with the
    smallest cell entry gives its box entry (clamped at 0, so 0 doubles as "nothing")."""
    g = grid or build_grid(V, F, log2dim)
    L, mask = log2dim, (1 << log2dim) - 1
    n = g["cells"]
    ijk = np.stack([n >> (2 * L), (n >> L) & mask, n & mask], -1).astype(np.float64)
    mn, cell = g["scene_info"][:3].astype(np.float64), float(g["scene_info"][3])
    lo, hi = mn + ijk * cell, mn + (ijk + 1) * cell
    blo, bhi = g["cell_box"][:, :3].astype(np.float64), g["cell_box"][:, 3:].astype(np.float64)
    out = np.zeros(len(o))
    o, d = o.astype(np.float64), d.astype(np.float64)
    for s in range(0, len(o), 64):
        oo, dd = o[s:s + 64, None], d[s:s + 64, None]
        tin, tout = _slab(oo, dd, lo[None], hi[None])
        bin_, bout = _slab(oo, dd, blo[None], bhi[None])
        ok = (tin < tout) & (bin_ <= bout)
        j = np.where(ok, tin, np.inf).argmin(1)
        r = np.arange(len(j))
        out[s:s + 64] = np.where(ok[r, j], bin_[r, j], 0.0)
    return out


# ---- a float64 DDA over the grid with both first-hit rules -----------------------------------------------------------------
def walk(o, d, V, F, grid):
    """-> (carried, early, enter) [B] float64: the nearest hit with the candidate carried across cells until it is not beyond
    the current cell's exit; the reference's rule (return at the first cell in which any registered face is hit, wherever
    that hit lies: fastMesh_kernel.cu:284-290); and first_enter by walking (the first occupied cell in walk order whose box the
    ray hits)."""
    V = V.astype(np.float64)
    A, E1, E2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    L, side = grid["log2dim"], grid["side"]
    mn, cell = grid["scene_info"][:3].astype(np.float64), float(grid["scene_info"][3])
    lists = {int(n): grid["cell_faces"][s:s + c] for n, (s, c) in zip(grid["cells"], grid["start_num"])}
    boxes = {int(n): b.astype(np.float64) for n, b in zip(grid["cells"], grid["cell_box"])}
    carried, early, enter = np.zeros(len(o)), np.zeros(len(o)), np.zeros(len(o))
    for i in range(len(o)):
        oo, dd = o[i].astype(np.float64), d[i].astype(np.float64)
        tin, tout = _slab(oo, dd, mn[None], (mn + side * cell)[None])
        if tin[0] > tout[0]:
            continue
        p = oo + tin[0] * dd - mn
        c = np.clip((p / cell).astype(int), 0, side - 1)
        step = np.where(dd >= 0, 1, -1)
        with np.errstate(divide="ignore", invalid="ignore"):
            tmax = np.where(dd != 0, ((c + (step > 0)) * cell - p) / dd, np.inf)
            tmax = np.maximum(tmax, 0) + tin[0]
            tdelta = np.where(dd != 0, np.abs(cell / dd), np.inf)
        best, first, ent, settled = np.inf, None, None, False
        while np.all(c >= 0) and np.all(c < side):
            k = int(np.argmin(tmax))
            n = (int(c[0]) << (2 * L)) | (int(c[1]) << L) | int(c[2])
            fs = lists.get(n)
            if fs is not None and ent is None:
                bin_, bout = _slab(oo, dd, boxes[n][None, :3], boxes[n][None, 3:])
                if bin_[0] <= bout[0]:
                    ent = bin_[0]
            if fs is not None and not settled:
                t, u, v, ok = _moller_trumbore(oo[None, None], dd[None, None], A[fs][None], E1[fs][None], E2[fs][None])
                hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
                th = np.where(hit, t, np.inf).min()
                if first is None and np.isfinite(th):
                    first = th
                best = min(best, th)
            settled = settled or best <= tmax[k]      # nothing in a later cell can be nearer
            if settled and ent is not None:
                break
            tmax[k] += tdelta[k]
            c[k] += step[k]
        carried[i] = best if np.isfinite(best) else 0.0
        early[i] = first or 0.0
        enter[i] = ent or 0.0
    return carried, early, enter


# ---- the composite methods' formulas, on given depths -----------------------------------------------------------------------------
def box_bounds(o, d, center, size):
    """Slab interval of each ray with the box (center, full side lengths), clamped to [0, 1e5]; (-1, -1) for a miss."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    out = np.full((len(o), 2), -1.0)
    lo, hi = (np.asarray(center, float) - np.asarray(size, float) / 2)[None], (np.asarray(center, float) + np.asarray(size, float) / 2)[None]
    for i in range(len(o)):
        tin, tout = _slab(o[i], d[i], lo, hi)
        if tin[0] <= tout[0]:
            out[i] = tin[0], tout[0]
    return out
