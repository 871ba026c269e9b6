"""Yardstick and case list of the scene mesh (csrc/isosurface.hip's scene source, meshing.extract_scene_mesh; test infrastructure,
CPU only: numpy / torch / oracle.oracle, no GPU import).

The definition is include/scanerf_hip.h's (scanerf_isosurface_count_tiles).  Per lattice point and tile everything that selects is
pinned in float32 by the kernel's expressions (numpy float32: no product feeds a sum unrounded),

    wp = box_corner + float(i) (box_size / n);  pts = (wp - corner_b) / size_b;  listed iff 0 <= pts <= 1 on the three axes;
    loc = clamp(int(pts 2^log2dim_b)) -> the occupancy cell;  x = 2 pts - 1 -> the hash cells (gradient_reference64.pinned_cells),

and what follows -- the density normals_reference.sigma_normals(x, table_b, res_b, unpack_blob(params_b), ones(32), dtype), the weight
w_b = xz_weight((0.5 - |pts - 0.5|) size_b), W = sum_b w_b over the listed tiles, the blend sum_b w_b sigma_b / W over the contributing
ones in ascending tile index -- runs in a dtype of the caller's choice: float64 = the reference, float32 = the yardstick for how much
rounding the problem allows.  The judgement is surface_nets_reference's (ambiguity band, CAP, MIN_JUDGED, judge_mesh, K): none of its
figures is re-fitted here."""
import collections
import functools

import numpy as np
import torch

import normals_reference as NR
import render_scenes as RS
from oracle import oracle as O
from surface_nets_reference import (CAP, K, MIN_JUDGED, ambiguous_points, canonical, judge_mesh, judged_cells,  # noqa: F401
                                    surface_nets, topology)

f32 = np.float32
F64, F32 = torch.float64, torch.float32
CENTRE = 4               # the centre tile of G9 (ix = 1, iz = 1)
BRICK = 8

SceneCase = collections.namedtuple("SceneCase", "scene n box")   # box: "bound", "grown" (25 % larger), "cut" (through tiles)


def case_id(c):
    return f"{c.scene}-n{'x'.join(map(str, c.n))}-{c.box}"


# every scene on (16,16,16) over its bound; the ragged, thin, grown and cutting lattices on the scenes that have tile faces inside
CASES = [SceneCase(s, (16, 16, 16), "bound") for s in ("G9", "STACK3", "STACK6", "G9-hole", "G9-zero", "single")] + [
    SceneCase("G9", (37, 5, 29), "bound"),        # thinner than a brick on y, no axis a multiple of 8: bricks straddle tile faces
    SceneCase("G9", (70, 1, 9), "bound"),
    SceneCase("G9", (88, 5, 88), "grown"),        # 8.8 cells of margin: whole bricks outside every tile
    SceneCase("G9", (19, 7, 21), "cut"),          # the box cuts through tiles
    SceneCase("STACK6", (11, 13, 9), "cut"),
    SceneCase("G65", (19, 5, 45), "bound"),       # 65 tiles: the kernel tests tile boxes 64 at a time, tile 64 is alone in the second round
    SceneCase("G9-hole", (72, 4, 72), "bound"),   # a brick of 1.11 inside the cleared tile's own 2 x 2: reached, nothing contributes
]


@functools.lru_cache(maxsize=None)
def scene(name):
    """Scene arrays (render_scenes' dict) of G9 / STACK3 / STACK6 / G65 and of the variants of G9: "G9-hole" (the centre tile's occupancy
    cleared: its neighbours' margins must close the hole), "G9-zero" (the centre tile's table zeroed), "single" (the centre tile
    alone).  Built once per process; callers leave them unchanged."""
    if name in ("G9", "STACK3", "STACK6", "G65"):
        return RS.named(name)[0]
    sc = dict(RS.named("G9")[0])
    lo = int(sc["starts"][CENTRE])
    hi = lo + int(np.prod(2 ** sc["l2d"][CENTRE].astype(np.int64)))
    if name == "G9-hole":
        sc["occ"] = sc["occ"].copy()
        sc["occ"][lo:hi] = False
    elif name == "G9-zero":
        sc["tables"] = sc["tables"].copy()
        sc["tables"][CENTRE] = 0
    else:
        assert name == "single"
        one = slice(CENTRE, CENTRE + 1)
        sc.update(corners=sc["corners"][one], sizes=sc["sizes"][one], l2d=sc["l2d"][one], starts=np.zeros(1, np.int64),
                  occ=sc["occ"][lo:hi], tables=sc["tables"][one], params=sc["params"][one], res=sc["res"][one])
    return sc


def scene_bound(sc):
    lo = np.asarray(sc["corners"], f32).min(0)
    hi = (np.asarray(sc["corners"], f32) + np.asarray(sc["sizes"], f32)).max(0)
    return lo, (hi - lo).astype(f32)


def case_box(c):
    """(corner, size) float32 [3] of the case's world box."""
    lo, size = scene_bound(scene(c.scene))
    if c.box == "grown":
        return (lo - f32(0.125) * size).astype(f32), (f32(1.25) * size).astype(f32)
    if c.box == "cut":   # starts inside the first tile and ends inside the last, off every tile face and off the lattice of the bound
        return (lo + f32(0.21) * size).astype(f32), (f32(0.63) * size).astype(f32)
    assert c.box == "bound"
    return lo, size


def _xz_weight(dx, dz, zero):
    return np.where((dx != 0) & (dz != 0), dx * dz, np.where(dx != 0, dx, np.where(dz != 0, dz, zero)))


def pinned_tiles(sc, corner, size, n):
    """The float32-pinned part, per tile b: {"pt": three per-axis arrays [n_k + 1] f32, "listed", "run" [nx+1,ny+1,nz+1] bool,
    "x" [M,3] f32 contracted positions of the contributing points (C order)}; also "wp"."""
    corner, size = np.asarray(corner, f32), np.asarray(size, f32)
    wp = [corner[k] + np.arange(n[k] + 1, dtype=f32) * (size[k] / f32(n[k])) for k in range(3)]
    assert all(a.dtype == f32 for a in wp)
    cn, sz = np.asarray(sc["corners"], f32), np.asarray(sc["sizes"], f32)
    occ, starts, l2d = np.asarray(sc["occ"]).astype(bool), np.asarray(sc["starts"], np.int64), np.asarray(sc["l2d"], np.int64)
    tiles = []
    for b in range(cn.shape[0]):
        pt = [((wp[k] - cn[b, k]) / sz[b, k]).astype(f32) for k in range(3)]
        inb = [(p >= 0) & (p <= 1) for p in pt]
        listed = inb[0][:, None, None] & inb[1][None, :, None] & inb[2][None, None, :]
        loc = []
        for k in range(3):
            r = 1 << int(l2d[b, k])
            loc.append(np.clip((pt[k] * f32(r)).astype(f32).astype(np.int64), 0, r - 1))
        off = (loc[0][:, None, None] << int(l2d[b, 1] + l2d[b, 2])) | (loc[1][None, :, None] << int(l2d[b, 2])) | loc[2][None, None, :]
        run = listed & occ[starts[b] + off]
        idx = np.argwhere(run)
        x = np.stack([(f32(2.0) * pt[k] - f32(1.0))[idx[:, k]] for k in range(3)], 1).astype(f32) if len(idx) else np.zeros((0, 3), f32)
        tiles.append({"pt": pt, "listed": listed, "run": run, "x": x})
    return {"wp": wp, "tiles": tiles}


def tile_sigma(sc, b, x, dtype, chunk=4096):
    """Density of tile b at contracted points x [M,3] float32 in `dtype` -> float64 numpy [M]."""
    sd = O.unpack_blob(torch.from_numpy(np.asarray(sc["params"], f32)[b]))
    ones, A = torch.ones(32, dtype=F32), np.ones(3, f32)
    out = [NR.sigma_normals(x[i:i + chunk], A, torch.from_numpy(sc["tables"][b]), np.asarray(sc["res"], np.int32)[b], sd, ones,
                            dtype)["sigma"].to(F64).numpy() for i in range(0, len(x), chunk)]
    return np.concatenate(out) if out else np.zeros(0)


def blend(sc, pin, dtype):
    """The blended field behind the pinned part, in numpy `dtype` (float64 / float32; the density in the matching torch dtype) ->
    {"v", "W" [points] in dtype, "listed", "run" [points] int: how many tiles list / contribute}."""
    tdt = F64 if dtype == np.float64 else F32
    shape = pin["tiles"][0]["listed"].shape
    sz = np.asarray(sc["sizes"], f32)
    num, W = np.zeros(shape, dtype), np.zeros(shape, dtype)
    n_listed, n_run = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    for b, t in enumerate(pin["tiles"]):
        dis = [((dtype(0.5) - np.abs(p.astype(dtype) - dtype(0.5))) * dtype(sz[b, k])).astype(dtype) for k, p in enumerate(t["pt"])]
        w2 = _xz_weight(dis[0][:, None], dis[2][None, :], dtype(0)).astype(dtype)
        w = np.broadcast_to(w2[:, None, :], shape)
        W = np.where(t["listed"], W + w, W).astype(dtype)
        n_listed += t["listed"]
        n_run += t["run"]
        if t["run"].any():
            sigma = tile_sigma(sc, b, t["x"], tdt).astype(dtype)
            num[t["run"]] = num[t["run"]] + (w[t["run"]] * sigma).astype(dtype)
    inv = np.where(W > 0, dtype(1) / np.where(W > 0, W, dtype(1)), dtype(1)).astype(dtype)
    return {"v": (num * inv).astype(dtype), "W": W, "listed": n_listed, "run": n_run}


def level_between(v64, live, quantile=0.5):
    """Midway between two adjacent sorted lattice values (as float32) near the quantile of the non-zero ones."""
    vals = np.sort(np.unique(v64[live].astype(f32)))
    i = min(max(int(quantile * len(vals)), 0), len(vals) - 2)
    return float(f32((np.float64(vals[i]) + np.float64(vals[i + 1])) / 2))


@functools.lru_cache(maxsize=None)
def reference(c):
    """(scene arrays, corner, size, float64 blend, float32 blend, live [points] bool, level) of a case -- computed once per process,
    shared, never written to."""
    sc = scene(c.scene)
    corner, size = case_box(c)
    pin = pinned_tiles(sc, corner, size, c.n)
    b64, b32 = blend(sc, pin, np.float64), blend(sc, pin, np.float32)
    live = b64["run"] > 0
    level = level_between(b64["v"], live)
    for d in (b64, b32):
        for a in d.values():
            a.setflags(write=False)
    return sc, corner, size, b64, b32, live, level


def judged(c):
    """(ambiguous points, judged cells) of a case: surface_nets_reference's band around the level."""
    _, _, _, b64, b32, live, level = reference(c)
    amb = ambiguous_points(b64["v"], b32["v"].astype(np.float64), live, level)
    return amb, judged_cells(amb)


def brick_has(mask):
    """[bx,by,bz] bool: the bricks (8^3 cells = 9^3 points, sharing their border points) that hold a point of mask [points]."""
    n = tuple(s - 1 for s in mask.shape)
    nb = tuple((m + BRICK - 1) // BRICK for m in n)
    out = np.zeros(nb, bool)
    for bx in range(nb[0]):
        for by in range(nb[1]):
            for bz in range(nb[2]):
                out[bx, by, bz] = mask[bx * BRICK:bx * BRICK + BRICK + 1, by * BRICK:by * BRICK + BRICK + 1, bz * BRICK:bz * BRICK + BRICK + 1].any()
    return out


# ------------------------------------------------------------------------------------------------------------------- the blob scene
BLOB_CENTRE, BLOB_RADIUS, BLOB_N = (3.5, 0.0, 3.5), 1.4, (40, 16, 40)


@functools.lru_cache(maxsize=None)
def blob_scene():
    """G9's tiles with zeroed tables (every tile's density is one constant > 0) and occupancies that hold a ball around the four-tile
    corner (3.5, 0, 3.5): the blended field is one closed blob that four tiles share, cut by a face of each of them."""
    sc = dict(RS.named("G9")[0])
    sc["tables"] = np.zeros_like(sc["tables"])
    occ = np.zeros_like(np.asarray(sc["occ"]).astype(bool))
    for b in range(sc["corners"].shape[0]):
        G = 2 ** sc["l2d"][b].astype(np.int64)
        lo = [sc["corners"][b][k] + np.arange(G[k]) * (sc["sizes"][b][k] / G[k]) for k in range(3)]
        d2 = 0.0
        for k, ax in enumerate(np.ix_(*lo)):   # distance of the ball's centre to the cell [lo, lo + h]
            h = sc["sizes"][b][k] / G[k]
            d2 = d2 + np.maximum(np.maximum(ax - BLOB_CENTRE[k], BLOB_CENTRE[k] - (ax + h)), 0.0) ** 2
        occ[int(sc["starts"][b]):int(sc["starts"][b]) + int(G.prod())] = (d2 <= BLOB_RADIUS ** 2).reshape(-1)
    sc["occ"] = occ
    return sc
