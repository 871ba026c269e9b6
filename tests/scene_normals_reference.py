"""Yardstick and point lists of the blended density's gradient (csrc/scene_normals.hip, meshing.scene_sigma_normals_points; test
infrastructure, CPU only: numpy / torch / oracle.oracle, no GPU import).

The definition is include/scanerf_hip.h's (scanerf_scene_sigma_normals_points).  Per point and tile everything that selects is pinned
in float32 by the kernel's expressions (numpy float32: no product feeds a sum unrounded):

    pt = (p - corner_b) / size_b;  listed iff 0 <= pt <= 1 on the three axes;  the branch of xz_weight (dis_x != 0, dis_z != 0) and the
    sides s_c = sign(0.5 - pt_c);  loc = clamp(int(pt 2^log2dim_b)) -> the occupancy cell;  x = 2 pt - 1 -> the hash cells
    (gradient_reference64.pinned_cells),

and what follows -- sigma_b, grad sigma_b and its conditioning scale cond_b (normals_reference.evaluate_cells with A = 2 / size_b), the
weight w_b, its gradient gw_b, and the sums W, C, num, A, B in ascending tile index,

    v = num inv(W);   g = ((A + B) - v C) inv(W);   n = -g / (|g| + 1e-8);   zeros where no tile contributes

-- runs in a dtype of the caller's choice: float64 = the reference, float32 = the yardstick for how much rounding the problem allows.
The conditioning scale per point and component,

    cond_k = (sum_b w_b cond_b,k + sum_b sigma_b |gw_b,k| + |v| sum_b |gw_b,k|) inv(W),

carries the weight terms: a point where they cancel is not held to a relative bound on the cancelled sum.

Judgement: g by normals_reference.judge_samples' rule over that scale, K = normals_reference.K and FLOOR = 2^-24 as the project has
them (not re-fitted), no point left out.  n by the same bound on |n - n64| at the points where |g64| > 100 K (the yardstick's error of
g): the unit normal of a near-zero gradient has no stable direction.  Points no tile contributes to have g = n = 0 exactly in every
dtype: they are judged with g (error 0), and left out of the SHARE below, which is taken among the contributing points and capped at
N_CAP on the reference alone (per list; the EDGES, a handful of points, pooled with their scene's random points)."""
import functools

import numpy as np
import torch

import normals_reference as NR
import scene_mesh_reference as SM
from gradient_reference64 import pinned_cells
from oracle import oracle as O

f32 = np.float32
F64, F32 = torch.float64, torch.float32
K, FLOOR = NR.K, NR.FLOOR
N_CAP = 0.02               # the largest share of contributing points whose unit normal is not judged
SCENES = ("G9", "STACK3", "STACK6", "G9-hole", "single", "G65")
LATTICE_CASES = [c for c in SM.CASES if (c.n == (16, 16, 16) and c.box == "bound" and c.scene in SCENES) or c.scene == "G65"]
MESH_CASES = [c for c in SM.CASES if (c.scene, c.n) in (("G9", (37, 5, 29)), ("STACK6", (11, 13, 9)))]
N_RANDOM = 1000
PREFIXES = (0, 1, 63, 64, 65)
BOTH, ONLY_X, ONLY_Z, NEITHER = 0, 1, 2, 3   # the branch xz_weight takes


# ----------------------------------------------------------------------------------------------------------------- the pinned part
def pinned(sc, p):
    """p [N,3] float32 world points -> per tile {"pt" [N,3] f32, "listed", "run" [N] bool, "branch" [N] int, "side" [N,3] f32,
    "x" [M,3] f32 (contracted positions of the contributing points), "cells", "t": pinned_cells of x}."""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    cn, sz = np.asarray(sc["corners"], f32), np.asarray(sc["sizes"], f32)
    occ, starts, l2d = np.asarray(sc["occ"]).astype(bool), np.asarray(sc["starts"], np.int64), np.asarray(sc["l2d"], np.int64)
    res = np.asarray(sc["res"], np.int32)
    half = f32(0.5)
    tiles = []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(cn.shape[0]):
            pt = ((p - cn[b]) / sz[b]).astype(f32)
            listed = ((pt >= 0) & (pt <= 1)).all(1)
            dis = ((half - np.abs(pt - half)) * sz[b]).astype(f32)
            nx, nz = dis[:, 0] != 0, dis[:, 2] != 0
            branch = np.where(nx & nz, BOTH, np.where(nx, ONLY_X, np.where(nz, ONLY_Z, NEITHER)))
            side = np.where(pt < half, f32(1), np.where(pt > half, f32(-1), f32(0))).astype(f32)
            r = (1 << l2d[b]).astype(np.int64)
            cc = (pt * r.astype(f32)).astype(f32)
            loc = np.clip(np.where(np.isfinite(cc), cc, 0).astype(np.int64), 0, r - 1)
            off = (loc[:, 0] << int(l2d[b, 1] + l2d[b, 2])) | (loc[:, 1] << int(l2d[b, 2])) | loc[:, 2]
            run = listed & occ[starts[b] + off]
            x = (f32(2.0) * pt[run] - f32(1.0)).astype(f32)
            cells, t = pinned_cells(x, res[b]) if len(x) else (np.zeros((0, 16, 3), np.int32), np.zeros((0, 16, 3), f32))
            tiles.append({"pt": pt, "listed": listed, "run": run, "branch": branch, "side": side, "x": x, "cells": cells, "t": t})
    return {"p": p, "tiles": tiles}


def _tile_terms(sc, b, tile, dtype, dt=None, chunk=4096):
    """(sigma [M], g [M,3], cond [M,3]) float64 numpy of tile b at its contributing points, evaluated in torch `dtype`; dt [M,16,3]:
    float64 displacement of the cell offsets (a finite difference inside the pinned cells)."""
    M = len(tile["x"])
    if M == 0:
        return np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3))
    sd = O.unpack_blob(torch.from_numpy(np.asarray(sc["params"], f32)[b]))
    A = (f32(2.0) / np.asarray(sc["sizes"], f32)[b]).astype(f32)
    res = np.asarray(sc["res"], np.int32)[b]
    ones = torch.ones(32, dtype=F32)
    out = {"sigma": [], "g": [], "cond": []}
    for i in range(0, M, chunk):
        t = torch.from_numpy(tile["t"][i:i + chunk])
        if dt is not None:
            t = t.to(F64) + torch.from_numpy(dt[i:i + chunk])
        r = NR.evaluate_cells(tile["cells"][i:i + chunk], t, A, torch.from_numpy(sc["tables"][b]), res, sd, ones, dtype)
        for k in out:
            out[k].append(r[k].to(F64).numpy())
    return tuple(np.concatenate(out[k]) for k in ("sigma", "g", "cond"))


def evaluate(sc, pin, dtype, shift=None):
    """The definition behind the pinned part in numpy `dtype` (float64 / float32; the density terms in the matching torch dtype) ->
    {"v" [N], "g", "n", "cond" [N,3], "W" [N] in dtype, "listed", "run" [N] int (how many tiles list / contribute)}.
    shift [N,3] float64 (float64 only): the points moved by it in the world with every selection left pinned -- pt and the cell offsets
    move, membership, branch, sides, occupancy cell and hash cells do not (a finite difference of the float64 field)."""
    assert shift is None or dtype == np.float64
    tdt = F64 if dtype == np.float64 else F32
    N = pin["p"].shape[0]
    sz = np.asarray(sc["sizes"], f32)
    res = np.asarray(sc["res"], np.int32)
    W, num, csum = np.zeros(N, dtype), np.zeros(N, dtype), np.zeros((N, 3), dtype)
    A, B, C, absgw = (np.zeros((N, 3), dtype) for _ in range(4))
    n_listed, n_run = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for b, t in enumerate(pin["tiles"]):
        if not t["listed"].any():
            continue
        size = sz[b].astype(dtype)
        pt = t["pt"].astype(dtype)
        dt = None
        if shift is not None:
            pt = pt + shift / size
            # d t_l,k / d p_k = (2 / size_k) (res_l,k - 1) / 4
            step = (2.0 / size)[None, :] * (res[b].astype(np.float64) - 1) / 4            # [16,3]
            dt = shift[t["run"]][:, None, :] * step[None, :, :]
        dis = ((dtype(0.5) - np.abs(pt - dtype(0.5))) * size).astype(dtype)
        dx, dz, br, side = dis[:, 0], dis[:, 2], t["branch"], t["side"].astype(dtype)
        zero = dtype(0)
        w = np.where(br == BOTH, dx * dz, np.where(br == ONLY_X, dx, np.where(br == ONLY_Z, dz, zero))).astype(dtype)
        gw = np.zeros((N, 3), dtype)
        gw[:, 0] = np.where(br == BOTH, side[:, 0] * dz, np.where(br == ONLY_X, side[:, 0], zero))
        gw[:, 2] = np.where(br == BOTH, side[:, 2] * dx, np.where(br == ONLY_Z, side[:, 2], zero))
        L = t["listed"]
        W = np.where(L, W + w, W).astype(dtype)
        C = np.where(L[:, None], C + gw, C).astype(dtype)
        absgw = np.where(L[:, None], absgw + np.abs(gw), absgw).astype(dtype)
        n_listed += L
        run = t["run"]
        n_run += run
        if not run.any():
            continue
        sigma, gs, cond = (a.astype(dtype) for a in _tile_terms(sc, b, t, tdt, dt))
        num[run] = num[run] + (w[run] * sigma).astype(dtype)
        A[run] = A[run] + (w[run, None] * gs).astype(dtype)
        B[run] = B[run] + (sigma[:, None] * gw[run]).astype(dtype)
        csum[run] = csum[run] + w[run, None] * cond + sigma[:, None] * np.abs(gw[run])
    inv = np.where(W > 0, dtype(1) / np.where(W > 0, W, dtype(1)), dtype(1)).astype(dtype)
    v = (num * inv).astype(dtype)
    g = (((A + B) - v[:, None] * C) * inv[:, None]).astype(dtype)
    q = g * g
    n = (g * (dtype(-1) / (np.sqrt((q[:, 0] + q[:, 1]) + q[:, 2]) + dtype(1e-8)))[:, None]).astype(dtype)
    cond = ((csum + np.abs(v)[:, None] * absgw) * inv[:, None]).astype(dtype)
    keep = n_run > 0
    z = dtype(0)
    return {"v": np.where(keep, v, z), "g": np.where(keep[:, None], g, z), "n": np.where(keep[:, None], n, z),
            "cond": np.where(keep[:, None], cond, z), "W": W, "listed": n_listed, "run": n_run}


def _freeze(*dicts):
    for d in dicts:
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


def reference_at(sc, p):
    """(float64 result, float32 result) at world points p [N,3] float32."""
    pin = pinned(sc, p)
    r64, r32 = evaluate(sc, pin, np.float64), evaluate(sc, pin, np.float32)
    _freeze(r64, r32)
    return r64, r32


# ----------------------------------------------------------------------------------------------------------------- the point lists
def lattice_points(c):
    """(a) the lattice points of a scene_mesh_reference case, as pinned_tiles forms them (C order) -> [P,3] float32."""
    corner, size = SM.case_box(c)
    wp = SM.pinned_tiles(SM.scene(c.scene), corner, size, c.n)["wp"]
    return np.stack(np.meshgrid(*wp, indexing="ij"), -1).reshape(-1, 3).astype(f32)


def random_points(name):
    """(b) N_RANDOM uniform points in a box 10 % larger than the scene's bound -> [N,3] float32."""
    lo, size = SM.scene_bound(SM.scene(name))
    rng = np.random.default_rng(1600 + SCENES.index(name))
    u = rng.uniform(-0.05, 1.05, (N_RANDOM, 3))
    return (lo.astype(np.float64) + u * size.astype(np.float64)).astype(f32)


def _dyadic_candidates(xs, ys, zs):
    return np.stack(np.meshgrid(f32(xs), f32(ys), f32(zs), indexing="ij"), -1).reshape(-1, 3).astype(f32)


def _first(name, cand, cond):
    """The first candidate point of scene `name` whose pinned part meets cond(listed count, run count, tiles, index)."""
    pin = pinned(SM.scene(name), cand)
    n_listed = sum(t["listed"].astype(int) for t in pin["tiles"])
    n_run = sum(t["run"].astype(int) for t in pin["tiles"])
    for i in range(len(cand)):
        if cond(int(n_listed[i]), int(n_run[i]), pin["tiles"], i):
            return cand[i]
    raise AssertionError(f"no candidate of {name} meets the condition")


@functools.lru_cache(maxsize=None)
def edges():
    """(c) name -> (scene, point [3] float32): every coordinate a small dyadic rational (exact in float32, as are the tile corners and
    sizes of G9: tile (ix, iz) = [3 ix, 3 ix + 4] x [-2, 2] x [3 iz, 3 iz + 4], index 3 ix + iz).  Where the condition asks for a
    contributing tile the remaining coordinates are searched on a dyadic grid for the first point that has one."""
    ys = np.arange(-1.75, 2.0, 0.5)
    inner = np.arange(0.25, 3.0, 0.25)        # inside tile (0, .) or (., 0) alone along that axis
    E = {}
    E["pt_x == 0.5 in a single tile"] = ("G9", _first("G9", _dyadic_candidates([2.0], ys, inner), lambda l, r, t, i: l == 1 and r == 1))
    E["interior face x == 3"] = ("G9", _first("G9", _dyadic_candidates([3.0], ys, inner), lambda l, r, t, i: l == 2 and t[3]["run"][i]))
    E["two faces x == 3, z == 3"] = ("G9", _first("G9", _dyadic_candidates([3.0], ys, [3.0]), lambda l, r, t, i: l == 4 and r >= 1))
    E["four-tile corner"] = ("G9", f32([3.5, 0.0, 3.5]))
    E["outer edge x == 0, z == 0"] = ("G9", _first("G9", _dyadic_candidates([0.0], ys, [0.0]), lambda l, r, t, i: l == 1 and r == 1))
    E["outside every tile"] = ("G9", f32([11.0, 0.0, 5.0]))
    E["y outside [-2, 2]"] = ("G9", f32([5.0, 2.5, 5.0]))
    margin = np.arange(3.125, 4.0, 0.25)      # the centre tile's margin with tile (0, 1): x in [3, 4], z in (4, 6)
    E["hole: the centre lists, a neighbour contributes"] = (
        "G9-hole", _first("G9-hole", _dyadic_candidates(margin, ys, np.arange(4.25, 6.0, 0.25)),
                          lambda l, r, t, i: l == 2 and t[SM.CENTRE]["listed"][i] and not t[SM.CENTRE]["run"][i] and t[1]["run"][i]))
    E["hole: a second one"] = (
        "G9-hole", _first("G9-hole", _dyadic_candidates(np.arange(4.25, 6.0, 0.25), ys, margin),
                          lambda l, r, t, i: l == 2 and t[SM.CENTRE]["listed"][i] and not t[SM.CENTRE]["run"][i] and t[3]["run"][i]))
    E["listed, none contributes"] = ("G9", _first("G9", _dyadic_candidates(margin, ys, margin), lambda l, r, t, i: l == 4 and r == 0))
    return E


def edge_points(name):
    """The EDGES entries of one scene -> (names, [n,3] float32)."""
    names = [k for k, (s, _) in edges().items() if s == name]
    return names, np.stack([edges()[k][1] for k in names]).astype(f32)


@functools.lru_cache(maxsize=None)
def lattice_reference(c):
    """(points, float64 result, float32 result) of list (a) for a case: computed once per process, shared, never written to."""
    p = lattice_points(c)
    p.setflags(write=False)
    return (p,) + reference_at(SM.scene(c.scene), p)


@functools.lru_cache(maxsize=None)
def random_reference(name):
    p = random_points(name)
    p.setflags(write=False)
    return (p,) + reference_at(SM.scene(name), p)


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    names, p = edge_points(name)
    return (names, p) + reference_at(SM.scene(name), p)


# ----------------------------------------------------------------------------------------------------------------- judgement
def normal_judged(r64, r32, k=K):
    """[N] bool: the points whose unit normal is judged -- |g64| > 100 k_max (the yardstick's error of g, at least FLOOR |cond|)."""
    yard = np.maximum(np.linalg.norm(r32["g"].astype(np.float64) - r64["g"], axis=1), FLOOR * np.linalg.norm(r64["cond"], axis=1))
    return (r64["run"] > 0) & (np.linalg.norm(r64["g"], axis=1) > 100.0 * k[1] * yard)


def left_out_share(r64, r32, k=K):
    """The share of the CONTRIBUTING points whose unit normal is not judged (reference alone)."""
    contributing = r64["run"] > 0
    return 0.0 if not contributing.any() else 1.0 - normal_judged(r64, r32, k).sum() / contributing.sum()


def judge_points(name, got_g, got_n, r64, r32, k=K, cap=True):
    """got_g, got_n [N,3] against float64 -> list of violations (empty: passes).  Prints every figure before anything binds.
    cap=False: the share of unjudged normals is stated, not capped -- for the EDGES alone, a handful of points of which one has
    W == 0 and g == 0 on purpose; their share is capped pooled with the scene's random points (test_scene_normals_cpu.py)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    N = r64["g"].shape[0]
    only = ("median", "p99", "max", "pooled") if N >= 16 else ("max", "pooled")
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    got_g, got_n = to_np(got_g), to_np(got_n)
    bad = NR.judge(name + " grad", T(got_g), T(r64["g"]), T(r32["g"]), k, scale=T(r64["cond"]).norm(dim=1), only=only, floor=FLOOR)
    idle = r64["run"] == 0
    if idle.any() and (np.any(got_g[idle] != 0) or np.any(got_n[idle] != 0)):
        bad.append(f"{name}: a point no tile contributes to is not zero")
    m = normal_judged(r64, r32, k)
    share = left_out_share(r64, r32, k)
    print(f"{name} normal: {int(m.sum())} of {int((r64['run'] > 0).sum())} contributing points judged (share left out {share:.4f})")
    if cap and share > N_CAP:
        bad.append(f"{name}: {share:.4f} of the contributing points have no judged normal (cap {N_CAP})")
    if m.any():
        only_n = ("median", "p99", "max", "pooled") if int(m.sum()) >= 16 else ("max", "pooled")
        bad += NR.judge(name + " normal", T(got_n[m]), T(r64["n"][m]), T(r32["n"][m]), k, only=only_n, floor=FLOOR)
    return bad
