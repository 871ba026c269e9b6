"""Yardstick and case list of the multi-tile renderer's normal maps (csrc/render_normals_tiles.hip, renderer.TileSetRenderer
normals=True; test infrastructure, CPU only: numpy / torch / oracle.oracle, no GPU import).

The definition is include/scanerf_hip.h's (scanerf_pts_normals / scanerf_accumulate_normal).  Per slot everything up to the cell is
pinned in float32 by the expressions pts_inference uses (numpy float32: no product feeds a sum unrounded),

    pts = (o + z d - corner_b) / size_b;  dis = (0.5 - |pts - 0.5|) size_b;  w_b = xz_weight(dis.x, dis.z);
    loc = clamp(int(pts 2^log2dim_b), 0, 2^log2dim_b - 1) -> the occupancy cell;  p01 = pts / 2 + 0.25;
    v = p01 (res - 1), i0 = int(v), t = v - i0 per level,

and what follows -- normals_reference.evaluate_cells(i0, t, 2 / size_b, table_b, res_b, unpack_blob(params_b), ones(32), dtype), the
opacity pa_b = 1 - exp(-sigma_b dist |d|), the blend sum_b w_b pa_b n_b / W and the per-ray accumulation -- runs in a dtype of the
caller's choice: float64 = the reference, float32 = the yardstick for how much rounding the problem allows.

Judgement (per_ray_reference.judge, the project's rule): the error against float64 per sample / per ray (the 2-norm of the
difference; the quantities are bounded by 1, no relative scale) is held to K = 8 times the float32 yardstick's own error per
statistic (median, 99th percentile, maximum, pooled), the yardstick's figure taken as at least FLOOR = 2^-24.  No sample and no ray
is left out."""
import functools

import numpy as np
import torch

import normals_reference as NR
import render_scenes as RS
from oracle import oracle as O
from per_ray_reference import judge

F64, F32 = torch.float64, torch.float32
K = (8.0, 8.0)
FLOOR = 2.0 ** -24
f32 = np.float32

ZERO_TILE = 4            # the zero-table variant "G9Z": G9 with the table of its centre tile zeroed
SCENES = ("G9", "STACK3", "STACK6", "G65")
# (scene, samples per ray) of the per-sample cases; the first four are the ones test_render_normals_cpu.py states conditions for
CPU_CASES = (("G9", 17), ("STACK3", 16), ("STACK6", 33), ("G65", 16))
SAMPLE_CASES = (("G9", 16), ("G9", 17), ("G9", 33), ("STACK3", 16), ("STACK6", 33), ("G65", 16), ("G9Z", 17))
ORDERS = ("shuffled", "sorted")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene arrays, rays) of render_scenes.named, plus "G9Z"; built once per process, callers leave them unchanged."""
    if name != "G9Z":
        return RS.named(name)
    sc, rays = RS.named("G9")
    sc = dict(sc)
    sc["tables"] = sc["tables"].copy()
    sc["tables"][ZERO_TILE] = 0
    return sc, rays


def _xz_weight(dx, dz):
    return np.where((dx != 0) & (dz != 0), dx * dz, np.where(dx != 0, dx, np.where(dz != 0, dz, f32(0)))).astype(f32)


def pinned_slots(sc, o, d, z, bi):
    """The float32-pinned part of every slot of every sample: o, d [B,3], z [B,S], bi [B,S,4] int16 ->
    {"listed" [N,4] bool (the list ends at its first -1), "b" [N,4], "w" [N,4] f32 (0 where not listed), "occ" [N,4] bool (listed and
    the cell set), "i0" [N,4,16,3] int32, "t" [N,4,16,3] f32}, N = B * S in ray-major order."""
    o, d, z = (np.asarray(a, f32) for a in (o, d, z))
    B, S = z.shape
    N = B * S
    b = np.asarray(bi, np.int64).reshape(N, 4)
    listed = np.cumprod(b != -1, axis=1).astype(bool)
    bb = np.where(listed, b, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        wp = (o[:, None, :] + z[..., None] * d[:, None, :]).astype(f32).reshape(N, 1, 3)
        corner, size = np.asarray(sc["corners"], f32)[bb], np.asarray(sc["sizes"], f32)[bb]        # [N,4,3]
        pts = ((wp - corner) / size).astype(f32)
        dis = ((f32(0.5) - np.abs(pts - f32(0.5))) * size).astype(f32)
        w = np.where(listed, _xz_weight(dis[..., 0], dis[..., 2]), f32(0)).astype(f32)
        l2d = np.asarray(sc["l2d"], np.int64)[bb]                                                    # [N,4,3]
        r = np.left_shift(1, l2d)
        cc = (pts * r.astype(f32)).astype(f32)
        cc = np.where(listed[..., None] & np.isfinite(cc), cc, 0).astype(np.int64)                   # C (int): truncation
        loc = np.clip(cc, 0, r - 1)
        off = (loc[..., 0] << (l2d[..., 1] + l2d[..., 2])) | (loc[..., 1] << l2d[..., 2]) | loc[..., 2]
        occ = listed & (np.asarray(sc["occ"]).astype(bool)[np.asarray(sc["starts"], np.int64)[bb] + off])
        p01 = (pts / f32(2.0) + f32(0.25)).astype(f32)
        r1 = (np.asarray(sc["res"], np.int32)[bb] - 1).astype(f32)                                   # [N,4,16,3]
        v = (p01[:, :, None, :] * r1).astype(f32)
        v = np.where(occ[..., None, None], v, f32(0))
        i0 = v.astype(np.int32)
        t = (v - i0.astype(f32)).astype(f32)
    return {"listed": listed, "b": bb, "w": w, "occ": occ, "i0": i0, "t": t}


def blend(sc, o, d, z, dd, bi, dtype, pin=None):
    """pts_normals in `dtype` behind the pinned slots -> {"normal" [N,3], "alpha" [N] = sum_b w_b pa_b occ_b / W, "W" [N], "n" [N,4,3],
    "pa" [N,4], "g" [N,4,3] (zeros where the slot does not run), "pin": pinned_slots' dict}."""
    pin = pin or pinned_slots(sc, o, d, z, bi)
    B, S = np.asarray(z).shape
    N = B * S
    n = torch.zeros(N, 4, 3, dtype=dtype)
    g = torch.zeros(N, 4, 3, dtype=dtype)
    sigma = torch.zeros(N, 4, dtype=dtype)
    ones = torch.ones(32, dtype=F32)
    occ, bb = pin["occ"], pin["b"]
    for b in np.unique(bb[occ]):
        rows, ks = np.nonzero(occ & (bb == b))
        A = (f32(2.0) / np.asarray(sc["sizes"], f32)[b]).astype(f32)
        ev = NR.evaluate_cells(pin["i0"][rows, ks], torch.from_numpy(pin["t"][rows, ks]), A, torch.from_numpy(sc["tables"][b]),
                               np.asarray(sc["res"], np.int32)[b], O.unpack_blob(torch.from_numpy(np.asarray(sc["params"], f32)[b])),
                               ones, dtype)
        n[rows, ks], g[rows, ks], sigma[rows, ks] = ev["n"], ev["g"], ev["sigma"]
    dnorm = torch.from_numpy(np.asarray(d, f32)).to(dtype).norm(dim=1)                                # |d|, un-normalised direction
    delta = (torch.from_numpy(np.asarray(dd, f32)).to(dtype) * dnorm[:, None]).reshape(N, 1)
    run = torch.from_numpy(occ)
    pa = torch.where(run, 1.0 - torch.exp(-sigma * delta), torch.zeros((), dtype=dtype))
    w = torch.from_numpy(pin["w"]).to(dtype)
    W = torch.zeros(N, dtype=dtype)
    normal, alpha = torch.zeros(N, 3, dtype=dtype), torch.zeros(N, dtype=dtype)
    for k in range(4):                                                                                # slot order
        W = W + w[:, k]
        normal = normal + torch.where(run[:, k, None], (w[:, k] * pa[:, k])[:, None] * n[:, k], torch.zeros((), dtype=dtype))
        alpha = alpha + w[:, k] * pa[:, k]
    pos = W > 0
    safe = torch.where(pos, W, torch.ones_like(W))
    normal = torch.where(pos[:, None], normal / safe[:, None], normal)
    alpha = torch.where(pos, alpha / safe, alpha)
    return {"normal": normal, "alpha": alpha, "W": W, "n": n, "pa": pa, "g": g, "pin": pin}


@functools.lru_cache(maxsize=None)
def sample_reference(name, S, order="shuffled"):
    """The first tracing pass of the scene's rays (render_scenes.trace_samples) and its blended normals: (inputs, float64, float32);
    inputs = {"sc", "o", "d", "z", "dd", "bi"}.  Computed once per process, shared, never written to."""
    sc, rays = scene(name)
    o, d = rays[order]
    z, dd, bi = RS.trace_samples(sc, o, d, S, passes=1)[0]
    pin = pinned_slots(sc, o, d, z, bi)
    args = (sc, o, d, z, dd, bi)
    return ({"sc": sc, "o": o, "d": d, "z": z, "dd": dd, "bi": bi}, blend(*args, F64, pin), blend(*args, F32, pin))


def slot_counts(bi):
    """samples with 0, 1, 2, 3, 4 listed tiles"""
    b = np.asarray(bi).reshape(-1, 4)
    return np.bincount(np.cumprod(b != -1, axis=1).sum(1), minlength=5)


# ------------------------------------------------------------------------------------------------------------ per-ray accumulation
def accumulate_normal(pts_normal, pts_alpha, transp, normal, dtype=np.float32, unsampled=None):
    """scanerf_accumulate_normal in `dtype`, in place on normal [B,3]: a ray whose transparency is < 1e-5 (or that `unsampled` [B]
    marks) is skipped; otherwise per sample, in order, normal += T pts_normal[s]; T <- T (1 - pts_alpha[s]).  The transparency is
    read, not written.  float32: the separate products and sums of oracle.accumulate_color."""
    pn = np.asarray(pts_normal).astype(dtype)
    B, S = pn.shape[:2]
    al = np.asarray(pts_alpha).astype(dtype).reshape(B, S)
    T = np.asarray(transp).astype(dtype).reshape(B).copy()
    go = np.asarray(transp, np.float32).reshape(B) >= np.float32(0.00001)
    if unsampled is not None:
        go &= ~np.asarray(unsampled, bool)
    acc = normal.astype(dtype)
    for s in range(S):
        acc = (acc + (T[:, None] * pn[:, s]).astype(dtype)).astype(dtype)
        T = (T * (dtype(1) - al[:, s])).astype(dtype)
    normal[go] = acc[go].astype(normal.dtype)
    return normal


def renderer_arrays(rnd):
    """The renderer's own scene arrays as a scene dict (what render_scenes.oracle_render_loop reads), plus its sampling grid."""
    c = lambda t: t.cpu().numpy()
    return {"corners": c(rnd.block_corner), "sizes": c(rnd.block_size), "occ": c(rnd.occupied_grid), "fake": c(rnd.fake_occupied_grid),
            "starts": c(rnd.grid_starts), "l2d": c(rnd.grid_log2dim), "tables": c(rnd.feature_tables), "params": c(rnd.params),
            "res": c(rnd.resolution)}


def render_loop(sc, o, d, num_sample, num_bg_sample):
    """render_scenes.oracle_render_loop extended by the normal: the colour state stays on O.pts_inference / O.accumulate_color (so the
    transmittance is the oracle's), the normal is accumulated before each O.accumulate_color from the pass's blended per-sample
    normals, in float64 and -- the yardstick -- in float32 through O.accumulate_color itself with the normal passed as the diffuse
    array.  -> {"dif", "spec", "depth", "T", "normal64" [B,3] float64, "normal32" [B,3] float32, "passes" [B] int: tracing passes in
    which the ray held a listed sample}.  sc: renderer_arrays' dict."""
    B = o.shape[0]
    corners, sizes, occ, fake, starts, l2d = (sc[k] for k in ("corners", "sizes", "occ", "fake", "starts", "l2d"))
    tabs, par, res = sc["tables"], sc["params"], sc["res"]
    inter = O.ray_block_intersection(o, d, corners, sizes)
    tb, max_tracing = RS.tracing_order(inter)
    T_, dF, sF, zF = np.ones((B, 1), f32), np.zeros((B, 3), f32), np.zeros((B, 3), f32), np.zeros((B, 1), f32)
    N64, N32 = np.zeros((B, 3), np.float64), np.zeros((B, 3), f32)
    passes = np.zeros(B, np.int64)
    ti, zs = np.zeros(B, np.int32), np.zeros(B, f32)
    for _ in range(max_tracing):
        running = (ti < max_tracing) & (T_[:, 0] > 1e-5)
        if running.sum() == 0:
            break
        z, dd = O.render_sample_points(o, d, corners, sizes, fake, starts, l2d, num_sample, tb, inter, ti, zs)
        bi = O.prepare_points(z, running, inter)
        pd, ps, pa = O.pts_inference(o, d, z, dd, bi, tabs, par, res, occ, starts, l2d, corners, sizes)
        pin = pinned_slots(sc, o, d, z, bi)
        passes += (bi[..., 0] != -1).any(1)
        n64 = blend(sc, o, d, z, dd, bi, F64, pin)["normal"].numpy().reshape(B, num_sample, 3)
        n32 = blend(sc, o, d, z, dd, bi, F32, pin)["normal"].numpy().reshape(B, num_sample, 3)
        accumulate_normal(n64, pa, T_, N64, np.float64)
        O.accumulate_color(n32, np.zeros_like(n32), pa, T_.copy(), z, N32, np.zeros((B, 3), f32), np.zeros((B, 1), f32))
        O.accumulate_color(pd, ps, pa, T_, z, dF, sF, zF)
    ob, bw = O.update_outgoing_bidx(o, d, corners, sizes, tb, inter, 0.12, False)
    with np.errstate(invalid="ignore", divide="ignore"):
        bwn = np.nan_to_num(bw / bw.sum(-1, keepdims=True))
    bd, bs, bz = np.zeros((B, 3), f32), np.zeros((B, 3), f32), np.zeros((B, 1), f32)
    for i in range(int((bwn > 0).sum(-1).max())):
        zb = O.render_inverse_z_sampling(inter, ob[:, i], num_bg_sample, 1e6)
        pd, ps, pa = O.bg_pts_inference_v2(o, d, zb, ob, i, corners, sizes, res, tabs, par)
        t1, td, ts, tz = np.ones((B, 1), f32), np.zeros((B, 3), f32), np.zeros((B, 3), f32), np.zeros((B, 1), f32)
        O.accumulate_color(pd, ps, pa, t1, zb, td, ts, tz)
        bd += td * bwn[:, i:i + 1]; bs += ts * bwn[:, i:i + 1]; bz += tz * bwn[:, i:i + 1]
    return {"dif": dF + T_ * bd, "spec": sF + T_ * bs, "depth": zF + T_ * bz, "T": T_, "normal64": N64, "normal32": N32, "passes": passes}


# ------------------------------------------------------------------------------------------------------------ judgement
def judge_normals(name, got, ref64, ref32, k=K):
    """got [N,3] (samples or rays) against the float64 result, the float32 yardstick as the measure -> list of violations."""
    ref64 = torch.as_tensor(ref64)
    return judge(name, got, ref64, torch.as_tensor(ref32), k, scale=torch.ones(ref64.shape[0], dtype=F64), floor=FLOOR)
