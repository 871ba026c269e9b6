"""Scenes and rays for the render-time tests at the tile counts of a large scene (a helper module, not a test): a 2-D grid of
overlapping tiles over x-z as rendering.py's scenes are laid out, a stack of coincident tiles, rays that meet the overlaps,
and the oracle's restatement of the novel-view loop.  numpy + oracle.oracle only; nothing here needs a GPU.

Geometry of grid_scene: tile (ix, iz) = index ix * nz + iz spans [3 ix, 3 ix + 4] x [-2, 2] x [3 iz, 3 iz + 4].  Neighbours
share a margin of 1, four tiles share the square [3 ix + 3, 3 ix + 4] x [3 iz + 3, 3 iz + 4] at every interior corner.
Whether a tile holds a point, or shares a ray's exit distance, is decided per axis, and each axis is covered once or twice:
a sample lies in 1, 2 or 4 tiles and a ray leaves 1, 2 or 4 tiles at one `far` -- never 3 (test_render_scenes_cpu.py asserts
it).  Lists of exactly three come from stacked_scene(n=3).
"""
import functools

import numpy as np
import torch

from oracle import oracle as O

PITCH, SIZE, Y0 = 3.0, 4.0, -2.0
GRIDS = {"G8": (2, 4), "G9": (3, 3), "G36": (6, 6), "G64": (8, 8), "G65": (5, 13)}
STACKS = {"STACK3": 3, "STACK6": 6}
B_RAYS = 509   # no multiple of 32: the renderer pads, the chunk kernels end on a ragged wave


def _finish(rng, corners, l2d, T, **extra):
    nb = corners.shape[0]
    sizes = np.full((nb, 3), SIZE, np.float32)
    grids = [rng.random(tuple(2 ** k for k in l)) < 0.35 for l in l2d]
    starts = np.cumsum([0] + [gr.size for gr in grids[:-1]]).astype(np.int64)
    occ = np.concatenate([gr.reshape(-1) for gr in grids])
    tables = (rng.normal(size=(nb, 16, T, 2)) * 0.6).astype(np.float16)
    params = []
    for b in range(nb):
        sd = O.init_mlp(seed=20 + b, bias_scale=0.05)
        sd["sigma_layer.mlp.0.bias"] = sd["sigma_layer.mlp.0.bias"] + 4.0  # visible densities
        params.append(O.pack_blob(sd).numpy())
    res1 = O.level_resolutions(torch.tensor([32, 32, 32]), torch.tensor([2048, 2048, 2048])).numpy()
    return dict(corners=corners, sizes=sizes, l2d=l2d, starts=starts, occ=occ, tables=tables, params=np.stack(params),
                res=np.stack([res1] * nb).astype(np.int32), T=T, **extra)


def grid_scene(rng, nx, nz, T=2 ** 10):
    """nx * nz tiles of 4x4x4 on a pitch of 3 in x and z (tile ix * nz + iz), log2dim alternating (3,3,3) / (4,3,3), occupancy
    fill 0.35, fp16 tables [nb,16,T,2], one decoder per tile: the keys of test_gpu_render_time._scene(), plus "grid"."""
    corners = np.float32([[PITCH * ix, Y0, PITCH * iz] for ix in range(nx) for iz in range(nz)])
    l2d = np.int32([[3, 3, 3] if b % 2 == 0 else [4, 3, 3] for b in range(nx * nz)])
    return _finish(rng, corners, l2d, T, grid=(nx, nz))


def stacked_scene(rng, n=6, T=2 ** 10):
    """n tiles over the SAME box with different tables and decoders: every sample lies in all of them and every ray leaves all
    of them at one `far`, so slot lists and exit lists truncate at four when n > 4."""
    corners = np.float32([[Y0, Y0, Y0]] * n)
    l2d = np.int32([[3, 3, 3] if b % 2 == 0 else [4, 3, 3] for b in range(n)])
    return _finish(rng, corners, l2d, T, grid=None)


def _unit_xz(rng, n):
    a = rng.uniform(0, 2 * np.pi, n)
    return np.cos(a), np.sin(a)


def _grid_rays(rng, sc, B):
    """Rays in generation order: the `high` group first (see scene_rays), then the five kinds the scene is tested with."""
    nx, nz = sc["grid"]
    nb = nx * nz
    X, Z = PITCH * (nx - 1) + SIZE, PITCH * (nz - 1) + SIZE
    U = rng.uniform
    os_, ds_ = [], []

    def add(o, d):
        os_.append(np.asarray(o, np.float64).reshape(-1, 3))
        ds_.append(np.asarray(d, np.float64).reshape(-1, 3))

    # (0) nb > 32: rays that come in over the z = Z face of the LAST tile, inside the part of its column no other column
    # overlaps, heading -z: the first pass samples tile nb - 1 and lists only it and tile nb - 2.  272 rays x 32 samples cover a
    # whole chunk of either chunk kernel (4096 samples in the 16-sample-tile kernel, 8192 in the 32-sample-tile one)
    n_hi = 272 if nb > 32 else 0
    if n_hi:
        x0 = U(PITCH * (nx - 1) + 1.8, X - 0.2, n_hi)
        add(np.stack([x0, U(-1.5, 1.5, n_hi), Z + U(1, 4, n_hi)], 1),
            np.stack([U(-0.05, 0.05, n_hi), rng.normal(0, 0.05, n_hi), -np.ones(n_hi)], 1) * U(0.7, 1.3, (n_hi, 1)))
    rest = B - n_hi
    n_miss, n_corner, n_margin, n_column = 24, rest * 3 // 10, rest * 2 // 10, rest * 2 // 10
    n_diag = rest - n_miss - n_corner - n_margin - n_column

    # (1) diagonal crossings from outside: entry faces cycle over the four sides and over the tiles along each side
    for k in range(n_diag):
        side, j = k % 4, k // 4
        along = (j % nz if side < 2 else j % nx) * PITCH + 2.0 + U(-0.8, 0.8)
        tang, dy = U(0.3, 1.0) * rng.choice([-1.0, 1.0]), rng.normal(0, 0.08)
        if side == 0:
            p, d = [0.0, U(-1.5, 1.5), along], [1.0, dy, tang]
        elif side == 1:
            p, d = [X, U(-1.5, 1.5), along], [-1.0, dy, tang]
        elif side == 2:
            p, d = [along, U(-1.5, 1.5), 0.0], [tang, dy, 1.0]
        else:
            p, d = [along, U(-1.5, 1.5), Z], [tang, dy, -1.0]
        d = np.float64(d) * U(0.7, 1.3)
        add(np.float64(p) - d * U(1, 5), d)

    # (2) origins inside a four-tile corner; every third one leaves through y = +-2 above the corner (four exit tiles)
    cs = [(ix, iz) for ix in range(nx - 1) for iz in range(nz - 1)]
    for k in range(n_corner):
        ix, iz = cs[k % len(cs)]
        steep = k % 3 == 2
        j = 0.3 if steep else 0.4
        o = [PITCH * ix + 3.5 + U(-j, j), U(-1.5, 1.5), PITCH * iz + 3.5 + U(-j, j)]
        if steep:
            d = [rng.normal(0, 0.04), rng.choice([-1.0, 1.0]), rng.normal(0, 0.04)]
        else:
            cx, cz = _unit_xz(rng, 1)
            d = [cx[0], rng.normal(0, 0.3), cz[0]]
        add(o, np.float64(d) * U(0.7, 1.3))

    # (3) along x / along z EXACTLY on the centre-line of an overlap margin (the lateral component is 0.0), both directions;
    # half of them level (d.y = 0.0: they leave two tiles through the last face), half climbing or falling
    for k in range(n_margin):
        along_x, fwd = k % 2 == 0, (k // 2) % 2 == 0
        m = (k // 4) % ((nz if along_x else nx) - 1)
        line = PITCH * m + 3.5
        dy = 0.0 if (k // 4) % 2 == 0 else U(0.05, 0.4) * rng.choice([-1.0, 1.0])
        y, s, far_side = U(-1.5, 1.5), U(0.7, 1.3), (X if along_x else Z)
        start = -U(1, 5) if fwd else far_side + U(1, 5)
        if along_x:
            add([start, y, line], [s if fwd else -s, dy * s, 0.0])
        else:
            add([line, y, start], [0.0, dy * s, s if fwd else -s])

    # (4) aimed at an interior corner column: through a point of it on y = +2 (leaving there), y = -2, or in between
    for k in range(n_column):
        ix, iz = cs[(k * 7 + 3) % len(cs)]
        kind = k % 3
        py = (2.0, -2.0, U(-1.5, 1.5))[kind]
        cx, cz = _unit_xz(rng, 1)
        dy = (U(0.2, 0.8), -U(0.2, 0.8), rng.normal(0, 0.1))[kind]
        d = np.float64([cx[0], dy, cz[0]]) * U(0.7, 1.3)
        p = np.float64([PITCH * ix + 3.5 + U(-0.3, 0.3), py, PITCH * iz + 3.5 + U(-0.3, 0.3)])
        add(p - d * U(3, 10), d)

    # (5) rays that miss everything
    add(np.stack([U(-22, -18, n_miss), U(28, 32, n_miss), U(-2, Z, n_miss)], 1),
        np.stack([np.ones(n_miss), rng.normal(0, 0.1, n_miss), rng.normal(0, 0.1, n_miss)], 1))
    return np.concatenate(os_).astype(np.float32), np.concatenate(ds_).astype(np.float32)


def _stack_rays(rng, sc, B):
    U = rng.uniform
    n_miss, n_in = 24, B // 4
    n_out = B - n_miss - n_in
    tgt = U(-1.5, 1.5, (n_out, 3))
    cx, cz = _unit_xz(rng, n_out)
    d = np.stack([cx, rng.normal(0, 0.3, n_out), cz], 1) * U(0.7, 1.3, (n_out, 1))
    cx, cz = _unit_xz(rng, n_in)
    o = np.concatenate([tgt - d * U(4, 9, (n_out, 1)), U(-1.8, 1.8, (n_in, 3)),
                        np.stack([U(-22, -18, n_miss), U(28, 32, n_miss), U(-2, 2, n_miss)], 1)])
    d = np.concatenate([d, np.stack([cx, rng.normal(0, 0.5, n_in), cz], 1),
                        np.stack([np.ones(n_miss), rng.normal(0, 0.1, n_miss), rng.normal(0, 0.1, n_miss)], 1)])
    return o.astype(np.float32), d.astype(np.float32)


def scene_rays(rng, sc, B=B_RAYS):
    """-> {"shuffled": (o, d), "sorted": (o, d)}, float32 [B,3] each: the same rays in two orders.  `sorted` is by the first
    tile a ray meets, HIGHEST first (stable over the generation order, misses last): with more than 32 tiles the batch then
    opens with >= 256 rays whose first-pass samples list tiles >= 32 only, i.e. >= 8192 consecutive samples from sample 0 on,
    aligned to the inference kernels' chunks in the layouts 0 and 2 alike."""
    o, d = (_grid_rays if sc["grid"] else _stack_rays)(rng, sc, B)
    assert o.shape == (B, 3) and d.shape == (B, 3)
    inter = O.ray_block_intersection(o, d, sc["corners"], sc["sizes"])
    first = np.argsort(inter[..., 0], axis=-1, kind="stable")[:, 0]
    key = np.where((inter[..., 0] != 1e7).any(-1), first, -1)
    by_tile = np.argsort(-key, kind="stable")
    mix = rng.permutation(B)
    return {"shuffled": (o[mix].copy(), d[mix].copy()), "sorted": (o[by_tile].copy(), d[by_tile].copy())}


@functools.lru_cache(maxsize=None)
def named(name):
    """(scene, rays) of G8 / G9 / G36 / G64 / G65 / STACK3 / STACK6, built once per process; callers leave them unchanged."""
    rng = np.random.default_rng(1000 + sorted(list(GRIDS) + list(STACKS)).index(name))
    sc = grid_scene(rng, *GRIDS[name]) if name in GRIDS else stacked_scene(rng, STACKS[name])
    return sc, scene_rays(rng, sc)


def tracing_order(inter):
    """rendering.py:301-303 -> (tracing_blocks [B,nb] i32, max_tracing)"""
    tb = np.argsort(inter[..., 0], axis=-1, kind="stable").astype(np.int32)
    return tb, int((inter != 1e7).astype(np.float32).mean(-1).sum(-1).max())


def trace_samples(sc, o, d, S, passes=None):
    """The sampler and slot-list half of the tracing loop on the oracle, every ray kept running (no decoder, so no
    transmittance): a list of (z_vals, dists, block_idxs) per pass, up to `passes` (default: max_tracing)."""
    inter = O.ray_block_intersection(o, d, sc["corners"], sc["sizes"])
    tb, max_tracing = tracing_order(inter)
    ti, zs = np.zeros(o.shape[0], np.int32), np.zeros(o.shape[0], np.float32)
    out = []
    for _ in range(max_tracing if passes is None else min(passes, max_tracing)):
        running = ti < max_tracing
        z, dd = O.render_sample_points(o, d, sc["corners"], sc["sizes"], sc["occ"], sc["starts"], sc["l2d"], S, tb, inter, ti, zs)
        out.append((z, dd, O.prepare_points(z, running, inter)))
    return out


def renderer_tiles(sc):
    """The scene as load_tile() dicts: feature.npz holds the 2x box around the box the renderer traces (renderer.render_box)."""
    grids = np.split(np.asarray(sc["occ"]), np.asarray(sc["starts"][1:]))
    return [{"features": sc["tables"][b], "occupied_grid": grids[b], "block_corner": sc["corners"][b] - sc["sizes"][b] / 2,
             "block_size": sc["sizes"][b] * 2, "grid_log2dim": sc["l2d"][b], "resolution": sc["res"][b], "blob": sc["params"][b]}
            for b in range(sc["corners"].shape[0])]


def oracle_render_loop(rnd, o, d, num_sample, num_bg_sample):
    """rendering.py:286-544's loop on the oracle's restatement of the render-time kernels, over the renderer's own scene arrays
    (numpy rays o, d [B,3]) -> {"dif", "spec", "depth", "T"}: what TileSetRenderer.render_rays must reproduce."""
    B = o.shape[0]
    corners, sizes = rnd.block_corner.cpu().numpy(), rnd.block_size.cpu().numpy()
    occ, fake = rnd.occupied_grid.cpu().numpy(), rnd.fake_occupied_grid.cpu().numpy()
    starts, l2d = rnd.grid_starts.cpu().numpy(), rnd.grid_log2dim.cpu().numpy()
    tabs, par, res = rnd.feature_tables.cpu().numpy(), rnd.params.cpu().numpy(), rnd.resolution.cpu().numpy()
    inter = O.ray_block_intersection(o, d, corners, sizes)
    tb = np.argsort(inter[..., 0], axis=-1, kind="stable").astype(np.int32)
    max_tracing = int((inter != 1e7).astype(np.float32).mean(-1).sum(-1).max())
    T_, dF, sF, zF = np.ones((B, 1), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 1), np.float32)
    ti, zs = np.zeros(B, np.int32), np.zeros(B, np.float32)
    for _ in range(max_tracing):
        running = (ti < max_tracing) & (T_[:, 0] > 1e-5)
        if running.sum() == 0:
            break
        z, dd = O.render_sample_points(o, d, corners, sizes, fake, starts, l2d, num_sample, tb, inter, ti, zs)
        bi = O.prepare_points(z, running, inter)
        pd, ps, pa = O.pts_inference(o, d, z, dd, bi, tabs, par, res, occ, starts, l2d, corners, sizes)
        O.accumulate_color(pd, ps, pa, T_, z, dF, sF, zF)
    ob, bw = O.update_outgoing_bidx(o, d, corners, sizes, tb, inter, 0.12, False)
    with np.errstate(invalid="ignore", divide="ignore"):
        bwn = np.nan_to_num(bw / bw.sum(-1, keepdims=True))
    bd, bs, bz = np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 1), np.float32)
    for i in range(int((bwn > 0).sum(-1).max())):
        zb = O.render_inverse_z_sampling(inter, ob[:, i], num_bg_sample, 1e6)
        pd, ps, pa = O.bg_pts_inference_v2(o, d, zb, ob, i, corners, sizes, res, tabs, par)
        t1, td, ts, tz = np.ones((B, 1), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 1), np.float32)
        O.accumulate_color(pd, ps, pa, t1, zb, td, ts, tz)
        bd += td * bwn[:, i:i + 1]; bs += ts * bwn[:, i:i + 1]; bz += tz * bwn[:, i:i + 1]
    return {"dif": dF + T_ * bd, "spec": sF + T_ * bs, "depth": zF + T_ * bz, "T": T_}
