"""Reference, yardstick and case list of render-time inference (csrc/render_infer.hip, csrc/render_time.hip: pts_inference,
pts_inference_tracing, bg_pts_inference_v2, bg_pts_inference, accumulate_color; test infrastructure, CPU only: numpy / torch /
oracle.oracle, no GPU import).

What oracle/scanerf_oracle.c states for the four ops, restated in a dtype of the caller's choice -- float64 = the reference, float32 =
the yardstick for how much rounding the problem allows -- behind float32-pinned geometry (a run with everything in float64 would move
a point by an ulp, and the cell offset amplifies that by the level's resolution):

  orc_pts_inference        render_normals_reference.pinned_slots (slot lists, blend weights w_b, occupancy cells, i0, t: float32), then
                           in slot order  feat = sum_c w_c(t) table_b[hash(i0 + c)];  decoder_one(blob_b, feat, d)  (weight_feature == 1,
                           direction d / sqrt(d.d) WITHOUT an epsilon, sigma = log(1 + exp(s)), specular = tint * sigmoid(.));
                           pa = 1 - exp(-sigma dist |d|);  sums w pa c_d, w pa c_s, w pa;  W += w for every LISTED slot, occupied or
                           not;  division by W where W > 0.
  orc_bg_pts_inference_v2  pinned_bg: x = 2 (o + z d - corner) / size - 1, n = |x|_inf, ratio = (2 - 1 / n) / n, p01 = (x ratio + 2) / 4,
                           v = p01 (res - 1), i0 = int(v), t = v - i0 by the oracle's very float32 expressions; then the step
                           z[s+1] - z[s] (1e7 on the last sample), pa = 1 - exp(-sigma step) (no |d|), out = pa c.
  orc_bg_pts_inference     the v1 blend of a ray's exit tiles, slots up to the first -1, with the ray's blend weights.
  orc_accumulate_color     serial, the transmittance carried over a SEQUENCE of passes: dif += T c, depth += (T a) z, T <- T (1 - a); a
                           ray whose transmittance is < 1e-5 when a pass starts is skipped in that pass.  The skip is a decision, so it
                           is pinned too: on the transmittance of the float32 run.

Judgement (per_ray_reference.judge): per sample the 2-norm of the error of diffuse, specular (3-vectors) and alpha against float64,
absolute (the quantities are bounded by 1) and over the size of the sample's float64 alpha (a faint sample counts as much as a dense
one), each
held to K x the float32 yardstick's own figure per statistic, the yardstick's figure taken as at least FLOOR = 2^-24.  No sample is
left out; a sample whose float64 alpha is exactly 0 must come out exactly 0 (per_ray_errors: an error over a zero scale is infinite).
Per ray, after accumulate_color: diffuse, specular, transmittance absolute, depth relative to its float64 value.  Rays whose pinned
transmittance lies within TIE_BAND of the 1e-5 threshold when some pass starts are set aside there -- rounding decides whether the
pass runs -- and at most TIE_CAP of a case's rays may be (test_render_infer_reference_cpu.py asserts it).

K: K_SPLIT for the split-f16 kernels is the factor test_gpu_gradient_groups.py derives (4 for 22-bit operands against 24, times 2 for
the summation order); K_F32 and K_ACC follow the project's rule (profiles/render_infer_error.md holds the run and the derivation).

The case list lives here, so that the CPU and the GPU tests read the same cases."""
import collections
import functools

import numpy as np
import torch

import render_normals_reference as RNR
import render_scenes as RS
from gradient_reference64 import corner_indices
from oracle import oracle as O
from per_ray_reference import judge

F64, F32 = torch.float64, torch.float32
f32 = np.float32
FLOOR = 2.0 ** -24
K_SPLIT = (8.0, 8.0)   # default (folded), plain, h3, both chunk-major kernels, the fused slot lists: given, not measured
# The project's rule for the other two: the largest ratio (op's figure / max(float32 yardstick's figure, FLOOR)) over all cases of the
# first MI355X run of the finished tests, doubled and rounded up to a power of two (profiles/render_infer_error.md holds the run).
K_F32 = (4.0, 4.0)     # the single-pass f32 kernel (also > 64 tiles): 1.05 (median / p99 / pooled) and 1.25 (maximum)
K_ACC = (4.0, 4.0)     # accumulate_color:                                1.31 and 1.84
SKIP_T = f32(0.00001)
TIE_BAND = 1e-3        # relative: |T - 1e-5| <= TIE_BAND * 1e-5 when a pass starts
TIE_CAP = 1e-3

FAMILIES = ("base", "dense", "thin", "bias", "wide", "fresh", "zero", "axis", "face", "long", "short")
DENSE_DISTS = 16.0     # "dense", per-sample cases: the intervals handed to the op are 16 times the sampler's (see family_scene)
THIN_BIAS = -9.0      # density bias of "thin": sigma ~ e^-9, times an interval of ~0.3: alpha ~ 4e-5
ZERO_TILE = {"G9": 4, "STACK6": 1}
SCALE_D = 2.0 ** 10    # "long" / "short": |d| ~ 1e3 / 1e-3 by an exact factor, so that points and dist |d| keep their bits

Case = collections.namedtuple("Case", "scene S family")
CASES_SCENES = [Case("G9", 16, "base"), Case("G9", 17, "base"), Case("G9", 33, "base"), Case("STACK6", 33, "base"),
                Case("G36", 16, "base"), Case("G65", 16, "base")]
CASES_FAMILIES = [Case(n, S, f) for n, S in (("G9", 17), ("STACK6", 33)) for f in FAMILIES[1:]]
PTS_CASES = CASES_SCENES + CASES_FAMILIES
CROSS_CASE = Case("G9", 17, "base")          # the one case every route and layout is crossed on
TRACING_CASE = Case("STACK6", 33, "base")    # pts_inference_tracing serves up to 8 tiles: the stack has 6

BgCase = collections.namedtuple("BgCase", "scene S step family")
BG_CASES = ([BgCase("G9", S, step, "base") for S in (16, 48) for step in (0, 1)]
            + [BgCase("STACK6", 16, step, "base") for step in (0, 1)] + [BgCase("G65", 16, 0, "base")]
            + [BgCase("G9", 16, 0, f) for f in ("dense", "thin", "bias", "wide", "fresh", "zero", "axis", "long", "short")])
BG_V1_CASES = [BgCase("G9", 16, None, "base"), BgCase("STACK6", 16, None, "base"), BgCase("STACK6", 48, None, "thin")]

RayCase = collections.namedtuple("RayCase", "scene S SB family")
RAY_CASES = [RayCase("G9", 17, 16, "base"), RayCase("G9", 17, 16, "dense"), RayCase("G9", 17, 16, "thin"), RayCase("STACK6", 33, 16, "base"),
             RayCase("G9", 16, 48, "fresh")]
RENDER_CASE = RayCase("G9", 17, 16, "base")  # TileSetRenderer.render_rays


def case_id(c):
    return "-".join(str(v) for v in c if v is not None)


# ------------------------------------------------------------------------------------------------------------ the families
def _rebias(params, delta):
    """the blobs with `delta` added to every tile's density bias"""
    out = []
    for blob in np.asarray(params, f32):
        sd = {k: v.clone() for k, v in O.unpack_blob(torch.from_numpy(blob.copy())).items()}
        sd["sigma_layer.mlp.0.bias"] = sd["sigma_layer.mlp.0.bias"] + delta
        out.append(O.pack_blob(sd).numpy())
    return np.stack(out)


_AXES = np.float64([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                    [1, 1, 0], [-1, 1, 0], [1, 0, -1], [0, 1, 1], [0, -1, 1], [1, -1, 0], [-1, 0, -1], [0, 1, -1]])


@functools.lru_cache(maxsize=None)
def family_scene(name, family):
    """(scene arrays, o, d) of a family on G9 / STACK6 (any scene for "base"): render_scenes.named's scene and its shuffled rays, then
      dense  density bias + 12 (the scenes' own is + 4).  The sampler's intervals are ~0.05, so sigma ~ 12 alone gives alpha ~ 0.5 and
             no sample saturates; a bias that would (sigma > 140) is past the point where float32 log(1 + exp(s)) overflows, another
             matter.  The per-sample cases therefore hand the op intervals DENSE_DISTS times the sampler's (scaled_samples): sigma
             dist |d| ~ 10.  The per-ray cases, whose intervals are the loop's own, keep the bias alone.
      thin   density bias THIN_BIAS;
      bias   decoders drawn with bias_scale = 1.0 (density bias + 4 as in the scenes);
      wide   tables x 8;       fresh  tables uniform in +-1e-4, stored in f16;       zero   the table of ZERO_TILE zeroed;
      axis   directions along +-x / y / z and diagonals with one zero component, speeds as drawn, origins moved into the tiles;
      face   rays that run INSIDE tile faces: x exactly on a face (d.x = 0), every fourth one x and z both (d along y);
      long / short   see scaled_samples: the rays are the scene's.
    Built once per process; callers leave them unchanged."""
    assert family in FAMILIES
    sc, rays = RS.named(name)
    o, d = rays["shuffled"]
    if family in ("base", "long", "short"):
        return sc, o, d
    sc = dict(sc)
    nb = sc["corners"].shape[0]
    rng = np.random.default_rng(77)
    if family == "dense":
        sc["params"] = _rebias(sc["params"], 8.0)
    elif family == "thin":
        sc["params"] = _rebias(sc["params"], THIN_BIAS - 4.0)
    elif family == "bias":
        blobs = []
        for b in range(nb):
            sd = O.init_mlp(seed=20 + b, bias_scale=1.0)
            sd["sigma_layer.mlp.0.bias"] = sd["sigma_layer.mlp.0.bias"] + 4.0
            blobs.append(O.pack_blob(sd).numpy())
        sc["params"] = np.stack(blobs)
    elif family == "wide":
        sc["tables"] = (sc["tables"].astype(f32) * f32(8)).astype(np.float16)
    elif family == "fresh":
        sc["tables"] = rng.uniform(-1e-4, 1e-4, sc["tables"].shape).astype(np.float16)
    elif family == "zero":
        sc["tables"] = sc["tables"].copy()
        sc["tables"][ZERO_TILE[name]] = 0
    elif family == "axis":
        B = o.shape[0]
        speed = np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
        d = (_AXES[np.arange(B) % len(_AXES)] / np.linalg.norm(_AXES, axis=1, keepdims=True)[np.arange(B) % len(_AXES)] * speed).astype(f32)
        lo, hi = sc["corners"].min(0) + 0.3, (sc["corners"] + sc["sizes"]).max(0) - 0.3
        o = rng.uniform(lo, hi, (B, 3)).astype(f32)
    elif family == "face":
        B = o.shape[0]
        lo, hi = sc["corners"].min(0), (sc["corners"] + sc["sizes"]).max(0)
        faces_x = np.unique(np.concatenate([sc["corners"][:, 0], sc["corners"][:, 0] + sc["sizes"][:, 0]]))
        faces_z = np.unique(np.concatenate([sc["corners"][:, 2], sc["corners"][:, 2] + sc["sizes"][:, 2]]))
        o = rng.uniform(lo + 0.2, hi - 0.2, (B, 3)).astype(f32)
        o[:, 0] = faces_x[np.arange(B) % len(faces_x)]
        both = np.arange(B) % 4 == 3
        o[both, 2] = faces_z[(np.arange(B) // 4 % len(faces_z))[both]]
        d = np.zeros((B, 3))
        d[:, 1] = rng.normal(0, 0.3, B)
        d[:, 2] = rng.choice([-1.0, 1.0], B)
        d[both] = [0.0, 1.0, 0.0]
        d[both, 1] = rng.choice([-1.0, 1.0], int(both.sum()))
        d = (d * rng.uniform(0.7, 1.3, (B, 1))).astype(f32)
    return sc, o, d


def scaled_samples(family, d, z, dd):
    """"long" / "short": d x SCALE_D^+-1, z and dists x SCALE_D^-+1 -- powers of two, so o + z d and dist |d| keep their bits in
    float32 and are unchanged in float64; only the size of the direction the decoder normalises changes."""
    k = f32({"long": SCALE_D, "short": 1.0 / SCALE_D}.get(family, 1.0))
    wide = f32(DENSE_DISTS if family == "dense" else 1.0)
    return (d * k).astype(f32), (z / k).astype(f32), (dd / k * wide).astype(f32)


# ------------------------------------------------------------------------------------------------------------ gather and decoder
def _corner_weights(t, dtype):
    """linear_weight from the pinned offsets t [N,L,3] (tensor) in `dtype` -> [N,L,8], corner c = dx << 2 | dy << 1 | dz"""
    t = t.to(dtype)
    one = torch.ones((), dtype=dtype)
    w = []
    for c in range(8):
        f = [t[..., k] if (c >> (2 - k)) & 1 else one - t[..., k] for k in range(3)]
        w.append(f[0] * f[1] * f[2])
    return torch.stack(w, -1)


def gather(i0, t, table, dtype):
    """multilevel_features_h behind the cell: i0 [N,16,3] int32, t [N,16,3] float32 (numpy), table [16,T,2] f16 -> feat [N,32]"""
    tab = torch.from_numpy(np.asarray(table)).to(dtype)
    idx = torch.from_numpy(corner_indices(np.asarray(i0, np.int32), tab.shape[1]))
    vals = tab[torch.arange(16)[None, :, None], idx]                           # [N,16,8,2]
    w = _corner_weights(torch.from_numpy(np.asarray(t, f32)), dtype)
    return (w[..., None] * vals).sum(2).reshape(-1, 32)


def _lin(sd, name, x):
    return x @ sd[name + ".weight"].t() + sd[name + ".bias"]


def decoder(blob, feat, d, dtype):
    """decoder_one in `dtype`: feat [N,32], d [N,3] (un-normalised) -> {"sigma" [N], "diffuse" [N,3], "specular" [N,3] (tinted),
    "acts": the three Gaussian-activated layers' outputs}.  (oracle.mlp_forward is the training decoder: it normalises the direction
    with an epsilon of 1e-8, which the render-time decoder does not have -- at |d| = 1e-3 that is 1e-5 of the direction.)"""
    sd = {k: v.to(dtype) for k, v in O.unpack_blob(torch.as_tensor(np.asarray(blob, f32))).items()}
    feat, d = feat.to(dtype), d.to(dtype)
    a0 = O.gaussian_act(_lin(sd, "Spatial_MLP.mlp.0", feat))
    H = _lin(sd, "Spatial_MLP.mlp.2", a0)
    sigma = torch.log(1.0 + torch.exp(_lin(sd, "sigma_layer.mlp.0", H[:, :32])))[:, 0]
    c_d = torch.sigmoid(_lin(sd, "diffuse_layer.mlp.0", H[:, :32]))
    tint = torch.sigmoid(_lin(sd, "tint_layer.mlp.0", H[:, :32]))
    u = d * (1.0 / torch.sqrt((d * d).sum(1, keepdim=True)))
    a1 = O.gaussian_act(_lin(sd, "Directional_MLP.mlp.0", torch.cat([H[:, 32:], O.sh_deg3(u)], 1)))
    a2 = O.gaussian_act(_lin(sd, "Directional_MLP.mlp.2", a1))
    c_s = tint * torch.sigmoid(_lin(sd, "Directional_MLP.mlp.4", a2))
    return {"sigma": sigma, "diffuse": c_d, "specular": c_s, "acts": (a0, a1, a2)}


class ActStats:
    """how far from their flat top the Gaussian activations ran (float64 runs only feed it)"""

    def __init__(self):
        self.units = self.below_half = self.first = self.first_dead = 0

    def add(self, acts):
        for i, a in enumerate(acts):
            self.units += a.numel()
            self.below_half += int((a < 0.5).sum())
            if i == 0:
                self.first += a.numel()
                self.first_dead += int((a < 1e-6).sum())


# ------------------------------------------------------------------------------------------------------------ pts_inference
def pts_inference(sc, o, d, z, dd, bi, dtype, pin=None):
    """orc_pts_inference in `dtype` -> {"dif", "spec" [N,3], "alpha" [N], "W" [N], "pa" [N,4] (0 where the slot does not run), "pin",
    "stats": ActStats}, N = B * S ray-major."""
    pin = pin or RNR.pinned_slots(sc, o, d, z, bi)
    B, S = np.asarray(z).shape
    N = B * S
    zero = torch.zeros((), dtype=dtype)
    pd, ps, sigma = torch.zeros(N, 4, 3, dtype=dtype), torch.zeros(N, 4, 3, dtype=dtype), torch.zeros(N, 4, dtype=dtype)
    occ, bb = pin["occ"], pin["b"]
    dirs = torch.from_numpy(np.repeat(np.asarray(d, f32), S, 0))
    stats = ActStats()
    for b in np.unique(bb[occ]):
        rows, ks = np.nonzero(occ & (bb == b))
        out = decoder(sc["params"][b], gather(pin["i0"][rows, ks], pin["t"][rows, ks], sc["tables"][b], dtype), dirs[rows], dtype)
        pd[rows, ks], ps[rows, ks], sigma[rows, ks] = out["diffuse"], out["specular"], out["sigma"]
        stats.add(out["acts"])
    dnorm = torch.sqrt((torch.from_numpy(np.asarray(d, f32)).to(dtype) ** 2).sum(1))
    dist = torch.from_numpy(np.asarray(dd, f32)).to(dtype).reshape(N, 1)
    run = torch.from_numpy(occ)
    pa = torch.where(run, 1.0 - torch.exp(-sigma * dist * dnorm.repeat_interleave(S)[:, None]), zero)
    w = torch.from_numpy(pin["w"]).to(dtype)
    W, alpha = torch.zeros(N, dtype=dtype), torch.zeros(N, dtype=dtype)
    dif, spec = torch.zeros(N, 3, dtype=dtype), torch.zeros(N, 3, dtype=dtype)
    for k in range(4):                                                          # slot order
        wp = torch.where(run[:, k], w[:, k] * pa[:, k], zero)
        dif, spec, alpha = dif + wp[:, None] * pd[:, k], spec + wp[:, None] * ps[:, k], alpha + wp
        W = W + w[:, k]
    pos = W > 0
    safe = torch.where(pos, W, torch.ones_like(W))
    dif, spec = (torch.where(pos[:, None], a / safe[:, None], a) for a in (dif, spec))
    alpha = torch.where(pos, alpha / safe, alpha)
    return {"dif": dif, "spec": spec, "alpha": alpha, "W": W, "pa": pa, "pin": pin, "stats": stats}


def case_samples(c):
    """(scene arrays, o, d, z, dists, block_idxs) of a per-sample case: the first tracing pass of the family's rays"""
    sc, o, d = family_scene(c.scene, c.family)
    z, dd, bi = RS.trace_samples(sc, o, d, c.S, passes=1)[0]
    d, z, dd = scaled_samples(c.family, d, z, dd)
    return sc, o, d, z, dd, bi


@functools.lru_cache(maxsize=None)
def pts_reference(c):
    """(inputs {"sc", "o", "d", "z", "dd", "bi"}, float64 result, float32 result) of a per-sample case: computed once per process,
    shared, never written to."""
    sc, o, d, z, dd, bi = case_samples(c)
    pin = RNR.pinned_slots(sc, o, d, z, bi)
    args = (sc, o, d, z, dd, bi)
    return ({"sc": sc, "o": o, "d": d, "z": z, "dd": dd, "bi": bi}, pts_inference(*args, F64, pin), pts_inference(*args, F32, pin))


# ------------------------------------------------------------------------------------------------------------ background
def pinned_bg(sc, o, d, z, tile):
    """The float32-pinned part of the background samples of the rays' tile `tile` [B] (-1: the ray has none): {"run" [N] bool,
    "b" [N], "i0" [N,16,3] int32, "t" [N,16,3] f32}, by orc_bg_pts_inference_v2's own expressions (numpy float32)."""
    o, d, z = (np.asarray(a, f32) for a in (o, d, z))
    B, S = z.shape
    tile = np.asarray(tile, np.int64).reshape(B)
    run = np.repeat(tile != -1, S)
    bb = np.repeat(np.where(tile != -1, tile, 0), S)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        wp = (o[:, None, :] + z[..., None] * d[:, None, :]).astype(f32).reshape(-1, 3)
        corner, size = np.asarray(sc["corners"], f32)[bb], np.asarray(sc["sizes"], f32)[bb]
        x = ((f32(2.0) * (wp - corner)).astype(f32) / size - f32(1.0)).astype(f32)
        n = np.abs(x).max(1).astype(f32)
        ratio = ((f32(2.0) - f32(1.0) / n).astype(f32) / n).astype(f32)
        p01 = (((x * ratio[:, None]).astype(f32) + f32(2.0)) / f32(4.0)).astype(f32)
        r1 = (np.asarray(sc["res"], np.int32)[bb] - 1).astype(f32)              # [N,16,3]
        v = (p01[:, None, :] * r1).astype(f32)
        v = np.where(run[:, None, None] & np.isfinite(v), v, f32(0))
        i0 = v.astype(np.int32)
        t = (v - i0.astype(f32)).astype(f32)
    return {"run": run, "b": bb, "i0": i0, "t": t}


def _bg_slot(sc, o, d, z, tile, dtype):
    """one exit tile per ray -> (pa [N], c_d [N,3], c_s [N,3], run [N]); zeros where the ray has no tile"""
    B, S = np.asarray(z).shape
    N = B * S
    pin = pinned_bg(sc, o, d, z, tile)
    pd, ps, sigma = torch.zeros(N, 3, dtype=dtype), torch.zeros(N, 3, dtype=dtype), torch.zeros(N, dtype=dtype)
    dirs = torch.from_numpy(np.repeat(np.asarray(d, f32), S, 0))
    for b in np.unique(pin["b"][pin["run"]]):
        rows = np.nonzero(pin["run"] & (pin["b"] == b))[0]
        out = decoder(sc["params"][b], gather(pin["i0"][rows], pin["t"][rows], sc["tables"][b], dtype), dirs[rows], dtype)
        pd[rows], ps[rows], sigma[rows] = out["diffuse"], out["specular"], out["sigma"]
    zt = torch.from_numpy(np.asarray(z, f32)).to(dtype)
    step = torch.cat([zt[:, 1:] - zt[:, :-1], torch.full((B, 1), 10000000.0, dtype=dtype)], 1).reshape(N)
    run = torch.from_numpy(pin["run"])
    pa = torch.where(run, 1.0 - torch.exp(-sigma * step), torch.zeros((), dtype=dtype))
    return pa, pd, ps, run


def bg_inference_v2(sc, o, d, z, bg_idxs, step, dtype):
    """orc_bg_pts_inference_v2 -> {"dif", "spec" [N,3], "alpha" [N]} (zeros for a ray without a tile in slot `step`)"""
    pa, pd, ps, _ = _bg_slot(sc, o, d, z, np.asarray(bg_idxs)[:, step], dtype)
    return {"dif": pa[:, None] * pd, "spec": pa[:, None] * ps, "alpha": pa}


def bg_inference_v1(sc, o, d, z, outgoing, blend, dtype):
    """orc_bg_pts_inference: slots of outgoing [B,4] up to the first -1, weights blend [B,4] float32"""
    B, S = np.asarray(z).shape
    N = B * S
    outgoing = np.asarray(outgoing, np.int64)
    live = np.cumprod(outgoing != -1, axis=1).astype(bool)
    dif, spec = torch.zeros(N, 3, dtype=dtype), torch.zeros(N, 3, dtype=dtype)
    alpha, W = torch.zeros(N, dtype=dtype), torch.zeros(N, dtype=dtype)
    for k in range(4):
        if not live[:, k].any():
            break
        pa, pd, ps, run = _bg_slot(sc, o, d, z, np.where(live[:, k], outgoing[:, k], -1), dtype)
        w = torch.from_numpy(np.repeat(np.where(live[:, k], np.asarray(blend, f32)[:, k], f32(0)), S)).to(dtype)
        wp = w * pa
        dif, spec, alpha, W = dif + wp[:, None] * pd, spec + wp[:, None] * ps, alpha + wp, W + w
    pos = W > 0
    safe = torch.where(pos, W, torch.ones_like(W))
    dif, spec = (torch.where(pos[:, None], a / safe[:, None], a) for a in (dif, spec))
    return {"dif": dif, "spec": spec, "alpha": torch.where(pos, alpha / safe, alpha)}


def exit_tiles(sc, o, d):
    """(intersections, exit tiles [B,4] int16, blend weights [B,4] float32) by the oracle's geometry ops"""
    inter = O.ray_block_intersection(o, d, sc["corners"], sc["sizes"])
    tb, _ = RS.tracing_order(inter)
    ob, bw = O.update_outgoing_bidx(o, d, sc["corners"], sc["sizes"], tb, inter, 0.12, False)
    return inter, ob, bw


def bg_case_samples(c):
    """(scene arrays, o, d, z [B,S], exit tiles, blend weights) of a background case (for v1: the depths of slot 0)"""
    sc, o, d = family_scene(c.scene, c.family)
    inter, ob, bw = exit_tiles(sc, o, d)
    z = O.render_inverse_z_sampling(inter, ob[:, c.step or 0], c.S, 1e6)
    d, z, _ = scaled_samples(c.family, d, z, z)
    return sc, o, d, z, ob, bw


@functools.lru_cache(maxsize=None)
def bg_reference(c):
    """(inputs {"sc", "o", "d", "z", "ob", "bw"}, float64 result, float32 result) of a background case (step None: the v1 blend)"""
    sc, o, d, z, ob, bw = bg_case_samples(c)
    run = (lambda dt: bg_inference_v1(sc, o, d, z, ob, bw, dt)) if c.step is None else (lambda dt: bg_inference_v2(sc, o, d, z, ob, c.step, dt))
    return {"sc": sc, "o": o, "d": d, "z": z, "ob": ob, "bw": bw}, run(F64), run(F32)


# ------------------------------------------------------------------------------------------------------------ accumulate_color
def new_state(B, dtype):
    return {"T": np.ones(B, dtype), "dif": np.zeros((B, 3), dtype), "spec": np.zeros((B, 3), dtype), "depth": np.zeros(B, dtype)}


def accumulate_color(state, pts_dif, pts_spec, pts_alpha, z, go=None):
    """orc_accumulate_color of one pass in the dtype of `state` (numpy; in place): pts_dif, pts_spec [B,S,3], pts_alpha, z [B,S].
    go [B] bool: the rays the pass runs for -- None: decided here, T >= 1e-5 in float32 (the float32 run); the float64 run is
    handed the float32 run's decision.  -> go.  float32: separate products and sums, in the oracle's order."""
    dt = state["T"].dtype.type
    pdif, pspec, pa, z = (np.asarray(a).astype(dt) for a in (pts_dif, pts_spec, pts_alpha, z))
    B, S = z.shape
    pa = pa.reshape(B, S)
    if go is None:
        go = ~(state["T"].astype(f32) < SKIP_T)
    T, dif, spec, depth = state["T"].copy(), state["dif"].copy(), state["spec"].copy(), state["depth"].copy()
    for s in range(S):
        dif = (dif + (T[:, None] * pdif[:, s]).astype(dt)).astype(dt)
        spec = (spec + (T[:, None] * pspec[:, s]).astype(dt)).astype(dt)
        depth = (depth + ((T * pa[:, s]).astype(dt) * z[:, s]).astype(dt)).astype(dt)
        T = (T * (dt(1) - pa[:, s]).astype(dt)).astype(dt)
    for k, v in (("T", T), ("dif", dif), ("spec", spec), ("depth", depth)):
        state[k][go] = v[go]
    return go


def accumulate_sequence(passes, dtype, gos=None):
    """accumulate_color over a sequence of passes [(pts_dif, pts_spec, pts_alpha, z)], the transmittance carried -> (state, [go per
    pass], [T when the pass starts])"""
    B = np.asarray(passes[0][3]).shape[0]
    st = new_state(B, dtype)
    out_go, starts = [], []
    for k, p in enumerate(passes):
        starts.append(st["T"].copy())
        out_go.append(accumulate_color(st, *p, go=None if gos is None else gos[k]))
    return st, out_go, starts


def tied(starts):
    """[B] bool: the transmittance lies within TIE_BAND of the skip threshold when some pass starts"""
    return np.any([np.abs(T.astype(np.float64) - 1e-5) <= TIE_BAND * 1e-5 for T in starts], axis=0)


# ------------------------------------------------------------------------------------------------------------ the novel-view loop
def fake_grid(sc):
    """the sampler's occupancy: every tile's grid dilated by process_occupied_grid, as renderer.TileSetRenderer prepares it"""
    tgt = np.asarray(sc["occ"]).astype(np.uint8).copy()
    for b in range(sc["corners"].shape[0]):
        O.process_occupied_grid(b, int(np.prod(2 ** sc["l2d"][b])), sc["corners"], sc["sizes"], sc["occ"], sc["starts"], sc["l2d"], tgt)
    return tgt


def render_loop(sc, o, d, num_sample, num_bg_sample):
    """render_scenes.oracle_render_loop with the per-sample values and the accumulation in float64 AND float32 (this file's
    restatements); the loop's decisions -- which rays run a tracing pass, which rays a pass skips -- are the float32 run's.  sc: scene
    arrays with "fake" (render_normals_reference.renderer_arrays, or fake_grid).  -> {"f64", "f32": {"dif", "spec" [B,3], "depth",
    "T" [B]}, "tied" [B] bool, "passes": [(z, dd, bi, float32 per-sample dict)] of the tracing passes, "bg": [(z, tile list, step,
    float32 per-sample dict)]}."""
    B = o.shape[0]
    corners, sizes, starts, l2d = (sc[k] for k in ("corners", "sizes", "starts", "l2d"))
    inter = O.ray_block_intersection(o, d, corners, sizes)
    tb, max_tracing = RS.tracing_order(inter)
    st = {F64: new_state(B, np.float64), F32: new_state(B, f32)}
    ti, zs = np.zeros(B, np.int32), np.zeros(B, f32)
    starts_T, passes = [], []
    shape = lambda r, S: (r["dif"].numpy().reshape(B, S, 3), r["spec"].numpy().reshape(B, S, 3), r["alpha"].numpy().reshape(B, S))
    for _ in range(max_tracing):
        running = (ti < max_tracing) & (st[F32]["T"] > 1e-5)
        if running.sum() == 0:
            break
        z, dd = O.render_sample_points(o, d, corners, sizes, sc["fake"], starts, l2d, num_sample, tb, inter, ti, zs)
        bi = O.prepare_points(z, running, inter)
        pin = RNR.pinned_slots(sc, o, d, z, bi)
        r = {dt: pts_inference(sc, o, d, z, dd, bi, dt, pin) for dt in (F64, F32)}
        starts_T.append(st[F32]["T"].copy())
        go = accumulate_color(st[F32], *shape(r[F32], num_sample), z)
        accumulate_color(st[F64], *shape(r[F64], num_sample), z, go=go)
        passes.append((z, dd, bi, r[F32]))
    _, ob, bw = exit_tiles(sc, o, d)
    with np.errstate(invalid="ignore", divide="ignore"):
        bwn = np.nan_to_num(bw / bw.sum(-1, keepdims=True))
    acc = {dt: {k: np.zeros_like(v) for k, v in st[dt].items() if k != "T"} for dt in (F64, F32)}
    bg = []
    for i in range(int((bwn > 0).sum(-1).max())):
        zb = O.render_inverse_z_sampling(inter, ob[:, i], num_bg_sample, 1e6)
        for dt, npdt in ((F64, np.float64), (F32, f32)):
            r = bg_inference_v2(sc, o, d, zb, ob, i, dt)
            one = new_state(B, npdt)
            accumulate_color(one, *shape(r, num_bg_sample), zb, go=np.ones(B, bool))
            for k in acc[dt]:
                wk = bwn[:, i].astype(npdt)
                acc[dt][k] = (acc[dt][k] + (one[k] * (wk[:, None] if one[k].ndim == 2 else wk)).astype(npdt)).astype(npdt)
            if dt == F32:
                bg.append((zb, ob, i, r))
    out = {}
    for dt, name in ((F64, "f64"), (F32, "f32")):
        T = st[dt]["T"]
        out[name] = {"dif": st[dt]["dif"] + T[:, None] * acc[dt]["dif"], "spec": st[dt]["spec"] + T[:, None] * acc[dt]["spec"],
                     "depth": st[dt]["depth"] + T * acc[dt]["depth"], "T": T}
    out.update(tied=tied(starts_T + [st[F32]["T"]]), passes=passes, bg=bg)
    return out


@functools.lru_cache(maxsize=None)
def ray_reference(c):
    """The novel-view loop of a per-ray case on the scene's own arrays (the sampler's grid: fake_grid) -> (scene arrays, o, d,
    render_loop's dict); computed once per process, shared, never written to."""
    sc, o, d = family_scene(c.scene, c.family)
    sc = dict(sc, fake=fake_grid(sc))
    return sc, o, d, render_loop(sc, o, d, c.S, c.SB)


def accumulate_reference(c):
    """The accumulate_color op on its own, over a case's passes: the tracing passes in sequence (transmittance carried), then every
    background step from transmittance 1.  Input of all three -- the op, the float64 run, the float32 run -- are the float32
    per-sample values.  -> [(passes [(pts_dif [B,S,3], pts_spec, pts_alpha [B,S], z)], float64 state, float32 state, tied [B])]."""
    sc, o, d, loop = ray_reference(c)
    B = o.shape[0]
    shape = lambda r, z: (r["dif"].numpy().reshape(*z.shape, 3), r["spec"].numpy().reshape(*z.shape, 3), r["alpha"].numpy().reshape(z.shape), z)
    seqs = [[shape(r, z) for z, _, _, r in loop["passes"]]] + [[shape(r, zb)] for zb, _, _, r in loop["bg"]]
    out = []
    for seq in seqs:
        s32, gos, starts = accumulate_sequence(seq, f32)
        s64, _, _ = accumulate_sequence(seq, np.float64, gos)
        out.append((seq, s64, s32, tied(starts)))
    return out


# ------------------------------------------------------------------------------------------------------------ judgement
def judge_samples(name, got, r64, r32, k):
    """got = (dif [N,3], spec [N,3], alpha [N]) of an op against the float64 result: every quantity twice -- absolute, and over the
    sample's float64 alpha.  -> list of violations; one judge line per quantity and scale."""
    a64 = r64["alpha"].reshape(-1).abs()   # (a blend weight just outside a tile's box is negative, and so may the blended alpha be)
    N = a64.shape[0]
    bad = []
    for what, g in zip(("dif", "spec", "alpha"), got):
        g = torch.as_tensor(np.ascontiguousarray(g)).reshape(N, -1)
        ref64, ref32 = r64[what].reshape(N, -1), r32[what].reshape(N, -1)
        bad += judge(f"{name} {what} abs", g, ref64, ref32, k, scale=torch.ones(N, dtype=F64), floor=FLOOR)
        bad += judge(f"{name} {what} /alpha", g, ref64, ref32, k, scale=a64, floor=FLOOR)
    return bad


def judge_rays(name, got, r64, r32, k, keep):
    """got = {"dif", "spec" [B,3], "depth", "T" [B]} per ray against the float64 state, over the rays `keep` [B] bool"""
    sel = lambda a: torch.as_tensor(np.asarray(a, np.float64).reshape(len(keep), -1)[keep])
    ones = torch.ones(int(keep.sum()), dtype=F64)
    bad = []
    for what in ("dif", "spec", "T"):
        bad += judge(f"{name} {what}", sel(got[what]), sel(r64[what]), sel(r32[what]), k, scale=ones, floor=FLOOR)
    return bad + judge(f"{name} depth", sel(got["depth"]), sel(r64["depth"]), sel(r32["depth"]), k, floor=FLOOR)
