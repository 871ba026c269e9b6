"""Cases, scenes and the per-element judgement of the warp-loss kernels (test infrastructure; CPU only, no GPU import).

tests/warp_reference.py stays the float64 restatement of the operation.  This module adds what a per-element comparison of
csrc/warp.hip with it needs, on the pattern of tests/per_ray_reference.py:

  * `scene`: a float32 scene builder with general cameras (skew, fx != fy, off-centre principal point, a roll about the optical
    axis -- every entry of R and of the first two rows of K non-zero and distinct), bit-identical duplicate cameras, blind cameras,
    rays that project into the half-pixel bands at the image border, and the clamp regimes of diffuse + specular;
  * the case lists (CASES_SELECT, CASES_PROJECT, CASES_LOSS) that tests/test_warp_cases_cpu.py and tests/test_gpu_warp_edges.py
    share: the CPU file asserts on the reference alone that every case contains the edge it is named for and that the rays left
    out stay under their caps, for exactly the cases the GPU file runs;
  * the references of the three entry points in a dtype of the caller's choice (float64 = the reference, float32 = the yardstick),
    built from warp_reference's functions, with the per-slot terms every per-ray and per-camera sum is formed of;
  * `judge` (per_ray_reference.judge with this module's margins): per slot, per ray and per camera, the kernel's median / 99th
    percentile / maximum / pooled figures against K x the float32 yardstick's own, floored at 2^-24.  No bound is a number taken
    from the kernel.  K_QUANTILE / K_MAX and the run they come from: profiles/warp_error.md.

How an element is scaled.  A slot's projection outputs: the error over the sum of the absolute values of the products that form
it (>= |value|).  A ray's gradient: the L2 error over the sum, over the ray's slots, of the absolute values of the per-slot terms
that are added (a ray whose slots cancel is not over-judged, a ray with a small gradient counts as much as any other).  A
camera's 12 grad_rts entries: the same over that camera's slots."""
import collections
import functools
import math

import torch

import per_ray_reference as PR
import warp_reference as WR

F64, F32 = torch.float64, torch.float32
TIE_BAND, TIE_CAP = PR.TIE_BAND, PR.TIE_CAP
FLOOR = 2.0 ** -24

# Margins of `judge`: the largest ratio (kernel's figure / float32 yardstick's figure) of the first GPU run of the finished tests
# over all cases, doubled and rounded up to a power of two (profiles/warp_error.md holds the run and the derivation).
K_QUANTILE = 16.0   # median, 99th percentile, pooled relative L2
K_MAX = 16.0        # maximum
K = (K_QUANTILE, K_MAX)

AMBIGUOUS_COST = 1e-5      # a cost this close to the 0.176 threshold, or to another camera's among the kept slots
AMBIGUOUS_BORDER = 1e-3    # px: a would-be neighbour this close to the image border
CAP_AMBIGUOUS = 0.03       # share of a case's rays that may be ambiguous (tests/test_gpu_warp.py's cap)
CAP_AMBIGUOUS_DUP = 0.005  # ... in the duplicate-camera scenes

MAX_NEIGHBORS = 16         # scanerf_warp_max_neighbors()


# ------------------------------------------------------------------------------------------------------------------ scenes
def _cameras(n, H, W, g, general, spread):
    """n cameras around the origin, looking at it -> ks [n,3,3], rts [n,3,4] world-to-camera, centres [n,3] (float64).  `spread`:
    elevations within +-60 degrees and radii 2.5 .. 4.5 instead of one jittered ring, and beyond 128 cameras all but about 128
    of them (the last one never) look away: hundreds of cameras that all see the scene tie in cost for most rays."""
    u = lambda: torch.rand(n, generator=g, dtype=F64)
    a = 0.37 + 2 * math.pi * torch.arange(n, dtype=F64) / n   # (off the axes: no entry of R is zero)
    if spread:
        a = 2 * math.pi * u()
        el = (u() * 2 - 1) * math.radians(60)
        r = 2.5 + 2.0 * u()
        c = torch.stack([r * el.cos() * a.cos(), r * el.sin(), r * el.cos() * a.sin()], 1)
    else:
        r = 3.0 * (1 + 0.1 * u())
        c = torch.stack([r * a.cos(), (0.08 + 0.2 * u()) * (1 - 2 * (torch.arange(n) % 2)), r * a.sin()], 1)
    z = -c / c.norm(dim=1, keepdim=True)
    x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=F64).expand(n, 3), z)
    x = x / x.norm(dim=1, keepdim=True)
    y = torch.linalg.cross(z, x)
    f = 0.625 * min(W, H * 4 / 3)
    ks = torch.zeros(n, 3, 3, dtype=F64)
    ks[:, 2, 2] = 1.0
    if general:
        th = (torch.randint(0, 4, (n,), generator=g) + 0.15 + 0.7 * u()) * math.pi / 2   # (off the axes too)
        x, y = th.cos()[:, None] * x + th.sin()[:, None] * y, -th.sin()[:, None] * x + th.cos()[:, None] * y
        ks[:, 0, 0] = f * (1.0 + 0.15 * u())
        ks[:, 1, 1] = f * (0.8 + 0.15 * u())
        ks[:, 0, 1] = 0.05 * f * (0.5 + u())
        ks[:, 1, 0] = -0.02 * f * (0.5 + u())
        ks[:, 0, 2] = (W - 1) / 2 + 0.05 * W * (2 * u() - 1)
        ks[:, 1, 2] = (H - 1) / 2 + 0.05 * H * (2 * u() - 1)
    else:
        ks[:, 0, 0] = ks[:, 1, 1] = f
        ks[:, 0, 2], ks[:, 1, 2] = W / 2, H / 2
    R = torch.stack([x, y, z], 1)
    t = -(R @ c[:, :, None])[:, :, 0]
    rts = torch.cat([R, t[:, :, None]], 2)
    if spread and n > 128:
        away = u() > 128.0 / n
        away[n - 1] = False
        rts = _look_away(rts, away.nonzero()[:, 0])
    return ks, rts, c


def _look_away(rts, idx):
    """Turn cameras idx by 180 degrees about their y axis (same centre): nothing of the scene is in front of them."""
    rts = rts.clone()
    rts[idx, 0] = -rts[idx, 0]
    rts[idx, 2] = -rts[idx, 2]
    return rts


REGIMES = ("inside", "above", "below", "zero", "one")


def clamp_regime(B):
    """[B,3] regime index of every channel of the clamp scene: channel c of ray b is REGIMES[(b + 2 c) % 5]."""
    return (torch.arange(B)[:, None] + 2 * torch.arange(3)[None, :]) % 5


Scene = collections.namedtuple("Scene", "ks rts images occlusions rays_o rays_d q ray_valid H W special")


def scene(N, B, H=48, W=64, seed=0, general=True, duplicates=False, blind=False, border=False, clamp=False, occl=True,
          ray_valid=None, spread=None):
    """A float32 CPU scene: ks [N,3,3], rts [N,3,4], images [N,H,W,3], occlusions [N,H,W] bool (None with occl=False), rays_o,
    rays_d [B,3], q [B,7] = (depth, diffuse, specular), ray_valid [B] bool or None.  Rays start near a camera centre and hit points
    near the origin.

      duplicates  camera j + N/2 is a bit-identical copy of camera j (N even).
      blind       every camera with index % 3 == 1 (but the last) looks away from the scene; the last camera looks down on it from
                  above, more than 60 degrees off every other ray, and owns exactly one valid slot: that of the last ray, which
                  starts at its centre (its occlusion mask is all true).  `special` = (that camera, that ray).
      border      every ray is aimed so that its owner camera sees its point in one of the four half-pixel bands at the image
                  border: pixel x in (0, 0.5) or (W - 1.5, W - 1) (grid x in (-0.5, 0) or (W - 2, W - 1.5)), or the same in y;
                  ray b takes band b % 4.
      clamp       diffuse + specular per channel by clamp_regime: inside (0, 1), above 1, below 0 (negative diffuse), exactly 0.0
                  (-0.25 + 0.25) and exactly 1.0 (0.25 + 0.75).
      ray_valid   None, "mixed" (about 85 % valid), "one" (only ray B // 2) or "none".
      spread      cameras over a sphere band instead of one ring (default: for N > 64)."""
    g = torch.Generator().manual_seed(seed)
    n_own = N // 2 if duplicates else (N - 1 if blind else N)
    spread = (N > 64) if spread is None else spread
    ks, rts, c = _cameras(n_own, H, W, g, general, spread)
    owners = torch.arange(n_own)
    special = None
    if blind:
        away = owners[owners % 3 == 1]
        rts = _look_away(rts, away)
        owners = owners[owners % 3 != 1]
        kt = _cameras(1, H, W, g, general, False)[0]
        # the extra camera: from (0.1, 3, 0.05) straight down, x along the world's x (then its own roll and K)
        top_c = torch.tensor([[0.1, 3.0, 0.05]], dtype=F64)
        zt = -top_c / top_c.norm()
        xt = torch.linalg.cross(torch.tensor([[0.0, 0.0, 1.0]], dtype=F64), zt)
        xt = xt / xt.norm()
        Rt = torch.stack([xt, torch.linalg.cross(zt, xt), zt], 1)
        rt = torch.cat([Rt, -(Rt @ top_c[:, :, None])], 2)
        ks, rts, c = torch.cat([ks, kt]), torch.cat([rts, rt]), torch.cat([c, top_c])
        special = (N - 1, B - 1)
    if duplicates:
        ks, rts, c = torch.cat([ks, ks]), torch.cat([rts, rts]), torch.cat([c, c])
    images = torch.rand(N, H, W, 3, generator=g)
    occ = (torch.rand(N, H, W, generator=g) > 0.2) if occl else None
    owner = owners[torch.randint(0, owners.numel(), (B,), generator=g)]
    p = (torch.rand(B, 3, generator=g, dtype=F64) - 0.5) * 1.0
    if border:
        band = torch.arange(B) % 4
        lo = 0.03 + 0.44 * torch.rand(B, generator=g, dtype=F64)
        px = 2 + (W - 5) * torch.rand(B, generator=g, dtype=F64)
        py = 2 + (H - 5) * torch.rand(B, generator=g, dtype=F64)
        px = torch.where(band == 0, lo, torch.where(band == 1, W - 1.5 + lo, px))
        py = torch.where(band == 2, lo, torch.where(band == 3, H - 1.5 + lo, py))
        zc = 2.5 + torch.rand(B, generator=g, dtype=F64)
        pix = torch.stack([px, py, torch.ones_like(px)], 1) * zc[:, None]
        cam = torch.linalg.solve(ks[owner], pix[:, :, None])[:, :, 0]
        R, t = rts[owner, :, :3], rts[owner, :, 3]
        p = (R.transpose(1, 2) @ (cam - t)[:, :, None])[:, :, 0]
    o = c[owner] + 0.05 * torch.randn(B, 3, generator=g, dtype=F64)
    if blind:
        if occ is not None:
            occ[N - 1] = True
        o[B - 1] = c[N - 1]
        p[B - 1] = torch.tensor([0.05, -0.1, 0.1], dtype=F64)
    depth = (0.5 + torch.rand(B, generator=g)).to(F32)
    o = o.to(F32)
    d = (p.to(F32) - o) / depth[:, None]
    colour = 0.6 * torch.rand(B, 6, generator=g)
    if clamp:
        reg = clamp_regime(B)
        r1, r2 = torch.rand(B, 3, generator=g), torch.rand(B, 3, generator=g)
        dif = torch.stack([0.02 + 0.43 * r1, 0.6 + 0.4 * r1, -0.5 - 0.3 * r1, torch.full_like(r1, -0.25), torch.full_like(r1, 0.25)])
        spec = torch.stack([0.02 + 0.43 * r2, 0.5 + 0.3 * r2, 0.3 * r2, torch.full_like(r2, 0.25), torch.full_like(r2, 0.75)])
        pick = lambda t: t.gather(0, reg[None])[0]
        colour = torch.cat([pick(dif), pick(spec)], 1)
    q = torch.cat([depth[:, None], colour], 1)
    rv = None
    if ray_valid == "mixed":
        rv = torch.rand(B, generator=g) > 0.15
        if special is not None:
            rv[special[1]] = True
    elif ray_valid == "one":
        rv = torch.zeros(B, dtype=torch.bool)
        rv[B // 2] = True
    elif ray_valid == "none":
        rv = torch.zeros(B, dtype=torch.bool)
    else:
        assert ray_valid is None, ray_valid
    return Scene(ks.to(F32).contiguous(), rts.to(F32).contiguous(), images, occ, o.contiguous(), d.contiguous(), q.contiguous(), rv,
                 H, W, special)


# ------------------------------------------------------------------------------------------------------------------ cases
SelectCase = collections.namedtuple("SelectCase", "name N B top_k ray_valid duplicates seed")
ProjectCase = collections.namedtuple("ProjectCase", "name N B H W supplied seed")
LossCase = collections.namedtuple("LossCase", "name N B top_k kind ray_valid zero_scores scale seed on_device")

CASES_SELECT = [SelectCase(f"N{N}-B{B}", N, B, 10, "mixed", False, 100 + N)
                for N, B in ((1, 1), (2, 255), (9, 256), (255, 257), (256, 1000), (257, 255), (513, 1000))]
CASES_SELECT += [SelectCase("N16-K16", 16, 257, 16, "mixed", False, 120),
                 SelectCase("N9-all-rays", 9, 257, 10, None, False, 121),
                 SelectCase("N9-no-valid-ray", 9, 257, 10, "none", False, 122)]
CASES_DUPLICATES = [SelectCase(f"dup-N{N}-K{k}", N, 1000, k, None, True, 130 + k) for N, k in ((24, 10), (24, 5), (24, 3), (40, 7))]
CASES_SELECT += CASES_DUPLICATES

CASES_PROJECT = [ProjectCase(f"{H}x{W}" + ("-supplied" if s else ""), 12, 1000, H, W, s, 200 + H + int(s))
                 for H, W in ((48, 64), (37, 53), (3, 2), (2, 2)) for s in (False, True)]


def _loss(name, N, B, top_k=10, kind="general", ray_valid="mixed", zero_scores=False, scale=1.0, seed=0, on_device=False):
    return LossCase(name, N, B, top_k, kind, ray_valid, zero_scores, scale, 300 + seed, on_device)


CASES_LOSS = [
    _loss("BK4090", 12, 409, seed=1),                     # one chunk of the grad_rts reduction ...
    _loss("BK4100", 12, 410, seed=2),                     # ... and two
    _loss("BK262150", 12, 26215, ray_valid=None, seed=3),  # 64 chunks of 4097 entries
    _loss("K1-B4096", 1, 4096, seed=4),
    _loss("K1-B4097", 1, 4097, seed=5),
    _loss("N2-B65541", 2, 65541, seed=6),                 # past one pass of the loss partials' 256 x 256 threads
    _loss("N1-B1048579", 1, 4096 * 256 + 3, ray_valid=None, seed=7, on_device=True),   # past the gradient kernel's grid cap
    _loss("B1", 12, 1, ray_valid=None, seed=19),
    _loss("N300-B2000", 300, 2000, seed=9),
    _loss("blind-N40", 40, 1500, kind="blind", seed=10),
    _loss("clamp", 12, 1000, kind="clamp", seed=11),
    _loss("border", 12, 800, kind="border", seed=12),
    _loss("all-rays", 12, 600, ray_valid=None, seed=13),
    _loss("one-valid-ray", 12, 600, ray_valid="one", seed=14),
    _loss("no-valid-ray", 12, 600, ray_valid="none", seed=15),
    _loss("zero-scores", 12, 600, zero_scores=True, seed=16),
    _loss("scale0.7", 12, 600, scale=0.7, seed=17),
]
CASE_NO_VALID_RAY = CASES_LOSS[14]
assert CASE_NO_VALID_RAY.ray_valid == "none"


def case_id(c):
    return c.name


@functools.lru_cache(maxsize=None)
def case_scene(c):
    """The scene of a case: built once per process, shared, never written to."""
    if isinstance(c, SelectCase):
        return scene(c.N, c.B, seed=c.seed, duplicates=c.duplicates, ray_valid=c.ray_valid)
    if isinstance(c, ProjectCase):
        sc = scene(c.N, c.B, H=c.H, W=c.W, seed=c.seed)
        if c.supplied:   # every third camera looks away, and the points lie anywhere along their rays: behind cameras, outside images
            stretch = 0.3 + 2.2 * torch.rand(c.B, 1, generator=torch.Generator().manual_seed(c.seed + 4))
            sc = sc._replace(rts=_look_away(sc.rts, torch.arange(1, c.N, 3)).contiguous(), rays_d=(sc.rays_d * stretch).contiguous())
        return sc
    return scene(c.N, c.B, seed=c.seed, blind=c.kind == "blind", border=c.kind == "border", clamp=c.kind == "clamp",
                 ray_valid=c.ray_valid)


def case_K(c):
    return min(c.top_k, c.N)


def case_scores(c, valid):
    """Scores in [0, 1) on the valid slots [B,K]; `zero_scores`: exactly 0 on every third slot."""
    B, Kn = valid.shape
    s = torch.rand(B, Kn, generator=torch.Generator().manual_seed(c.seed + 2))
    if c.zero_scores:
        s[(torch.arange(B)[:, None] + torch.arange(Kn)[None, :]) % 3 == 0] = 0.0
    return s * valid.cpu()


def supplied_slots(c, sc, K=10):
    """Caller-supplied slots of a projection case: views uniform in [-1, N] (both ends outside), valid_in all true.  With views drawn
    blindly the points lie behind many of the cameras and outside most images."""
    g = torch.Generator().manual_seed(c.seed + 3)
    views = torch.randint(-1, c.N + 1, (c.B, K), generator=g).to(torch.int32)
    return views, torch.ones(c.B, K, dtype=torch.bool)


# ------------------------------------------------------------------------------------------------------------------ selection
def points(sc, dtype=F64):
    return sc.rays_o.to(dtype) + sc.q[:, :1].to(dtype) * sc.rays_d.to(dtype)


def costs(sc, dtype=F64, H=None, W=None):
    return WR.view_costs(sc.rays_o.to(dtype), sc.rays_d.to(dtype), points(sc, dtype), sc.ks.to(dtype), sc.rts.to(dtype),
                         sc.H if H is None else H, sc.W if W is None else W)


def same_camera(sc):
    """[N,N] bool: cameras whose ks and rts are bit-identical (their costs are too: index decides their order)."""
    cam = torch.cat([sc.ks.reshape(-1, 9), sc.rts.reshape(-1, 12)], 1)
    return (cam[:, None, :] == cam[None, :, :]).all(-1)


def ambiguous_rays(sc, K):
    """[B] bool: rays whose selection float32 cannot decide.  Any of
      * a cost within AMBIGUOUS_COST of the 0.176 threshold;
      * among the K kept slots and the first one left out, two neighbours in the sorted order that are distinct, non-duplicate
        cameras within AMBIGUOUS_COST of each other, the lower at or below the threshold (cameras further down the order decide
        nothing that is returned);
      * a camera that would be a neighbour but for the image bounds projects within AMBIGUOUS_BORDER px of the border.
    Bit-identical duplicates are not ambiguous."""
    full = costs(sc)
    N = full.shape[1]
    amb = ((full - WR.VALID_COST).abs() < AMBIGUOUS_COST).any(1)
    srt, idx = torch.sort(full, dim=1, stable=True)
    m = min(K + 1, N)
    if m > 1:
        same = same_camera(sc)[idx[:, :m - 1], idx[:, 1:m]]
        close = ((srt[:, 1:m] - srt[:, :m - 1]) < AMBIGUOUS_COST) & (srt[:, :m - 1] <= WR.VALID_COST + AMBIGUOUS_COST)
        amb |= (close & ~same).any(1)
    ks, rts, pts = sc.ks.to(F64), sc.rts.to(F64), points(sc)
    uv = torch.einsum("nij,bnj->bni", ks, torch.einsum("nij,bj->bni", rts[:, :, :3], pts) + rts[None, :, :, 3])
    x, y = uv[..., 0] / uv[..., 2], uv[..., 1] / uv[..., 2]
    edge = torch.minimum(torch.minimum(x.abs(), (x - (sc.W - 1)).abs()), torch.minimum(y.abs(), (y - (sc.H - 1)).abs()))
    free = costs(sc, H=1e9, W=1e9)
    amb |= ((edge < AMBIGUOUS_BORDER) & (free <= WR.VALID_COST + AMBIGUOUS_COST)).any(1)
    return amb


def select_reference(sc, K, dtype=F64):
    return WR.select(costs(sc, dtype), K, sc.ray_valid)


def tie_model(cost_row, K, fixed):
    """Python model of k_select's sorted insert over one ray's costs -> the K camera indices.  fixed=False: the loop as it was (the
    new camera and the entry it displaces both move on under a strict <, so a carried entry that ties with the next one is dropped:
    the lower index goes); fixed=True: once the new camera is placed every later entry shifts."""
    best, bidx = [float("inf")] * K, [0] * K
    for i, cc in enumerate(cost_row):
        ci, placed = i, False
        for j in range(K):
            if placed or cc < best[j]:
                best[j], cc = cc, best[j]
                bidx[j], ci = ci, bidx[j]
                placed = fixed
    return bidx


# ------------------------------------------------------------------------------------------------------------------ projection
def project_reference(sc, views, dtype=F64):
    """warp_reference.project in `dtype` -> dict grid, proj_depth, nei_origin, nei_direction (views clamped into range: the
    caller masks the slots outside)."""
    v = views.long().clamp(0, sc.ks.shape[0] - 1)
    grid, depth, org, dirn = WR.project(points(sc, dtype), sc.ks.to(dtype), sc.rts.to(dtype), v)
    return {"grid": grid, "proj_depth": depth, "nei_origin": org, "nei_direction": dirn}


def project_scales(sc, views):
    """Per slot, the size of the sums each projection output is formed of (float64): |K| (|R| |p| + |t|) for the pixel, and so
    on.  Every scale is >= the magnitude of the value it scales."""
    v = views.long().clamp(0, sc.ks.shape[0] - 1)
    ks, rts = sc.ks.to(F64)[v].abs(), sc.rts.to(F64)[v]
    Ra, ta = rts[..., :3].abs(), rts[..., 3].abs()
    pa = sc.rays_o.to(F64).abs() + (sc.q[:, :1].to(F64) * sc.rays_d.to(F64)).abs()
    qa = (Ra @ pa[:, None, :, None])[..., 0] + ta
    pixa = (ks @ qa[..., None])[..., 0]
    ref = project_reference(sc, views)
    R, t = rts[..., :3], rts[..., 3]
    qz = ((R @ points(sc)[:, None, :, None])[..., 0] + t)[..., 2].abs() + 1e-8
    z = ref["proj_depth"].abs() + 1e-8
    g = pixa[..., :2].norm(dim=-1) / z + (ref["grid"] + 0.5).norm(dim=-1) * pixa[..., 2] / z + 0.5
    cam_d = torch.stack([qa[..., 0] / qz * (1 + qa[..., 2] / qz), qa[..., 1] / qz * (1 + qa[..., 2] / qz), torch.ones_like(qz)], -1)
    return {"grid": g, "proj_depth": pixa[..., 2], "nei_origin": (Ra.transpose(-1, -2) @ ta[..., None])[..., 0].norm(dim=-1),
            "nei_direction": (Ra.transpose(-1, -2) @ cam_d[..., None])[..., 0].norm(dim=-1)}


def color_reference(sc, grid, views, valid, dtype=F64):
    """warp_reference.sample_color on the given (the kernel's) grid -> colour [B,K,3], flags [B,K], and the per-slot scale: the sum
    of the absolute bilinear weights (pixel values are at most 1; the weights leave [0, 1] for slots outside the image)."""
    v = views.long().clamp(0, sc.ks.shape[0] - 1)
    color, flags = WR.sample_color(sc.images.to(dtype), sc.occlusions, grid.to(dtype), v, valid)
    g = grid.to(F64)
    lx = g[..., 0].long().clamp(0, sc.W - 2)
    ly = g[..., 1].long().clamp(0, sc.H - 2)
    ox, oy = g[..., 0] - lx, g[..., 1] - ly
    scale = ((1 - ox).abs() + ox.abs()) * ((1 - oy).abs() + oy.abs())
    return color, flags, scale


# ------------------------------------------------------------------------------------------------------------------ loss
def loss_reference(sc, views, valid, score, corner_grid, scale, dtype=F64, device="cpu"):
    """The loss and its gradients in `dtype` by torch autograd of warp_reference's functions, with selection, flags, scores and the
    bilinear corners (corner_grid: the kernel's grid) frozen.

    Every (ray, slot) is handed to warp_reference as a ray of its own with one slot and a camera of its own (rts[views], ks[views]),
    so that autograd keeps the per-slot terms: the per-ray gradients are their sums over the slots, grad_rts their sums over each
    camera's slots (in index order), and the conditioning scales the same sums of their absolute values.

    -> dict loss (float), grad_q [B,7], grad_o, grad_d [B,3], grad_rts [N,3,4], owned [N] bool (cameras with a slot that counts),
    and scales grad_depth, grad_color, grad_o, grad_d [B], grad_rts [N]."""
    dev = torch.device(device)
    N = sc.ks.shape[0]
    B, Kn = views.shape
    t = lambda x, dt=dtype: x.detach().to(dev, dt)
    rv = None if sc.ray_valid is None else sc.ray_valid.to(dev)
    v = views.to(dev).long()
    valid = valid.to(dev) & (v >= 0) & (v < N)
    if rv is not None:
        valid = valid & rv[:, None]
    v = v.clamp(0, N - 1)
    n = B if rv is None else int(rv.sum())
    o, d, q = (t(x).requires_grad_(True) for x in (sc.rays_o, sc.rays_d, sc.q))
    pts = o + q[:, :1] * d
    flat = lambda x: x[:, None].expand((B, Kn) + x.shape[1:]).reshape((B * Kn,) + x.shape[1:])
    pts_s, dif_s, spec_s = flat(pts), flat(q[:, 1:4]), flat(q[:, 4:7])
    rts_s = t(sc.rts)[v.reshape(-1)].requires_grad_(True)
    for x in (pts_s, dif_s, spec_s):
        x.retain_grad()
    own = torch.arange(B * Kn, device=dev)[:, None]
    grid, _, _, _ = WR.project(pts_s, t(sc.ks)[v.reshape(-1)], rts_s, own)
    color, _ = WR.sample_color(t(sc.images), None, grid, v.reshape(-1, 1), valid.reshape(-1, 1), t(corner_grid, F64).reshape(-1, 1, 2))
    s = torch.where(valid, t(score), torch.zeros((), dtype=dtype, device=dev)).reshape(-1, 1)
    if n:
        loss = scale * WR.compute_loss(dif_s, spec_s, color, s, n * Kn)
    else:
        loss = (s.sum() + pts_s.sum() + dif_s.sum() + spec_s.sum() + rts_s.sum()) * 0.0
    loss.backward()
    per = lambda x: x.grad.reshape(B, Kn, -1)
    gp, gc = per(pts_s), torch.cat([per(dif_s), per(spec_s)], 2)
    da, depth = d.detach().abs(), q.detach()[:, 0].abs()
    gpa = gp.abs().sum(1)
    counts = valid.reshape(-1)
    g_rts = _per_camera_sum(rts_s.grad.reshape(-1, 12), v.reshape(-1), N)
    a_rts = _per_camera_sum(rts_s.grad.reshape(-1, 12).abs(), v.reshape(-1), N)
    owned = torch.zeros(N, dtype=torch.bool, device=dev)
    owned[v.reshape(-1)[counts]] = True
    return {"loss": float(loss.detach()), "grad_q": q.grad, "grad_o": o.grad, "grad_d": d.grad, "grad_rts": g_rts.reshape(N, 3, 4),
            "owned": owned, "n_valid_slots": int(counts.sum()),
            "scale": {"grad_depth": (gpa * da).sum(1), "grad_color": gc.abs().sum(1).norm(dim=1), "grad_o": gpa.norm(dim=1),
                      "grad_d": depth * gpa.norm(dim=1), "grad_rts": a_rts.norm(dim=1)}}


def _per_camera_sum(x, v, N):
    """[N,12]: the rows of x summed per camera v.  On the CPU index_add_ adds them in index order; on a device it would add them
    with atomics (in no fixed order, and slowly where a million rows meet one camera), so there each camera's rows are masked
    and summed."""
    if x.is_cuda:
        return torch.stack([x[v == n].sum(0) for n in range(N)])
    return torch.zeros(N, x.shape[1], dtype=x.dtype).index_add_(0, v, x)


def untied_rays(sc):
    """[B] bool: rays whose float64 diffuse + specular stays TIE_BAND away from 0 and from 1 in every channel, or sits on one of
    them exactly (the clamp passes the gradient at 0.0 and at 1.0 in every precision; nearer than TIE_BAND but not on it, float32
    rounding decides)."""
    s = sc.q[:, 1:4].to(F64) + sc.q[:, 4:7].to(F64)
    near = lambda x: ((s - x).abs() <= TIE_BAND) & (s != x)
    return ~(near(0.0) | near(1.0)).any(1)


def loss_quantities(res, ref64, keep):
    """The per-ray and per-camera rows `judge` compares -> {name: (rows of res, rows of ref64, scale)}; `keep` [B] bool: the rays
    judged on the colour gradient (untied_rays)."""
    own = ref64["owned"].cpu()
    k = keep.cpu()
    s = {n: x.cpu() for n, x in ref64["scale"].items()}
    c = lambda x: x.detach().cpu()
    return {"grad_depth": (c(res["grad_q"])[:, :1], c(ref64["grad_q"])[:, :1], s["grad_depth"]),
            "grad_color": (c(res["grad_q"])[k, 1:7], c(ref64["grad_q"])[k, 1:7], s["grad_color"][k]),
            "grad_o": (c(res["grad_o"]), c(ref64["grad_o"]), s["grad_o"]),
            "grad_d": (c(res["grad_d"]), c(ref64["grad_d"]), s["grad_d"]),
            "grad_rts": (c(res["grad_rts"])[own].reshape(-1, 12), c(ref64["grad_rts"])[own].reshape(-1, 12), s["grad_rts"][own])}


def judge(name, got, ref64, ref32, scale=None, k=None):
    """per_ray_reference.judge with this module's margins, the float32 yardstick's figures floored at 2^-24."""
    return PR.judge(name, got, ref64, ref32, k=K if k is None else k, scale=scale, floor=FLOOR)


def judge_loss(name, res, ref64, ref32, keep):
    """Every quantity of a loss case -> the list of violations (empty = pass); prints one line per quantity."""
    bad = []
    got, yard = loss_quantities(res, ref64, keep), loss_quantities(ref32, ref64, keep)
    for qn, (g, r, s) in got.items():
        if r.shape[0]:
            bad += judge(f"{name} {qn}", g, r, yard[qn][0], scale=s)
    one = lambda x: torch.tensor([[float(x)]], dtype=F64)
    bad += judge(f"{name} loss", one(res["loss"]), one(ref64["loss"]), one(ref32["loss"]))
    return bad


@functools.lru_cache(maxsize=None)
def cpu_pipeline(c):
    """A loss case on the reference alone (what tests/test_warp_cases_cpu.py looks at): the float32 restatement stands in for the
    kernels' selection, grid and flags -> (scene, views, flags, grid32, score)."""
    sc = case_scene(c)
    Kn = case_K(c)
    views, _, valid = select_reference(sc, Kn, F32)
    grid = project_reference(sc, views, F32)["grid"]
    _, flags, _ = color_reference(sc, grid, views, valid, F32)
    return sc, views, flags, grid, case_scores(c, flags)
