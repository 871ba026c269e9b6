"""Yardstick and case list of the surface-normal kernels (csrc/normals.hip; test infrastructure, CPU only, no GPU import).

The formulas, in a dtype of the caller's choice (float64 = the reference, float32 = the yardstick for how much rounding the problem
allows), behind float32-pinned sample points, cells and mask values (tests/gradient_reference64.py: pinned_points, pinned_cells,
corner_indices, mask64 -- a run with everything in float64 would move the points by an ulp, and the cell offset amplifies that by the
level's resolution):

    x_k = contract_fore(p)_k, A_k = 4 / bbox_size_k (float32, as the entry point forms it);  point form: x = p, A = axis_scale
    feat_l = sum_c w_c(t) tab_l[idx_c];   d feat_l / d p_k = A_k (res_l,k - 1) / 4 * sum_c (d w_c / d t_k) tab_l[idx_c]
    f = feat * mask;  u0 = W0 f + b0;  s = ws . (W1[:32] G(u0) + b1[:32]) + bs;  sigma = softplus(s);  G(u) = exp(-50 u^2)
    g_k = sigmoid(s) sum_j a_j G'(u0_j) (W0 (mask * d feat / d p_k))_j,   a = W1[:32]^T ws^T,  G'(u) = -100 u G(u)
    n = -g / (|g|_2 + 1e-8);   ray form: w_i of oracle.cal_integrate_weight -> (sum_i w_i n_i, sum_i w_i)

sigma itself comes out of oracle.mlp_forward on the interpolated features (the formula's s is asserted against it), the weights out
of oracle.cal_integrate_weight.

Judgement (tests/per_ray_reference.py's rule: a bound is never a number taken from the kernel, it is K x the error the float32
yardstick makes against float64 on the same inputs; median, 99th percentile, maximum and pooled):
  * per ray:     |out[:3] - n64|_2 / sum_i w_i,64;   sum_i w_i relative to its float64 value;
  * per sample:  |g - g64|_2 / |cond|_2 with cond_k = sum_j |d sigma / d feat_j| |d feat_j / d p_k| (float64): a sample whose terms
                 cancel is not held to a relative bound on the cancelled sum.
No ray and no sample is left out.  The yardstick's figure is taken as at least FLOOR = 2^-24 (half an ulp of float32 at the scale of
the denominator: with a handful of rays its error may be anything down to 0 by chance), and with fewer than 16 rays only the maximum
and the pooled figure bind (quantiles of three rays mean nothing).  K_QUANTILE / K_MAX: profiles/normals_error.md."""
import collections
import functools

import numpy as np
import torch

from gradient_reference64 import corner_indices, mask64, pinned_cells, pinned_points
from oracle import oracle as O
from per_ray_reference import figures, judge  # noqa: F401  (figures: re-exported for the profile tool)

F64, F32 = torch.float64, torch.float32

# Margins: the largest ratio (kernel's figure / max(float32 yardstick's figure, FLOOR)) over all cases of the first MI355X run of the
# finished tests, doubled and rounded up to a power of two: 2.71 and 3.18 (profiles/normals_error.md holds the run).
K_QUANTILE = 8.0   # median, 99th percentile, pooled
K_MAX = 8.0        # maximum
K = (K_QUANTILE, K_MAX)
FLOOR = 2.0 ** -24

Case = collections.namedtuple("Case", "family B S log2_T infinity half valid seed")
FAMILIES = ("base", "opaque", "empty", "aniso", "mask", "bias", "fresh", "scaled", "zero", "faces")
VALID = ("all", "none", "alternate")   # which rays ray_valid keeps ("all": no ray_valid tensor)


def case_id(c):
    return f"{c.family}-B{c.B}-S{c.S}-T{c.log2_T}-inf{int(c.infinity)}-{'f16' if c.half else 'f32'}-{c.valid}"


CASES_S = [Case("base", 65, S, 10 + i % 4, bool(i & 1), False, "all", 100 + S) for i, S in enumerate((1, 2, 15, 16, 17, 33, 128))]
CASES_B = [Case("base", B, 17, 10 + i % 4, not (i & 1), False, "all", 200 + B) for i, B in enumerate((1, 3, 63, 64, 65, 261))]
CASES_VALID = [Case("base", 65, 16, 11, False, False, v, 300) for v in VALID]
CASES_HALF = [Case("base", 65, 17, 12, True, True, "alternate", 400), Case("base", 3, 128, 13, False, True, "all", 401)]
CASES_FAMILY = [Case(f, 65, 33, 10 + i % 4, f == "opaque", half, "all", 500 + i) for i, f in enumerate(FAMILIES) for half in (False, True)]
CASE_LARGE = Case("base", 65, 33, 19, False, True, "all", 600)   # the shipped table size and resolutions [32, 2048], f16 as exported
ALL_CASES = CASES_S + CASES_B + CASES_VALID + CASES_HALF + CASES_FAMILY + [CASE_LARGE]

MASK_STEP_PARTLY, MASK_STEP_OPEN = 5000, 20000


# ------------------------------------------------------------------------------------------------------------------- inputs
def _boundary_coordinates(mn, sz, res0, n):
    """World coordinates (float32) whose level-0 cell offset is EXACTLY zero under the pinned float32 expressions."""
    out = []
    for i in range(1, int(res0) - 1):
        w0 = np.float32(mn + sz * i / (res0 - 1))
        for w in (w0, np.nextafter(w0, np.float32(np.inf)), np.nextafter(w0, np.float32(-np.inf))):
            x = (np.float32(w) - np.float32(mn)) / np.float32(sz) * np.float32(4.0) - np.float32(2.0)
            v = (x + np.float32(2.0)) / np.float32(4.0) * np.float32(res0 - 1)
            if v == np.floor(v):
                out.append(np.float32(w))
                break
    assert len(out) >= n, len(out)
    return np.asarray(out, np.float32)


def case_inputs(c):
    """-> dict: o, d [B,3], z, dist [B,S] (float32 numpy), table [16,T,2] torch (f32 or f16), res [16,3] int32 torch, sd (float32 state
    dict), mn, sz [3] float32 torch (the 2x box), step (coarse-to-fine mask), infinity, valid [B] bool numpy or None."""
    assert c.family in FAMILIES and c.valid in VALID
    rng = np.random.default_rng(c.seed)
    B, S, T = c.B, c.S, 2 ** c.log2_T
    size = np.asarray({"aniso": [8.0, 2.5, 20.0], "scaled": [4.0, 4.0, 4.0]}.get(c.family, [16.0, 16.0, 16.0]), np.float32)
    mn = -size / 2
    half = size / 2
    d = rng.normal(size=(B, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (B, 1))).astype(np.float32)
    # rays stay inside the box: |o| <= 0.35 half, z |d| <= 0.6 min(half)
    o = (rng.uniform(-0.35, 0.35, (B, 3)) * half).astype(np.float32)
    zmax = 0.6 * float(half.min()) / 1.5
    z = np.sort(rng.uniform(0.05 * zmax, zmax, (B, S)), 1).astype(np.float32)
    dist = np.concatenate([np.diff(z, axis=1), np.full((B, 1), zmax / max(S, 1), np.float32)], 1).astype(np.float32)
    res = O.level_resolutions(torch.from_numpy(size / size.min() * 32).int(), torch.from_numpy(size / size.min() * 2048).int())
    sd = O.init_mlp(seed=c.seed % 7 + 1, bias_scale=0.05 if c.family == "bias" else 0.0)
    scale = {"fresh": 1e-4, "scaled": 100.0, "zero": 0.0}.get(c.family, 0.5)
    g = torch.Generator().manual_seed(c.seed)
    table = torch.randn(16, T, 2, generator=g) * scale
    if c.family == "scaled":   # a table 200 times the usual 0.5 (in a small box) behind a first layer that takes it: tangents far
        sd["Spatial_MLP.mlp.0.weight"] = sd["Spatial_MLP.mlp.0.weight"] / 200.0   # outside f16's range on the fine levels
    if c.family == "opaque":   # sigma ~ 8, every interval 1: transmittance below 1e-5 within four samples
        sd["sigma_layer.mlp.0.bias"] = sd["sigma_layer.mlp.0.bias"] + 8.0
        dist = np.ones_like(dist)
    if c.family == "empty":    # sigma ~ 6e-6
        sd["sigma_layer.mlp.0.bias"] = sd["sigma_layer.mlp.0.bias"] - 12.0
    if c.family == "faces":
        # axis-parallel rays (o_k + z * 0 == o_k exactly): x on the box's upper face, y exactly on a cell boundary of level 0
        ys = _boundary_coordinates(float(mn[1]), float(size[1]), int(res[0, 1]), 4)
        d = np.zeros((B, 3), np.float32)
        d[:, 2] = rng.uniform(0.5, 1.5, B).astype(np.float32)
        o[:, 0] = np.where(np.arange(B) % 2 == 0, np.float32(mn[0] + size[0]), o[:, 0])
        o[:, 1] = ys[np.arange(B) % len(ys)]
    valid = None
    if c.valid == "none":
        valid = np.zeros(B, bool)
    elif c.valid == "alternate":
        valid = np.arange(B) % 2 == 0
    table = table.half() if c.half else table
    return {"o": o, "d": d, "z": z, "dist": dist, "table": table, "res": res.int(), "sd": sd, "mn": torch.from_numpy(mn), "sz": torch.from_numpy(size),
            "step": MASK_STEP_PARTLY if c.family == "mask" else MASK_STEP_OPEN, "infinity": c.infinity, "valid": valid}


# ------------------------------------------------------------------------------------------------------------------- the formulas
def _weights_and_tangents(t, dtype):
    """t [N,L,3] (tensor) -> w [N,L,8], dw [N,L,8,3] = d w_c / d t_k in `dtype` (corner c = dx << 2 | dy << 1 | dz)."""
    t = t.to(dtype)
    one = torch.ones((), dtype=dtype)
    w, dw = [], []
    for c in range(8):
        bit = [(c >> 2) & 1, (c >> 1) & 1, c & 1]
        f = [t[..., k] if bit[k] else one - t[..., k] for k in range(3)]
        s = [one if bit[k] else -one for k in range(3)]
        w.append(f[0] * f[1] * f[2])
        dw.append(torch.stack([s[0] * f[1] * f[2], f[0] * s[1] * f[2], f[0] * f[1] * s[2]], -1))
    return torch.stack(w, -1), torch.stack(dw, -2)


def sigma_normals(x, ascale, table, res, sd, mask, dtype=F64):
    """The point form at pinned contracted points x [N,3] float32 (numpy), ascale [3] float32, mask [32] (float32 values) ->
    {"sigma" [N], "s" [N], "g" [N,3], "n" [N,3], "cond" [N,3], "feat" [N,32], "dfeat" [N,32,3]} in `dtype`."""
    res = np.asarray(torch.as_tensor(res).numpy(), np.int32)
    b, t = pinned_cells(x, res)
    return evaluate_cells(b, torch.from_numpy(t), ascale, table, res, sd, mask, dtype)


def evaluate_cells(b, t, ascale, table, res, sd, mask, dtype=F64):
    """sigma_normals behind the cell location: cells b [N,L,3] int32 (numpy), offsets t [N,L,3] (tensor; the pinned float32 values,
    or float64 ones for a finite difference inside the cells)."""
    tab = torch.as_tensor(table).detach().to(dtype)
    T = tab.shape[1]
    idx = torch.from_numpy(corner_indices(b, T))                        # [N,L,8]
    w, dw = _weights_and_tangents(t, dtype)
    vals = tab[torch.arange(16)[None, :, None], idx]                    # [N,L,8,2]
    feat = (w[..., None] * vals).sum(2)                                  # [N,L,2]
    A = torch.from_numpy(np.asarray(ascale, np.float32)).to(dtype)
    scale = A[None, :] * (torch.from_numpy(res.astype(np.float32)).to(dtype) - 1) / 4     # [L,3]
    dfeat = (dw[:, :, :, None, :] * vals[..., None]).sum(2) * scale[None, :, None, :]      # [N,L,2,3]
    N = feat.shape[0]
    feat, dfeat = feat.reshape(N, 32), dfeat.reshape(N, 32, 3)
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    m = torch.as_tensor(mask).to(dtype)
    W0, b0 = sd["Spatial_MLP.mlp.0.weight"], sd["Spatial_MLP.mlp.0.bias"]
    W1, b1 = sd["Spatial_MLP.mlp.2.weight"], sd["Spatial_MLP.mlp.2.bias"]
    ws, bs = sd["sigma_layer.mlp.0.weight"][0], sd["sigma_layer.mlp.0.bias"][0]
    a = W1[:32].t() @ ws
    u0 = (feat * m) @ W0.t() + b0
    G = O.gaussian_act(u0)
    s = G @ a + (ws @ b1[:32] + bs)
    dirs = torch.zeros(N, 3, dtype=dtype)
    dirs[:, 0] = 1
    sigma = O.mlp_forward(sd, torch.cat([feat, dirs], -1), m)["sigma"][:, 0]
    assert torch.allclose(torch.nn.functional.softplus(s), sigma, rtol=1e-4 if dtype == F32 else 1e-10, atol=1e-30)
    dsdu = a * (-100.0 * u0 * G)                                         # [N,64]
    dsdf = (dsdu @ W0) * m                                               # [N,32] = d s / d feat
    sg = torch.sigmoid(s)
    g = sg[:, None] * torch.einsum("nj,njk->nk", dsdf, dfeat)
    cond = sg[:, None] * torch.einsum("nj,njk->nk", dsdf.abs(), dfeat.abs())
    n = -g / (g.norm(2, dim=-1, keepdim=True) + 1e-8)
    return {"sigma": sigma, "s": s, "g": g, "n": n, "cond": cond, "feat": feat, "dfeat": dfeat}


def ascale_of(sz):
    return (np.float32(4.0) / np.asarray(torch.as_tensor(sz).numpy(), np.float32)).astype(np.float32)


def render_normals(o, d, z, dist, table, res, sd, mn, sz, mask, infinity, dtype=F64, valid=None):
    """The ray form -> {"out" [B,4] = (sum w n, sum w), "w" [B,S], "x" [B*S,3] pinned float32 points, "pts": sigma_normals' dict}.
    Rays with valid == False give zeros."""
    B, S = z.shape
    x = pinned_points(o, d, z, False, mn, sz)
    pts = sigma_normals(x, ascale_of(sz), table, res, sd, mask, dtype)
    d_t = torch.as_tensor(d, dtype=F32).to(dtype)
    w, _ = O.cal_integrate_weight(pts["sigma"].reshape(B, S, 1), torch.as_tensor(dist, dtype=F32).to(dtype), d_t, infinity=infinity)
    w = w.to(dtype)
    out = torch.cat([(w * pts["n"].reshape(B, S, 3)).sum(1), w.sum(1)], 1)
    if valid is not None:
        out = out * torch.as_tensor(valid).to(dtype)[:, None]
    return {"out": out, "w": w[..., 0], "x": x, "pts": pts}


def case_mask(ins):
    return mask64(ins["step"]).to(F32)


@functools.lru_cache(maxsize=None)
def case_reference(c):
    """(inputs, float64 result, float32 result) of a case: computed once per process, shared, never written to."""
    ins = case_inputs(c)
    args = (ins["o"], ins["d"], ins["z"], ins["dist"], ins["table"], ins["res"], ins["sd"], ins["mn"], ins["sz"], case_mask(ins), ins["infinity"])
    return ins, render_normals(*args, dtype=F64, valid=ins["valid"]), render_normals(*args, dtype=F32, valid=ins["valid"])


# ------------------------------------------------------------------------------------------------------------------- judgement
def judge_rays(name, got_out, r64, r32, k=K):
    """got_out [B,4] against the float64 result: the composited normal per ray over sum_i w_i,64, and sum_i w_i relative to its
    float64 value.  -> list of violations."""
    B = r64["out"].shape[0]
    only = ("median", "p99", "max", "pooled") if B >= 16 else ("max", "pooled")
    got = torch.as_tensor(got_out).detach().cpu().to(F64)
    wsum = r64["out"][:, 3]
    bad = judge(name + " normal", got[:, :3], r64["out"][:, :3], r32["out"][:, :3], k, scale=wsum, only=only, floor=FLOOR)
    return bad + judge(name + " sum_w", got[:, 3:], r64["out"][:, 3:], r32["out"][:, 3:], k, only=only, floor=FLOOR)


def judge_samples(name, got_g, p64, p32, k=K):
    """got_g [N,3] (the unnormalised gradient) per sample over the float64 conditioning scale."""
    N = p64["g"].shape[0]
    only = ("median", "p99", "max", "pooled") if N >= 16 else ("max", "pooled")
    return judge(name + " grad", got_g, p64["g"], p32["g"], k, scale=p64["cond"].norm(dim=1), only=only, floor=FLOOR)
