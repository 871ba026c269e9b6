"""Per-ray references for the tail of a training step (test infrastructure; CPU only, no GPU import).

What they restate, each in a dtype of the caller's choice (float64 = the reference, float32 = the yardstick):

  * the stand-alone compositing op (csrc/composite.hip, render.CompositeRays): the reference's sequence
    (hashgrid/__init__.py:344-366, :564-574, :591-594) with the weights from oracle.cal_integrate_weight, under torch autograd;
  * the ray-gradient epilogue (csrc/loss.hip k_ray_grad_epilogue, render.ray_gradients_fused): the |d| path and the path through
    oracle.sh_deg3(d / (|d| + 1e-8)) and the directional layer's harmonic rows, under torch autograd;
  * the two photometric-loss entries of csrc/loss.hip.

How an op is judged (`judge`): per RAY, not per tensor.  A ray's error is the L2 norm of its error over the L2 norm of its float64
value (or over a conditioning scale where the value is a sum formed with cancellation), so a ray whose gradients are a thousand
times smaller than the batch's largest counts as much as any other.  The bound is never a number taken from the kernel: it is
K x the error the SAME reference code makes in float32 on the SAME inputs against float64 -- median, 99th percentile, maximum and
pooled relative L2 over the rays.  K_QUANTILE / K_MAX and the table they come from: profiles/per_ray_ops_error.md.

The case list of tests/test_gpu_per_ray_ops.py lives here (CASES_*), so that tests/test_per_ray_reference_cpu.py asserts the
families' conditions and the clamp-tie cap for exactly the cases the GPU file runs."""
import collections
import functools

import numpy as np
import torch

from oracle import oracle as O
from test_gpu_composite import _inputs

F64, F32 = torch.float64, torch.float32

# Margins of `judge`: the largest ratio (op's figure / float32 reference's figure) of the first GPU run of the finished tests over
# all cases, doubled and rounded up to a power of two (profiles/per_ray_ops_error.md holds the run and the derivation).
K_QUANTILE = 16.0  # median, 99th percentile, pooled relative L2
K_MAX = 32.0       # maximum over the rays
K = (K_QUANTILE, K_MAX)

S_MAX_BACKWARD = 512   # scanerf_composite_backward keeps the transmittance entering each round of 64 samples in 8 registers

Case = collections.namedtuple("Case", "family B S infinity seed")
FAMILIES = ("base", "opaque", "empty", "thin", "mixed")

CASES_ROUNDS = [Case("base", 261, S, inf, 1000 + S) for S in (1, 2, 63, 64, 65, 129, 449, 512) for inf in (False, True)]
CASES_REGIMES = [Case(f, 261, S, inf, 2000 + S) for f in ("opaque", "empty", "thin") for S in (65, 512) for inf in (False, True)]
CASES_TINY = [Case("mixed", B, 65, inf, 3000 + B) for B in (1, 3, 5) for inf in (False, True)]
CASE_PAST_CAP = Case("mixed", 16384 + 5, 65, True, 4000)
CASES_S513 = [Case("base", 261, 513, inf, 5000) for inf in (False, True)]
ALL_CASES = CASES_ROUNDS + CASES_REGIMES + CASES_TINY + [CASE_PAST_CAP] + CASES_S513

TIE_BAND = 1e-5     # a ray whose float64 diffuse + specular lies this close to 1 in a channel is left out of the gradient judgement
TIE_CAP = 1e-3      # ... and at most this share of a case's rays may be


def case_id(c):
    return f"{c.family}-B{c.B}-S{c.S}-inf{int(c.infinity)}"


# ------------------------------------------------------------------------------------------------------------ input families
def family_inputs(family, B, S, seed):
    """(sigma [B,S], diffuse, specular, tint [B,S,3], z [B,S], dists [B,S], rays_d [B,3]) in float32: the draws of
    test_gpu_composite._inputs, then
      * in half the rays the last dists entry becomes an ordinary interval instead of 1e-6 (the last sample carries weight when
        `infinity` is off),
      * the last ray of every batch of 5 or more has rays_d = 0,
      * the family's density: "base" unchanged; "opaque" one sample per ray at a random index set to 4000 (dists >= 0.01 and
        |d| >= 0.5: sigma delta >= 20, alpha == 1.0f); "empty" all zero; "thin" x 1e-3; "mixed" ray i takes family i mod 4 of
        (base, opaque, empty, thin)."""
    assert family in FAMILIES
    sigma, dif, spec, tint, z, dists, rays_d = _inputs(B, S, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    ordinary = torch.rand(B, generator=g) < 0.5
    last = torch.rand(B, generator=g) * 0.1 + 0.01
    dists[:, -1] = torch.where(ordinary, last, dists[:, -1])
    hit = torch.randint(0, S, (B,), generator=g)
    if B >= 5:
        rays_d[B - 1] = 0.0
    which = {"base": 0, "opaque": 1, "empty": 2, "thin": 3}
    fam = torch.arange(B) % 4 if family == "mixed" else torch.full((B,), which[family])
    opaque = sigma.clone()
    opaque[torch.arange(B), hit] = 4000.0
    sigma = torch.where((fam == 1)[:, None], opaque, sigma)
    sigma = torch.where((fam == 2)[:, None], torch.zeros_like(sigma), sigma)
    sigma = torch.where((fam == 3)[:, None], sigma * 1e-3, sigma)
    return sigma, dif, spec, tint, z, dists, rays_d


def case_inputs(c):
    return family_inputs(c.family, c.B, c.S, c.seed)


def upstream(B, S, seed=7):
    """Random upstream gradients on columns 0..14 of out_ray and on the weights (tests/test_gpu_composite.py's)."""
    g = torch.Generator().manual_seed(seed)
    go = torch.randn(B, 16, generator=g)
    go[:, 15] = 0.0
    gw = torch.randn(B, S, generator=g) * 0.1
    return go, gw


# ------------------------------------------------------------------------------------------------------------ compositing
_UNIT = torch.tensor([[1.0, 0.0, 0.0]])


def composite64(sigma, dif, spec, tint, z, dists, rays_d, infinity, dtype=F64):
    """The reference's compositing in `dtype` -> {"out" [B,16] (out_ray's columns), "weights" [B,S], "presum" [B,3] = diffuse +
    specular before the clamp, "delta" [B,S] = dists |d|}.  The weights are oracle.cal_integrate_weight's: it is handed delta as
    its `dists` and a unit direction (so its own `dists * |d|` multiplies by exactly 1.0), which leaves delta a tensor of this
    graph whose gradient is kept per sample (retain_grad): the conditioning scale of the rays_d gradient needs it."""
    sigma, dif, spec, tint, z, dists, rays_d = (t.to(dtype) for t in (sigma, dif, spec, tint, z, dists, rays_d))
    B, S = z.shape
    delta = dists * rays_d.norm(dim=-1, keepdim=True)
    if delta.requires_grad:
        delta.retain_grad()
    w, T_left = O.cal_integrate_weight(sigma.reshape(B, S, 1), delta, _UNIT.to(dtype).expand(B, 3), infinity=infinity)
    w, T_left = w.to(dtype), T_left.to(dtype)
    acc = lambda v: (w * v).sum(1)
    diffuse, tn, specular = acc(dif), acc(tint), acc(tint * spec)
    out = torch.cat([torch.clamp(diffuse + specular, 0, 1), acc(z[..., None]), T_left[:, None], diffuse, specular, tn,
                     (w.detach() * spec ** 2).sum((1, 2))[:, None], torch.zeros(B, 1, dtype=dtype)], 1)
    return {"out": out, "weights": w[..., 0], "presum": diffuse + specular, "delta": delta}


GRAD_NAMES = ("sigma", "diffuse", "specular", "tint", "rays_d")


def composite_grads(inputs, g_out, g_w, infinity, dtype=F64):
    """Forward and torch autograd of sum(out * g_out) + sum(weights * g_w) in `dtype` -> the gradients of sigma, diffuse, specular,
    tint and rays_d, the forward's "out" / "weights" / "presum", and "dnorm_terms" [B] = sum_s |dL/d(delta_s) dists_s| (the
    `infinity` sample left out, as the kernel leaves it out): the size of the terms of the one per-ray sum the backward forms with
    cancellation, dL/d|d| -- the scale on which the rays_d gradient is judged."""
    leaf = [t.detach().to(dtype).clone().requires_grad_(i in (0, 1, 2, 3, 6)) for i, t in enumerate(inputs)]
    r = composite64(*leaf, infinity, dtype)
    ((r["out"] * g_out.to(dtype)).sum() + (r["weights"] * g_w.to(dtype)).sum()).backward()
    terms = (r["delta"].grad * leaf[5]).abs()
    if infinity:
        terms = terms[:, :-1]
    res = {n: leaf[i].grad for n, i in zip(GRAD_NAMES, (0, 1, 2, 3, 6))}
    res.update(out=r["out"].detach(), weights=r["weights"].detach(), presum=r["presum"].detach(), dnorm_terms=terms.sum(1))
    return res


def untied_rays(presum64):
    """[B] bool: rays whose float64 diffuse + specular stays TIE_BAND away from 1 in every channel.  Nearer than that, float32
    rounding decides on which side of the clamp the ray falls, and the rgb column's upstream gradient passes or not."""
    return ((presum64 - 1.0).abs() > TIE_BAND).all(1)


# ------------------------------------------------------------------------------------------------------------ ray-gradient epilogue
BLOB_FLOATS = 13994
W_SH_OFFSET = 6503 + 64 + 32 * 64   # Directional_MLP.mlp.0: [bias 64][W^T 48 x 64]; rows 32..47 of W^T take the harmonics


def blob_with_harmonic_rows(rows):
    """A decoder blob (oracle.pack_blob's layout), zero but for the [16, 64] harmonic rows of the directional layer's W^T."""
    blob = torch.zeros(BLOB_FLOATS, dtype=F32)
    blob[W_SH_OFFSET:W_SH_OFFSET + 16 * 64] = rows.reshape(-1).to(F32)
    return blob


def epilogue_loss(rays_o, rays_d, blob, g_raypos, g_dnorm, g_rowsum, ray_valid, dtype):
    """The scalar whose gradients w.r.t. rays_o / rays_d the epilogue forms: the position path's per-ray gradients as given
    (g_raypos [B,6]), g_dnorm [B,ntile] on |d|, and g_rowsum [B,2,64] -- row sums of the directional layer-0 pre-activation gradient --
    through W[:, 32:48] onto sh_deg3(d / (|d| + 1e-8)).  Masked rays contribute nothing.  Also returns the unit vector (a graph
    tensor: its gradient is the conditioning scale)."""
    W = O.unpack_blob(blob)["Directional_MLP.mlp.0.weight"].to(dtype)   # [64, 48]
    g_sh = g_rowsum.to(dtype).sum(1) @ W[:, 32:48]
    g_dn = g_dnorm.to(dtype).sum(1)
    rp = g_raypos.to(dtype)
    keep = torch.ones(rays_d.shape[0], dtype=dtype) if ray_valid is None else ray_valid.to(dtype)
    dn = rays_d.norm(2, dim=-1)
    u = rays_d / (dn[:, None] + 1e-8)
    per_ray = (O.sh_deg3(u) * g_sh).sum(1) + g_dn * dn + (rp[:, 0:3] * rays_o).sum(1) + (rp[:, 3:6] * rays_d).sum(1)
    return (per_ray * keep).sum(), u


def epilogue_grads(rays_d, blob, g_raypos, g_dnorm, g_rowsum, ray_valid=None, dtype=F64):
    """-> (dL/d(rays_o) [B,3], dL/d(rays_d) [B,3], scale [B]) by torch autograd of epilogue_loss.  scale = |dL/du| / (|d| + 1e-8) +
    |sum g_dnorm| + |g_raypos[:, 3:6]|: the size of the terms dL/d(rays_d) is the sum of.  (The normalisation removes the radial
    part of dL/du, so for a gradient along d the result is the rounding of a difference and only this scale says how large that
    may be.)"""
    o = torch.zeros(rays_d.shape, dtype=dtype, requires_grad=True)
    d = rays_d.detach().to(dtype).clone().requires_grad_(True)
    L, u = epilogue_loss(o, d, blob, g_raypos, g_dnorm, g_rowsum, ray_valid, dtype)
    u.retain_grad()
    L.backward()
    keep = 1.0 if ray_valid is None else ray_valid.to(dtype)
    scale = u.grad.norm(dim=-1) / (d.detach().norm(dim=-1) + 1e-8) + \
        (g_dnorm.to(dtype).sum(1).abs() + g_raypos.to(dtype)[:, 3:6].norm(dim=-1)) * keep
    return o.grad, d.grad, scale


# ------------------------------------------------------------------------------------------------------------ losses
def _mean_sq(pred, tgt, v):
    n = int(v.sum())
    return ((pred[v] - tgt[v]) ** 2).sum() / (3 * n) if n else pred.sum() * 0.0


def _l2_term(col, v):
    n = int(v.sum())
    return col[v].sum() / (3 * n) if n else col.sum() * 0.0


def loss64(out, tgt, valid, reg):
    """photometric_loss_grad in float64 -> (loss, dL/d(out) [B,16]); no valid ray: loss 0, gradient 0."""
    leaf = out.detach().cpu().double().requires_grad_(True)
    v = torch.ones(leaf.shape[0], dtype=torch.bool) if valid is None else valid.cpu().bool()
    L = _mean_sq(leaf[:, 0:3], tgt.cpu().double(), v) + reg * _l2_term(leaf[:, 14], v)
    L.backward()
    return float(L), leaf.grad


def loss_fgbg64(fg, bg, tgt, vf, vb, reg):
    """photometric_loss_grad_fgbg in float64: pred = fg.rgb + fg.T_left * bg.rgb, the mean over the rays valid in either branch,
    + reg * each branch's l2_reg_specular over its own valid rays; a branch without a valid ray contributes no l2 term (as
    oracle.render_rays) -> (loss, dL/d(fg), dL/d(bg))."""
    lf, lb = (t.detach().cpu().double().requires_grad_(True) for t in (fg, bg))
    vf, vb = vf.cpu().bool(), vb.cpu().bool()
    pred = lf[:, 0:3] + lf[:, 4:5] * lb[:, 0:3]
    L = _mean_sq(pred, tgt.cpu().double(), vf | vb) + reg * (_l2_term(lf[:, 14], vf) + _l2_term(lb[:, 14], vb))
    L.backward()
    return float(L), lf.grad, lb.grad


# ------------------------------------------------------------------------------------------------------------ judgement
def _rows(t):
    t = torch.as_tensor(t).detach().cpu().to(F64)
    return t.reshape(t.shape[0], -1)


def per_ray_errors(got, ref64, scale=None):
    """[B] float64: per ray, |got - ref64|_2 / |ref64|_2, or / scale where given.  A ray whose error is exactly zero gives 0
    whatever the denominator (reference and result both exactly zero; a sum without terms); an error over a zero denominator is
    infinite."""
    got, ref = _rows(got), _rows(ref64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).norm(dim=1)
    den = ref.norm(dim=1) if scale is None else torch.as_tensor(scale).detach().cpu().to(F64).reshape(-1)
    safe = torch.where(den > 0, den, torch.ones_like(den))
    return torch.where(err == 0, torch.zeros_like(err), torch.where(den > 0, err / safe, torch.full_like(err, float("inf"))))


FIGURES = ("median", "p99", "max", "pooled")


def figures(got, ref64, scale=None):
    """median / 99th percentile / maximum of per_ray_errors, and the pooled relative L2 over all rays (the root of the summed
    squared errors over the root of the summed squared float64 values, or scales)."""
    e = per_ray_errors(got, ref64, scale)
    den = _rows(ref64).norm() if scale is None else torch.as_tensor(scale).detach().cpu().to(F64).norm()
    num = (_rows(got) - _rows(ref64)).norm()
    pooled = 0.0 if float(num) == 0 else (float(num / den) if float(den) > 0 else float("inf"))
    q = np.asarray(e.numpy(), np.float64)
    return {"median": float(np.median(q)), "p99": float(np.quantile(q, 0.99)), "max": float(q.max()), "pooled": pooled}


TABLE = []   # every judge() line of the process: tools and the error profile read it


def judge(name, got, ref64, ref32, k=K, scale=None, only=FIGURES, floor=0.0):
    """The op's four figures against k x the float32 reference's own (k = (for median / p99 / pooled, for the maximum)); where the
    float32 reference's figure is exactly 0 the op's must be 0 too.  Prints one line (name, the op's figures, the reference's, the
    ratios) and returns the list of violations -- empty when the op passes -- so that a test prints every tensor before it
    asserts.  `only`: the figures that bind (quantiles of five rays mean nothing); `floor`: the float32 reference's figure is
    taken as at least this (for a handful of rays, whose float32 error may be anything down to 0 by chance)."""
    a, b = figures(got, ref64, scale), figures(ref32, ref64, scale)
    ratio = {f: (0.0 if a[f] == 0 else (a[f] / b[f] if b[f] > 0 else float("inf"))) for f in FIGURES}
    fmt = lambda d: " / ".join(f"{d[f]:.2e}" for f in FIGURES)
    line = f"{name}: op {fmt(a)} | f32 ref {fmt(b)} | ratio " + " / ".join(f"{ratio[f]:.2f}" for f in FIGURES)
    if floor:
        line += "  [few rays: bound from the rounding floor]"
    print(line)
    TABLE.append(line)
    bad = []
    for f in only:
        bound = (k[1] if f == "max" else k[0]) * max(b[f], floor)
        if not (np.isfinite(a[f]) and a[f] <= bound):
            bad.append(f"{name} {f}: {a[f]:.3e} > {bound:.3e} (ratio {ratio[f]:.2f})")
    return bad


@functools.lru_cache(maxsize=None)
def case_reference(c):
    """(inputs, g_out, g_w, composite_grads in float64, composite_grads in float32) of a case: computed once per process, shared by
    the tests that need it, and never written to."""
    ins = case_inputs(c)
    go, gw = upstream(c.B, c.S)
    return ins, go, gw, composite_grads(ins, go, gw, c.infinity, F64), composite_grads(ins, go, gw, c.infinity, F32)
