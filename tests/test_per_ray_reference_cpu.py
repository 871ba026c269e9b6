"""tests/per_ray_reference.py judged on its own, without a GPU: the input families hold the regimes they are named for, the
clamp-tie cap holds for every case tests/test_gpu_per_ray_ops.py runs, the closed-form adjoint csrc/composite.hip implements
equals autograd of the reference, and the epilogue reference equals a finite difference of its own forward."""
import numpy as np
import pytest
import torch

import per_ray_reference as P

F64 = torch.float64
IDS = [P.case_id(c) for c in P.ALL_CASES]


def _alpha32(c):
    sigma, _, _, _, _, dists, rays_d = P.case_inputs(c)
    delta = dists * rays_d.norm(dim=-1, keepdim=True)
    return sigma * delta, 1.0 - torch.exp(-sigma * delta)


@pytest.mark.parametrize("c", P.ALL_CASES, ids=IDS)
def test_family_conditions_and_clamp_tie_cap(c):
    """Conditions of the draws, not measurements of any op.  One of them cannot hold at every S the round-boundary cases need: the
    draws zero every seventh sample from the first, so a "base" ray of S = 1 composites nothing and one of S = 2 a single sample,
    and neither reaches the clamp without the `infinity` sample: the clamped / unclamped shares are asserted from S = 63 on and
    for batches large enough for a share to mean anything (B >= 261)."""
    ins, go, gw, r64, r32 = P.case_reference(c)
    x, alpha = _alpha32(c)
    assert all(torch.isfinite(t).all() for t in ins)
    share = lambda m: float(m.float().mean())
    kinds = {"base": [0], "opaque": [1], "empty": [2], "thin": [3], "mixed": [0, 1, 2, 3]}[c.family]
    fam = torch.arange(c.B) % 4 if c.family == "mixed" else torch.full((c.B,), kinds[0])
    if 1 in kinds and c.B >= 2:
        rows = fam == 1
        assert share((alpha[rows][:, :-1] == 1.0).any(1)) >= 0.9
    if 2 in kinds and c.B >= 3:
        rows = fam == 2
        assert float(r64["weights"][rows].abs().max()) == 0.0
        np.testing.assert_allclose(r64["out"][rows, 4].numpy(), (1.0 + 1e-6) ** (c.S - 1), rtol=1e-12)
    if 3 in kinds and c.B >= 4:
        assert float(x[fam == 3].max()) < 1e-2
    if 0 in kinds and c.B >= 261 and c.S >= 63:
        clamped = (r64["presum"] > 1.0).any(1)
        assert share(clamped) >= 0.05 and share(~clamped) >= 0.05, (share(clamped), share(~clamped))
    if c.B >= 5:
        assert float(ins[6][c.B - 1].abs().max()) == 0.0 and float(r64["rays_d"][c.B - 1].abs().max()) == 0.0
    assert share(ins[5][:, -1] > 1e-3) > 0.25 or c.B < 261
    # clamp ties
    tied = ~P.untied_rays(r64["presum"])
    assert int(tied.sum()) <= P.TIE_CAP * c.B, int(tied.sum())
    # the float32 reference is a finite yardstick everywhere, and a tight one on the ordinary draws
    keep = ~tied
    for name in P.GRAD_NAMES:
        f = P.figures(r32[name][keep], r64[name][keep], r64["dnorm_terms"][keep] if name == "rays_d" else None)
        assert all(np.isfinite(v) for v in f.values()), (name, f)
        if c.family == "base" and c.S >= 63:   # (S = 1, 2: the ray is one sample of dists = 1e-6, and 1 - exp(-x) at x ~ 1e-6 is float32's worst case)
            assert f["p99"] < 1e-5, (name, f)
    for name in ("out", "weights"):
        assert all(np.isfinite(v) for v in P.figures(r32[name], r64[name]).values())


def closed_form_adjoint(sigma, dif, spec, tint, z, dists, rays_d, g_out, g_w, infinity):
    """The header comment of k_composite_bwd (csrc/composite.hip) as float64 torch, no autograd:
      dL/dw_s     = g_depth z + g_dif . c_d + g_tint . t + g_spec . (t c_s) + g_w
      dL/dalpha_s = dL/dw_s T_s - (sum_{k>s} dL/dw_k w_k + g_Tleft T_left [s < S-1]) / u_s,   dalpha/dsigma = delta (1 - alpha)
    with the rgb column's gradient added to g_dif and g_spec where diffuse + specular lies inside the clamp."""
    sigma, dif, spec, tint, z, dists, rays_d, g_out, g_w = (t.to(F64) for t in (sigma, dif, spec, tint, z, dists, rays_d, g_out, g_w))
    B, S = z.shape
    dn = rays_d.norm(dim=-1, keepdim=True)
    delta = dists * dn
    live = torch.ones(B, S, dtype=F64)   # samples whose delta depends on |d|
    if infinity:
        delta = torch.cat([delta[:, :-1], torch.full((B, 1), 1e10, dtype=F64)], 1)
        live[:, -1] = 0.0
    E = torch.exp(-sigma * delta)   # = 1 - alpha, written as the exponential: behind alpha = 1 - 1e-20 the difference would be 0
    alpha = 1.0 - E
    u = 1.0 - alpha + 1e-6
    T = torch.cumprod(torch.cat([torch.ones(B, 1, dtype=F64), u], 1), 1)[:, :-1]
    w = alpha * T
    T_left = T[:, -1]
    presum = (w[..., None] * (dif + tint * spec)).sum(1)
    inside = ((presum >= 0) & (presum <= 1)).to(F64)
    gd = g_out[:, 5:8] + g_out[:, 0:3] * inside
    gs = g_out[:, 8:11] + g_out[:, 0:3] * inside
    gt = g_out[:, 11:14]
    gw = g_out[:, 3:4] * z + g_w + (gd[:, None] * dif + gt[:, None] * tint + gs[:, None] * tint * spec).sum(-1)
    incl = torch.flip(torch.cumsum(torch.flip(gw * w, [1]), 1), [1])
    later = torch.cat([incl[:, 1:], torch.zeros(B, 1, dtype=F64)], 1)   # (not incl - own: behind u = 1e-6 that difference loses ten digits)
    tl = (g_out[:, 4] * T_left)[:, None].repeat(1, S)
    tl[:, -1] = 0.0
    galpha = gw * T - (later + tl) / u
    g_dnorm = (galpha * sigma * E * dists * live).sum(1, keepdim=True)
    unit = torch.where(dn == 0, torch.zeros_like(rays_d), rays_d / torch.where(dn == 0, torch.ones_like(dn), dn))
    return {"sigma": galpha * delta * E, "diffuse": w[..., None] * gd[:, None],
            "tint": w[..., None] * (gt[:, None] + gs[:, None] * spec),
            "specular": w[..., None] * (gs[:, None] * tint + 2.0 * g_out[:, 14, None, None] * spec), "rays_d": g_dnorm * unit}


@pytest.mark.parametrize("infinity", [False, True])
@pytest.mark.parametrize("S", [1, 2, 65])
def test_closed_form_adjoint_equals_autograd_of_the_reference(S, infinity):
    """The formula the backward kernel implements is right: 1e-11 relative per ray against autograd of composite64."""
    B = 261
    ins = P.family_inputs("mixed", B, S, 600 + S)
    go, gw = P.upstream(B, S)
    ref = P.composite_grads(ins, go, gw, infinity)
    got = closed_form_adjoint(*ins, go, gw, infinity)
    for name in P.GRAD_NAMES:
        e = P.per_ray_errors(got[name], ref[name], ref["dnorm_terms"] if name == "rays_d" else None)
        assert float(e.max()) <= 1e-11, (name, float(e.max()))


def _epilogue_case(B, ntile, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(B, 3, generator=g) * (0.5 + torch.rand(B, 1, generator=g))
    blob = P.blob_with_harmonic_rows(torch.randn(16, 64, generator=g))
    return d, blob, torch.randn(B, 6, generator=g), torch.randn(B, ntile, generator=g), torch.randn(B, 2, 64, generator=g)


def test_epilogue_reference_equals_a_central_difference_of_its_forward():
    B = 8
    d, blob, rp, gdn, grs = _epilogue_case(B, 3, 5)
    g_o, g_d, scale = P.epilogue_grads(d, blob, rp, gdn, grs)
    assert torch.equal(g_o, rp[:, 0:3].double()) and bool((scale > 0).all())
    o, d64, h = torch.zeros(B, 3, dtype=F64), d.double(), 1e-6
    L = lambda dd: float(P.epilogue_loss(o, dd, blob, rp, gdn, grs, None, F64)[0])
    for b in range(B):
        for k in range(3):
            e = torch.zeros(B, 3, dtype=F64)
            e[b, k] = h
            fd = (L(d64 + e) - L(d64 - e)) / (2 * h)
            assert abs(fd - float(g_d[b, k])) <= 1e-6 * float(scale[b]), (b, k, fd, float(g_d[b, k]))
    g_o, g_d, scale = P.epilogue_grads(d, blob, rp, gdn, grs, ray_valid=torch.zeros(B, dtype=torch.bool))
    assert float(g_o.abs().max()) == 0.0 and float(g_d.abs().max()) == 0.0 and float(scale.abs().max()) == 0.0
    # a zero direction: only the degree-1 harmonics and the position path reach it, through 1 / 1e-8
    d[3] = 0.0
    _, g_d, _ = P.epilogue_grads(d, blob, rp, gdn, grs)
    assert torch.isfinite(g_d).all()


def test_per_ray_errors_and_judge_on_known_errors():
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1e-6, 0.0], [0.0, 0.0]], dtype=F64)
    got = ref.clone()
    got[0, 0] += 0.5
    got[2, 0] *= 2.0
    got[3, 1] = 1e-30
    e = P.per_ray_errors(got, ref)
    assert e[0] == 0.1 and e[1] == 0.0 and abs(float(e[2]) - 1.0) < 1e-12 and e[3] == float("inf")
    assert torch.equal(P.per_ray_errors(got, ref, torch.tensor([5.0, 0.0, 1.0, 1e-30], dtype=F64))[[1, 3]], torch.tensor([0.0, 1.0], dtype=F64))
    # the small ray decides the maximum although it is invisible in a whole-tensor figure
    ref32 = ref + torch.tensor([[1e-7, 0.0], [0.0, 0.0], [1e-13, 0.0], [0.0, 0.0]], dtype=F64)
    assert P.judge("same", ref32, ref, ref32) == []
    bad = P.judge("small ray wrong", got[:3], ref[:3], ref32[:3])
    assert any("max" in b for b in bad) and float((got[:3] - ref[:3]).abs().max() / ref.abs().max()) > 0
    # a zero figure of the float32 reference demands a zero figure of the op
    assert P.judge("exact", ref, ref, ref) == [] and P.judge("inexact", ref32, ref, ref) != []
