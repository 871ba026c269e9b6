"""The per-ray tail of a training step -- scanerf_composite_forward / _backward (csrc/composite.hip, render.CompositeRays),
scanerf_ray_grad_epilogue and the two photometric-loss entries (csrc/loss.hip) -- judged PER RAY against float64 at the edges of
their launch shapes: round boundaries of the 64-sample rounds, the last legal S, batches past the grid caps (the second trip of the
grid-stride loops), partial last blocks, B < 4, and the density regimes where a carry or a 1/u term can be wrong without moving a
whole-tensor figure (opaque, empty, thin rays; a zero direction).  References, input families, case list and the judgement:
tests/per_ray_reference.py; the margins and the run they come from: profiles/per_ray_ops_error.md."""
import numpy as np
import pytest
import torch

import per_ray_reference as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_IN = (0, 1, 2, 3, 6)
COLUMNS = {"rgb": slice(0, 3), "depth": slice(3, 4), "T_left": slice(4, 5), "diffuse": slice(5, 8), "specular": slice(8, 11),
           "tint": slice(11, 14), "w_spec2": slice(14, 15)}
FLOOR = 2.0 ** -24   # half an ulp: where one ray (or five) is all there is, no float32 evaluation is asked to do better than one rounding


def _render():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import render
    return render


def _op(c, grad=True, rows=None):
    """render.composite_rays on a case's inputs (optionally its first `rows` rays) -> out, weights, {name: gradient} on the CPU."""
    render = _render()
    ins, go, gw, _, _ = P.case_reference(c)
    n = c.B if rows is None else rows
    dev_in = [t[:n].to(DEV).requires_grad_(grad and i in GRAD_IN) for i, t in enumerate(ins)]
    out, w = render.composite_rays(*dev_in, c.infinity)
    grads = {}
    if grad:
        ((out * go[:n].to(DEV)).sum() + (w * gw[:n].to(DEV)).sum()).backward()
        grads = {name: dev_in[i].grad.cpu() for name, i in zip(P.GRAD_NAMES, GRAD_IN)}
    return out.detach().cpu(), w.detach().cpu(), grads


def _forward_close(out, w, r64, rows=slice(None)):
    """The project's own forward tolerances (tests/test_gpu_composite.py)."""
    for k, cs in COLUMNS.items():
        np.testing.assert_allclose(out[rows, cs].numpy(), r64["out"][rows, cs].numpy(), rtol=2e-5, atol=2e-6, err_msg=k)
    assert float(out[rows, 15].abs().max()) == 0.0
    np.testing.assert_allclose(w[rows].numpy(), r64["weights"][rows].numpy(), rtol=2e-5, atol=1e-7, err_msg="weights")


def _judge_forward(tag, out, w, r64, r32, rows=slice(None), **kw):
    bad = []
    for k, cs in COLUMNS.items():
        bad += P.judge(f"{tag} {k}", out[rows, cs], r64["out"][rows, cs], r32["out"][rows, cs], **kw)
    return bad + P.judge(f"{tag} weights", w[rows], r64["weights"][rows], r32["weights"][rows], **kw)


def _judge_grads(tag, grads, r64, r32, rows=None, **kw):
    """Every gradient per ray; rays_d on the scale of the terms of its per-ray sum.  Rays at a clamp tie are left out."""
    keep = P.untied_rays(r64["presum"])
    if rows is not None:
        keep = keep & rows
    bad = []
    for name in P.GRAD_NAMES:
        scale = r64["dnorm_terms"][keep] if name == "rays_d" else None
        bad += P.judge(f"{tag} g_{name}", grads[name][keep], r64[name][keep], r32[name][keep], scale=scale, **kw)
    return bad


def _ids(cases):
    return [P.case_id(c) for c in cases]


@pytest.mark.parametrize("c", P.CASES_ROUNDS, ids=_ids(P.CASES_ROUNDS))
def test_composite_round_boundaries(c):
    """S = 1 (T_left = 1, no sample sees the g_Tleft term), 2, 63 / 64 / 65 (a one-lane round), 129, and the eighth round up to the
    last legal S, at a batch with a partial last block.  At S = 512 the all-empty zero-direction ray's T_left = (1 + 1e-6)^511 is where a float32 product of
    float32 factors misses the forward tolerance (1 + 1e-6 rounds to 1 + 9.5367e-7: 2.38e-5 over 511 factors, against the 2e-5 + 2e-6
    allowed): the kernels carry the transmittance in double."""
    _, _, _, r64, r32 = P.case_reference(c)
    out, w, grads = _op(c)
    bad = _judge_grads(P.case_id(c), grads, r64, r32)
    _forward_close(out, w, r64)
    assert not bad, bad


def test_zero_direction_guard_leaves_every_other_ray_bit_equal():
    """CompositeRays.backward: g_rays_d = g_dnorm d / |d| with a `where` on |d| == 0; for every other ray the very bits of the
    unguarded expression on the kernel's own g_dnorm."""
    render = _render()
    c = next(k for k in P.CASES_ROUNDS if k.S == 65 and not k.infinity)
    ins, go, gw, _, _ = P.case_reference(c)
    dev_in = [t.to(DEV).requires_grad_(i in GRAD_IN) for i, t in enumerate(ins)]
    out, w = render.composite_rays(*dev_in, c.infinity)
    ((out * go.to(DEV)).sum() + (w * gw.to(DEV)).sum()).backward()
    sg, z, dd, rd = dev_in[0].detach().reshape(-1), dev_in[4], dev_in[5], dev_in[6].detach()
    cd, cs, tn = (dev_in[i].detach().reshape(-1, 3) for i in (1, 2, 3))
    f32, ptr = torch.float32, render.dev_ptr
    g_sigma, g_cd, g_cs, g_tn = torch.empty_like(sg), torch.empty_like(cd), torch.empty_like(cs), torch.empty_like(tn)
    g_dn = torch.empty(c.B, device=DEV)
    gout, gwd = go.to(DEV).contiguous(), gw.to(DEV).contiguous()
    render.check(render.lib().scanerf_composite_backward(
        ptr(sg, f32, "sigma"), ptr(cd, f32, "diffuse"), ptr(cs, f32, "specular"), ptr(tn, f32, "tint"), ptr(z, f32, "z_vals"),
        ptr(dd, f32, "dists"), ptr(rd, f32, "rays_d"), ptr(out.detach(), f32, "out_ray"), ptr(gout, f32, "grad_out"),
        ptr(gwd, f32, "grad_weights"), ptr(g_sigma, f32, "g_sigma"), ptr(g_cd, f32, "g_diffuse"), ptr(g_cs, f32, "g_specular"),
        ptr(g_tn, f32, "g_tint"), ptr(g_dn, f32, "g_dnorm"), c.B, c.S, 0, render.stream()), "composite_backward")
    assert torch.equal(g_sigma, dev_in[0].grad.reshape(-1))
    unguarded = g_dn[:, None] * rd / rd.norm(dim=-1, keepdim=True)
    nz = rd.norm(dim=-1) > 0
    assert int((~nz).sum()) == 1 and torch.equal(dev_in[6].grad[nz], unguarded[nz])
    assert float(dev_in[6].grad[~nz].abs().max()) == 0.0


@pytest.mark.parametrize("c", P.CASES_REGIMES, ids=_ids(P.CASES_REGIMES))
def test_composite_regimes(c):
    """Opaque (a sample whose alpha is exactly 1.0f: u = 1e-6 and the backward divides by it), empty (T = (1 + 1e-6)^s) and thin
    (1 - exp(-x) at x ~ 1e-4) rays; the forward per ray as well, since a relative tolerance on an output means little on a thin
    ray.  The zero-direction ray: outputs as float64 gives them, finite gradients, a rays_d gradient of exactly 0."""
    _, _, _, r64, r32 = P.case_reference(c)
    out, w, grads = _op(c)
    tag = P.case_id(c)
    bad = _judge_forward(tag, out, w, r64, r32) + _judge_grads(tag, grads, r64, r32)
    z = c.B - 1   # (delta = 0: an all-empty ray whatever the family; it is one of the rays judged above, and once more by itself)
    bad += _judge_forward(tag + " zero-direction ray", out, w, r64, r32, rows=slice(z, z + 1), only=("max",), floor=FLOOR)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert float(grads["rays_d"][z].abs().max()) == 0.0
    assert not bad, bad


@pytest.mark.parametrize("c", P.CASES_TINY, ids=_ids(P.CASES_TINY))
def test_composite_tiny_batches(c):
    """B = 1, 3, 5: fewer rays than a block has waves.  Quantiles of five rays mean nothing: the whole batch's relative L2, on the
    maximum's margin (with so few rays the pooled figure IS the largest ray's) and never asked below one float32 rounding."""
    _, _, _, r64, r32 = P.case_reference(c)
    out, w, grads = _op(c)
    bad = _judge_grads(P.case_id(c), grads, r64, r32, only=("pooled",), k=(P.K_MAX, P.K_MAX), floor=FLOOR)
    _forward_close(out, w, r64)
    assert not bad, bad


def test_composite_past_the_grid_cap():
    """16 384 + 5 rays: the launch is capped at 4096 blocks of four waves, so the last five rays are the second trip of the
    grid-stride loop (forward and backward).  Judged over all rays and over the second trip alone; and a ray's result does not
    depend on the batch it is in: the first 16 384 rays bit-equal to a call on those rays only."""
    c = P.CASE_PAST_CAP
    cap = 16384
    _, _, _, r64, r32 = P.case_reference(c)
    out, w, grads = _op(c)
    tag = P.case_id(c)
    second = torch.arange(c.B) >= cap
    bad = _judge_forward(tag, out, w, r64, r32) + _judge_grads(tag, grads, r64, r32)
    bad += _judge_forward(tag + " rays>=16384", out, w, r64, r32, rows=slice(cap, None), only=("pooled",), k=(P.K_MAX, P.K_MAX), floor=FLOOR)
    bad += _judge_grads(tag + " rays>=16384", grads, r64, r32, rows=second, only=("pooled",), k=(P.K_MAX, P.K_MAX), floor=FLOOR)
    _forward_close(out, w, r64)
    out1, w1, grads1 = _op(c, rows=cap)
    assert torch.equal(out[:cap], out1) and torch.equal(w[:cap], w1)
    assert all(torch.equal(grads[n][:cap], grads1[n]) for n in P.GRAD_NAMES)
    assert not bad, bad


@pytest.mark.parametrize("c", P.CASES_S513, ids=_ids(P.CASES_S513))
def test_composite_beyond_the_backward_limit(c):
    """S = 513: the forward kernel has no limit (a ninth round of one lane) and is judged as any other; with a differentiable
    input the call is refused in the FORWARD, naming the limit -- not inside loss.backward()."""
    render = _render()
    ins, _, _, r64, r32 = P.case_reference(c)
    out, w, _ = _op(c, grad=False)
    bad = _judge_forward(P.case_id(c), out, w, r64, r32)
    assert not bad, bad
    for i in GRAD_IN:
        dev_in = [t.to(DEV).requires_grad_(j == i) for j, t in enumerate(ins)]
        with pytest.raises(RuntimeError, match="512"):
            render.composite_rays(*dev_in, c.infinity)
    with torch.no_grad():
        render.composite_rays(*[t.to(DEV).requires_grad_(j in GRAD_IN) for j, t in enumerate(ins)], c.infinity)


def test_render_fore_ops_trains_at_513_samples():
    """TileModel.render_fore_ops beyond the compositing op's limit: the HIP decoder with the torch compositing.  loss.backward()
    completes; loss, table gradient and decoder gradient agree with the same model's all-torch graph (hip_decoder = False) to what
    test_fused_and_ops_training_steps_agree allows between routes (2e-5 on the loss, 2e-3 of the largest entry)."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd.tile_model import TileModel
    torch.manual_seed(4)
    B, S = 256, 513
    o = torch.rand(B, 3, device=DEV) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1) * (0.5 + torch.rand(B, 1, device=DEV))
    tgt = torch.rand(B, 3, device=DEV)
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=12, seed=1)
    with torch.no_grad():
        m.features.mul_(30.0)
    res = []
    for hip in (True, False):
        m.hip_decoder = hip
        m.zero_grad(set_to_none=True)
        out = m.render_fore_ops(o, d, S, 2000, train=True)
        assert int(out["valid"].sum()) > B // 4 and out["weights"].shape[1] == S
        loss = torch.nn.functional.mse_loss(out["rgb"], tgt[out["valid"]]) + 0.01 * out["l2_reg_specular"]
        loss.backward()
        res.append((float(loss.detach()), m.features.grad.detach().clone(), torch.cat([p.grad.reshape(-1) for p in m.decoder.parameters()])))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=2e-5)
    for a, b, name in ((res[0][1], res[1][1], "table"), (res[0][2], res[1][2], "decoder")):
        assert float(b.abs().max()) > 0 and float((a - b).abs().max() / b.abs().max()) < 2e-3, name


# ------------------------------------------------------------------------------------------------------------ ray-gradient epilogue
def _epilogue_inputs(B, ntile, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * (0.5 + torch.rand(B, 1, generator=g))
    rows = torch.randn(16, 64, generator=g) * 0.2 if rows is None else rows
    return d, P.blob_with_harmonic_rows(rows), torch.randn(B, 6, generator=g), torch.randn(B, ntile, generator=g), torch.randn(B, 2, 64, generator=g)


def _epilogue_op(d, blob, rp, gdn, grs, valid):
    render = _render()
    to = lambda t: None if t is None else t.to(DEV).contiguous()
    g_o, g_d = render.ray_gradients_fused(torch.zeros_like(d).to(DEV), to(d), to(blob), to(rp), to(gdn), to(grs), ray_valid=to(valid))
    return g_o.cpu(), g_d.cpu()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ntile", [1, 2, 65])
@pytest.mark.parametrize("B", [1, 4099])
def test_epilogue_shapes(B, ntile, masked):
    """B = 4099: past the 1024-block cap (4096 rays a pass) with a partial last block; ntile = 65: the second trip of the lane-
    strided sum over g_dnorm's tiles.  g_o is a copy (or zero where masked); g_d per ray against float64, on the scale of its
    terms."""
    d, blob, rp, gdn, grs = _epilogue_inputs(B, ntile, 31 * B + ntile)
    if B > 1:
        d[B - 1] = 0.0
    valid = (torch.rand(B, generator=torch.Generator().manual_seed(B)) < 0.7) if masked else None
    if masked and B == 1:
        valid[0] = False
    g_o, g_d = _epilogue_op(d, blob, rp, gdn, grs, valid)
    o64, d64, scale = P.epilogue_grads(d, blob, rp, gdn, grs, valid, P.F64)
    _, d32, _ = P.epilogue_grads(d, blob, rp, gdn, grs, valid, P.F32)
    keep = torch.ones(B, dtype=torch.bool) if valid is None else valid
    assert torch.equal(g_o, torch.where(keep[:, None], rp[:, 0:3], torch.zeros(B, 3)))
    assert float(g_d[~keep].abs().max() if int((~keep).sum()) else 0.0) == 0.0 and bool(torch.isfinite(g_d).all())
    tag = f"epilogue B{B} ntile{ntile} masked{int(masked)}"
    kw = dict(only=("pooled",), k=(P.K_MAX, P.K_MAX), floor=FLOOR) if B == 1 else {}
    bad = P.judge(tag, g_d, d64, d32, scale=scale, **kw)
    if B > 4096:
        bad += P.judge(tag + " rays>=4096", g_d[4096:], d64[4096:], d32[4096:], scale=scale[4096:], only=("pooled",), k=(P.K_MAX, P.K_MAX), floor=FLOOR)
    assert not bad, bad


def _directions():
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    diag = [[a, b, c] for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    g = torch.Generator().manual_seed(9)
    rest = torch.nn.functional.normalize(torch.randn(50, 3, generator=g), dim=-1)
    d = torch.cat([torch.tensor(axes + diag, dtype=torch.float32), rest], 0)
    return d * (0.5 + torch.rand(64, 1, generator=g))


@pytest.mark.parametrize("i", range(1, 16))
def test_epilogue_one_harmonic_at_a_time(i):
    """A directional layer whose only non-zero harmonic weight is row i, lane 0: g_sh is non-zero in harmonic i alone, so each
    coefficient of the hand-written Jacobian stands by itself -- on 64 directions that include the axes and the diagonals, where
    most of the other harmonics' derivatives vanish."""
    rows = torch.zeros(16, 64)
    rows[i, 0] = 1.0
    d = _directions()
    _, blob, _, _, grs = _epilogue_inputs(64, 1, 70 + i, rows=rows)
    rp, gdn = torch.zeros(64, 6), torch.zeros(64, 1)
    _, g_d = _epilogue_op(d, blob, rp, gdn, grs, None)
    _, d64, scale = P.epilogue_grads(d, blob, rp, gdn, grs, None, P.F64)
    _, d32, _ = P.epilogue_grads(d, blob, rp, gdn, grs, None, P.F32)
    assert float(d64.abs().max()) > 0
    bad = P.judge(f"epilogue harmonic {i}", g_d, d64, d32, scale=scale)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ losses
def _branches(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 16, generator=g), torch.rand(B, 16, generator=g), torch.rand(B, 3, generator=g),
            torch.rand(B, generator=g) < 0.6)


@pytest.mark.parametrize("B", [5, 65536, 65537])
@pytest.mark.parametrize("case", ["fg_none", "bg_none", "none"])
def test_photometric_loss_fgbg_with_a_branch_without_valid_rays(case, B):
    """A branch no ray is valid in (l2f / l2b = 0) and a batch no ray is valid in at all (in3 = 0), at the pass boundary of the
    partial sums (256 blocks x 256 threads = 65 536 rays) and one past it; tolerances of
    test_photometric_loss_grad_fgbg_masks_rays_invalid_in_both_branches, reference in float64."""
    render = _render()
    fg, bg, tgt, mixed = _branches(B, B + len(case))
    mixed[0], mixed[1] = True, False
    none = torch.zeros(B, dtype=torch.bool)
    vf, vb = {"fg_none": (none, mixed), "bg_none": (mixed, none), "none": (none, none)}[case]
    fg[~vf], bg[~vb] = 0.0, 0.0          # what the forward writes for rays a branch does not render: zeros, T_left = 1
    fg[~vf, 4], bg[~vb, 4] = 1.0, 1.0
    loss, gfg, gbg = render.photometric_loss_grad_fgbg(*(t.to(DEV) for t in (fg, bg, tgt, vf, vb)), 0.01)
    if case == "none":
        assert float(loss) == 0.0 and float(gfg.abs().max()) == 0.0 and float(gbg.abs().max()) == 0.0
        return
    ref, rf, rb = P.loss_fgbg64(fg, bg, tgt, vf, vb, 0.01)
    np.testing.assert_allclose(loss.item(), ref, rtol=3e-6)
    atol = 2.0 * 2.0 ** -23 / (3.0 * float((vf | vb).sum()))
    np.testing.assert_allclose(gfg.cpu().numpy(), rf.numpy(), rtol=2e-6, atol=atol)
    np.testing.assert_allclose(gbg.cpu().numpy(), rb.numpy(), rtol=2e-6, atol=atol)
    both = ~(vf | vb)
    assert int(both.sum()) > 0 and float(gfg.cpu()[both].abs().max()) == 0.0 and float(gbg.cpu()[both].abs().max()) == 0.0
    empty = gfg if case == "fg_none" else gbg
    assert float(empty[:, 14].abs().max()) == 0.0


@pytest.mark.parametrize("B", [5, 65536, 65537])
def test_photometric_loss_at_the_pass_boundary_and_without_valid_rays(B):
    """tolerances of test_photometric_loss_grad_vs_autograd, reference in float64."""
    render = _render()
    out, _, tgt, _ = _branches(B, 3 * B)
    valid = torch.rand(B, generator=torch.Generator().manual_seed(B)) < 0.8
    valid[0] = True
    loss, g = render.photometric_loss_grad(out.to(DEV), tgt.to(DEV), valid.to(DEV), 0.01)
    ref, rg = P.loss64(out, tgt, valid, 0.01)
    np.testing.assert_allclose(loss.item(), ref, rtol=2e-6)
    np.testing.assert_allclose(g.cpu().numpy(), rg.numpy(), rtol=1e-6, atol=1e-12)
    loss, g = render.photometric_loss_grad(out.to(DEV), tgt.to(DEV), torch.zeros(B, dtype=torch.bool, device=DEV), 0.01)
    assert float(loss) == 0.0 and float(g.abs().max()) == 0.0
