"""GPU checks of the monocular prior losses (csrc/mono.hip, scanerf_amd.mono) against the float64 restatement of
tests/mono_reference.py (pinned to the reference by tests/test_mono_cpu.py): loss and dL/d(depth) on golden G22's inputs and on
a 64-view batch, bit-reproducibility, the edge cases, the fg+bg chain rule, the whole fg+bg gradient against the autograd route,
the no-op of mono=None / zero weights on both training steps, and a short training run on a procedural scene."""
import numpy as np
import pytest
import torch

import mono_reference as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _mono_from(md, mn, kinv, **kw):
    """MonoLoss over maps given in float64 (cast to float32; K from K^-1)."""
    from scanerf_amd.mono import MonoLoss
    ks = torch.linalg.inv(kinv.to(F64).cpu())
    return MonoLoss(ks, None if md is None else md.float().to(DEV), None if mn is None else mn.float().to(DEV), **kw)


def _check_against_reference(depth, locs, valid, md, mn, kinv, wd=0.7, ws=0.3, tol=1e-5):
    mono = _mono_from(md, mn, kinv)
    loss, grad = mono.loss_grad(locs.to(DEV), depth.float().to(DEV), None if valid is None else valid.to(DEV), wd, ws)
    kinv32 = mono.kinv.reshape(-1, 3, 3).double().cpu()    # the kernel's K^-1 (float32)
    ld, ls, gd, gs = MR.losses_and_grads(depth.float().double(), locs, valid, None if md is None else md.float().double(),
                                         None if mn is None else mn.float().double(), kinv32)
    want = torch.stack([wd * ld + ws * ls, ld, ls])
    got = loss.double().cpu()
    for i in range(3):
        assert abs(float(got[i] - want[i])) <= tol * max(abs(float(want[i])), 1e-30), (i, got, want)
    g_want = wd * gd + ws * gs
    if float(g_want.norm()) > 0:
        assert _rel_l2(grad, g_want) <= tol, _rel_l2(grad, g_want)
    else:
        assert bool((grad == 0).all())
    return loss, grad, (ld, ls)


@pytest.mark.parametrize("kind", ["main", "nopatch", "empty"])
def test_kernel_matches_reference_on_golden_inputs(golden, kind):
    g = {k: torch.from_numpy(v) if v.ndim else v for k, v in golden("g22_mono").items()}
    depth, locs, valid, md, mn, kinv = MR.golden_case(g, kind)
    loss, grad, (ld, ls) = _check_against_reference(depth, locs, valid, md, mn, kinv)
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    if kind == "main":   # and the reference's own numbers (float64, G22)
        np.testing.assert_allclose(float(loss[1]), float(g["main_loss_depth"]), rtol=1e-5)
        np.testing.assert_allclose(float(loss[2]), float(g["main_loss_smooth"]), rtol=1e-5)
    if kind == "nopatch":
        assert float(loss[2]) == 0.0                      # the reference: NaN
    if kind == "empty":
        assert float(loss[0]) == 0.0 and bool((grad == 0).all())


def random_batch(N=64, Bc=256, H=120, W=160, seed=0, shuffle=True):
    """N views x Bc rays (2x2 patches, the same pixel set in every view as tile.py draws it), a third of the views at 50 +- 1
    (2 % variation), some masked rays, normals that agree on most patches; patches shuffled across views when shuffle."""
    from scanerf_amd import cameras as CM
    from scanerf_amd.trainer import sample_patch_ray_idx
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    idx = sample_patch_ray_idx(N * Bc, N, H, W, "cpu")
    locs = CM.pixel_locs(N, idx, W, "cpu")
    B = locs.shape[0]
    depth = 2.0 + 3.0 * torch.rand(B, generator=gen, dtype=F64)
    far = locs[:, 0] % 3 == 0
    depth[far] = 50.0 + 2.0 * torch.rand(int(far.sum()), generator=gen, dtype=F64) - 1.0
    a = 0.5 + torch.rand(N, generator=gen, dtype=F64)
    b = torch.rand(N, generator=gen, dtype=F64) - 0.5
    md = (a[:, None, None] * (2.0 + 3.0 * torch.rand(N, H, W, generator=gen, dtype=F64)) + b[:, None, None])
    v, x, y = locs[:, 0].long(), locs[:, 1].long(), locs[:, 2].long()
    md[v, y, x] = a[v] * depth + b[v] + 0.05 * torch.randn(B, generator=gen, dtype=F64)
    base = torch.nn.functional.normalize(torch.randn(N, 1, 1, 3, generator=gen, dtype=F64) + torch.tensor([0, 0, -2.0], dtype=F64), dim=-1)
    mn = torch.nn.functional.normalize(base + 0.1 * torch.randn(N, H, W, 3, generator=gen, dtype=F64), dim=-1)
    valid = torch.rand(B, generator=gen) > 0.05
    kinv = torch.linalg.inv(torch.tensor([[150.0, 0, W / 2], [0, 150.0, H / 2], [0, 0, 1]], dtype=F64))[None].repeat(N, 1, 1)
    kinv[:, 0, 0] *= 1 + 0.01 * torch.arange(N, dtype=F64)
    if shuffle:
        perm = torch.randperm(B // 4, generator=gen)
        sel = (perm[:, None] * 4 + torch.arange(4)[None]).reshape(-1)
        depth, locs, valid = depth[sel], locs[sel], valid[sel]
    return depth.float().double(), locs, valid, md, mn, kinv


@pytest.mark.parametrize("shuffle", [False, True])
def test_kernel_matches_reference_on_64_views(shuffle):
    depth, locs, valid, md, mn, kinv = random_batch(shuffle=shuffle)
    _check_against_reference(depth, locs, valid, md, mn, kinv)


def test_repeated_launches_are_bit_identical():
    depth, locs, valid, md, mn, kinv = random_batch(seed=3)
    mono = _mono_from(md, mn, kinv)
    args = (locs.to(DEV), depth.float().to(DEV), valid.to(DEV), 0.01, 0.001)
    l0, g0 = mono.loss_grad(*args)
    for _ in range(5):
        l1, g1 = mono.loss_grad(*args)
        assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_edge_cases():
    depth, locs, valid, md, mn, kinv = random_batch(N=4, Bc=64, seed=5, shuffle=False)
    mono = _mono_from(md, mn, kinv)
    L, D = locs.to(DEV), depth.float().to(DEV)
    # no valid ray: 0 and a zero gradient
    loss, grad = mono.loss_grad(L, D, torch.zeros_like(valid).to(DEV), 1.0, 1.0)
    assert bool((loss == 0).all()) and bool((grad == 0).all())
    # rays outside the maps count as invalid
    bad = L.clone()
    bad[:, 1] += 10 ** 6
    loss, grad = mono.loss_grad(bad, D, None, 1.0, 1.0)
    assert bool((loss == 0).all()) and bool((grad == 0).all())
    # no valid patch (the normals disagree everywhere): 0, not NaN, and no gradient from the term
    mn_bad = mn.clone()
    mn_bad[..., 0] = torch.where(torch.arange(mn.shape[2])[None, None, :] % 2 == 0, 1.0, -1.0).to(F64)
    mn_bad[..., 1:] = 0
    mono2 = _mono_from(md, mn_bad, kinv)
    loss, grad = mono2.loss_grad(L, D, valid.to(DEV), 0.0, 1.0)
    assert float(loss[2]) == 0.0 and bool(torch.isfinite(loss).all()) and bool((grad == 0).all())
    # one valid ray per view: each contributes t^2, no gradient
    one = torch.zeros_like(valid)
    Bv = depth.numel() // 4
    one[::Bv] = True
    loss, grad = mono.loss_grad(L, D, one.to(DEV), 1.0, 0.0)
    t = md[locs[one, 0].long(), locs[one, 2].long(), locs[one, 1].long()]
    np.testing.assert_allclose(float(loss[1]), float((t.float().double() ** 2).mean()), rtol=1e-6)
    assert bool((grad == 0).all())


def test_fgbg_chain_rule():
    """pred_depth = d_fg + T_left d_bg (tile.py:675-677): the foreground depth column gets g, its T_left column g d_bg, the background
    depth column T_left g -- against autograd of the composition."""
    from scanerf_amd import render
    depth, locs, valid, md, mn, kinv = random_batch(N=8, Bc=128, seed=7)
    mono = _mono_from(md, mn, kinv, weight_depth=1.0, weight_smooth=1.0)
    B = depth.numel()
    g = torch.Generator(device=DEV).manual_seed(0)
    out_fg = torch.rand(B, 16, device=DEV, generator=g)
    out_bg = torch.rand(B, 16, device=DEV, generator=g)
    out_fg[:, render.DEPTH] = depth.float().to(DEV) * 0.6
    out_bg[:, render.DEPTH] = depth.float().to(DEV) * 0.8
    vf = torch.rand(B, device=DEV, generator=g) > 0.3
    vb = torch.rand(B, device=DEV, generator=g) > 0.3
    out_fg[~vf] = 0.0
    out_fg[~vf, render.T_LEFT] = 1.0
    out_bg[~vb] = 0.0
    gfg, gbg = torch.zeros(B, 16, device=DEV), torch.zeros(B, 16, device=DEV)
    L = locs.to(DEV)
    r = mono.fgbg_term(5, L, out_fg, out_bg, vf, vb, gfg, gbg)
    assert r is not None and mono.last_depth_loss is not None and mono.last_smooth_loss is not None
    fg = out_fg.clone().requires_grad_(True)
    bg = out_bg.clone().requires_grad_(True)
    dm = fg[:, render.DEPTH] + fg[:, render.T_LEFT] * bg[:, render.DEPTH]
    gd = mono(5, L, dm.detach().contiguous(), vf | vb)[1]
    (dm * gd).sum().backward()
    assert float(gd.abs().sum()) > 0
    torch.testing.assert_close(gfg, fg.grad, rtol=1e-6, atol=1e-9)
    torch.testing.assert_close(gbg, bg.grad, rtol=1e-6, atol=1e-9)
    assert bool((gfg[~(vf | vb)] == 0).all()) and bool((gbg[~(vf | vb)] == 0).all())


def _tile(seed=4, log2_T=14):
    from scanerf_amd.tile_model import TileModel
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=log2_T, seed=seed)
    with torch.no_grad():
        m.features.mul_(200.0)
    return m


def _batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(B, 3, generator=g) * 7.8 - 3.9).to(DEV)
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1).to(DEV)
    tgt = torch.rand(B, 3, generator=g).to(DEV)
    return o.contiguous(), d.contiguous(), tgt


def test_fgbg_gradients_match_the_autograd_route():
    """fgbg_gradients(mono=...) against two render.FusedRenderRays calls (foreground; background with infinity) merged in torch,
    with the loss = the photometric term + w * mono_reference(pred_depth): loss, table and decoder gradients."""
    from scanerf_amd import network, render
    from scanerf_amd import tile_model as TM
    N, Bc, Sf, Sb, step = 8, 128, 64, 40, 6000
    depth, locs, valid, md, mn, kinv = random_batch(N=N, Bc=Bc, H=40, W=48, seed=9, shuffle=False)
    B = depth.numel()
    md = md * 0.5   # depths near those the tile renders
    m = _tile()
    o, d, tgt = _batch(B, 1)
    mono = _mono_from(md, mn, kinv, weight_depth=1.0, weight_smooth=1.0, depth_start=-1, smooth_start=-1)
    L = locs.to(DEV)
    loss0, gtab0, gblob0 = TM.fgbg_gradients(m, o, d, tgt, Sf, Sb, step, invalid_underground=True)
    loss, gtab, gblob = TM.fgbg_gradients(m, o, d, tgt, Sf, Sb, step, invalid_underground=True, mono=mono, locs=L)
    # the autograd route
    with torch.no_grad():
        z, dist = m.sample(o, d, Sf)
        vf = torch.all(z != -1, dim=-1)
        zb, db, vb = m.inverse_z_sampling(o, d, Sb, True)
    F = m.features.detach().clone().requires_grad_(True)
    blob = m.decoder.blob().detach().clone().requires_grad_(True)
    wf = network.weight_feature(step, DEV)
    skip = network.skip_levels(step) if TM.LEVEL_SKIP else 0
    box = (m.min_bbox.tolist(), m.bbox_size.tolist())
    out_fg, _ = render.fused_render_rays(o, d, z, dist, F, blob, m.resolution, wf, *box, render.FORE, False, vf, skip, False)
    out_bg, _ = render.fused_render_rays(o, d, zb, db, F, blob, m.resolution, wf, *box, render.BG, True, vb, skip, False)
    lp, gfg, gbg = render.photometric_loss_grad_fgbg(out_fg.detach(), out_bg.detach(), tgt, vf, vb, 0.01)
    fg = out_fg.detach().double().requires_grad_(True)
    bg = out_bg.detach().double().requires_grad_(True)
    pd = fg[:, render.DEPTH] + fg[:, render.T_LEFT] * bg[:, render.DEPTH]
    lv = (vf | vb).cpu()
    kinv32 = mono.kinv.reshape(-1, 3, 3).double().to(DEV)
    wd, ws = MR.weight(1.0, -1, step), MR.weight(1.0, -1, step)
    lm = (wd * MR.depth_loss(pd, L, lv.to(DEV), mono.mono_depths.double())
          + ws * MR.smooth_loss(pd, L, lv.to(DEV), mono.mono_normals.double(), kinv32))
    lm.backward()
    torch.autograd.backward([out_fg, out_bg], [gfg + fg.grad.float(), gbg + bg.grad.float()])
    np.testing.assert_allclose(float(loss), float(lp) + float(lm.detach()), rtol=1e-5)
    assert _rel_l2(gtab0, gtab) > 1e-4            # the term moved the gradients
    assert _rel_l2(gtab, F.grad) < 1e-5, _rel_l2(gtab, F.grad)
    assert _rel_l2(gblob, blob.grad) < 1e-5, _rel_l2(gblob, blob.grad)


def _state(m):
    return [t.detach().clone() for t in (m.features, m.exp_avg, m.exp_avg_sq, m.decoder.params)]


@pytest.mark.parametrize("fgbg", [False, True])
def test_mono_none_and_zero_weights_are_bit_identical(fgbg):
    """mono=None and a MonoLoss with both weights 0 leave train_step_fused / train_step_fgbg exactly as they are: parameters and
    Adam moments after 3 steps."""
    from scanerf_amd import tile_model as TM
    depth, locs, valid, md, mn, kinv = random_batch(N=4, Bc=256, H=80, W=96, seed=2, shuffle=False)
    B = depth.numel()
    o, d, tgt = _batch(B, 3)
    L = locs.to(DEV)
    states, losses = [], []
    for mono in (None, _mono_from(md, mn, kinv, weight_depth=0.0, weight_smooth=0.0)):
        m = _tile(seed=6)
        opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3)
        kw = {} if mono is None else dict(mono=mono, locs=L)
        ls = []
        for s in range(3):
            if fgbg:
                ls.append(TM.train_step_fgbg(m, opt, o, d, tgt, 64, 32, 100 + s, **kw))
            else:
                ls.append(TM.train_step_fused(m, opt, o, d, tgt, 64, 100 + s, **kw))
        states.append(_state(m) + [opt.state_dict()["state"][0]["exp_avg"].clone()])
        losses.append(torch.stack(ls))
    assert torch.equal(losses[0], losses[1])
    for a, b in zip(*states):
        assert torch.equal(a, b)


def _plane_scene(C=4, H=72, W=96):
    """C cameras at z = -3 looking along +z at the plane z = 1 + 0.3 x; true depth along each pixel's ray."""
    from scanerf_amd import cameras as CM
    eye = torch.eye(3)
    c2w = torch.stack([torch.cat([eye, torch.tensor([[x0], [0.1 * x0], [-3.0]])], -1) for x0 in (-0.6, -0.2, 0.2, 0.6)][:C])
    ks = torch.tensor([[90.0, 0, W / 2, 0, 90.0, H / 2, 0, 0, 1]]).repeat(C, 1).reshape(C, 3, 3)
    cams = CM.CameraSet(ks, c2w, DEV)
    all_locs = CM.pixel_locs(C, torch.arange(H * W), W, DEV)
    with torch.no_grad():
        o, d = cams.get_rays(all_locs)
    t = (1.0 - o[:, 2] + 0.3 * o[:, 0]) / (d[:, 2] - 0.3 * d[:, 0])
    return cams, ks, t.reshape(C, H, W), H, W


def _affine_rmse(p, t, v):
    """Per-view least-squares affine fit of p to t, then the RMSE over all rays (the error the term is invariant to removed)."""
    err = []
    for i in range(int(v.max()) + 1):
        s = v == i
        A = torch.stack([p[s], torch.ones_like(p[s])], -1).double()
        h = torch.linalg.lstsq(A, t[s].double()[:, None]).solution
        err.append(((A @ h)[:, 0] - t[s].double()) ** 2)
    return float(torch.cat(err).mean().sqrt())


def test_mono_term_pulls_depth_towards_the_truth():
    """A textureless plane (the photometric term says nothing about depth) seen by 4 views; monocular depth = a_v true + b_v.
    After the same 60 steps of train_step_fused, the rendered depth's error against the truth is lower with the term on
    (measured: DESIGN.md 4.9)."""
    from scanerf_amd import cameras as CM
    from scanerf_amd import tile_model as TM
    from scanerf_amd.mono import MonoLoss
    from scanerf_amd.trainer import sample_patch_ray_idx
    cams, ks, t_true, H, W = _plane_scene()
    C = ks.shape[0]
    a = torch.tensor([0.8, 1.1, 0.9, 1.3], device=DEV)[:C]
    b = torch.tensor([0.2, -0.1, 0.4, 0.0], device=DEV)[:C]
    md = a[:, None, None] * t_true + b[:, None, None]
    res = {}
    for on in (False, True):
        m = _tile(seed=8)
        opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3)
        mono = MonoLoss(ks, mono_depths=md, weight_depth=1.0, weight_smooth=0.0, depth_start=-1) if on else None
        gen = torch.Generator(device=DEV).manual_seed(0)
        for s in range(60):
            idx = sample_patch_ray_idx(C * 256, C, H, W, DEV, generator=gen)
            locs = CM.pixel_locs(C, idx, W, DEV)
            with torch.no_grad():
                o, d = cams.get_rays(locs)
            tgt = torch.full((locs.shape[0], 3), 0.5, device=DEV)
            kw = dict(mono=mono, locs=locs) if on else {}
            TM.train_step_fused(m, opt, o.contiguous(), d.contiguous(), tgt, 64, 1000 + s, table_lr=1e-2, **kw)
        locs = CM.pixel_locs(C, torch.arange(0, H * W, 5), W, DEV)
        with torch.no_grad():
            o, d = cams.get_rays(locs)
            out, _, _ = m.render_fore_fused(o.contiguous(), d.contiguous(), 64, 1059)
        p = out[:, 3]
        t = t_true[locs[:, 0].long(), locs[:, 2].long(), locs[:, 1].long()]
        res[on] = (_affine_rmse(p, t, locs[:, 0].long()), float((p - t).abs().mean()))
    print("mono behaviour: affine-aligned depth RMSE off %.4f on %.4f; mean |depth - truth| off %.4f on %.4f"
          % (res[False][0], res[True][0], res[False][1], res[True][1]))
    assert res[True][0] < 0.5 * res[False][0], res
