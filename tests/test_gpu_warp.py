"""GPU checks of the multi-view warp loss (csrc/warp.hip, scanerf_amd.warp) against the float64 restatement of
tests/warp_reference.py (pinned to the reference by tests/test_warp_cpu.py): view selection, projection and colour fetch, loss
and gradients (rays, prediction, cameras' rts), determinism, the fg+bg chain rule, a finite-difference check of the pose
gradient on se3_refine, the training hook's no-op at weight 0, and a small bundle-adjustment run driven by the warp term."""
import numpy as np
import pytest
import torch

import warp_reference as WR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def ring(n, radius=3.0, f=40.0, H=48, W=64, seed=0):
    """n cameras on a ring around the origin (jittered heights and radii), looking at the origin: ks [n,3,3], c2w [n,3,4]."""
    g = torch.Generator().manual_seed(seed)
    c2w, ks = [], []
    for i in range(n):
        a = 2 * np.pi * i / n
        r = radius * (1 + 0.1 * float(torch.rand(1, generator=g)))
        c = torch.tensor([float(r * np.cos(a)), 0.4 * float(torch.rand(1, generator=g)) - 0.2, float(r * np.sin(a))])
        z = -c / c.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), z)
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        c2w.append(torch.cat([torch.stack([x, y, z], 1), c[:, None]], 1))
        ks.append(torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]))
    return torch.stack(ks), torch.stack(c2w)


def scene(N, B, H=48, W=64, seed=0, occl=True):
    """Cameras, images, occlusions, and rays that start near a camera centre and hit points near the origin."""
    import scanerf_amd  # noqa
    from scanerf_amd import cameras as CM
    ks, c2w = ring(N, H=H, W=W, seed=seed)
    cams = CM.CameraSet(ks, c2w, DEV)
    g = torch.Generator().manual_seed(seed + 1)
    images = torch.rand(N, H, W, 3, generator=g).to(DEV)
    occ = (torch.rand(N, H, W, generator=g) > 0.2).to(DEV) if occl else None
    owner = torch.randint(0, N, (B,), generator=g)
    o = c2w[owner, :, 3] + 0.05 * torch.randn(B, 3, generator=g)
    p = (torch.rand(B, 3, generator=g) - 0.5) * 1.0
    depth = 0.5 + torch.rand(B, generator=g)
    d = (p - o) / depth[:, None]
    q = torch.cat([depth[:, None], 0.6 * torch.rand(B, 6, generator=g)], 1)
    return cams, images, occ, o.to(DEV).contiguous(), d.to(DEV).contiguous(), q.to(DEV).contiguous()


def _f64(*t):
    return [x.detach().to(DEV, F64) for x in t]


@pytest.mark.parametrize("N", [1, 7, 300])
@pytest.mark.parametrize("B", [1, 1000, 16384])
def test_selection_matches_restatement(N, B):
    """The valid slots per ray equal the restatement's as sets of (view, cost), costs within 1e-6; rays whose answer float32
    cannot decide (a cost within 1e-5 of the 0.176 threshold or of the K-th / (K+1)-th boundary, a neighbour on the image border)
    are excluded, and rare."""
    from scanerf_amd.warp import WarpLoss
    cams, images, occ, o, d, q = scene(N, B, seed=N + B)
    w = WarpLoss(cams, images, occ, voxel_size=0.05)
    assert w.K == min(10, N)
    ray_valid = torch.ones(B, dtype=torch.bool, device=DEV)
    ray_valid[::7] = False
    views, cost, valid = w.select(o, d, q, ray_valid)
    torch.cuda.synchronize()
    o64, d64, q64, ks64, rts64 = _f64(o, d, q, cams.ks, cams.get_rts())
    pts = o64 + q64[:, :1] * d64
    full = WR.view_costs(o64, d64, pts, ks64, rts64, w.H, w.W)
    rv, rc, rvalid = WR.select(full, w.K, ray_valid)
    srt = torch.sort(full, dim=1, stable=True)[0]
    amb = ((full - WR.VALID_COST).abs() < 1e-5).any(1)
    if N > w.K:
        amb |= ((srt[:, w.K] - srt[:, w.K - 1]).abs() < 1e-5) & (srt[:, w.K - 1] <= WR.VALID_COST + 1e-5)
    # projections within 1e-3 px of the image border (the open interval of view_selection_kernel.cu:50) of a camera that would
    # otherwise be a neighbour
    R, t = rts64[:, :, :3], rts64[:, :, 3]
    uv = torch.einsum("nij,bnj->bni", ks64, torch.einsum("nij,bj->bni", R, pts) + t[None])
    x, y = uv[..., 0] / uv[..., 2], uv[..., 1] / uv[..., 2]
    edge = torch.minimum(torch.minimum(x.abs(), (x - (w.W - 1)).abs()), torch.minimum(y.abs(), (y - (w.H - 1)).abs())) < 1e-3
    free = WR.view_costs(o64, d64, pts, ks64, rts64, 1e9, 1e9)   # the cost without the image bounds
    amb |= (edge & (free <= WR.VALID_COST + 1e-5)).any(1)
    amb = amb.cpu().tolist()
    assert sum(amb) <= 0.03 * B   # (300 cameras on one ring: near-ties at the K-th slot are common)
    views, cost, valid = views.tolist(), cost.double().tolist(), valid.tolist()
    rv, rc, rvalid = rv.tolist(), rc.tolist(), rvalid.tolist()
    n_valid = 0
    for b in range(B):
        if amb[b]:
            continue
        got = {int(v): float(c) for v, c, ok in zip(views[b], cost[b], valid[b]) if ok}
        want = {int(v): float(c) for v, c, ok in zip(rv[b], rc[b], rvalid[b]) if ok}
        assert set(got) == set(want), (b, got, want)
        for v, c in got.items():
            assert abs(c - want[v]) <= 1e-6, (b, v, c, want[v])
        n_valid += len(got)
    if B > 1:
        assert n_valid > B // 2   # the fixture does produce neighbours


def test_projection_and_fetch_match_restatement():
    from scanerf_amd.warp import WarpLoss
    cams, images, occ, o, d, q = scene(12, 4000, seed=3)
    w = WarpLoss(cams, images, occ, voxel_size=0.05)
    views, _, valid = w.select(o, d, q)
    pr = w.project(o, d, q, views, valid)
    torch.cuda.synchronize()
    o64, d64, q64, ks64, rts64, img64 = _f64(o, d, q, cams.ks, cams.get_rts(), images)
    pts = o64 + q64[:, :1] * d64
    grid, depth, org, dirn = WR.project(pts, ks64, rts64, views.long())
    m = valid
    assert int(m.sum()) > 4000
    np.testing.assert_allclose(pr["grid"][m].cpu().double().numpy(), grid[m].cpu().numpy(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(pr["proj_depth"][m].cpu().double().numpy(), depth[m].cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(pr["nei_origin"][m].cpu().double().numpy(), org[m].cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(pr["nei_direction"][m].cpu().double().numpy(), dirn[m].cpu().numpy(), rtol=1e-5, atol=1e-5)
    # the fetch on the kernel's own grid: colours within 1e-6, the occlusion-masked flags exact
    col, vflag = WR.sample_color(img64, occ, pr["grid"].double(), views, valid)
    assert torch.equal(pr["valid"], vflag)
    assert bool((valid & ~vflag).any())
    np.testing.assert_allclose(pr["color"][vflag].cpu().double().numpy(), col[vflag].cpu().numpy(), rtol=0, atol=1e-6)
    assert bool((pr["color"][~pr["valid"] & ~valid] == 0).all())


def _rel_l2(a, b):
    a, b = a.detach().double().reshape(-1).cpu(), b.detach().double().reshape(-1).cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _loss_case(seed=5, N=12, B=3000):
    from scanerf_amd.warp import WarpLoss
    cams, images, occ, o, d, q = scene(N, B, seed=seed)
    w = WarpLoss(cams, images, occ, voxel_size=0.05)
    rv = torch.rand(B, device=DEV) > 0.1
    views, _, valid = w.select(o, d, q, rv)
    pr = w.project(o, d, q, views, valid)
    score = torch.rand(B, w.K, device=DEV) * pr["valid"]
    return w, cams, images, occ, o, d, q, rv, pr, score


def test_loss_and_gradients_match_float64_autograd():
    w, cams, images, occ, o, d, q, rv, pr, score = _loss_case()
    loss, gq, g_o, g_d, g_rts = w.loss_grad(o, d, q, rv, pr, score, 0.7)
    torch.cuda.synchronize()
    o64, d64, q64, ks64, rts64, img64, s64 = _f64(o, d, q, cams.ks, cams.get_rts(), images, score)
    for t in (o64, d64, q64, rts64):
        t.requires_grad_(True)
    ref = WR.warp_loss(o64, d64, q64[:, 0], q64[:, 1:4], q64[:, 4:7], rts64, ks64, img64, None, pr["views"], pr["valid"], s64,
                       scale=0.7, ray_valid=rv, corner_grid=pr["grid"].double())
    ref.backward()
    assert float(ref.detach()) > 0
    np.testing.assert_allclose(float(loss), float(ref), rtol=1e-5)
    assert _rel_l2(gq[:, 0], q64.grad[:, 0]) <= 1e-5
    assert _rel_l2(gq[:, 1:4], q64.grad[:, 1:4]) <= 1e-5
    assert _rel_l2(gq[:, 4:7], q64.grad[:, 4:7]) <= 1e-5
    assert _rel_l2(g_o, o64.grad) <= 1e-5
    assert _rel_l2(g_d, d64.grad) <= 1e-5
    assert _rel_l2(g_rts, rts64.grad) <= 1e-5
    assert bool((gq[~rv] == 0).all()) and bool((g_o[~rv] == 0).all())


def test_gradients_are_bit_reproducible():
    """Two launches give bit-identical grad_rts and grad_out (fixed-order reduction, no float atomics)."""
    w, cams, images, occ, o, d, q, rv, pr, score = _loss_case(seed=8, N=40, B=16384)
    r1 = w.loss_grad(o, d, q, rv, pr, score, 1.0)
    r2 = w.loss_grad(o, d, q, rv, pr, score, 1.0)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    # through the training hook: the photometric grad_out plus the warp columns, twice (a voxel size that leaves the constant
    # render's visibility scores well above zero)
    w.voxel_size = 50.0
    out = torch.zeros(o.shape[0], 16, device=DEV)
    out[:, [3, 5, 6, 7, 8, 9, 10]] = q
    render_fn = lambda ro, rd: (torch.full((ro.shape[0],), 1.0, device=DEV), torch.full((ro.shape[0], 3), 0.01, device=DEV))
    gs = []
    for _ in range(2):
        g = torch.full((o.shape[0], 16), 0.25, device=DEV)
        w.fused_term(10000, o, d, out, rv, g, render_fn)
        gs.append((g, w.last_grad_rts))
    assert torch.equal(gs[0][0], gs[1][0]) and torch.equal(gs[0][1], gs[1][1])
    assert not torch.equal(gs[0][0], torch.full_like(gs[0][0], 0.25))


def test_fgbg_chain_rule():
    """tile.py:675-677: q = q_fg + T_left q_bg -> the foreground columns, its T_left column and the background columns, against
    autograd of the composition."""
    from scanerf_amd.warp import WarpLoss, Q_COLS
    cams, images, occ, o, d, q, = scene(12, 3000, seed=11)
    w = WarpLoss(cams, images, occ, voxel_size=0.3, gamma=2.0, warming=False)
    B = o.shape[0]
    g = torch.Generator(device=DEV).manual_seed(0)
    out_fg = torch.rand(B, 16, device=DEV, generator=g) * 0.4
    out_bg = torch.rand(B, 16, device=DEV, generator=g) * 0.4
    out_fg[:, 3] = q[:, 0] * 0.8
    out_bg[:, 3] = q[:, 0] * 0.8
    vf = torch.rand(B, device=DEV, generator=g) > 0.3
    vb = torch.rand(B, device=DEV, generator=g) > 0.3
    out_fg[~vf] = 0.0
    out_fg[~vf, 4] = 1.0
    out_bg[~vb] = 0.0
    render_fn = lambda ro, rd: (rd.norm(dim=-1) * 0.9 + ro[:, 0] * 0.01, 0.05 * rd.abs())
    gfg, gbg = torch.zeros(B, 16, device=DEV), torch.zeros(B, 16, device=DEV)
    r = w.fgbg_term(1, o, d, out_fg, out_bg, vf, vb, gfg, gbg, render_fn)
    assert r is not None
    # the same term on the merged q directly (same kernels) gives dL/dq; autograd of the composition gives the chain
    fg = out_fg.clone().requires_grad_(True)
    bg = out_bg.clone().requires_grad_(True)
    cols = list(Q_COLS)
    qm = fg[:, cols] + fg[:, 4:5] * bg[:, cols]
    gq = w(1, o, d, qm.detach().contiguous(), vf | vb, render_fn)[1]
    (qm * gq).sum().backward()
    assert float(gq.abs().sum()) > 0
    torch.testing.assert_close(gfg, fg.grad, rtol=1e-6, atol=1e-9)
    torch.testing.assert_close(gbg, bg.grad, rtol=1e-6, atol=1e-9)
    assert bool((gfg[~(vf | vb)] == 0).all()) and bool((gbg[~(vf | vb)] == 0).all())


def test_pose_gradient_matches_central_difference_on_se3_refine():
    """dL/dse3_refine from the kernel's grad_rts (through torch.autograd.backward(cameras.get_rts(), grad_rts)) against a central
    finite difference of the whole warp loss (float64 restatement) along random directions, selection and scores frozen."""
    from scanerf_amd import cameras as CM
    from scanerf_amd.warp import WarpLoss
    ks, c2w = ring(10, seed=4)
    noise = torch.randn(10, 6, generator=torch.Generator().manual_seed(1)) * 0.01
    cams = CM.CameraSet(ks, c2w, DEV, noise=noise)
    _, images, _, o, d, q = scene(10, 3000, seed=4, occl=False)
    w = WarpLoss(cams, images, None, voxel_size=0.05)
    views, _, valid = w.select(o, d, q)
    pr = w.project(o, d, q, views, valid)
    score = torch.rand(valid.shape, device=DEV) * pr["valid"]
    _, _, _, _, g_rts = w.loss_grad(o, d, q, None, pr, score, 1.0)
    cams.se3_refine.grad = None
    torch.autograd.backward(cams.get_rts(), g_rts)
    grad = cams.se3_refine.grad.double()
    o64, d64, q64, ks64, img64, s64, rts0 = _f64(o, d, q, cams.ks, images, score, cams.rts)

    def f(se3):
        rts = CM.pose_compose([CM.se3_to_SE3(se3), rts0])
        return float(WR.warp_loss(o64, d64, q64[:, 0], q64[:, 1:4], q64[:, 4:7], rts, ks64, img64, None, pr["views"], pr["valid"],
                                  s64, corner_grid=pr["grid"].double()))
    gen = torch.Generator().manual_seed(7)
    h = 1e-6
    for _ in range(3):
        u = torch.randn(10, 6, generator=gen, dtype=F64).to(DEV)
        fd = (f(h * u) - f(-h * u)) / (2 * h)
        an = float((grad * u).sum())
        assert abs(an - fd) <= 2e-4 * abs(fd) + 1e-9, (an, fd)


def _tiny_trainer(warp, seed=0):
    from scanerf_amd import trainer
    from scanerf_amd.tile_model import TileModel
    torch.manual_seed(seed)
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=14, seed=seed)
    with torch.no_grad():
        m.features.mul_(150.0)
    g = torch.Generator().manual_seed(seed)
    B = 2048
    o = (torch.tensor([0.0, 0.0, -3.0]) + 0.1 * torch.randn(B, 3, generator=g)).to(DEV).contiguous()
    d = torch.cat([0.3 * torch.randn(B, 2, generator=g), torch.ones(B, 1)], 1).to(DEV).contiguous()
    tgt = torch.rand(B, 3, generator=g).to(DEV)
    return m, trainer.TileTrainer(m, lambda s: (o, d, tgt), total_step=100, num_sample=32, adjust_step=1000, warp=warp)


def test_warp_weight_zero_is_bit_identical_to_no_warp():
    from scanerf_amd.warp import WarpLoss
    cams, images, occ, *_ = scene(6, 1, seed=2)
    m0, t0 = _tiny_trainer(None)
    m1, t1 = _tiny_trainer(WarpLoss(cams, images, occ, voxel_size=0.05, weight=0.0))
    for _ in range(3):
        l0, l1 = t0.train_one_step(), t1.train_one_step()
        assert torch.equal(l0, l1)
    assert torch.equal(m0.features, m1.features)
    assert torch.equal(m0.decoder.params, m1.decoder.params)


def test_warp_term_refines_poses():
    """Bundle-adjustment smoke: a fixed synthetic scene seen by 4 overlapping views, images rendered from the true cameras, start
    poses perturbed; a few dozen TileTrainer iterations with the warp term (table and decoder frozen) lower the warp loss and the
    camera-centre error."""
    from scanerf_amd import cameras as CM
    from scanerf_amd import trainer
    from scanerf_amd.tile_model import TileModel
    from scanerf_amd.warp import WarpLoss
    torch.manual_seed(0)
    H, W, C, S_ = 48, 64, 4, 64
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=15, seed=5)
    with torch.no_grad():
        m.features.mul_(150.0)
    eye = torch.eye(3)
    c2w = torch.stack([torch.cat([eye, torch.tensor([[x0], [0.1 * x0], [-3.0]])], -1) for x0 in (-0.6, -0.2, 0.2, 0.6)])
    ks = torch.tensor([[60.0, 0, W / 2, 0, 60.0, H / 2, 0, 0, 1]]).repeat(C, 1).reshape(C, 3, 3)
    true_cams = CM.CameraSet(ks, c2w, DEV)
    locs = CM.pixel_locs(C, torch.arange(H * W), W, DEV)
    with torch.no_grad():
        o, d = true_cams.get_rays(locs)
        images = m.render_fore_fused(o.contiguous(), d.contiguous(), S_, 0)[0][:, 0:3].reshape(C, H, W, 3).contiguous()
    noise = torch.tensor([[0.0, 0.01, 0.0, 0.05, -0.04, 0.0], [0.01, 0.0, 0.0, -0.04, 0.05, 0.02],
                          [0.0, -0.01, 0.005, 0.04, 0.03, -0.03], [0.0, 0.0, 0.01, -0.03, -0.03, 0.02]])
    cams = CM.CameraSet(ks, c2w, DEV, noise=noise)
    warp = WarpLoss(cams, images, None, voxel_size=0.2, gamma=2.0, weight=1.0, start_step=-1, warming=False)
    batch = CM.pixel_locs(C, torch.arange(0, H * W, 2), W, DEV)
    tgt = images.reshape(-1, 3)[(batch[:, 0].long() * H + batch[:, 2].long()) * W + batch[:, 1].long()].contiguous()
    tr = trainer.TileTrainer(m, lambda s: (batch, tgt), total_step=1000, eta_hash=1e-12, eta_decoder=1e-12, num_sample=S_,
                             adjust_step=100000, cameras=cams, eta_cam=3e-3, warp=warp)
    losses = []
    for _ in range(40):
        tr.train_one_step()
        assert warp.last_loss is not None and warp.last_grad_rts is not None
        losses.append(float(warp.last_loss))
    with torch.no_grad():
        err0 = float(torch.linalg.norm(CM.pose_invert(cams.rts)[..., 3] - true_cams.get_poses()[..., 3], dim=-1).mean())
        err1 = float(torch.linalg.norm(cams.get_poses()[..., 3] - true_cams.get_poses()[..., 3], dim=-1).mean())
    print("warp pose refinement: warp loss %.6f -> %.6f, camera centre error %.4f -> %.4f" % (losses[0], losses[-1], err0, err1))
    assert losses[0] > 0
    assert np.mean(losses[-5:]) < 0.9 * np.mean(losses[:5]), losses
    assert err1 < 0.8 * err0, (err0, err1)
