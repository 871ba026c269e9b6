"""CPU checks of the monocular losses' yardstick (tests/mono_reference.py, the float64 restatement the GPU tests compare the HIP
kernels with), pinned to golden G22 (the reference's own mono_loss.py / criterions.py, tests/golden/make_golden_mono.py); and
the argument rules of scanerf_amd.mono.MonoLoss and of the training entry points that take it."""
import numpy as np
import pytest
import torch

import mono_reference as MR

F64 = torch.float64


@pytest.fixture(scope="module")
def g22(golden):
    return {k: torch.from_numpy(v) if v.ndim else v for k, v in golden("g22_mono").items()}


def _close(a, b, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * max(1e-300, float(np.abs(b).max(initial=0.0))))


def test_main_case_matches_reference(g22):
    """8 views x 128 rays: one view with a single valid ray (det = 0), one with none, two at 50 +- 1, failing and masked patches."""
    depth, locs, valid, md, mn, kinv = MR.golden_case(g22, "main")
    N = md.shape[0]
    m = valid.reshape(N, -1)
    assert int(m[0].sum()) == 1 and int(m[1].sum()) == 0
    d = depth.reshape(N, -1)
    assert float((d[2:4].max(1)[0] - d[2:4].min(1)[0]).max()) < 0.05 * 50
    ok = MR.patch_valid(locs, valid, mn).reshape(N, -1)
    masked_one = (m.reshape(N, -1, 4).sum(-1) == 3)
    assert bool(ok.any()) and bool((~ok).any()) and bool(masked_one.any())
    ld, ls, gd, gs = MR.losses_and_grads(depth, locs, valid, md, mn, kinv)
    assert bool(g22["main_has_depth"])
    _close(ld, g22["main_loss_depth"])
    _close(ls, g22["main_loss_smooth"])
    _close(gd, g22["main_grad_depth"].reshape(-1))
    _close(gs, g22["main_grad_smooth"].reshape(-1))


def test_single_ray_view_contributes_t_squared_and_no_gradient(g22):
    depth, locs, valid, md, mn, kinv = MR.golden_case(g22, "main")
    h0, h1 = MR.scale_shift(depth, md[locs[:, 0].long(), locs[:, 2].long(), locs[:, 1].long()], valid, locs[:, 0].long(), md.shape[0])
    assert float(h0[0]) == 0.0 and float(h1[0]) == 0.0 and float(h0[1]) == 0.0
    B0 = depth.numel() // md.shape[0]
    assert bool((g22["main_grad_depth"][0] == 0).all()) and bool((g22["main_grad_depth"][1] == 0).all())
    # the single ray's t^2 is part of the reference's sum
    t = g22["main_mono_depth"][0][valid[:B0]]
    assert t.numel() == 1
    num = float(g22["main_loss_depth"]) * float(valid.sum())
    assert num > float(t[0]) ** 2


def test_no_valid_patch_is_nan_in_reference_zero_here(g22):
    """Deliberate difference: the reference's torch.mean of an empty tensor is NaN; the restatement (and the kernels) give 0."""
    depth, locs, valid, md, mn, kinv = MR.golden_case(g22, "nopatch")
    assert np.isnan(float(g22["nopatch_loss_smooth"]))
    ld, ls, gd, gs = MR.losses_and_grads(depth, locs, valid, md, mn, kinv)
    assert float(ls) == 0.0 and bool((gs == 0).all())
    _close(ld, g22["nopatch_loss_depth"])
    _close(gd, g22["nopatch_grad_depth"].reshape(-1))


def test_no_valid_ray_is_skipped(g22):
    depth, locs, valid, md, mn, kinv = MR.golden_case(g22, "empty")
    assert not bool(g22["empty_has_depth"])
    ld, ls, gd, gs = MR.losses_and_grads(depth, locs, valid, md, mn, kinv)
    assert float(ld) == 0.0 and float(ls) == 0.0 and bool((gd == 0).all()) and bool((gs == 0).all())


def test_ray_order_does_not_matter(g22):
    """Views are grouped by locs[:, 0]: permuting whole patches (the patch structure is positional) changes nothing."""
    depth, locs, valid, md, mn, kinv = MR.golden_case(g22, "main")
    perm = torch.randperm(depth.numel() // 4, generator=torch.Generator().manual_seed(0))
    idx = (perm[:, None] * 4 + torch.arange(4)[None]).reshape(-1)
    a = MR.losses_and_grads(depth, locs, valid, md, mn, kinv)
    b = MR.losses_and_grads(depth[idx], locs[idx], valid[idx], md, mn, kinv)
    _close(b[0], a[0])
    _close(b[1], a[1])
    _close(b[2], a[2][idx])
    _close(b[3], a[3][idx])


@pytest.mark.parametrize("name,w", [("depth", 0.01), ("smooth", 0.001)])
@pytest.mark.parametrize("start", [0, 500])
def test_schedule_matches_loss_item(g22, name, w, start):
    """criterions.LossItem: added for start < step < end, weight w 0.1^((step - start) / 30000) -- steps 0, start, start + 1,
    30 000 and end among them."""
    steps = [int(s) for s in g22["sched_steps"]]
    want = g22[f"sched_{name}_{start}"].numpy()
    got = np.array([MR.weight(w, start, s, 40000) for s in steps])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    from scanerf_amd.mono import MonoLoss
    ks = torch.eye(3, dtype=torch.float32)[None].repeat(2, 1, 1)
    maps = dict(mono_depths=torch.ones(2, 4, 4)) if name == "depth" else dict(mono_normals=torch.ones(2, 4, 4, 3))
    kw = dict(depth_start=start) if name == "depth" else dict(smooth_start=start)
    m = MonoLoss(ks, weight_depth=0.01, weight_smooth=0.001, end_step=40000, **maps, **kw)
    got = np.array([(m.scale_depth if name == "depth" else m.scale_smooth)(s) for s in steps])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    other = m.scale_smooth if name == "depth" else m.scale_depth   # that map is None: the term is off
    assert all(other(s) == 0.0 for s in steps)


def _mono(N=2, H=4, W=4, **kw):
    from scanerf_amd.mono import MonoLoss
    return MonoLoss(torch.eye(3)[None].repeat(N, 1, 1), mono_depths=torch.ones(N, H, W), mono_normals=torch.ones(N, H, W, 3), **kw)


def test_monoloss_argument_rules():
    from scanerf_amd.mono import MonoLoss
    with pytest.raises(ValueError, match="needs mono_depths"):
        MonoLoss(torch.eye(3)[None])
    with pytest.raises(ValueError, match="ks"):
        MonoLoss(torch.eye(3), mono_depths=torch.ones(1, 4, 4))
    with pytest.raises(ValueError, match="mono_normals must be"):
        MonoLoss(torch.eye(3)[None].repeat(2, 1, 1), mono_depths=torch.ones(2, 4, 4), mono_normals=torch.ones(2, 4, 5, 3))
    with pytest.raises(ValueError, match="mono_depths must be"):
        MonoLoss(torch.eye(3)[None].repeat(2, 1, 1), mono_depths=torch.ones(2, 4, 4, 1))
    with pytest.raises(ValueError, match="maps"):
        MonoLoss(torch.eye(3)[None].repeat(2, 1, 1), mono_depths=torch.ones(3, 4, 4))
    with pytest.raises(ValueError, match="mono_normals"):
        MonoLoss(torch.eye(3)[None].repeat(2, 1, 1), mono_normals=torch.ones(2, 4, 4))
    m = _mono()
    assert m.N == 2 and (m.H, m.W) == (4, 4) and m.kinv.shape == (2, 9) and m.kinv.dtype == torch.float32
    with pytest.raises(ValueError, match="locs"):
        m.loss_grad(torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8), None, 0.01, 0.001)
    with pytest.raises(ValueError, match="depth"):
        m.loss_grad(torch.zeros(8, 3, dtype=torch.int32), torch.zeros(8, 1), None, 0.01, 0.001)
    with pytest.raises(ValueError, match="valid"):
        m.loss_grad(torch.zeros(8, 3, dtype=torch.int32), torch.zeros(8), torch.ones(7, dtype=torch.bool), 0.01, 0.001)
    with pytest.raises(ValueError, match="multiple of 4"):
        m.loss_grad(torch.zeros(6, 3, dtype=torch.int32), torch.zeros(6), None, 0.01, 0.001)
    # the step is outside the schedule: no call at all (and nothing is validated or launched)
    assert m(0, torch.zeros(6, 3, dtype=torch.int32), torch.zeros(6)) is None
    assert m.last_depth_loss is None and m.last_smooth_loss is None


def test_entry_points_need_locs_with_mono():
    from scanerf_amd import tile_model as TM
    m = _mono()
    o = torch.zeros(8, 3)
    with pytest.raises(ValueError, match="needs locs"):
        TM.train_step_fused(None, None, o, o, o, 8, 1, mono=m)
    with pytest.raises(ValueError, match="compact_rays=True"):
        TM.train_step_fused(None, None, o, o, o, 8, 1, mono=m, locs=torch.zeros(8, 3, dtype=torch.int32), compact_rays=True)
    with pytest.raises(ValueError, match="needs locs"):
        TM.fgbg_gradients(None, o, o, o, 8, 8, 1, mono=m)
    with pytest.raises(ValueError, match="needs locs"):
        TM.train_step_fgbg(None, None, o, o, o, 8, 8, 1, mono=m)


def test_trainer_without_cameras_needs_locs_from_get_batch():
    from scanerf_amd import trainer
    model = type("M", (), {"decoder": torch.nn.Linear(2, 2)})()
    o = torch.zeros(8, 3)
    tr = trainer.TileTrainer(model, lambda s: (o, o, o), total_step=10, mono=_mono())
    with pytest.raises(ValueError, match="get_batch must return"):
        tr.train_one_step()
