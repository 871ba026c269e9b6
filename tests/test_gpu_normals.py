"""Surface normals on the GPU (csrc/normals.hip): scanerf_render_normals / scanerf_sigma_normals_points and the Python surface on
top of them, judged per ray and per sample against the float64 closed form of tests/normals_reference.py -- a bound is K x the error
the float32 yardstick makes on the same inputs (K: profiles/normals_error.md), never a number taken from the kernel."""
import numpy as np
import pytest
import torch

import normals_reference as R
from conftest import need_symbol
from per_ray_reference import FIGURES
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _launch(c, want_sample_normals=True):
    """Both forms on a case's inputs -> (out [B,4], sample_normals [B,S,3], (sigma [N], grad [N,3], normal [N,3]) of the point form at
    the case's pinned contracted points with axis_scale = 4 / bbox_size)."""
    import scanerf_amd  # noqa
    from scanerf_amd import render
    ins, r64, _ = R.case_reference(c)
    table, res = ins["table"].to(DEV), ins["res"].to(DEV).contiguous()
    blob, wf = O.pack_blob(ins["sd"]).to(DEV), R.case_mask(ins).to(DEV)
    valid = None if ins["valid"] is None else _dev(ins["valid"])
    out, sn = render.render_normals(_dev(ins["o"]), _dev(ins["d"]), _dev(ins["z"]), _dev(ins["dist"]), table, res, blob, wf,
                                    ins["mn"].tolist(), ins["sz"].tolist(), ins["infinity"], ray_valid=valid,
                                    want_sample_normals=want_sample_normals)
    pts = render.sigma_normals_points(_dev(r64["x"]), table, res, blob, wf, axis_scale=R.ascale_of(ins["sz"]).tolist(), want_grad=True)
    torch.cuda.synchronize()
    return out, sn, pts


@pytest.mark.parametrize("c", R.ALL_CASES, ids=R.case_id)
def test_both_forms_against_float64_per_ray_and_per_sample(c):
    """Every shape at which the kernel takes another path (S below / at / above a wave, rays per wave 64 .. 1, several 64-sample
    rounds; one ray .. more rays than one pass of the grid's waves), ray_valid, infinity, f32 and f16 tables, T = 2^10 .. 2^13 and
    2^19, and every family of the case list: per ray |out[:3] - n64| / sum w64 and sum w; per sample |g - g64| / |cond|."""
    ins, r64, r32 = R.case_reference(c)
    out, sn, (sigma, grad, normal) = _launch(c)
    B, S = ins["z"].shape
    for name, t in (("out", out), ("sample_normals", sn), ("sigma", sigma), ("grad", grad), ("normal", normal)):
        assert bool(torch.isfinite(t).all()), name
    assert out.shape == (B, 4) and sn.shape == (B, S, 3) and sigma.shape == (B * S,) and grad.shape == normal.shape == (B * S, 3)
    bad = R.judge_rays(R.case_id(c), out, r64, r32)
    bad += R.judge_samples(R.case_id(c), grad, r64["pts"], r32["pts"])
    # the per-sample normals the ray form hands out, composited with the float64 weights: the same per-ray judgement
    keep = torch.ones(B, dtype=torch.float64) if ins["valid"] is None else T(ins["valid"]).double()
    comp = torch.cat([(r64["w"][..., None] * sn.cpu().double()).sum(1) * keep[:, None], r64["out"][:, 3:]], 1)
    bad += R.judge_rays(R.case_id(c) + " (sample_normals)", comp, r64, r32)
    bad += R.judge(R.case_id(c) + " sigma", sigma, r64["pts"]["sigma"][:, None], r32["pts"]["sigma"][:, None], R.K, floor=R.FLOOR)
    if ins["valid"] is not None:   # invalid rays: exactly zero, per-sample normals included
        off = ~T(ins["valid"])
        assert float(out.cpu()[off].abs().max()) == 0.0 and float(sn.cpu()[off].abs().max()) == 0.0
    if c.family == "zero":         # g = 0 exactly: the 1e-8 of the normalisation makes n = 0, no NaN
        assert float(grad.abs().max()) == 0.0 and float(normal.abs().max()) == 0.0 and float(out[:, :3].abs().max()) == 0.0
        assert float(out[:, 3].min()) > 0.1
    elif c.valid != "none" and c.family != "empty":
        assert float(out[:, :3].abs().max()) > 1e-3
    assert float(normal.norm(dim=1).max()) <= 1.0 + 1e-5 and float(sn.norm(dim=-1).max()) <= 1.0 + 1e-5
    assert not bad, bad


def _hashgrid_from_g15(g):
    import scanerf_amd  # noqa
    from scanerf_amd import network
    from scanerf_amd.hashgrid import HashGrid
    hg = HashGrid(DEV, T(g["tile_corner"]), T(g["tile_size"]), log2_hashmap_size=10, grid_resolution=[32, 2048], sampler_log2dim=4)
    assert np.array_equal(hg.HE.resolution.cpu().numpy(), g["res"])
    hg.occupied_grid = T(g["occ"]).to(DEV)
    with torch.no_grad():
        hg.HE.features.copy_(T(g["features"]).to(DEV))
    dec = network.ShallowMLP(32)
    sd = {k[3:]: T(v) for k, v in g.items() if k.startswith("sd.")}
    dec.load_state_dict(sd)
    return hg, dec.to(DEV), sd


def _g18_reference(g15, g18, sd, hg, dtype):
    step = int(g18["global_step"])
    return R.render_normals(g18["rays_o"], g18["rays_d"], g18["z_vals"], g18["dists"], T(g15["features"]), T(g15["res"]), sd,
                            hg.min_bbox.cpu(), hg.bbox_size.cpu(), R.mask64(step).to(R.F32), False, dtype=dtype)


def test_hashgrid_render_normals_against_the_reference_golden_g18(golden):
    """G18 (the reference's own autograd normals, B = 26, S = 16) through HashGrid.render_normals: the fused route under the per-ray
    judgement with the golden as the reference, and the op-by-op route of the same call within the same bound of the fused one."""
    g15, g18 = golden("g15_render_masks"), golden("g18_normals")
    hg, dec, sd = _hashgrid_from_g15(g15)
    o, d, z, dist = (T(g18[k]).to(DEV) for k in ("rays_o", "rays_d", "z_vals", "dists"))
    step = int(g18["global_step"])
    n = hg.render_normals(o, d, z, dist, dec, global_step=step)
    assert hg.last_render_route == "fused_normals" and n.shape == (26, 3) and n.dtype == torch.float32 and not n.requires_grad
    r64, r32 = _g18_reference(g15, g18, sd, hg, R.F64), _g18_reference(g15, g18, sd, hg, R.F32)
    gold = T(g18["normal"]).double()
    # the golden is a float32 result itself: the yardstick's figure against it is what float32 rounding allows
    bad = R.judge("G18 fused vs golden", n, gold, r32["out"][:, :3], R.K, scale=r64["out"][:, 3], floor=R.FLOOR)
    bad += R.judge("G18 fused vs float64", n, r64["out"][:, :3], r32["out"][:, :3], R.K, scale=r64["out"][:, 3], floor=R.FLOOR)
    hg.fused = False
    n_ops = hg.render_normals(o, d, z, dist, dec, global_step=step)
    assert hg.last_render_route == "ops" and n_ops.shape == (26, 3)
    bad += R.judge("G18 ops vs fused", n_ops, n.cpu().double(), r32["out"][:, :3] - r64["out"][:, :3] + n.cpu().double(), R.K,
                   scale=r64["out"][:, 3], floor=R.FLOOR)
    assert not bad, bad


@pytest.mark.parametrize("half", [False, True])
def test_compute_normal_point_form(golden, half):
    """HashGrid.compute_normal / inference_sigma on [5,7,3]-shaped samples (axis_scale = ones: the reference applies no contraction
    there): shapes, dtypes, detached; normal and sigma against the yardstick; sigma against decoder.inference_sigma on the encoder
    op's features within the decoder op's bound (tests/test_gpu_decoder_op.py: rtol 1e-4, atol 1e-6)."""
    g15 = golden("g15_render_masks")
    hg, dec, sd = _hashgrid_from_g15(g15)
    if half:
        hg.HE.features.data = hg.HE.features.data.half()
    rng = np.random.default_rng(5)
    x = T(rng.uniform(-1.9, 1.9, (5, 7, 3)).astype(np.float32)).to(DEV)
    normal, sigma = hg.compute_normal(x, dec)
    assert normal.shape == (5, 7, 3) and sigma.shape == (5, 7, 1) and normal.dtype == sigma.dtype == torch.float32
    assert not normal.requires_grad and not sigma.requires_grad
    assert torch.equal(hg.inference_sigma(x, dec), sigma)
    table = hg.HE.features.detach().cpu()
    ones = torch.ones(32)
    p64 = R.sigma_normals(x.cpu().numpy().reshape(-1, 3), np.ones(3, np.float32), table, T(g15["res"]), sd, ones, R.F64)
    p32 = R.sigma_normals(x.cpu().numpy().reshape(-1, 3), np.ones(3, np.float32), table, T(g15["res"]), sd, ones, R.F32)
    unit = torch.ones(35, dtype=torch.float64)
    bad = R.judge("compute_normal normal", normal.reshape(-1, 3), p64["n"], p32["n"], R.K, scale=unit, floor=R.FLOOR)
    bad += R.judge("compute_normal sigma", sigma.reshape(-1, 1), p64["sigma"][:, None], p32["sigma"][:, None], R.K, floor=R.FLOOR)
    assert float(normal.norm(dim=-1).min()) > 0.99
    if not half:
        with torch.no_grad():
            ref = dec.inference_sigma(hg.HE(x.reshape(-1, 3))).reshape(5, 7, 1)
        np.testing.assert_allclose(sigma.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-6)
        hg.fused = False   # the torch autograd route of the same call
        n_t, s_t = hg.compute_normal(x, dec)
        assert n_t.shape == (5, 7, 3) and s_t.shape == (5, 7, 1) and not n_t.requires_grad
        # (tests/test_gpu_autograd_boundary.py's bound on the op-by-op normals: 2e-3 relative L2)
        assert float((n_t.reshape(-1, 3).cpu().double() - p64["n"]).norm() / p64["n"].norm()) < 2e-3
        np.testing.assert_allclose(s_t.cpu().numpy(), sigma.cpu().numpy(), rtol=1e-4, atol=1e-6)
    assert not bad, bad


@pytest.mark.parametrize("N", [1, 777])
def test_point_form_sizes(N):
    import scanerf_amd  # noqa
    from scanerf_amd import render
    ins = R.case_inputs(R.CASES_S[3])
    rng = np.random.default_rng(N)
    x = rng.uniform(-2, 2, (N, 3)).astype(np.float32)
    A = np.asarray([1.0, 0.5, 3.0], np.float32)
    mask = R.case_mask(ins)
    sigma, grad, normal = render.sigma_normals_points(_dev(x), ins["table"].to(DEV), ins["res"].to(DEV), O.pack_blob(ins["sd"]).to(DEV),
                                                      mask.to(DEV), axis_scale=A.tolist(), want_grad=True)
    assert sigma.shape == (N,) and grad.shape == normal.shape == (N, 3)
    p64, p32 = (R.sigma_normals(x, A, ins["table"], ins["res"], ins["sd"], mask, dt) for dt in (R.F64, R.F32))
    bad = R.judge_samples(f"points N={N}", grad, p64, p32)
    bad += R.judge(f"points N={N} normal", normal, p64["n"], p32["n"], R.K, scale=torch.ones(N, dtype=torch.float64),
                   only=("max", "pooled") if N < 16 else FIGURES, floor=R.FLOOR)
    _, none_grad, n2 = render.sigma_normals_points(_dev(x), ins["table"].to(DEV), ins["res"].to(DEV), O.pack_blob(ins["sd"]).to(DEV),
                                                   mask.to(DEV), axis_scale=A.tolist())
    assert none_grad is None and torch.equal(n2, normal)
    assert not bad, bad


@pytest.mark.parametrize("c", [R.CASES_S[6], R.CASES_HALF[0], R.CASES_B[5]], ids=R.case_id)
def test_two_launches_give_equal_bits_with_and_without_cold_instruction_caches(c):
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    need_symbol("scanerf_icache_sweep")
    a = _launch(c)
    _capi.check(_capi.lib().scanerf_icache_sweep(_capi.stream()), "icache_sweep")
    b = _launch(c)
    for x, y in zip((a[0], a[1]) + a[2], (b[0], b[1]) + b[2]):
        assert torch.equal(x, y)


def _tile_model(table_dtype=torch.float32):
    import scanerf_amd  # noqa
    from scanerf_amd import tile_model
    m = tile_model.TileModel([-4.0, -4.0, -4.0], [8.0, 8.0, 8.0], DEV, log2_T=12, seed=3, table_dtype=table_dtype)
    with torch.no_grad():   # a table and a density with something to see
        m.features.mul_(0.5 / float(m.features.std()))
    grid = torch.ones_like(m.occupied_grid)
    grid[: grid.shape[0] // 2] = False    # half of the box is empty along the grid's first axis
    m.set_occupancy(grid)
    return m


def _view(H, W):
    ys, xs = np.meshgrid(np.linspace(-0.6, 0.6, H), np.linspace(-0.9, 0.9, W), indexing="ij")
    # from the empty corner, every component of the directions taking both signs: whichever axis the grid's first one is, some
    # rays reach the occupied half and some never do
    d = np.stack([xs, ys, 0.5 * xs - 0.3 * ys + 0.05], -1).reshape(-1, 3).astype(np.float32)
    o = np.tile(np.asarray([[-0.3, -0.2, -0.25]], np.float32), (H * W, 1))
    return _dev(o), _dev(d)


@pytest.mark.parametrize("table_dtype", [torch.float32, torch.float16])
def test_tile_model_render_normals(table_dtype):
    """(sum w n + 1) / 2 of the fore-valid rays in their order, on gather_table(); None when the sampler serves no ray."""
    import scanerf_amd  # noqa
    from scanerf_amd import render
    m = _tile_model(table_dtype)
    o, d = _view(8, 12)
    S = 16
    got = m.render_normals(o, d, S)
    z, dist = m.sample(o, d, S)
    valid = torch.all(z != -1, dim=-1)
    assert 0 < int(valid.sum()) < o.shape[0]
    assert got.shape == (int(valid.sum()), 3) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert m.gather_table().dtype == table_dtype
    out, _ = render.render_normals(o[valid].contiguous(), d[valid].contiguous(), z[valid].contiguous(), dist[valid].contiguous(), m.gather_table().detach(),
                                   m.resolution, m.decoder.blob().detach(), torch.ones(32, device=DEV), m.min_bbox.tolist(), m.bbox_size.tolist(), False)
    assert torch.equal(got, (out[:, :3] + 1.0) / 2.0)
    assert float((got - 0.5).abs().max()) > 1e-3
    if table_dtype == torch.float32:
        # the other harness layer: a HashGrid on the same tile, table and decoder gives the same normals
        from scanerf_amd import network
        from scanerf_amd.hashgrid import HashGrid
        hg = HashGrid(DEV, [-4.0, -4.0, -4.0], [8.0, 8.0, 8.0], log2_hashmap_size=12, grid_resolution=[32, 2048], sampler_log2dim=4)
        assert torch.equal(hg.HE.resolution.cpu().int(), m.resolution.cpu().int())
        with torch.no_grad():
            hg.HE.features.copy_(m.features)
        dec = network.ShallowMLP(32)
        dec.load_state_dict({k: v.detach().cpu().clone() for k, v in m.decoder.ref_state_dict().items()})
        n_hg = hg.render_normals(o[valid], d[valid], z[valid], dist[valid], dec.to(DEV))
        assert hg.last_render_route == "fused_normals" and torch.equal(got, (n_hg + 1.0) / 2.0)
    # against the yardstick (no mask: hashgrid/__init__.py:368-392 applies none)
    sd = {k: v.detach().cpu() for k, v in m.decoder.ref_state_dict().items()}
    args = (o[valid].cpu().numpy(), d[valid].cpu().numpy(), z[valid].cpu().numpy(), dist[valid].cpu().numpy(), m.gather_table().detach().cpu(),
            m.resolution.cpu(), sd, m.min_bbox, m.bbox_size, torch.ones(32), False)
    r64, r32 = R.render_normals(*args, dtype=R.F64), R.render_normals(*args, dtype=R.F32)
    bad = R.judge_rays("TileModel.render_normals", out, r64, r32)
    away = _dev(np.tile(np.asarray([[-1.0, -1.0, -1.0]], np.float32), (5, 1)))
    assert m.render_normals(_dev(np.tile(np.asarray([[-0.5, -0.5, -0.5]], np.float32), (5, 1))), away, S) is None
    assert not bad, bad


def test_render_image_rays_in_ragged_chunks():
    """A 24 x 16 view in chunks of 100 rays (the last one ragged): the reference's eight maps; rgb / depth / diffuse / specular are
    render_rays_fused's on the whole view (rays are independent: equal bits); the normal map is non-zero exactly on the fore-valid
    rays; normals=False leaves it black."""
    import scanerf_amd  # noqa
    from scanerf_amd import render
    m = _tile_model()
    H, W = 16, 24
    o, d = _view(H, W)
    occ = torch.ones(H * W, 1, dtype=torch.bool, device=DEV)
    occ[5::7] = False
    for mask in (None, occ):
        img = m.render_image_rays(o, d, 16, 8, 20000, occlusion_mask=mask, batch_size=100)
        assert set(img) == {"rgb", "fore_depth", "depth", "diffuse", "specular", "fore", "normal", "tint"}
        for k, v in img.items():
            assert v.shape == (H * W, 1 if "depth" in k else 3) and bool(torch.isfinite(v).all()), k
        whole = m.render_rays_fused(o, d, 16, 8, 20000, occlusion_mask=mask)
        vf = whole["fore_valid"]
        assert 0 < int(vf.sum()) < H * W
        assert torch.equal(img["rgb"], whole["pred_color"]) and torch.equal(img["depth"], whole["pred_depth"])
        assert torch.equal(img["diffuse"], whole["fg"][:, render.DIFFUSE]) and torch.equal(img["specular"], whole["fg"][:, render.SPECULAR])
        assert torch.equal(img["fore"], whole["fg"][:, render.RGB]) and torch.equal(img["fore_depth"], whole["fg"][:, render.DEPTH, None])
        assert torch.equal(img["tint"], whole["fg"][:, render.TINT])
        assert torch.equal(img["normal"].abs().sum(1) > 0, vf)
        if mask is None:
            assert torch.equal(img["normal"][vf], m.render_normals(o, d, 16))
        black = m.render_image_rays(o, d, 16, 8, 20000, occlusion_mask=mask, batch_size=100, normals=False)
        assert float(black["normal"].abs().max()) == 0.0 and torch.equal(black["rgb"], img["rgb"])


def test_trainer_validate_panels():
    import scanerf_amd  # noqa
    from scanerf_amd import trainer
    m = _tile_model()
    H, W = 16, 24
    o, d = _view(H, W)
    tr = trainer.TileTrainer(m, None, num_sample=16, num_bg_sample=8)
    tr.global_step = 20000
    target = np.random.default_rng(0).uniform(0, 1, (H, W, 3)).astype(np.float32)
    occ = torch.ones(H * W, 1, dtype=torch.bool, device=DEV)
    occ[::5] = False
    rows = tr.validate([(o, d, target, None, H, W), (o, d, None, occ, H, W)], batch_size=100)
    assert len(rows) == 2
    assert np.isfinite(rows[0]["psnr"]) and np.isfinite(rows[0]["ssim"]) and 0 < rows[0]["psnr"] < 100 and -1 <= rows[0]["ssim"] <= 1
    assert rows[1]["psnr"] is None and rows[1]["ssim"] is None
    img = m.render_image_rays(o, d, 16, 8, 20000, batch_size=100)
    for r in rows:
        for k in ("panel", "novel_panel"):
            assert r[k].shape == (2 * H, 3 * W, 3) and r[k].dtype == np.float32 and r[k].min() >= 0.0 and r[k].max() <= 1.0
    np.testing.assert_array_equal(rows[0]["panel"][H:, 2 * W:], target)
    np.testing.assert_array_equal(rows[0]["panel"][:H, :W], img["rgb"].reshape(H, W, 3).clamp(0, 1).cpu().numpy())
    # the normal map sits bottom-left of the novel-view panel with its channels reversed (tile.py:856)
    np.testing.assert_array_equal(rows[0]["novel_panel"][H:, :W], img["normal"].reshape(H, W, 3).flip(-1).cpu().numpy())
    assert rows[0]["novel_panel"][H:, :W].max() > 0


def test_arguments_are_validated_before_any_launch():
    """Wrong dtype or contiguity, S < 1 and a table size that is no power of two raise (Python surface and C entry points) and
    leave the stream clean."""
    import scanerf_amd  # noqa
    from scanerf_amd import _capi, render
    ins = R.case_inputs(R.CASES_S[3])
    B, S = ins["z"].shape
    table, res = ins["table"].to(DEV), ins["res"].to(DEV).contiguous()
    blob, wf = O.pack_blob(ins["sd"]).to(DEV), R.case_mask(ins).to(DEV)
    good = dict(rays_o=_dev(ins["o"]), rays_d=_dev(ins["d"]), z_vals=_dev(ins["z"]), dists=_dev(ins["dist"]), features=table, resolutions=res,
                blob=blob, weight_feature=wf, min_bbox=ins["mn"].tolist(), bbox_size=ins["sz"].tolist())
    ref, _ = render.render_normals(**good)
    torch.cuda.synchronize()
    bad_calls = {
        "rays_o dtype": dict(rays_o=good["rays_o"].double()),
        "z_vals contiguity": dict(z_vals=_dev(np.ascontiguousarray(ins["z"].T)).t()),
        "resolutions dtype": dict(resolutions=res.long()),
        "S < 1": dict(z_vals=good["z_vals"][:, :0].contiguous(), dists=good["dists"][:, :0].contiguous()),
        "T not a power of two": dict(features=table[:, :1000].contiguous()),
        "features dtype": dict(features=table.double()),
        "bf16 table": dict(features=table.bfloat16()),
        "blob size": dict(blob=blob[:-1].contiguous()),
        "cpu tensor": dict(dists=good["dists"].cpu()),
    }
    for what, change in bad_calls.items():
        with pytest.raises(RuntimeError):
            render.render_normals(**{**good, **change})
    x = _dev(R.case_reference(R.CASES_S[3])[1]["x"])
    for what, kw in {"points dtype": dict(points=x.double()), "points contiguity": dict(points=_dev(np.zeros((3, 8), np.float32)).t()),
                     "T not a power of two": dict(points=x, features=table[:, :1000].contiguous())}.items():
        with pytest.raises(RuntimeError):
            render.sigma_normals_points(**{**dict(points=x, features=table, resolutions=res, blob=blob, weight_feature=wf), **kw})
    # the C entry points themselves (a caller that bypasses the Python checks): status 2, nothing launched
    import ctypes
    f3 = (ctypes.c_float * 3)(16.0, 16.0, 16.0)
    out = torch.full((B, 4), 7.0, device=DEV)
    ptrs = [good[k].data_ptr() for k in ("rays_o", "rays_d", "z_vals", "dists")] + [table.data_ptr(), _capi.F32, res.data_ptr(), blob.data_ptr(), wf.data_ptr(), f3, f3]
    tail = [0, None, out.data_ptr(), None]
    for B_, S_, T_ in ((B, 0, 1024), (B, S, 1000), (-1, S, 1024)):
        args = ptrs + tail + [B_, S_, T_, _capi.stream()]
        assert _capi.lib().scanerf_render_normals(*args) == 2
    args = ptrs[:5] + [7] + ptrs[6:] + tail + [B, S, table.shape[1], _capi.stream()]
    assert _capi.lib().scanerf_render_normals(*args) == 2   # feat_dtype
    pargs = [x.data_ptr(), f3, table.data_ptr(), _capi.F32, res.data_ptr(), blob.data_ptr(), wf.data_ptr(), out.data_ptr(), None, out.data_ptr(), 4, 1000, _capi.stream()]
    assert _capi.lib().scanerf_sigma_normals_points(*pargs) == 2
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0
    again, _ = render.render_normals(**good)
    assert torch.equal(again, ref)
