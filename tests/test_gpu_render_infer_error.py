"""Render-time inference judged per sample and per ray against float64 (needs an MI355X): pts_inference, pts_inference_tracing,
bg_pts_inference_v2, bg_pts_inference and accumulate_color through the scanerf_amd.hashgrid bindings, and
TileSetRenderer.render_rays, on the cases of tests/render_infer_reference.py -- whose docstring states the reference, the judgement
and where each K comes from; tests/test_render_infer_reference_cpu.py judges that reference on its own.

Every route is judged against the SAME float64 result: the default (16-sample tiles, folded activation), the plain images, "h3",
the single-pass "f32" kernel (layout 0), the fused slot lists with and without SKIP_UNSAMPLED, both chunk-major kernels on G36, the
single-pass fallback above 64 tiles on G65, and the layouts 0 / 1 / 2.  Everything is crossed on one case (G9, S = 17); the others
run the layout the renderer uses by default.  Run with -s for one judge line per op, route, case and figure."""
import functools

import numpy as np
import pytest
import torch

import render_infer_reference as R
import render_normals_reference as RNR
import render_scenes as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = RS.B_RAYS
BP = B + -B % 32
NAN = float("nan")
ROUTES = {"default": ("t16", True), "plain": ("t16", False), "h3": ("h3", True), "f32": ("f32", True)}


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def n(t):
    return t.detach().cpu().numpy()


def ops():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import hashgrid as H
    return H


def HG():
    import scanerf_amd  # noqa: F401
    from scanerf_amd.hashgrid.lib import HASHGRID
    return HASHGRID


@functools.lru_cache(maxsize=None)
def dev_scene(name, family):
    """A family's scene arrays on the GPU, uploaded and packed once (read-only for the tests)"""
    sc = R.family_scene(name, family)[0]
    D = {k: g(sc[k]) for k in ("corners", "sizes", "occ", "starts", "l2d", "tables", "params", "res")}
    D["params"] = HG().PackedDecoders(D["params"])
    return D


def scene_tail(D):
    return D["tables"], D["params"], D["res"], D["occ"], D["starts"], D["l2d"], D["corners"], D["sizes"]


def route(monkeypatch, name):
    arith, fold = ROUTES[name]
    monkeypatch.setattr(HG(), "INFER_ARITH", arith)
    monkeypatch.setattr(HG(), "FOLD_ACTIVATION", fold)


def pad32(a):
    pad = -a.shape[0] % 32
    return np.concatenate([a, np.repeat(a[-1:], pad, 0)]) if pad else a


def to_layout(a, lay):
    """[B,S,...] -> the layout's array (scanerf_hip.h sample_major): 1 = [S,B,...], 2 = [B/32,S,32,...] with B padded to 32"""
    if lay == 0:
        return np.ascontiguousarray(a)
    if lay == 1:
        return np.ascontiguousarray(np.swapaxes(a, 0, 1))
    a = pad32(a)
    return np.ascontiguousarray(np.swapaxes(a.reshape(a.shape[0] // 32, 32, *a.shape[1:]), 1, 2))


def from_layout(a, lay):
    if lay == 0:
        return a
    if lay == 1:
        return np.swapaxes(a, 0, 1)
    return np.swapaxes(a, 1, 2).reshape(a.shape[0] * 32, a.shape[1], *a.shape[3:])[:B]


def outputs(z, fill=NAN):
    return [torch.full(tuple(z.shape) + (k,), fill, device=DEV) for k in (3, 3, 1)]


def rays_of(ins, lay):
    return (g(pad32(ins["o"])), g(pad32(ins["d"]))) if lay == 2 else (g(ins["o"]), g(ins["d"]))


def run_pts(c, ins, lay):
    """pts_inference under the current route, the outputs prefilled with NaN -> (dif [N,3], spec [N,3], alpha [N]) numpy"""
    z, dd, bi = (g(to_layout(ins[k], lay)) for k in ("z", "dd", "bi"))
    out = outputs(z)
    ops().pts_inference(*rays_of(ins, lay), z, dd, bi, *scene_tail(dev_scene(c.scene, c.family)), *out, sample_major=lay)
    return flat(out, lay)


def flat(out, lay):
    dif, spec, alpha = (from_layout(n(t), lay) for t in out)
    return dif.reshape(-1, 3), spec.reshape(-1, 3), alpha.reshape(-1)


def check_samples(name, got, r64, r32, k):
    """judge, then the two things no statistic shows: every sample written, and exact zeros where float64 has them"""
    bad = R.judge_samples(name, got, r64, r32, k)
    assert not any(np.isnan(a).any() for a in got), f"{name}: a sample was left unwritten (or is NaN)"
    zero = (r64["alpha"] == 0).numpy()
    assert zero.any() and not any(a[zero].any() for a in got), f"{name}: a sample whose float64 alpha is 0 is not 0"
    assert not bad, bad


def default_layout(c):
    return 0 if RS.named(c.scene)[0]["corners"].shape[0] > 64 else 2   # above 64 tiles: the single-pass kernel reads [B,S] only


def default_k(c):
    return R.K_F32 if RS.named(c.scene)[0]["corners"].shape[0] > 64 else R.K_SPLIT


# ------------------------------------------------------------------------------------------------------------ per sample
@pytest.mark.parametrize("c", R.PTS_CASES, ids=R.case_id)
def test_pts_inference_per_sample(c):
    """Every case on the default route in the renderer's layout (ray blocks; G65: the single-pass fallback, [B,S])."""
    ins, r64, r32 = R.pts_reference(c)
    assert HG().INFER_ARITH == "t16" and HG().FOLD_ACTIVATION
    check_samples(f"pts_inference {R.case_id(c)} default", run_pts(c, ins, default_layout(c)), r64, r32, default_k(c))


# (the single-pass f32 kernel reads [B,S] arrays only; its refusal of the others: test_gpu_render_many_tiles.py)
CROSS = [(name, lay) for name in ROUTES for lay in (0, 1, 2) if name != "f32" or lay == 0]


@pytest.mark.parametrize("name,lay", CROSS)
def test_pts_inference_every_route_and_layout(name, lay, monkeypatch):
    """The cross case through every arithmetic and layout, each against the same float64 result."""
    c = R.CROSS_CASE
    ins, r64, r32 = R.pts_reference(c)
    route(monkeypatch, name)
    check_samples(f"pts_inference {R.case_id(c)} {name} layout {lay}", run_pts(c, ins, lay), r64, r32, R.K_F32 if name == "f32" else R.K_SPLIT)


@pytest.mark.parametrize("lay", (0, 2))
@pytest.mark.parametrize("name", ("default", "h3"))
def test_pts_inference_chunk_major_kernels(name, lay, monkeypatch):
    """G36: both chunk-major kernels (16- and 32-sample tiles) with a second word of tiles"""
    c = R.Case("G36", 16, "base")
    ins, r64, r32 = R.pts_reference(c)
    assert (ins["bi"] >= 32).any()
    route(monkeypatch, name)
    check_samples(f"pts_inference {R.case_id(c)} {name} layout {lay}", run_pts(c, ins, lay), r64, r32, R.K_SPLIT)


@pytest.mark.parametrize("lay", (0, 2))
@pytest.mark.parametrize("skip", (False, True))
def test_pts_inference_tracing_per_sample(skip, lay):
    """The fused slot lists (nb <= 8: the stack's six tiles) with and without SKIP_UNSAMPLED, every ray running.  With the flag the
    rays whose first depth is -1 may be left unwritten (accumulate_color does not read them under the same flag): there the prefill
    counts as the zeros they stand for."""
    H = ops()
    c = R.TRACING_CASE
    ins, r64, r32 = R.pts_reference(c)
    sc = ins["sc"]
    assert H.tracing_fusable(sc["corners"].shape[0])
    from oracle import oracle as O
    inter = O.ray_block_intersection(ins["o"], ins["d"], sc["corners"], sc["sizes"])
    assert np.array_equal(O.prepare_points(ins["z"], np.ones(B, bool), inter), ins["bi"])
    z, dd = (g(to_layout(ins[k], lay)) for k in ("z", "dd"))
    out = outputs(z)
    run = torch.ones(BP if lay == 2 else B, dtype=torch.bool, device=DEV)
    H.pts_inference_tracing(*rays_of(ins, lay), z, dd, run, g(pad32(inter) if lay == 2 else inter), *scene_tail(dev_scene(c.scene, c.family)),
                            *out, sample_major=lay | (H.SKIP_UNSAMPLED if skip else 0))
    got = flat(out, lay)
    unsampled = np.repeat(ins["z"][:, 0] == -1, c.S)
    assert unsampled.sum() >= 20 * c.S
    if skip:   # what such a ray holds is not read: only NaN (the prefill) may stand for the zeros
        got = tuple(np.where(unsampled.reshape((-1,) + (1,) * (a.ndim - 1)) & np.isnan(a), np.float32(0), a) for a in got)
    check_samples(f"pts_inference_tracing {R.case_id(c)} skip {int(skip)} layout {lay}", got, r64, r32, R.K_SPLIT)


def run_bg(c, ins, lay):
    D = dev_scene(c.scene, c.family)
    z = g(to_layout(ins["z"], lay))
    out = outputs(z)
    ob = g(pad32(ins["ob"]) if lay == 2 else ins["ob"])
    ops().bg_pts_inference_v2(*rays_of(ins, lay), z, ob, c.step, D["corners"], D["sizes"], D["res"], D["tables"], D["params"], *out, sample_major=lay)
    return flat(out, lay)


def check_bg(name, got, r64, r32, k):
    bad = R.judge_samples(name, got, r64, r32, k)
    assert not any(np.isnan(a).any() for a in got), f"{name}: NaN"
    assert not bad, bad


@pytest.mark.parametrize("c", R.BG_CASES, ids=R.case_id)
def test_bg_pts_inference_v2_per_sample(c):
    ins, r64, r32 = R.bg_reference(c)
    check_bg(f"bg_pts_inference_v2 {R.case_id(c)} default", run_bg(c, ins, 0), r64, r32, default_k(c))


@pytest.mark.parametrize("name,lay", [(name, lay) for name, lay in CROSS if name == "f32" or lay])
def test_bg_pts_inference_v2_every_route(name, lay, monkeypatch):
    """G9, 16 samples, step 1 (rays with and without a second exit tile) through every arithmetic and the other layouts"""
    c = R.BgCase("G9", 16, 1, "base")
    ins, r64, r32 = R.bg_reference(c)
    route(monkeypatch, name)
    check_bg(f"bg_pts_inference_v2 {R.case_id(c)} {name} layout {lay}", run_bg(c, ins, lay), r64, r32, R.K_F32 if name == "f32" else R.K_SPLIT)


@pytest.mark.parametrize("c", R.BG_V1_CASES, ids=R.case_id)
def test_bg_pts_inference_v1_per_sample(c):
    ins, r64, r32 = R.bg_reference(c)
    D = dev_scene(c.scene, c.family)
    z = g(ins["z"])
    out = outputs(z, 5.0)
    ops().bg_pts_inference(g(ins["o"]), g(ins["d"]), z, g(ins["ob"]), g(ins["bw"]), D["corners"], D["sizes"], D["res"], D["tables"], D["params"], *out)
    check_bg(f"bg_pts_inference {R.case_id(c)}", flat(out, 0), r64, r32, R.K_SPLIT)


# ------------------------------------------------------------------------------------------------------------ per ray
def run_accumulate(seq, lay, flags=0):
    """accumulate_color over a sequence of passes, the state carried on the GPU -> {"dif", "spec", "depth", "T"} numpy"""
    Bl = BP if lay == 2 else B
    T, dif, spec, depth = (torch.ones(Bl, 1, device=DEV), torch.zeros(Bl, 3, device=DEV), torch.zeros(Bl, 3, device=DEV), torch.zeros(Bl, 1, device=DEV))
    for pd, ps, pa, z in seq:
        ops().accumulate_color(g(to_layout(pd, lay)), g(to_layout(ps, lay)), g(to_layout(pa[..., None], lay)), T, g(to_layout(z, lay)), dif, spec,
                               depth, sample_major=lay | flags)
    return {"dif": n(dif)[:B], "spec": n(spec)[:B], "depth": n(depth)[:B, 0], "T": n(T)[:B, 0]}


@pytest.mark.parametrize("lay", (0, 1, 2))
@pytest.mark.parametrize("c", R.RAY_CASES, ids=R.case_id)
def test_accumulate_color_per_ray(c, lay):
    """The op alone, fed the float32 yardstick's per-sample values: the case's tracing passes in sequence (the transmittance carried,
    rays dropping below 1e-5 on the way), then each background step; in the ray-block layout also with SKIP_UNSAMPLED, which must
    not change a bit."""
    H = ops()
    bad = []
    for k, (seq, s64, s32, tied) in enumerate(R.accumulate_reference(c)):
        got = run_accumulate(seq, lay)
        bad += R.judge_rays(f"accumulate_color {R.case_id(c)} sequence {k} layout {lay}", got, s64, s32, R.K_ACC, ~tied)
        if lay == 2 and k == 0:
            again = run_accumulate(seq, lay, H.SKIP_UNSAMPLED)
            assert all(np.array_equal(got[q], again[q]) for q in got), "SKIP_UNSAMPLED changes the result"
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def renderer(name):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import renderer as Rd
    return Rd.TileSetRenderer(DEV, RS.renderer_tiles(RS.named(name)[0]))


@pytest.mark.parametrize("layout", (2, 0))
def test_render_rays_per_ray(layout):
    """TileSetRenderer.render_rays on G9 against the same float64 loop, over the renderer's own scene arrays: colour, depth and
    transmittance per ray.  The whole chain runs the default arithmetic, so its bound is the split-f16 kernels'."""
    c = R.RENDER_CASE
    rnd = renderer(c.scene)
    o, d = RS.named(c.scene)[1]["shuffled"]
    sc = RNR.renderer_arrays(rnd)
    mine = R.ray_reference(c)[0]
    same = all(np.array_equal(sc[k], mine[k]) for k in ("corners", "sizes", "tables", "params", "res", "occ", "fake"))
    print(f"the renderer's scene arrays are the CPU test's: {same}")
    loop = R.ray_reference(c)[3] if same else R.render_loop(sc, o, d, c.S, c.SB)
    assert loop["tied"].mean() <= R.TIE_CAP
    dif, spec, depth, T = (n(t) for t in rnd.render_rays(g(o), g(d), num_sample=c.S, num_bg_sample=c.SB, layout=layout))
    got = {"dif": dif, "spec": spec, "depth": depth.reshape(B), "T": T.reshape(B)}
    bad = R.judge_rays(f"render_rays {R.case_id(c)} layout {layout}", got, loop["f64"], loop["f32"], R.K_SPLIT, ~loop["tied"])
    assert not bad, bad
