"""The hit record of the tracer and the rendered mesh on the GPU (csrc/mesh_render.hip) against tests/mesh_render_reference.py.

trace: t has first_hit's bits on every ray, at log2dim 4, 6, 7 and in both triangle forms; (t, u, v) are the float32 restatement's on the
returned face, bit for bit; the grid route equals the brute-force route and the float64 face on every ray that is not grazing, and t
keeps test_gpu_fastmesh's bound |t - t64| <= 1e-4 max(t64, 1e-3) there.  render_views: the fused launch equals the composed route
(compute_ray_forward, trace, one torch op per operation) in every bit, at every image size that leaves partial 8 x 8 blocks, and the
float32 restatement over all faces on the pixels that are not grazing.  Guard regions, refusals, the stream, and the public routes
(evaluation.render_mesh, TileSetRenderer.score_mesh, fuse_mesh(score=True), the two commands)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_render_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
_i32, _f32 = torch.int32, torch.float32
GUARD, SENTINEL = 96, -7.0


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _gpu(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ---- the terrain fixture, its float64 answers (computed once, never written to) and its tracers ------------------------------------------
@functools.lru_cache(maxsize=None)
def terrain():
    V, F, sets = R.terrain_fixture()
    rng = np.random.default_rng(24)
    normals = rng.normal(size=V.shape).astype(f32)                      # any vectors: the interpolation does not need unit normals
    colors = rng.uniform(0, 1, V.shape).astype(f32)
    return V, F, sets, normals, colors


@functools.lru_cache(maxsize=None)
def terrain_answers(name):
    """float64 (t, face) over all faces and the grazing flag of one ray set."""
    V, F, sets, _, _ = terrain()
    o, d = sets[name]
    t64, face64, _, _ = R.nearest(o, d, V, F, f64)
    return t64, face64, R.grazing_rays(o, d, V, F)


@functools.lru_cache(maxsize=None)
def tracer(log2dim=6, pregather=True):
    import scanerf_amd  # noqa: F401
    from scanerf_amd.fastmesh import FastMesh
    V, F, _, _, _ = terrain()
    fm = FastMesh.from_arrays(V, F, DEV, log2dim=log2dim, pregather=pregather)
    assert (fm.tris is not None) == pregather
    return fm


@functools.lru_cache(maxsize=None)
def traced(name, log2dim=6, pregather=True, route="grid"):
    _, _, sets, _, _ = terrain()
    o, d = sets[name]
    t, face, bary = tracer(log2dim, pregather).trace(_gpu(o), _gpu(d), route=route)
    assert t.dtype == _f32 and face.dtype == _i32 and bary.dtype == _f32 and bary.shape == (len(o), 2)
    return _np(t), _np(face), _np(bary)


SETS = ["inside", "outside", "axial"]


@pytest.mark.parametrize("name", SETS)
def test_trace_t_has_first_hits_bits_and_the_record_is_the_restatement_on_the_returned_face(name):
    V, F, sets, _, _ = terrain()
    o, d = sets[name]
    t0, face0, bary0 = traced(name)
    for log2dim in (4, 6, 7):
        for pregather in (True, False):
            fm = tracer(log2dim, pregather)
            first = _np(fm.first_hit(_gpu(o), _gpu(d)))
            t, face, bary = traced(name, log2dim, pregather)
            assert _same(t, first), (name, log2dim, pregather)
            hit = face >= 0
            assert hit.sum() > 100 and (face[hit] < len(F)).all()
            assert not t[~hit].any() and not bary[~hit].any() and (face[~hit] == -1).all() and (t[hit] > 0).all()      # the miss
            rt, ru, rv, rhit = R.on_face(o[hit], d[hit], V, F, face[hit], f32)
            assert rhit.all(), "a returned face is not hit in the float32 restatement"
            assert _same(t[hit], rt.astype(f32)) and _same(bary[hit, 0], ru.astype(f32)) and _same(bary[hit, 1], rv.astype(f32))
            # both triangle forms and every log2dim agree on the whole record wherever the answer is not a tie at a cell's exit
            grazing = terrain_answers(name)[2]
            assert _same(t, t0) and np.array_equal(face[~grazing], face0[~grazing]) and _same(bary[~grazing], bary0[~grazing])


@pytest.mark.parametrize("name", SETS)
def test_trace_grid_equals_brute_and_float64_on_every_ray_that_is_not_grazing(name):
    t64, face64, grazing = terrain_answers(name)
    t, face, bary = traced(name)
    bt, bface, bbary = traced(name, route="brute")
    keep = ~grazing
    print(f"mesh trace {name}: {len(t)} rays, {int(grazing.sum())} grazing, {int((face >= 0).sum())} hits; grid and brute differ on "
          f"{int((face != bface).sum())} rays; max relative |t - t64| {np.max(np.abs(t - t64)[keep] / np.maximum(t64[keep], 1e-3)):.2e}")
    assert grazing.mean() <= 0.01
    assert _same(t[keep], bt[keep]) and np.array_equal(face[keep], bface[keep]) and _same(bary[keep], bbary[keep])
    assert np.all(np.abs(t - t64)[keep] <= 1e-4 * np.maximum(t64[keep], 1e-3))
    assert np.array_equal(face[keep], face64[keep])


def test_trace_of_nothing_and_of_non_finite_rays():
    fm = tracer()
    t, face, bary = fm.trace(torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), device=DEV))
    assert t.shape == (0,) and face.shape == (0,) and bary.shape == (0, 2)
    nan, inf = float("nan"), float("inf")
    o = _gpu([[0, 0, 5], [nan, 0, 5], [0, 0, 5], [0, 0, 5], [0, 0, 500]], _f32)
    d = _gpu([[0, 0, -1], [0, 0, -1], [0, nan, -1], [inf, 0, -1], [0, 0, 1]], _f32)        # the last one misses the grid cube
    for route in ("grid", "brute"):
        t, face, bary = (_np(x) for x in fm.trace(o, d, route=route))
        assert t[0] > 0 and face[0] >= 0
        assert not t[1:].any() and (face[1:] == -1).all() and not bary[1:].any(), route


# ---- render_views -----------------------------------------------------------------------------------------------------------------------
def _render(fm, ks, c2ws, H, W, route="fused", **kw):
    out = fm.render_views(_gpu(ks, _f32), _gpu(c2ws, _f32), H, W, route=route, **kw)
    C = len(ks)
    assert out["depth"].shape == (C, H, W) and out["depth"].dtype == _f32 and out["face"].shape == (C, H, W) and out["face"].dtype == _i32
    for k in ("normal", "color"):
        assert k not in out or (out[k].shape == (C, H, W, 3) and out[k].dtype == _f32)
    return {k: _np(v) for k, v in out.items()}


def _equal(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert _same(a[k], b[k]), (what, k, int((_bits(a[k]) != _bits(b[k])).sum()))


def _attributes():
    _, _, _, normals, colors = terrain()
    return _gpu(normals), _gpu(colors)


CONFIGS = {"plain": {}, "normals": {"normals": True}, "colors": {"colors": True}, "both": {"normals": True, "colors": True},
           "face_normals": {"want_normals": True}, "face_normals_colors": {"want_normals": True, "colors": True}}


def _kw(config):
    vn, vc = _attributes()
    kw = dict(CONFIGS[config])
    if kw.get("normals"):
        kw["normals"] = vn
    if kw.get("colors"):
        kw["colors"] = vc
    return kw


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_fused_equals_composed_in_every_bit_and_the_restatement_where_not_grazing(config):
    V, F, _, normals, colors = terrain()
    ks, c2ws = R.terrain_cameras()
    kw = _kw(config)
    fused = _render(tracer(), ks, c2ws, 24, 32, **kw)
    assert set(fused) == {"depth", "face"} | ({"normal"} if "normals" in kw or "want_normals" in kw else set()) | ({"color"} if "colors" in kw else set())
    _equal(fused, _render(tracer(), ks, c2ws, 24, 32, route="composed", **kw), config)
    _equal(fused, _render(tracer(), ks, c2ws, 24, 32, **kw), config + ": a second run")
    _equal(fused, _render(tracer(7, False), ks, c2ws, 24, 32, **kw), config + ": log2dim 7, indexed triangles")
    hit = fused["face"] >= 0
    assert 0.3 < hit.mean() < 1.0                                       # the views hold hits and misses
    assert not fused["depth"][~hit].any() and all(not fused[k][~hit].any() for k in ("normal", "color") if k in fused)
    ref = R.render(ks, c2ws, 24, 32, V, F, normals=normals if "normals" in kw else None, colors=colors if "colors" in kw else None,
                   face_normals="want_normals" in kw, dtype=f32)
    keep = ~np.stack([R.grazing_rays(*R.pixel_rays(K, M, 24, 32, f32), V, F).reshape(24, 32) for K, M in zip(ks, c2ws)])
    assert keep.mean() >= 0.99
    for k in fused:
        assert _same(fused[k][keep], ref[k][keep].astype(fused[k].dtype)), (config, k)
    if "normal" in fused:
        length = np.linalg.norm(fused["normal"].astype(f64), axis=-1)
        assert np.abs(length[hit] - 1.0).max() <= 1e-5


SIZES = [(1, 1), (1, 65), (8, 8), (9, 7), (3, 63), (3, 64), (3, 65), (17, 1)]


@pytest.mark.parametrize("H,W", SIZES)
def test_image_sizes_with_partial_blocks_on_both_borders(H, W):
    ks, c2ws = R.terrain_cameras(H, W)
    kw = _kw("both")
    fused = _render(tracer(), ks, c2ws, H, W, **kw)
    _equal(fused, _render(tracer(), ks, c2ws, H, W, route="composed", **kw), (H, W))
    _equal({k: v[:1] for k, v in fused.items()}, _render(tracer(), ks[:1], c2ws[:1], H, W, **kw), "C = 1")
    assert (fused["face"] >= 0).any()


def test_no_camera_a_camera_that_looks_away_and_a_camera_inside_the_mesh():
    fm = tracer()
    kw = _kw("both")
    none = fm.render_views(torch.zeros((0, 3, 3)), torch.zeros((0, 3, 4)), 5, 6, **kw)
    assert none["depth"].shape == (0, 5, 6) and none["color"].shape == (0, 5, 6, 3) and none["depth"].device.type == "cuda"
    K = R.look_at((0.0, 0.0, 5.0), (1.0, 0.0, 5.0), 9, 12, 12.0)[1]
    away_c2w = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 5]], f32)             # inside the grid cube, above the terrain, looking straight up
    away = _render(fm, K[None], away_c2w[None], 9, 12, **kw)
    assert (away["face"] == -1).all() and not away["depth"].any() and not away["normal"].any() and not away["color"].any()
    _equal(away, _render(fm, K[None], away_c2w[None], 9, 12, route="composed", **kw), "looking away")
    # inside a closed shell every pixel is a hit, whichever way the camera looks
    import scanerf_amd  # noqa: F401
    from scanerf_amd.fastmesh import FastMesh
    V, F = R.shell_fixture(12.0, 8)
    shell = FastMesh.from_arrays(V, F, DEV)
    cams = [R.look_at((1.3, -2.1, 0.7), t, 20, 28, 17.0) for t in ((9.0, 4.0, 3.0), (-5.0, 1.0, -8.0))]
    ks, c2ws = np.stack([k for _, k in cams]), np.stack([m for m, _ in cams])
    inside = _render(shell, ks, c2ws, 20, 28, want_normals=True)
    assert (inside["face"] >= 0).all() and (inside["depth"] > 0).all()
    _equal(inside, _render(shell, ks, c2ws, 20, 28, want_normals=True, route="composed"), "inside the shell")
    ref = R.render(ks, c2ws, 20, 28, V, F, face_normals=True, dtype=f64)
    keep = ~np.stack([R.grazing_rays(*R.pixel_rays(K, M, 20, 28, f32), V, F).reshape(20, 28) for K, M in zip(ks, c2ws)])
    assert np.array_equal(inside["face"][keep], ref["face"][keep])
    assert np.all(np.abs(inside["depth"] - ref["depth"])[keep] <= 1e-4 * ref["depth"][keep])
    assert np.abs(inside["normal"] - ref["normal"])[keep].max() <= 1e-5


# ---- guard regions, refusals --------------------------------------------------------------------------------------------------------------
def _entry(fm, k9, c12, H, W, vn, vc, depth, face, normal, color, C=None, log2dim=None):
    from scanerf_amd import _capi
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    return _capi.tool("scanerf_mesh_render_views")(
        p(k9), p(c12), k9.shape[0] if C is None else C, H, W, p(fm.vertices), p(fm.faces), p(fm.tris), p(fm.bitmask), p(fm.rank),
        p(fm.start_num), p(fm.cell_faces), p(fm.scene_info), fm.log2dim if log2dim is None else log2dim, p(vn), p(vc), p(depth), p(face),
        p(normal), p(color), _capi.stream())


def _buffers(C, H, W):
    n = C * H * W
    return {"depth": torch.full((GUARD + n + GUARD,), SENTINEL, dtype=_f32, device=DEV),
            "face": torch.full((GUARD + n + GUARD,), int(SENTINEL), dtype=_i32, device=DEV),
            "normal": torch.full((GUARD + 3 * n + GUARD,), SENTINEL, dtype=_f32, device=DEV),
            "color": torch.full((GUARD + 3 * n + GUARD,), SENTINEL, dtype=_f32, device=DEV)}


@pytest.mark.parametrize("pregather", [True, False])
def test_guard_regions_are_untouched_every_element_is_written_and_skipped_outputs_stay(pregather):
    from scanerf_amd.allocation import _cameras
    H, W = 9, 13                                                        # partial blocks on both borders
    ks, c2ws = R.terrain_cameras(H, W)
    k9, c12 = _cameras(ks, c2ws, DEV)
    fm = tracer(6, pregather)
    vn, vc = _attributes()
    want = _render(fm, ks, c2ws, H, W, normals=vn, colors=vc)
    n = 3 * H * W
    for outputs in (("normal", "color"), ("normal",), ("color",), ()):
        buf = _buffers(3, H, W)
        body = {k: buf[k][GUARD:] for k in buf}
        status = _entry(fm, k9, c12, H, W, vn, vc, body["depth"], body["face"], body["normal"] if "normal" in outputs else None,
                        body["color"] if "color" in outputs else None)
        torch.cuda.synchronize()
        assert status == 0
        for k, b in buf.items():
            size = n * (3 if k in ("normal", "color") else 1)
            assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + size:] == SENTINEL).all()), f"a guard region of {k} was written"
            got = _np(b[GUARD:GUARD + size]).reshape(want[k].shape)
            if k in ("depth", "face") or k in outputs:
                assert _same(got, want[k]), (k, outputs)               # no sentinel left: the answer, every element
            else:
                assert (got == SENTINEL).all(), f"the skipped output {k} was written"


def test_refusals_with_device_pointers_write_nothing():
    from scanerf_amd import _capi
    from scanerf_amd.allocation import _cameras
    ks, c2ws = R.terrain_cameras(8, 8)
    k9, c12 = _cameras(ks, c2ws, DEV)
    fm = tracer()
    vn, vc = _attributes()
    buf = _buffers(3, 8, 8)
    a = (buf["depth"], buf["face"], buf["normal"], buf["color"])
    for args, kw, text in (((fm, k9, c12, 0, 8, vn, vc, *a), {}, b"H=0"), ((fm, k9, c12, 8, 8, vn, None, *a), {}, b"needs vertex_colors"),
                           ((fm, k9, c12, 8, 8, vn, vc, *a), {"C": -1}, b"C=-1"), ((fm, k9, c12, 8, 8, vn, vc, *a), {"log2dim": 8}, b"log2dim=8"),
                           ((fm, k9, c12, 8, 8, vn, vc, None, *a[1:]), {}, b"null pointer"),
                           ((fm, k9, c12, 2 ** 15, 2 ** 15, vn, vc, *a), {}, b"does not fit 31 bits")):
        assert _entry(*args, **kw) != 0 and text in _capi.lib().scanerf_last_error(), text
    o = torch.zeros((4, 3), device=DEV)
    t, face, bary = torch.full((4,), SENTINEL, device=DEV), torch.full((4,), -7, dtype=_i32, device=DEV), torch.full((4, 2), SENTINEL, device=DEV)
    p = lambda x: None if x is None else x.data_ptr()
    tail = (p(fm.vertices), p(fm.faces), p(fm.tris), p(fm.bitmask), p(fm.rank), p(fm.start_num), p(fm.cell_faces), p(fm.scene_info))
    assert _capi.tool("scanerf_mesh_trace")(p(o), p(o), 4, *tail, 3, p(t), p(face), p(bary), _capi.stream()) != 0
    assert _capi.tool("scanerf_mesh_trace")(p(o), p(o), 4, *tail[:6], None, tail[7], 6, p(t), p(face), p(bary), _capi.stream()) != 0
    assert _capi.tool("scanerf_mesh_trace_brute")(p(o), p(o), -4, tail[0], tail[1], 4, 2, tail[7], 6, p(t), p(face), p(bary), _capi.stream()) != 0
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in buf.values())
    assert bool((t == SENTINEL).all()) and bool((face == -7).all()) and bool((bary == SENTINEL).all())


# ---- the stream -----------------------------------------------------------------------------------------------------------------------
def _stream_case():
    """The stale-data construction of tests/stream_cases.py for entries its registry cannot claim (the registry follows
    include/scanerf_hip.h): two seeds whose every float input differs, refilled in place."""
    import stream_cases as SC
    V, _, _, _, _ = terrain()

    def build(seed):
        rng = np.random.default_rng(2400 + seed)
        cams = [R.look_at((11.0 * np.cos(a + 0.4 * seed), 11.0 * np.sin(a + 0.4 * seed), 7.0 + seed), (0.5 * seed, 0.0, 0.0), 24, 32, 30.0 + 3.0 * seed)
                for a in np.linspace(0, 2 * np.pi, 6, endpoint=False)]
        o = np.stack([rng.uniform(-9, 9, 1000), rng.uniform(-9, 9, 1000), rng.uniform(2, 6, 1000)], -1).astype(f32)
        d = rng.normal(size=(1000, 3)).astype(f32) - f32([0, 0, 1.5])
        return {"ks": torch.from_numpy(np.stack([K for _, K in cams])), "c2ws": torch.from_numpy(np.stack([c for c, _ in cams])),
                "normals": torch.from_numpy(rng.normal(size=V.shape).astype(f32)), "colors": torch.from_numpy(rng.uniform(0, 1, V.shape).astype(f32)),
                "o": torch.from_numpy(o), "d": torch.from_numpy(d)}

    def setup(state):
        state["fm"] = tracer()

    def run_(state):
        i = state["in"]
        out = state["fm"].render_views(i["ks"], i["c2ws"], 24, 32, normals=i["normals"], colors=i["colors"])
        return (out["depth"], out["face"], out["normal"], out["color"], *state["fm"].trace(i["o"], i["d"]),
                *state["fm"].trace(i["o"][:64], i["d"][:64], route="brute"))

    return SC.Case("mesh_render", list(NAMES), build, run_, setup=setup)


NAMES = ("scanerf_mesh_render_views", "scanerf_mesh_trace", "scanerf_mesh_trace_brute")


def test_stream_the_ops_run_on_the_callers_stream(monkeypatch):
    import stream_cases as SC
    from scanerf_amd import _capi
    from test_gpu_stream_contract import Delay, same_bits
    c = _stream_case()
    X, Y = c.build(1), c.build(2)
    assert list(X) == list(Y) and all(not torch.equal(X[k], Y[k]) and X[k].shape == Y[k].shape for k in X)
    state = c.to_device(X)
    Xd, Yd = SC.stage(X), SC.stage(Y)
    handles = []
    for name in NAMES:
        real = _capi.tool(name)

        def recorded(*a, _real=real):
            handles.append(int(a[-1] or 0))
            return _real(*a)
        monkeypatch.setitem(_capi._tools, name, recorded)
    torch.cuda.synchronize()
    R_X = c.run(state)
    c.refill(state, Yd)
    R_Y = c.run(state)               # leaves every output and input with Y's values
    torch.cuda.synchronize()
    assert not same_bits(R_X, R_Y), "the two seeds give the same answer: a stale read would not show"
    assert all(not same_bits(R_X[k:k + 1], R_Y[k:k + 1]) for k in (0, 2, 3, 4, 7))      # every entry's own outputs differ
    assert handles == [torch.cuda.current_stream().cuda_stream] * 6
    delay = Delay()
    s = torch.cuda.Stream()
    del handles[:]
    with torch.cuda.stream(s):
        pending = delay(20.0)
        c.refill(state, Xd)           # queued behind the delay: a launch on any other stream reads Y
        R_ = c.run(state)
        still = not pending.query()
    s.synchronize()
    torch.cuda.synchronize()
    assert handles == [s.cuda_stream] * 3 and s.cuda_stream != 0, "a call did not carry the caller's stream"
    assert still, "a call waited for its stream (the delay ran out before it returned)"
    assert same_bits(R_, R_X), "under a side stream an op read stale inputs: a launch went to another stream"


# ---- the public routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vpb", [1, 2, 3])
def test_render_mesh_equals_render_views_per_batch(vpb):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation, meshing
    V, F, _, normals, colors = terrain()
    ks, c2ws = R.terrain_cameras()
    vn, vc = _attributes()
    whole = tracer().render_views(_gpu(ks), _gpu(c2ws), 24, 32, normals=vn, colors=vc)
    mesh = meshing.Mesh(_gpu(V), _gpu(F), None, None, vn)
    firsts = []
    for first, batch in evaluation.render_mesh(mesh, (ks, c2ws, 24, 32), colors=colors, views_per_batch=vpb):
        firsts.append(first)
        assert set(batch) == set(whole)
        for k in batch:
            assert batch[k].shape[0] == min(vpb, 3 - first) and torch.equal(batch[k], whole[k][first:first + vpb]), (k, first)
    assert firsts == list(range(0, 3, vpb))
    got = evaluation.render_mesh((V, F), (ks, c2ws, 24, 32), colors=colors, normals=normals, views_per_batch=vpb, collect=True)
    assert all(torch.equal(got[k], whole[k]) for k in whole)
    faces_only = evaluation.render_mesh((V, F), (ks, c2ws, 24, 32), views_per_batch=vpb, collect=True)     # no vertex normals: the faces'
    assert torch.equal(faces_only["normal"], tracer().render_views(_gpu(ks), _gpu(c2ws), 24, 32, want_normals=True)["normal"])
    assert set(evaluation.render_mesh((V, F), (ks, c2ws, 24, 32), normals=False, collect=True)) == {"depth", "face"}


from test_gpu_tsdf import tile_scene  # noqa: E402,F401


def test_score_mesh_and_fuse_mesh_with_score_agree_and_the_mesh_does_not_move(tile_scene):  # noqa: F811
    from scanerf_amd import evaluation
    from test_gpu_mesh_components import _same as same_mesh
    rnd, cams = tile_scene["rnd"], tile_scene["cameras"]
    kw = dict(cells_per_axis=20, max_transparency=0.9, scale=2, views_per_batch=2)
    report, plain_report = {}, {}
    mesh, rgb = rnd.fuse_mesh(cams, report=report, colors="diffuse", score=True, **kw)
    plain, plain_rgb = rnd.fuse_mesh(cams, report=plain_report, colors="diffuse", **kw)
    same_mesh(mesh, plain, "fuse_mesh with score=True against the call without")
    assert torch.equal(rgb.view(_i32), plain_rgb.view(_i32)) and "render_score" not in plain_report
    assert {k: v for k, v in report.items() if k != "render_score"} == plain_report
    score = report["render_score"]
    assert score["n_views"] == 5 and len(score["per_view"]) == 5 and "psnr" in score["pooled"] and "normal_deg_mean" not in score["pooled"]
    again = rnd.score_mesh(mesh, cams, colors=rgb, which="diffuse", scale=2, max_transparency=0.9, views_per_batch=2)
    assert evaluation.render_score_line(again) == evaluation.render_score_line(score)
    print("render score, tile fixture (5 cameras, 24 x 32):", json.dumps(score["pooled"]))
    assert 0.0 < score["pooled"]["coverage"] <= 1.0 and np.isfinite(score["pooled"]["psnr"])
    geometry = rnd.score_mesh((mesh.vertices, mesh.faces), cams, scale=2, max_transparency=0.9, views_per_batch=5)      # no colours
    assert "psnr" not in geometry["pooled"] and geometry["pooled"]["coverage"] == score["pooled"]["coverage"]
    assert geometry["pooled"]["depth_abs_mean"] == pytest.approx(score["pooled"]["depth_abs_mean"], rel=1e-12)
    with_normals = rnd.score_mesh(mesh, cams, scale=2, max_transparency=0.9, views_per_batch=2, normals=True)
    assert np.isfinite(with_normals["pooled"]["normal_deg_mean"])
    print("render score, tile fixture, face normals against the field's:", with_normals["pooled"]["normal_deg_mean"], "degrees")


VIEWS = (0, 17, 39)       # the views whose reference images are computed in numpy (all faces, every pixel): the rest of the 40 would take minutes


def test_end_to_end_on_a_traced_icosphere_with_radial_colours():
    import tsdf_color_reference as CR
    import tsdf_reference as TR
    from scanerf_amd import evaluation, fusion
    from scanerf_amd.fastmesh import FastMesh
    from test_gpu_tsdf import _icosphere, _trace_depth
    c = TR.case("sphere40")
    V, F = _icosphere(TR.RADIUS, 3)
    H, W = c["depths"].shape[1:]
    depths = _trace_depth(FastMesh.from_arrays(V, F, DEV), c["ks"], c["c2ws"], H, W)
    colors = torch.from_numpy(CR.radial_colors(c["ks"], c["c2ws"], _np(depths))).to(DEV)
    mesh, rgb = fusion.fuse_depth_maps(depths, c["ks"], c["c2ws"], c["origin"], [TR.BOX[1]] * 3, c["n"], trunc=TR.TRUNC, views_per_batch=7,
                                       near=TR.NEAR, far=TR.FAR, colors=colors)
    cams = (c["ks"], c["c2ws"], H, W)
    target = {"depth": depths, "color": colors}
    pred = evaluation.render_mesh(mesh, cams, colors=rgb, normals=False, views_per_batch=16, collect=True)
    score = evaluation.compare_renders(pred, target)
    acc = evaluation.RenderScore()
    for first, batch in evaluation.render_mesh(mesh, cams, colors=rgb, normals=False, views_per_batch=16):
        acc.add(batch, {k: v[first:first + 16] for k, v in target.items()})
    assert evaluation.render_score_line(acc.result()) == evaluation.render_score_line(score)
    spacing = TR.BOX[1] / min(c["n"])                                                # the largest lattice spacing
    print(f"render score, fused icosphere (40 cameras, {H} x {W}, {mesh.faces.shape[0]} faces):", json.dumps(score["pooled"]),
          f"depth_abs_mean in spacings: {score['pooled']['depth_abs_mean'] / spacing:.4f}")
    # the same dict from the numpy reference's images, on the pixels where neither side is grazing (the others count as uncovered)
    mv, mf, mc = _np(mesh.vertices), _np(mesh.faces), _np(rgb)
    ks, c2ws = np.asarray(c["ks"])[list(VIEWS)], np.asarray(c["c2ws"])[list(VIEWS)]
    ref = R.render(ks, c2ws, H, W, mv, mf, colors=mc, dtype=f32)
    grazing = np.stack([R.grazing_rays(*R.pixel_rays(K, M, H, W, f32), mv, mf).reshape(H, W) for K, M in zip(ks, c2ws)])
    assert grazing.mean() <= 0.01
    keep = torch.from_numpy(~grazing).to(DEV)
    idx = torch.tensor(VIEWS, device=DEV)
    sub = lambda maps: {"depth": maps["depth"][idx] * keep, "color": maps["color"][idx]}
    got = evaluation.compare_renders(sub(pred), sub(target))
    want = evaluation.compare_renders({"depth": _gpu(ref["depth"]) * keep, "color": _gpu(ref["color"])}, sub(target))
    assert evaluation.render_score_line(got) == evaluation.render_score_line(want)
    assert got["pooled"]["coverage"] > 0.5 and np.isfinite(got["pooled"]["psnr"])


def test_the_commands_outputs_read_back_as_the_librarys_arrays(tile_scene, tmp_path, capsys):  # noqa: F811
    from scanerf_amd import evaluation, formats, fusion
    from test_gpu_mesh_components import _tool
    V, F, _, normals, colors = terrain()
    ks, c2ws = R.terrain_cameras(48, 64)
    log, ply, out = str(tmp_path / "camera.log"), str(tmp_path / "terrain.ply"), str(tmp_path / "views")
    formats.write_campara(log, ks, c2ws, 48, 64)
    unit = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(f32)
    formats.write_ply(ply, V, F, normals=unit, colors=colors)
    assert _tool("render_mesh").main([ply, "--cameras", log, "--out", out, "--scale", "2", "--views-per-batch", "2"]) == 0
    assert "3 views of 24 x 32" in capsys.readouterr().out
    rv, rf, rn, rc = formats.read_ply(ply, normals=True, colors=True)
    cams = formats.read_campara(log, return_shape=True)
    want = evaluation.render_mesh((rv, rf), (fusion.scale_cameras(cams[0], 2), cams[1], 24, 32), normals=torch.from_numpy(rn),
                                  colors=torch.from_numpy(rc.astype(f32) / f32(255.0)), collect=True)
    assert sorted(os.listdir(out)) == [f"view_{i:05d}.npz" for i in range(3)]
    for i in range(3):
        got = np.load(os.path.join(out, f"view_{i:05d}.npz"))
        assert set(got.files) == {"depth", "face", "normal", "color"}
        assert all(_same(got[k], _np(want[k][i])) for k in got.files), i
    plain = str(tmp_path / "plain.ply")
    formats.write_ply(plain, V, F)
    assert _tool("render_mesh").main([plain, "--cameras", log, "--out", str(tmp_path / "plain")]) == 0
    got = np.load(str(tmp_path / "plain" / "view_00001.npz"))
    assert set(got.files) == {"depth", "face", "normal"} and got["depth"].shape == (48, 64)      # no nx / ny / nz: the face normals
    capsys.readouterr()
    # fuse_mesh --render-score prints the library's dict as one JSON line
    fused = str(tmp_path / "fused.ply")
    assert _tool("fuse_mesh").main([tile_scene["path"], "--cameras", tile_scene["log"], "--out", fused, "--cells-per-axis", "20", "--scale", "2",
                                    "--max-transparency", "0.9", "--views-per-batch", "2", "--colors", "diffuse", "--render-score"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    report = {}
    tile_scene["rnd"].fuse_mesh(tile_scene["cameras"], cells_per_axis=20, max_transparency=0.9, scale=2, views_per_batch=2, colors="diffuse",
                                report=report, score=True)
    assert lines == [evaluation.render_score_line(report["render_score"])]
    assert json.loads(lines[0])["n_views"] == 5
