"""Point visibility on the GPU (csrc/mesh_visibility.hip; FastMesh.point_views, meshing.vertex_views / cull_unseen and the extractors'
cameras / min_views).  The outputs are integers: the fused route equals the float64 reference
(tests/mesh_visibility_reference.py) on every pair the reference does not flag as ambiguous, equals the composed route bit for bit,
and gives the same bits at every log2dim, for both triangle forms, on a second launch, with and without the mask, under a side stream."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_visibility_reference as MV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {"terrain": MV.terrain, "nested": MV.nested, "nested_extra": lambda: MV.nested(True), "edges": MV.edges,
         "many_cameras": MV.many_cameras}
_i32 = torch.int32


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _gpu(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def tracer(name, log2dim=6, pregather=True):
    import scanerf_amd  # noqa: F401
    from scanerf_amd.fastmesh import FastMesh
    case = CASES[name]()
    return FastMesh.from_arrays(case["V"], case["F"], DEV, log2dim=log2dim, pregather=pregather)


def run(name, route="fused", want_mask=True, log2dim=6, pregather=True, case=None):
    """-> (views [N] int32, mask [N, words] uint32 or None) as numpy."""
    case = case or CASES[name]()
    views, mask = tracer(name, log2dim, pregather).point_views(_gpu(case["points"]), _gpu(case["ks"]), _gpu(case["c2ws"]), case["H"], case["W"],
                                                               case["bias"], near=case["near"], far=case["far"], want_mask=want_mask, route=route)
    assert views.dtype == _i32 and views.shape == (len(case["points"]),)
    if want_mask:
        assert mask.dtype == _i32 and mask.shape == (len(case["points"]), (len(case["ks"]) + 31) // 32)
    else:
        assert mask is None
    return _np(views), (_np(mask).view(np.uint32) if want_mask else None)


@functools.lru_cache(maxsize=None)
def fused(name):
    """The fused answer of a case, computed once and never written to."""
    return run(name)


def _against_reference(case, views, mask, what):
    ref, C = case["ref"], len(case["ks"])
    got = MV.unpack_mask(mask, C)
    wrong = (got != ref["seen"]) & ~ref["ambiguous"]
    print(f"mesh_visibility {what}: {got.size} pairs, {int(ref['inview'].sum())} in view, {int(ref['ambiguous'].sum())} ambiguous, "
          f"{int((got != ref['seen']).sum())} differ from float64 (all of them ambiguous: {not wrong.any()})")
    assert not wrong.any(), (what, np.argwhere(wrong)[:10])
    assert np.array_equal(views, got.sum(1)), what                                     # views is the popcount of the words
    assert (ref["lo"] <= views).all() and (views <= ref["hi"]).all(), what
    if C % 32:
        assert not (mask[:, -1] >> np.uint32(C % 32)).any(), "unused high bits are set"


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_against_the_float64_reference(name):
    case = CASES[name]()
    views, mask = fused(name)
    _against_reference(case, views, mask, name)
    if name == "edges":
        assert np.array_equal(MV.unpack_mask(mask, 2), case["expected"])               # the answers worked out by hand
        assert views[~np.isfinite(case["points"]).all(1)].tolist() == [0, 0, 0]
    if name.startswith("nested"):
        assert (views[case["n_outer"]:] == (0 if name == "nested" else MV.unpack_mask(mask, 9)[case["n_outer"]:, 8])).all()
        assert (views[:case["n_outer"]] >= 1).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_equals_the_composed_route(name):
    """Per camera the same operands as separate torch elementwise ops, first_hit on the pairs in view, 0 < h < 1: the same bits."""
    case = CASES[name]()
    views, mask = fused(name)
    cviews, cmask = run(name, route="composed")
    differ = MV.unpack_mask(mask, len(case["ks"])) != MV.unpack_mask(cmask, len(case["ks"]))
    print(f"mesh_visibility {name}: fused and composed differ in {int(differ.sum())} pairs {np.argwhere(differ)[:10].tolist()}")
    assert not (differ & ~case["ref"]["ambiguous"]).any()
    assert np.array_equal(mask, cmask) and np.array_equal(views, cviews)


def test_equal_bits_at_every_log2dim_both_triangle_forms_two_launches_with_and_without_the_mask():
    for name in ("terrain", "edges"):
        views, mask = fused(name)
        for log2dim in (4, 5, 6, 7):
            for pregather in (True, False):
                assert (tracer(name, log2dim, pregather).tris is not None) == pregather
                v, m = run(name, log2dim=log2dim, pregather=pregather)
                assert np.array_equal(v, views) and np.array_equal(m, mask), (name, log2dim, pregather)
        v, m = run(name)
        assert np.array_equal(v, views) and np.array_equal(m, mask), name
        v, m = run(name, want_mask=False)
        assert np.array_equal(v, views) and m is None


def _entry(fm, pts, k9, c12, H, W, bias, near, far, views_ptr, mask_ptr):
    from scanerf_amd import _capi
    p = lambda t: None if t is None else t.data_ptr()
    return _capi.tool("scanerf_mesh_point_views")(
        p(pts), pts.shape[0], p(k9), p(c12), k9.shape[0], H, W, bias, near, far, p(fm.vertices), p(fm.faces), p(fm.tris), p(fm.bitmask),
        p(fm.rank), p(fm.start_num), p(fm.cell_faces), p(fm.scene_info), fm.log2dim, views_ptr, mask_ptr, _capi.stream())


GUARD, SENTINEL = 96, -7


def _guarded(name, case, pregather=True, want_mask=True):
    """The entry itself on sentinel-filled buffers with guard regions -> (views, mask) bodies as numpy; asserts the guards."""
    from scanerf_amd.allocation import _cameras
    fm = tracer(name, 6, pregather)
    pts = _gpu(case["points"])
    k9, c12 = _cameras(case["ks"], case["c2ws"], DEV)
    N, nw = pts.shape[0], (k9.shape[0] + 31) // 32
    vbuf = torch.full((GUARD + N + GUARD,), SENTINEL, dtype=_i32, device=DEV)
    mbuf = torch.full((GUARD + N * nw + GUARD,), SENTINEL, dtype=_i32, device=DEV)
    status = _entry(fm, pts, k9, c12, case["H"], case["W"], case["bias"], case["near"], case["far"], vbuf[GUARD:].data_ptr(),
                    mbuf[GUARD:].data_ptr() if want_mask else None)
    torch.cuda.synchronize()
    assert status == 0
    for buf, n in ((vbuf, N), (mbuf, N * nw if want_mask else 0)):
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "a guard region was written"
    return _np(vbuf[GUARD:GUARD + N]), _np(mbuf[GUARD:GUARD + N * nw]).reshape(N, nw).view(np.uint32)


def test_guard_regions_are_untouched_and_every_element_is_written():
    for name in ("terrain", "many_cameras"):
        case = CASES[name]()
        views, mask = fused(name)
        for pregather in (True, False):
            v, m = _guarded(name, case, pregather)
            assert np.array_equal(v, views) and np.array_equal(m, mask), name          # no sentinel left: the fused answer, every row
        v, m = _guarded(name, case, want_mask=False)
        assert np.array_equal(v, views) and (m.view(np.int32) == SENTINEL).all()       # mask == NULL: not written


@pytest.mark.parametrize("c", MV.SIZES_C)
@pytest.mark.parametrize("n", MV.SIZES_N)
def test_sizes(n, c):
    case = MV.sizes(n, c)
    v, m = _guarded("terrain", case)
    assert v.shape == (n,) and m.shape == (n, c)      # (c is 0 or 1: as many words)
    if c == 0:
        assert not v.any()
    else:
        _against_reference(case, v, m, f"N={n} C={c}")
        full_v, full_m = fused("terrain")
        assert np.array_equal(m[:, 0], full_m[:n, 0] & np.uint32(1))
    views, mask = tracer("terrain").point_views(_gpu(case["points"]).reshape(-1, 3), _gpu(case["ks"]).reshape(-1, 3, 3),
                                                _gpu(case["c2ws"]).reshape(-1, 3, 4), case["H"], case["W"], case["bias"], want_mask=True)
    assert np.array_equal(_np(views), v) and np.array_equal(_np(mask).view(np.uint32), m)


def test_refusals_with_device_pointers_write_nothing():
    case = MV.edges()
    from scanerf_amd import _capi
    from scanerf_amd.allocation import _cameras
    fm, pts = tracer("edges"), _gpu(case["points"])
    k9, c12 = _cameras(case["ks"], case["c2ws"], DEV)
    views = torch.full((pts.shape[0],), SENTINEL, dtype=_i32, device=DEV)
    mask = torch.full((pts.shape[0], 1), SENTINEL, dtype=_i32, device=DEV)
    for kw, text in ((dict(H=0), b"H=0"), (dict(bias=0.0), b"bias=0"), (dict(near=-1.0), b"near=-1"), (dict(far=0.0), b"far=0")):
        a = dict(H=case["H"], W=case["W"], bias=case["bias"], near=case["near"], far=case["far"])
        a.update(kw)
        assert _entry(fm, pts, k9, c12, a["H"], a["W"], a["bias"], a["near"], a["far"], views.data_ptr(), mask.data_ptr()) != 0
        assert text in _capi.lib().scanerf_last_error()
    torch.cuda.synchronize()
    assert bool((views == SENTINEL).all()) and bool((mask == SENTINEL).all())


# ---- the cull -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nested", "terrain"])
def test_cull_unseen_is_the_numpy_cull_of_the_fused_views(name):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import meshing
    case = CASES[name]()
    V, F = case["V"], case["F"]
    extra = np.arange(3 * len(V), dtype=np.float32).reshape(-1, 3)
    mesh = meshing.Mesh(_gpu(V), _gpu(F), _gpu(extra.astype(np.int32)), _gpu(extra + 0.5), _gpu(-extra))
    views, _ = fused(name)
    cam = (_gpu(case["ks"]), _gpu(case["c2ws"]), case["H"], case["W"])
    vv, _ = meshing.vertex_views(mesh, *cam, case["bias"])
    assert np.array_equal(_np(vv), views)
    for min_views in (1, 2):
        report = {}
        got = meshing.cull_unseen(mesh, *cam, min_views=min_views, bias=case["bias"], report=report)
        wv, wf, (wc, wl, wn) = MV.cull(V, F, views, min_views, (extra.astype(np.int32), extra + 0.5, -extra))
        for a, b in ((got.vertices, wv), (got.faces, wf), (got.cells, wc), (got.lattice, wl), (got.normals, wn)):
            assert _np(a).dtype == b.dtype and np.array_equal(_np(a), b)
        assert report["vertices"] == (len(V), len(wv)) and report["faces"] == (len(F), len(wf))
        assert report["views_histogram"] == np.bincount(views).tolist()
    assert meshing.cull_unseen(mesh, *cam, min_views=0, bias=case["bias"]) is mesh
    if name == "nested":
        got = meshing.cull_unseen(mesh, *cam, min_views=1, bias=case["bias"])
        # exactly the inner cube goes: its 8 vertices and 12 faces are the last rows
        assert np.array_equal(_np(got.vertices), V[:case["n_outer"]]) and np.array_equal(_np(got.faces), F[:case["f_outer"]])
        composed = meshing.cull_unseen(mesh, *cam, min_views=1, bias=case["bias"], route="composed")
        assert torch.equal(composed.faces, got.faces) and torch.equal(composed.vertices, got.vertices)


# ---- the extractors and the commands -------------------------------------------------------------------------------------------------
def _ring(center, radius, n, H, W, focal, phase=0.3, height=0.35, arc=2 * np.pi):
    import fastmesh_reference as FR
    ks, c2ws = [], []
    for k in range(n):
        a = phase + arc * k / n
        eye = np.asarray(center) + radius * np.array([np.cos(a), np.sin(a), height + 0.05 * k])
        c2w, K = FR.look_at(eye, center, H, W, focal)
        ks.append(K)
        c2ws.append(c2w)
    return np.stack(ks), np.stack(c2ws)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The G9 scene of the scene-mesh tests written as tiles, its renderer, a level, and two cameras on ONE side of it."""
    import render_scenes as RS
    from scanerf_amd import formats, renderer
    from test_gpu_mesh_components import _scene_args
    M, _ = _scene_args()
    root = tmp_path_factory.mktemp("visibility_scene")
    dirs = []
    for b, tile in enumerate(RS.renderer_tiles(M.scene("G9"))):
        path = str(root / f"tile-{b}")
        os.makedirs(path)
        t = torch.as_tensor
        renderer.write_feature_npz(path, t(tile["features"]), t(tile["occupied_grid"]), t(tile["block_corner"]), t(tile["block_size"]),
                                   t(tile["grid_log2dim"]), t(tile["resolution"]))
        torch.save(dict(M.O.unpack_blob(torch.from_numpy(tile["blob"]))), os.path.join(path, "decoder.pth"))
        dirs.append(path)
    rnd = renderer.TileSetRenderer(DEV, [renderer.load_tile(p) for p in dirs])
    corner, size = (np.asarray([float(v) for v in x]) for x in rnd.scene_box())
    H, W = 96, 128
    ks, c2ws = _ring(corner + size / 2, 1.6 * float(size.max()), 2, H, W, 90.0, arc=0.8)
    log = str(root / "camera.log")
    formats.write_campara(log, ks, c2ws, H, W)
    return dict(dirs=dirs, rnd=rnd, level=M.reference(M.CASES[0])[6], log=log, cameras=formats.read_campara(log, return_shape=True), root=root)


def test_extract_mesh_culls_then_filters_then_evaluates_normals(scene):
    from scanerf_amd import meshing, renderer
    from test_gpu_mesh_components import _same, _tool
    tool = _tool("extract_mesh")
    tile = renderer.load_tile(scene["dirs"][0])
    cams = scene["cameras"]
    n, level = 24, scene["level"]
    plain = tool.extract_tile(tile, n, level, DEV, normals=True)
    assert plain.vertices.shape[0] > 0
    _same(tool.extract_tile(tile, n, level, DEV, normals=True, cameras=cams), plain, "cameras alone change nothing")
    _same(tool.extract_tile(tile, n, level, DEV, normals=True, cameras=cams, min_views=0, view_bias=0.3), plain, "min_views=0")
    # by hand, in the documented order: views on the raw mesh, the cull, the component rule; the normals are those of the kept rows
    corner, size = renderer.render_box(np.asarray(tile["block_corner"], np.float32), np.asarray(tile["block_size"], np.float32))
    bias = meshing.default_view_bias(size.tolist(), meshing.cells_per_axis(size.tolist(), n))
    culled = meshing.cull_unseen(plain, *cams, min_views=1, bias=bias)
    print(f"mesh_visibility extract: {plain.vertices.shape[0]} -> {culled.vertices.shape[0]} vertices, {plain.faces.shape[0]} -> "
          f"{culled.faces.shape[0]} faces by the cull")
    assert 0 < culled.faces.shape[0] < plain.faces.shape[0], "the two cameras on one side must see part of the tile's surface, not all"
    want = meshing.filter_mesh(culled, min_faces=4)
    report = {}
    got = tool.extract_tile(tile, n, level, DEV, normals=True, cameras=cams, min_views=1, min_faces=4, report=report)
    _same(got, want, "cull -> component rule -> normals")
    assert report["cull"]["vertices"] == (plain.vertices.shape[0], culled.vertices.shape[0])
    assert report["vertices"] == (culled.vertices.shape[0], want.vertices.shape[0])     # the component rule saw the culled mesh
    # the other order is another mesh whenever the cull fragments something: not asserted, but the pieces are
    dense = tool.extract_tile(tile, n, level, DEV, route="dense", cameras=cams, min_views=1, min_faces=4)
    assert torch.equal(dense.faces, got.faces) and torch.equal(dense.vertices, got.vertices)


def test_the_commands_with_cameras(scene, capsys):
    from scanerf_amd import formats
    from test_gpu_mesh_components import _tool
    rnd, level, root = scene["rnd"], scene["level"], scene["root"]
    out = str(root / "scene.ply")
    assert _tool("extract_scene_mesh").main([*scene["dirs"], "--level", repr(level), "--cells-per-axis", "20", "--out", out, "--cameras",
                                             scene["log"], "--min-views", "1", "--min-faces", "2", "--normals"]) == 0
    plain = rnd.extract_mesh(level, cells_per_axis=20)
    want = rnd.extract_mesh(level, cells_per_axis=20, cameras=scene["cameras"], min_views=1, min_faces=2, normals=True)
    assert 0 < want.faces.shape[0] < plain.faces.shape[0]
    ply = formats.read_ply(out)
    assert np.array_equal(np.asarray(ply[0], np.float32), _np(want.vertices)) and np.array_equal(np.asarray(ply[1], np.int32), _np(want.faces))
    printed = capsys.readouterr().out
    assert "unseen parts culled first" in printed and f"vertices {plain.vertices.shape[0]} -> " in printed
    tool = _tool("extract_mesh")
    assert tool.main([scene["dirs"][0], "--level", repr(level), "--cells-per-axis", "24", "--out", str(root / "out"), "--cameras", scene["log"],
                      "--min-views", "1", "--view-far", "1000"]) == 0
    from scanerf_amd import renderer
    want = tool.extract_tile(renderer.load_tile(scene["dirs"][0]), 24, level, DEV, cameras=scene["cameras"], min_views=1, view_far=1000.0)
    tv, tf = formats.read_ply(str(root / "out" / "tile-0.ply"))[:2]
    assert np.array_equal(np.asarray(tv, np.float32), _np(want.vertices)) and np.array_equal(np.asarray(tf, np.int32), _np(want.faces))
    assert "unseen parts culled first" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        tool.main([scene["dirs"][0], "--level", repr(level), "--min-views", "1"])      # --min-views needs --cameras


# ---- the stream -----------------------------------------------------------------------------------------------------------------------
def _stream_case():
    """The stale-data construction of tests/stream_cases.py for the entry its registry cannot claim (the registry follows
    include/scanerf_hip.h): two seeds whose every float input differs, refilled in place."""
    import fastmesh_reference as FR
    import stream_cases as SC
    import tile_allocation_reference as TA

    def build(seed):
        rng = np.random.default_rng(4100 + seed)
        pts = np.stack([rng.uniform(-9, 9, 1000), rng.uniform(-9, 9, 1000), rng.uniform(-1, 3, 1000)], -1).astype(np.float32)
        cams = [FR.look_at((7.5 * np.cos(a + 0.4 * seed), 7.5 * np.sin(a + 0.4 * seed), 3.0 + 0.2 * seed), (0.3 * seed, 0.0, 0.0), TA.H, TA.W,
                           TA.FOCAL + 6.0 * seed) for a in np.linspace(0, 2 * np.pi, 40, endpoint=False)]
        return {"points": torch.from_numpy(pts), "ks": torch.from_numpy(np.stack([K for _, K in cams])),
                "c2ws": torch.from_numpy(np.stack([c for c, _ in cams]))}

    def setup(state):
        state["fm"] = tracer("terrain")

    def run_(state):
        i = state["in"]
        views, mask = state["fm"].point_views(i["points"], i["ks"], i["c2ws"], TA.H, TA.W, MV.TERRAIN_BIAS, want_mask=True)
        return views, mask

    return SC.Case("mesh_point_views", ["scanerf_mesh_point_views"], build, run_, setup=setup)


def test_stream_the_op_runs_on_the_callers_stream(monkeypatch):
    import stream_cases as SC
    from scanerf_amd import _capi
    from test_gpu_stream_contract import Delay, same_bits
    c = _stream_case()
    X, Y = c.build(1), c.build(2)
    assert list(X) == list(Y) and all(not torch.equal(X[k], Y[k]) and X[k].shape == Y[k].shape for k in X)
    state = c.to_device(X)
    Xd, Yd = SC.stage(X), SC.stage(Y)
    handles = []
    real = _capi.tool("scanerf_mesh_point_views")

    def recorded(*a):
        handles.append(int(a[-1] or 0))
        return real(*a)
    monkeypatch.setitem(_capi._tools, "scanerf_mesh_point_views", recorded)
    torch.cuda.synchronize()
    R_X = c.run(state)
    c.refill(state, Yd)
    R_Y = c.run(state)               # leaves every output and input with Y's values
    torch.cuda.synchronize()
    assert not same_bits(R_X, R_Y), "the two seeds give the same answer: a stale read would not show"
    assert handles == [torch.cuda.current_stream().cuda_stream] * 2
    delay = Delay()
    s = torch.cuda.Stream()
    del handles[:]
    with torch.cuda.stream(s):
        pending = delay(20.0)
        c.refill(state, Xd)           # queued behind the delay: a launch on any other stream reads Y
        R = c.run(state)
        still = not pending.query()
    s.synchronize()
    torch.cuda.synchronize()
    assert handles == [s.cuda_stream] and s.cuda_stream != 0, "the call did not carry the caller's stream"
    assert still, "the call waited for its stream (the delay ran out before it returned)"
    assert same_bits(R, R_X), "under a side stream the op read stale inputs: a launch went to another stream"
