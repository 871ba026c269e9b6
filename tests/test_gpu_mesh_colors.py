"""Vertex colours from posed images on the GPU (csrc/mesh_colors.hip; FastMesh.project_colors, meshing.resolve_colors /
color_from_views, TileSetRenderer.color_mesh / extract_mesh(colors=) and the commands).  The fused route equals the
composed route bit for bit, equals the float32 restatement of tests/mesh_colors_reference.py bit for bit on every row without a flagged
pair, and lies within the reference's derived bound of its float64 yardstick wherever the counts agree."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_colors_reference as MC
import mesh_visibility_reference as MV
from test_gpu_mesh_visibility import scene  # noqa: F401  (the tile fixture: the G9 scene as tiles, its renderer, a level, two cameras)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
_i32, _f32 = torch.int32, torch.float32
BITS = ["terrain", "nested", "nested_extra", "edges", "many_cameras", "plates"]


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _gpu(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV).contiguous()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


@functools.lru_cache(maxsize=None)
def tracer(mesh, log2dim=6, pregather=True):
    """The tracer of a named case's mesh (terrain, many_cameras and their small-image forms share the terrain's)."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd.fastmesh import FastMesh
    case = MC.CASES[mesh]()
    return FastMesh.from_arrays(case["V"], case["F"], DEV, log2dim=log2dim, pregather=pregather)


def project(case, mesh, images="random", route="fused", normals="case", cameras=None, acc=None, count=None, log2dim=6, pregather=True, rows=None):
    """-> (acc [N,4] f32, count [N] i32) as numpy.  cameras: the columns to take, in this order; rows: the points to take."""
    img = case[images] if isinstance(images, str) else images
    nrm = case["normals"] if isinstance(normals, str) else normals
    cols = np.arange(len(case["ks"])) if cameras is None else np.asarray(cameras, np.int64)
    rows = slice(None) if rows is None else rows
    pts = _gpu(case["points"][rows])
    a = None if acc is None else _gpu(acc)
    c = None if count is None else _gpu(count)
    out = tracer(mesh, log2dim, pregather).project_colors(
        pts, _gpu(np.asarray(img)[cols]), _gpu(case["ks"][cols]), _gpu(case["c2ws"][cols]), case["bias"], normals=None if nrm is None else _gpu(nrm[rows]),
        near=case["near"], far=case["far"], min_cos=case["min_cos"], acc=a, count=c, route=route)
    assert out[0].dtype == _f32 and out[0].shape == (pts.shape[0], 4) and out[1].dtype == _i32 and out[1].shape == (pts.shape[0],)
    if a is not None:
        assert out[0].data_ptr() == a.data_ptr() and out[1].data_ptr() == c.data_ptr(), "acc / count are continued in place"
    return _np(out[0]), _np(out[1])


@functools.lru_cache(maxsize=None)
def fused(name, images="random"):
    """The fused answer of a case, computed once and never written to."""
    return project(MC.CASES[name](), name, images)


def _resolve(acc, fill=MC.FILL):
    from scanerf_amd import meshing
    colors, valid = meshing.resolve_colors(_gpu(acc), fill)
    assert colors.dtype == _f32 and valid.dtype == torch.bool
    return _np(colors), _np(valid)


def _same(a, b, what):
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]), what


def _against_restatement(got, r32, r64, what):
    """Bit for bit on the rows without a flagged pair; the others may differ only in the flagged pairs' contribution."""
    ok = ~r64["flagged_rows"]
    differ = (_bits(got[0]) != _bits(r32["acc"])).any(1) | (got[1] != r32["count"])
    print(f"mesh_colors {what}: {len(ok)} rows, {int((~ok).sum())} with a flagged pair, {int(differ.sum())} differ from the float32 restatement "
          f"(all of them flagged: {not (differ & ok).any()})")
    assert not (differ & ok).any(), (what, np.nonzero(differ & ok)[0][:10])


def _within_bound(got, case, images, what, r64=None, r32=None):
    r64 = r64 or MC.evaluate(case, f64, images)
    r32 = r32 or MC.evaluate(case, f32, images)
    B, judged = MC.bound(r32, r64, case[images] if isinstance(images, str) else images)
    colors, valid = _resolve(got[0])
    rows = judged & (got[1] == r64["count"])
    err = np.abs(colors.astype(f64) - r64["colors"])
    print(f"mesh_colors {what}: {int(rows.sum())} of {len(rows)} rows judged against float64, max error {err[rows].max() if rows.any() else 0:.3e}, "
          f"worst error / bound {(err[rows] / B[rows]).max() if rows.any() else 0:.3f}")
    assert rows.sum() >= 0.9 * r64["valid"].sum()
    assert (err[rows] <= B[rows]).all(), (what, np.argwhere(err > B)[:10])
    assert np.array_equal(valid[rows], r64["valid"][rows])


# ---- the three routes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BITS)
def test_fused_equals_composed_bit_for_bit(name):
    case = MC.CASES[name]()
    got = fused(name)
    composed = project(case, name, route="composed")
    _same(got, composed, name)
    colors, valid = _resolve(got[0])
    want_colors, want_valid = MC.resolve(got[0])      # one correctly rounded division per element
    assert np.array_equal(_bits(colors), _bits(want_colors)) and np.array_equal(valid, want_valid)
    ccolors, cvalid = _resolve(composed[0])
    assert np.array_equal(_bits(colors), _bits(ccolors)) and np.array_equal(valid, cvalid)
    assert valid.any() and (name == "nested_extra" or not valid.all())


@pytest.mark.parametrize("name", BITS)
def test_fused_equals_the_float32_restatement_and_stays_within_the_bound_of_float64(name):
    case = MC.CASES[name]()
    r64 = MC.evaluate(case, f64, "random")
    _against_restatement(fused(name), MC.evaluate(case, f32, "random"), r64, name)
    _within_bound(fused(name, "smooth"), case, "smooth", name)
    if name == "plates":      # the answers worked out by hand
        acc, count = project(case, name, images=case["constant"])
        assert count.tolist() == [2, 2, 2, 0, 0, 0, 0] and not acc[3:].any()
        colors, valid = _resolve(acc, (0.25, 0.5, 0.75))
        assert valid.tolist() == [True] * 3 + [False] * 4 and np.array_equal(colors[3:], np.tile(np.array([0.25, 0.5, 0.75], f32), (4, 1)))
        want = MC.evaluate(case, f64, images=case["constant"])
        assert np.abs(colors[:3] - want["colors"][:3]).max() < 1e-6


def test_normals_none_is_the_equal_weight_blend():
    case = MC.terrain()
    got = project(case, "terrain", normals=None)
    r64 = MC.evaluate(case, f64, "random", normals=None)
    _against_restatement(got, MC.evaluate(case, f32, "random", normals=None), r64, "terrain without normals")
    ok = ~r64["flagged_rows"]
    assert np.array_equal(got[0][ok, 3], got[1][ok].astype(f32))      # Wt is the count
    assert (got[1] >= fused("terrain")[1]).all() and (got[1] > fused("terrain")[1]).any()
    _same(got, project(case, "terrain", normals=None, route="composed"), "terrain without normals, composed")


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_points_around_a_wavefront(n):
    case = MC.terrain()
    rows = slice(1000, 1000 + n)      # rows in the middle of the terrain, where most points are seen
    got = project(case, "terrain", rows=rows)
    full = fused("terrain")
    _same(got, (full[0][rows], full[1][rows]), f"N={n}")
    assert got[1].any() or n == 1
    _same(got, project(case, "terrain", rows=rows, route="composed"), f"N={n} composed")


@pytest.mark.parametrize("c", [0, 1, 63, 64, 65, 130])
def test_cameras_around_a_pass_and_the_word_seams(c):
    case = MC.many_cameras()
    cams = np.concatenate([np.arange(65), np.arange(65)])[:c]
    got = project(case, "many_cameras", cameras=cams)
    if c == 0:
        assert not got[0].any() and not got[1].any()
        start = (np.random.default_rng(1).uniform(0, 2, (MV.MANY_POINTS, 4)).astype(f32), np.arange(MV.MANY_POINTS, dtype=np.int32))
        _same(project(case, "many_cameras", cameras=cams, acc=start[0], count=start[1]), start, "C=0 leaves acc and count as they are")
        return
    r64 = MC.evaluate(case, f64, "random", cameras=cams)
    _against_restatement(got, MC.evaluate(case, f32, "random", cameras=cams), r64, f"C={c}")
    _same(got, project(case, "many_cameras", cameras=cams, route="composed"), f"C={c} composed")
    if c == 65:
        _same(got, fused("many_cameras"), "C=65")
    if c > 64:
        assert got[1].max() > 64 or c == 65


@pytest.mark.parametrize("hw", [(5, 7), (33, 17)])
def test_small_images_clamps_and_partial_taps(hw):
    case = MC.small("many_cameras", *hw)
    got = project(case, "many_cameras")
    r64 = MC.evaluate(case, f64, "random")
    px, py = r64["px"][r64["contributed"]], r64["py"][r64["contributed"]]
    assert ((px < 0.5) | (px > hw[1] - 0.5) | (py < 0.5) | (py > hw[0] - 0.5)).sum() >= 20
    _against_restatement(got, MC.evaluate(case, f32, "random"), r64, f"{hw[0]} x {hw[1]}")
    _same(got, project(case, "many_cameras", route="composed"), f"{hw} composed")
    _within_bound(project(case, "many_cameras", images="smooth"), case, "smooth", f"{hw[0]} x {hw[1]}")


# ---- order and repeatability ------------------------------------------------------------------------------------------------------------
def test_batch_splits_give_equal_bits():
    case = MC.many_cameras()
    cams = np.concatenate([np.arange(65), np.arange(65)])
    whole = project(case, "many_cameras", cameras=cams)
    for cuts in ((64,), tuple(range(1, 130))):
        acc = count = None
        for a, b in zip((0,) + cuts, cuts + (130,)):
            acc, count = project(case, "many_cameras", cameras=cams[a:b], acc=acc, count=count)
        _same((acc, count), whole, f"splits at {cuts[:3]}...")


def test_equal_bits_for_both_triangle_forms_every_log2dim_and_a_second_launch():
    for name in ("terrain", "edges"):
        case = MC.CASES[name]()
        want = fused(name)
        for log2dim in (4, 6, 7):
            for pregather in (True, False):
                assert (tracer(name, log2dim, pregather).tris is not None) == pregather
                _same(project(case, name, log2dim=log2dim, pregather=pregather), want, (name, log2dim, pregather))
        _same(project(case, name), want, f"{name}: a second launch")


def test_prefilled_sums_continue():
    case = MC.terrain()
    rng = np.random.default_rng(9)
    N = len(case["points"])
    acc0, count0 = rng.uniform(0, 3, (N, 4)).astype(f32), rng.integers(0, 5, N).astype(np.int32)
    got = project(case, "terrain", acc=acc0, count=count0)
    r64 = MC.evaluate(case, f64, "random")
    _against_restatement(got, MC.evaluate(case, f32, "random", acc=acc0, count=count0), r64, "terrain, pre-filled")
    untouched = (got[1] == count0) & ~r64["flagged_rows"]
    assert untouched.any() and np.array_equal(_bits(got[0][untouched]), _bits(acc0[untouched]))      # nobody contributed: the bits it held


def test_non_finite_points_and_pixels():
    case = MC.edges()
    assert not np.isfinite(case["points"]).all() and not np.isfinite(case["normals"]).all()
    img = case["random"].copy()
    r = MC.evaluate(case, f64, "random")
    i, c = np.argwhere(r["contributed"])[0]
    img[c, int(np.floor(r["py"][i, c] - 0.5)) + 1, int(np.floor(r["px"][i, c] - 0.5)) + 1, 1] = np.nan      # one tap of one contributing pair
    img[1 - c if c < 2 else 0, 0, 0, :] = np.inf
    got = project(case, "edges", images=img)
    r64, r32 = MC.evaluate(case, f64, img), MC.evaluate(case, f32, img)
    assert r["contributed"][i, c] and not r64["contributed"][i, c]
    _against_restatement(got, r32, r64, "edges with non-finite pixels")
    assert np.isfinite(got[0]).all()
    _same(got, project(case, "edges", images=img, route="composed"), "edges with non-finite pixels, composed")
    bad = ~np.isfinite(case["points"]).all(1)
    assert not got[1][bad].any() and not got[0][bad].any()


# ---- the entries themselves: guard regions ----------------------------------------------------------------------------------------------
GUARD, SENTINEL = 96, -7.0


def test_guard_regions_stay_untouched_and_every_row_is_written():
    from scanerf_amd import _capi
    from scanerf_amd.allocation import _cameras
    p = lambda t: None if t is None else t.data_ptr()
    for name in ("terrain", "many_cameras"):
        case = MC.CASES[name]()
        want = fused(name)
        for pregather in (True, False):
            fm = tracer(name, 6, pregather)
            pts, nrm, img = _gpu(case["points"]), _gpu(case["normals"]), _gpu(case["random"])
            k9, c12 = _cameras(case["ks"], case["c2ws"], DEV)
            N = pts.shape[0]
            abuf = torch.full((GUARD + 4 * N + GUARD,), SENTINEL, dtype=_f32, device=DEV)
            cbuf = torch.full((GUARD + N + GUARD,), int(SENTINEL), dtype=_i32, device=DEV)
            abuf[GUARD:GUARD + 4 * N] = 0
            cbuf[GUARD:GUARD + N] = 0
            counters = torch.zeros(4, dtype=torch.int64, device=DEV)
            args = (p(pts), p(nrm), N, p(img), p(k9), p(c12), k9.shape[0], case["H"], case["W"], case["bias"], case["near"], case["far"],
                    case["min_cos"], p(fm.vertices), p(fm.faces), p(fm.tris), p(fm.bitmask), p(fm.rank), p(fm.start_num), p(fm.cell_faces),
                    p(fm.scene_info), fm.log2dim, abuf[GUARD:].data_ptr(), cbuf[GUARD:].data_ptr())
            assert _capi.tool("scanerf_mesh_project_colors_counted")(*args, p(counters), _capi.stream()) == 0
            torch.cuda.synchronize()
            for buf, n in ((abuf, 4 * N), (cbuf, N)):
                assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "a guard region was written"
            _same((_np(abuf[GUARD:GUARD + 4 * N]).reshape(N, 4), _np(cbuf[GUARD:GUARD + N])), want, (name, pregather))
            pairs, cells, tests, used = counters.tolist()
            r64 = MC.evaluate(case, f64, "random")
            assert pairs == int(case["ref"]["inview"].sum()) or abs(pairs - int(case["ref"]["inview"].sum())) <= int(case["ref"]["ambiguous"].sum())
            assert used == int(want[1].sum()) and cells > 0 and tests > 0
            assert abs(used - int(r64["contributed"].sum())) <= int(r64["flagged"].sum())
            # resolve: every element of colors and valid written, nothing beyond
            colors = torch.full((GUARD + 3 * N + GUARD,), SENTINEL, dtype=_f32, device=DEV)
            valid = torch.full((GUARD + N + GUARD,), 9, dtype=torch.uint8, device=DEV)
            import ctypes
            fill = (ctypes.c_float * 3)(*MC.FILL)
            assert _capi.tool("scanerf_mesh_resolve_colors")(abuf[GUARD:].data_ptr(), N, fill, colors[GUARD:].data_ptr(), valid[GUARD:].data_ptr(),
                                                             _capi.stream()) == 0
            torch.cuda.synchronize()
            assert bool((colors[:GUARD] == SENTINEL).all()) and bool((colors[GUARD + 3 * N:] == SENTINEL).all())
            assert bool((valid[:GUARD] == 9).all()) and bool((valid[GUARD + N:] == 9).all())
            wc, wv = MC.resolve(want[0])
            assert np.array_equal(_bits(_np(colors[GUARD:GUARD + 3 * N]).reshape(N, 3)), _bits(wc))
            assert np.array_equal(_np(valid[GUARD:GUARD + N]), wv.astype(np.uint8))


def test_refusals_with_device_pointers_write_nothing():
    from scanerf_amd import _capi
    from scanerf_amd.allocation import _cameras
    case = MC.edges()
    fm, pts, img = tracer("edges"), _gpu(case["points"]), _gpu(case["random"])
    k9, c12 = _cameras(case["ks"], case["c2ws"], DEV)
    N = pts.shape[0]
    acc = torch.full((N, 4), SENTINEL, dtype=_f32, device=DEV)
    count = torch.full((N,), int(SENTINEL), dtype=_i32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    for kw, text in ((dict(H=0), b"H=0"), (dict(bias=0.0), b"bias=0"), (dict(near=-1.0), b"near=-1"), (dict(far=0.0), b"far=0"),
                     (dict(min_cos=1.0), b"min_cos=1"), (dict(log2dim=9), b"log2dim=9")):
        a = dict(H=case["H"], W=case["W"], bias=case["bias"], near=case["near"], far=case["far"], min_cos=0.0, log2dim=fm.log2dim)
        a.update(kw)
        status = _capi.tool("scanerf_mesh_project_colors")(
            p(pts), None, N, p(img), p(k9), p(c12), 2, a["H"], a["W"], a["bias"], a["near"], a["far"], a["min_cos"], p(fm.vertices), p(fm.faces),
            p(fm.tris), p(fm.bitmask), p(fm.rank), p(fm.start_num), p(fm.cell_faces), p(fm.scene_info), a["log2dim"], p(acc), p(count), _capi.stream())
        assert status != 0 and text in _capi.lib().scanerf_last_error(), kw
    torch.cuda.synchronize()
    assert bool((acc == SENTINEL).all()) and bool((count == int(SENTINEL)).all())


# ---- the stream -------------------------------------------------------------------------------------------------------------------------
def test_stream_the_op_runs_on_the_callers_stream(monkeypatch):
    """The stale-data construction of tests/stream_cases.py for entries its registry cannot claim (it follows include/scanerf_hip.h)."""
    import fastmesh_reference as FR
    import stream_cases as SC
    import tile_allocation_reference as TA
    from scanerf_amd import _capi, meshing
    from test_gpu_stream_contract import Delay, same_bits

    def build(seed):
        rng = np.random.default_rng(5200 + seed)
        pts = np.stack([rng.uniform(-9, 9, 1000), rng.uniform(-9, 9, 1000), rng.uniform(-1, 3, 1000)], -1).astype(f32)
        cams = [FR.look_at((7.5 * np.cos(a + 0.4 * seed), 7.5 * np.sin(a + 0.4 * seed), 3.0 + 0.2 * seed), (0.3 * seed, 0.0, 0.0), 24, 32,
                           26.0 + 2.0 * seed) for a in np.linspace(0, 2 * np.pi, 12, endpoint=False)]
        return {"points": torch.from_numpy(pts), "ks": torch.from_numpy(np.stack([K for _, K in cams])),
                "c2ws": torch.from_numpy(np.stack([c for c, _ in cams])), "images": torch.from_numpy(rng.uniform(0, 1, (12, 24, 32, 3)).astype(f32))}

    def run_(state):
        i = state["in"]
        acc, count = state["fm"].project_colors(i["points"], i["images"], i["ks"], i["c2ws"], MV.TERRAIN_BIAS)
        return (acc, count, *meshing.resolve_colors(acc))

    c = SC.Case("mesh_project_colors", ["scanerf_mesh_project_colors", "scanerf_mesh_resolve_colors"], build, run_,
                setup=lambda state: state.update(fm=tracer("terrain")))
    X, Y = c.build(1), c.build(2)
    assert all(not torch.equal(X[k], Y[k]) and X[k].shape == Y[k].shape for k in X)
    state = c.to_device(X)
    Xd, Yd = SC.stage(X), SC.stage(Y)
    handles = []
    for name in c.entries:
        real = _capi.tool(name)
        monkeypatch.setitem(_capi._tools, name, lambda *a, _real=real: (handles.append(int(a[-1] or 0)), _real(*a))[1])
    torch.cuda.synchronize()
    R_X = c.run(state)
    c.refill(state, Yd)
    R_Y = c.run(state)
    torch.cuda.synchronize()
    assert not same_bits(R_X, R_Y), "the two seeds give the same answer: a stale read would not show"
    assert handles == [torch.cuda.current_stream().cuda_stream] * 4
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
    assert handles == [s.cuda_stream] * 2 and s.cuda_stream != 0, "a call did not carry the caller's stream"
    assert still, "a call waited for its stream (the delay ran out before it returned)"
    assert same_bits(R, R_X), "under a side stream the op read stale inputs: a launch went to another stream"


# ---- the Python layers --------------------------------------------------------------------------------------------------------------------
def test_color_from_views_on_the_terrain():
    from scanerf_amd import meshing
    case = MC.terrain()
    mesh = meshing.Mesh(_gpu(case["V"]), _gpu(case["F"]), None, None, _gpu(case["normals"]))
    want = fused("terrain")
    wc, wv = MC.resolve(want[0])
    kw = dict(min_cos=case["min_cos"])
    report = {}
    for images, vpb in ((case["random"], 8), (case["random"], 3), (torch.from_numpy(case["random"]), 1), (_gpu(case["random"]), 5),
                        (lambda a, b: case["random"][a:b], 3)):
        colors, valid = meshing.color_from_views(mesh, images, case["ks"], case["c2ws"], case["bias"], views_per_batch=vpb, report=report, **kw)
        assert np.array_equal(_bits(_np(colors)), _bits(wc)) and np.array_equal(_np(valid), wv), vpb
    assert report == {"count_histogram": np.bincount(want[1]).tolist(), "invalid": int((~wv).sum())}
    composed = meshing.color_from_views(mesh, case["random"], case["ks"], case["c2ws"], case["bias"], route="composed", **kw)
    assert np.array_equal(_bits(_np(composed[0])), _bits(wc))
    # uint8 images are read as 0..255 -> 0..1; normals=None and a tensor; a mesh without faces gets the fill
    u8 = (case["random"] * 255).astype(np.uint8)
    a = meshing.color_from_views(mesh, u8, case["ks"], case["c2ws"], case["bias"], **kw)
    b = meshing.color_from_views(mesh, u8.astype(f32) / f32(255.0), case["ks"], case["c2ws"], case["bias"], **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    plain = meshing.color_from_views(mesh._replace(normals=None), case["random"], case["ks"], case["c2ws"], case["bias"], **kw)
    none = meshing.color_from_views(mesh, case["random"], case["ks"], case["c2ws"], case["bias"], normals=None, **kw)
    assert torch.equal(plain[0], none[0]) and not torch.equal(plain[0], a[0])
    given = meshing.color_from_views(mesh._replace(normals=None), case["random"], case["ks"], case["c2ws"], case["bias"], normals=mesh.normals, **kw)
    assert np.array_equal(_bits(_np(given[0])), _bits(wc))
    empty = meshing.Mesh(mesh.vertices, mesh.faces[:0], None, None, None)
    colors, valid = meshing.color_from_views(empty, case["random"], case["ks"], case["c2ws"], case["bias"], fill=(0.1, 0.2, 0.3), report=report)
    assert not valid.any() and np.array_equal(_np(colors), np.tile(np.array([0.1, 0.2, 0.3], f32), (len(case["V"]), 1)))
    assert report == {"count_histogram": [len(case["V"])], "invalid": len(case["V"])}
    colors, valid = meshing.color_from_views(meshing.Mesh(mesh.vertices[:0], mesh.faces[:0], None, None, None), case["random"], case["ks"],
                                             case["c2ws"], case["bias"])
    assert colors.shape == (0, 3) and valid.shape == (0,)


def test_round_trip_on_the_icosphere():
    """render_views draws the coloured icosphere, project_colors with min_cos = 0.5 brings the colours back to the vertices; judged
    against the numpy reference of the same pipeline (mesh_render_reference's float32 images into mesh_colors_reference)."""
    from scanerf_amd.fastmesh import FastMesh
    case = MC.round_trip()
    img, r64, r32 = MC.round_trip_reference()
    fm = FastMesh.from_arrays(case["V"], case["F"], DEV)
    rendered = fm.render_views(_gpu(case["ks"]), _gpu(case["c2ws"]), case["H"], case["W"], colors=_gpu(case["colors"]))["color"]
    differ = (_np(rendered) != img).any(-1)
    print(f"mesh_colors round trip: {int(differ.sum())} of {differ.size} rendered pixels differ from mesh_render_reference's float32 images")
    acc, count = fm.project_colors(_gpu(case["points"]), rendered.contiguous(), _gpu(case["ks"]), _gpu(case["c2ws"]), case["bias"],
                                   normals=_gpu(case["normals"]), min_cos=case["min_cos"])
    got = (_np(acc), _np(count))
    # a vertex whose taps hold a pixel the two renderers disagree about is not the projection's to answer for
    touched = np.zeros(len(case["points"]), bool)
    for c in range(len(case["ks"])):
        j = np.nonzero(r64["contributed"][:, c])[0]
        x0, y0 = np.floor(r64["px"][j, c] - 0.5).astype(int), np.floor(r64["py"][j, c] - 0.5).astype(int)
        for dx in (0, 1):
            for dy in (0, 1):
                touched[j] |= differ[c, np.clip(y0 + dy, 0, case["H"] - 1), np.clip(x0 + dx, 0, case["W"] - 1)]
    assert touched.mean() < 0.05
    B, judged = MC.bound(r32, r64, img)
    colors, valid = _resolve(got[0])
    rows = judged & (got[1] == r64["count"]) & ~touched
    err = np.abs(colors.astype(f64) - r64["colors"])
    dev = np.abs(colors - case["colors"])
    print(f"mesh_colors round trip: {int(rows.sum())} of {len(rows)} vertices judged, worst error / bound {(err[rows] / B[rows]).max():.3f}; "
          f"|colour - original| mean {dev.mean():.4f} max {dev.max():.4f}")
    assert valid.all() and rows.sum() >= 0.9 * len(rows)
    assert (err[rows] <= B[rows]).all()
    ok = ~r64["flagged_rows"] & ~touched
    assert np.array_equal(_bits(got[0][ok]), _bits(r32["acc"][ok])) and np.array_equal(got[1][ok], r32["count"][ok])


def test_extract_mesh_with_colors_on_the_tile_fixture(scene):
    from scanerf_amd import meshing
    from test_gpu_mesh_components import _same as same_mesh
    rnd, level, cams = scene["rnd"], scene["level"], scene["cameras"]
    kw = dict(cells_per_axis=20, cameras=cams, min_views=1, min_faces=2, normals=True)
    plain = rnd.extract_mesh(level, **kw)
    same_mesh(rnd.extract_mesh(level, colors=None, **kw), plain, "colors=None")
    mesh, rgb = rnd.extract_mesh(level, colors="diffuse", **kw)
    same_mesh(mesh, plain, "the mesh of the call without colours")
    V = mesh.vertices.shape[0]
    assert V > 0 and rgb.shape == (V, 3) and rgb.dtype == _f32 and bool(torch.isfinite(rgb).all())
    # the same colours by hand: color_mesh on the finished mesh with the extractors' bias
    corner, size = rnd.scene_box()
    bias = meshing.default_view_bias(size, meshing.cells_per_axis(size, 20))
    report = {}
    by_hand, valid = rnd.color_mesh(mesh, cams, which="diffuse", bias=bias, report=report)
    assert torch.equal(by_hand, rgb) and report["invalid"] == int((~valid).sum()) and sum(report["count_histogram"]) == V
    print(f"mesh_colors extract: {V} vertices, {report['invalid']} without a colour, histogram {report['count_histogram']}")
    # who gets a colour: with equal weights exactly the vertices vertex_views counts a camera for (the renders are finite); with the
    # mesh's normals those of them that face a camera that sees them.  (This fixture's field is random features: its level set is
    # mostly seen from the dense side through the open faces of the world box, so the facing rule drops most of the seen vertices.)
    views, _ = meshing.vertex_views(mesh, *cams, bias)
    flat, flat_valid = rnd.color_mesh(mesh, cams, which="diffuse", bias=bias, normals=None)
    assert torch.equal(flat_valid, views > 0) and flat_valid.any() and not flat_valid.all()
    assert valid.any() and not bool((valid & ~flat_valid).any())
    _, unweighted = rnd.extract_mesh(level, colors="diffuse", **dict(kw, normals=False))      # no normals on the mesh: equal weights
    assert torch.equal(unweighted, flat)
    score = rnd.score_mesh(mesh, cams, colors=rgb)
    pooled = score["pooled"]
    print(f"mesh_colors extract: score_mesh psnr {pooled['psnr']:.2f} dB, coverage {pooled['coverage']:.3f} over {score['n_views']} views")
    assert np.isfinite(pooled["psnr"]) and pooled["coverage"] > 0      # (the PSNR is NaN over an empty covered set)
    # the colours follow simplify: taken at the FINAL vertices
    cell = 2.5 * bias
    smesh, srgb = rnd.extract_mesh(level, colors="rgb", simplify=cell, color_scale=2, **kw)
    assert 0 < smesh.vertices.shape[0] < V and srgb.shape == (smesh.vertices.shape[0], 3)
    same_mesh(smesh, rnd.extract_mesh(level, simplify=cell, **kw), "simplified, with and without colours")


def test_the_commands_end_to_end(scene, tmp_path, capsys):
    from scanerf_amd import formats
    from test_gpu_mesh_components import _tool
    rnd, level, cams = scene["rnd"], scene["level"], scene["cameras"]
    out = str(tmp_path / "scene.ply")
    assert _tool("extract_scene_mesh").main([*scene["dirs"], "--level", repr(level), "--cells-per-axis", "20", "--out", out, "--cameras", scene["log"],
                                             "--min-views", "1", "--min-faces", "2", "--colors", "diffuse"]) == 0
    mesh, rgb = rnd.extract_mesh(level, cells_per_axis=20, cameras=cams, min_views=1, min_faces=2, colors="diffuse")
    v, f, c = formats.read_ply(out, colors=True)
    assert np.array_equal(v, _np(mesh.vertices)) and np.array_equal(f, _np(mesh.faces))
    assert np.array_equal(c, formats.quantize_colors(_np(rgb.clamp(0, 1))).reshape(-1, 3))
    assert "vertex colours (diffuse) from 2 cameras" in capsys.readouterr().out
    # color_mesh.py: that PLY coloured again from images on disk: the scene's own renders, saved as float32 and as uint8
    ks, c2ws, H, W = cams
    images = torch.cat([im for _, _, im, _ in rnd._scene_batches(torch.as_tensor(ks), torch.as_tensor(c2ws).to(_f32), int(H), int(W), 8, "diffuse", 0.5, {})])
    plain = str(tmp_path / "plain.ply")
    formats.write_ply(plain, v, f)
    for dtype in (f32, np.uint8):
        npy, col = str(tmp_path / f"images_{np.dtype(dtype).name}.npy"), str(tmp_path / f"colored_{np.dtype(dtype).name}.ply")
        np.save(npy, _np(images) if dtype == f32 else np.floor(_np(images) * 255 + 0.5).astype(np.uint8))
        assert _tool("color_mesh").main([plain, "--cameras", scene["log"], "--images", npy, "-o", col, "--views-per-batch", "1"]) == 0
        v2, f2, c2 = formats.read_ply(col, colors=True)
        assert np.array_equal(v2, v) and np.array_equal(f2, f) and c2.shape == c.shape and c2.dtype == np.uint8
        printed = capsys.readouterr().out
        assert "equal weights" in printed and "vertices coloured from 2 images" in printed
        close = np.abs(c2.astype(int) - c.astype(int)).max(1) <= 16
        print(f"mesh_colors commands ({np.dtype(dtype).name}): {100 * close.mean():.1f} % of the vertices within 16 / 255 of the extractor's colours")
        assert close.mean() > 0.5      # (another bias and no normals: the same picture, not the same numbers)
    assert _tool("color_mesh").main([plain, "--cameras", scene["log"], "--images", npy]) == 0      # the default output name
    assert os.path.exists(str(tmp_path / "plain.colored.ply"))
