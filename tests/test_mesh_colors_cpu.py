"""The project-and-blend op without a GPU: the numpy reference's own facts (tests/mesh_colors_reference.py), its float32
restatement within the derived bound of its float64 yardstick, the answers worked out by hand, the new entries of the second public
header against _capi.TOOL_PROTOTYPES, every refusal that happens before a launch, and the commands' arguments."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mesh_colors_reference as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
NEW = ("scanerf_mesh_project_colors", "scanerf_mesh_project_colors_counted", "scanerf_mesh_resolve_colors")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("images", ["smooth", "random"])
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_float32_restatement_within_the_derived_bound_of_float64(name, images):
    case = MC.CASES[name]()
    r64, r32 = MC.evaluate(case, f64, images), MC.evaluate(case, f32, images)
    B, judged = MC.bound(r32, r64, case[images])
    err = np.abs(r32["colors"].astype(f64) - r64["colors"])
    ratio = float((err[judged] / B[judged]).max()) if judged.any() else 0.0
    print(f"mesh_colors_reference {name}/{images}: {len(judged)} rows, {int(r64['valid'].sum())} coloured, {int(judged.sum())} judged, "
          f"max |c32 - c64| {err[judged].max():.3e}, max bound {B[judged].max():.3e}, worst error / bound {ratio:.3f}")
    assert judged.sum() >= 3 and judged.sum() >= 0.9 * r64["valid"].sum(), "the two evaluations disagree about too many rows to judge"
    assert (err[judged] <= B[judged]).all(), (name, images, np.argwhere(err > B)[:10])
    unflagged = ~r64["flagged_rows"]
    assert np.array_equal(r32["count"][unflagged], r64["count"][unflagged])
    assert np.array_equal(r32["contributed"][unflagged], r64["contributed"][unflagged])


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_flagged_rows_stay_under_the_cap(name):
    """At most 10 % of a case's rows hold a flagged pair (MC.FLAGGED_ROWS_CAP): the bit comparisons of the GPU tests cover the rest."""
    case = MC.CASES[name]()
    r64 = MC.evaluate(case, f64)
    share = r64["flagged_rows"].mean()
    print(f"mesh_colors_reference {name}: {int(r64['flagged_rows'].sum())} of {len(r64['flagged_rows'])} rows flagged ({100 * share:.2f} %), "
          f"{int(r64['seen'].sum())} pairs seen, {int(r64['contributed'].sum())} contributed, {int((~r64['valid']).sum())} rows get the fill")
    assert MC.FLAGGED_ROWS_CAP == 0.10 and share <= MC.FLAGGED_ROWS_CAP
    assert r64["contributed"].any() and (r64["seen"] & ~r64["contributed"]).any() == (case["normals"] is not None)
    assert not (r64["contributed"] & ~r64["seen"]).any()
    assert np.array_equal(r64["count"], r64["contributed"].sum(1)) and np.array_equal(r64["valid"], r64["count"] > 0)


def test_small_images_reach_the_clamps():
    """5 x 7 and 33 x 17: a good share of the seen pairs project into the border half pixel, where an index clamps."""
    for H, W in ((5, 7), (33, 17)):
        case = MC.small("many_cameras", H, W)
        r = MC.evaluate(case, f64)
        px, py = r["px"][r["contributed"]], r["py"][r["contributed"]]
        clamped = (px < 0.5) | (px > W - 0.5) | (py < 0.5) | (py > H - 0.5)
        print(f"mesh_colors_reference {case['name']}: {len(px)} contributing pairs, {int(clamped.sum())} with a clamped index")
        assert clamped.sum() >= 20 and (~clamped).sum() >= 20
        r32 = MC.evaluate(case, f32)
        B, judged = MC.bound(r32, r, case["smooth"])
        assert (np.abs(r32["colors"].astype(f64) - r["colors"])[judged] <= B[judged]).all()


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def _plates_cos(case):
    """cos(normal (0, 0, 1), direction to the eye) for every (point, camera), by hand."""
    d = case["eyes"][None] - case["points"].astype(f64)[:, None]
    return d[..., 2] / np.linalg.norm(d, axis=-1)


def test_plates_constant_images_give_the_weight_normalised_mix():
    case = MC.plates()
    cos = _plates_cos(case)
    assert not case["ref"]["ambiguous"].any()
    want_seen = np.array([[1, 1, 1]] * 4 + [[0, 0, 1]] * 3, bool)
    assert np.array_equal(case["ref"]["seen"], want_seen)
    assert (cos[:4, 2] < MC.PLATES_MIN_COS).all() and (cos[4:, 2] < MC.PLATES_MIN_COS).all() and (cos[:, :2] > 0.8).all()
    for dtype, tol in ((f64, 1e-12), (f32, 1e-6)):
        r = MC.evaluate(case, dtype, images=case["constant"])
        for i in range(3):      # the front plate: cameras 0 and 1, the grazing camera 2 falls to min_cos
            mix = (cos[i, 0] * MC.CONSTANTS[0].astype(f64) + cos[i, 1] * MC.CONSTANTS[1]) / (cos[i, 0] + cos[i, 1])
            assert r["count"][i] == 2 and np.abs(r["colors"][i] - mix).max() < tol, (dtype, i)
            assert abs(r["acc"][i, 3] - (cos[i, 0] + cos[i, 1])) < tol * 10
        # point 3 has a zero normal: cosv is NaN, nothing contributes; the rear plate: hidden from above, grazing from the side
        assert r["count"][3:].tolist() == [0, 0, 0, 0] and not r["valid"][3:].any()
        assert np.array_equal(r["colors"][3:], np.tile(np.asarray(MC.FILL, dtype), (4, 1)))
        assert not r["acc"][3:].any()


def test_plates_min_cos_removes_the_grazing_camera_and_no_normals_weigh_equally():
    case = MC.plates()
    r = MC.evaluate(dict(case, min_cos=0.0), f64, images=case["constant"])
    assert r["count"].tolist() == [3, 3, 3, 0, 1, 1, 1]      # with min_cos = 0 the grazing camera counts; the zero normal still does not
    assert np.allclose(r["colors"][4:], MC.CONSTANTS[2].astype(f64)[None])      # the rear plate is then camera 2's constant
    r = MC.evaluate(case, f64, images=case["constant"], normals=None)
    assert r["count"].tolist() == [3, 3, 3, 3, 1, 1, 1]
    assert np.allclose(r["colors"][:4], MC.CONSTANTS.astype(f64).mean(0)[None]) and np.allclose(r["acc"][:4, 3], 3.0)


def test_linear_images_give_the_linear_function_at_the_pixel_coordinates():
    case = MC.terrain()
    img, co = MC.linear_images(len(case["ks"]), case["H"], case["W"])
    r = MC.evaluate(case, f64, images=img)
    H, W = case["H"], case["W"]
    inner = r["contributed"] & (r["px"] >= 0.5) & (r["px"] <= W - 0.5) & (r["py"] >= 0.5) & (r["py"] <= H - 0.5)
    assert inner.sum() > 1000
    for c in range(len(case["ks"])):
        j = np.nonzero(inner[:, c])[0]
        want = co[c, None, :, 0] + co[c, None, :, 1] * r["px"][j, c, None] + co[c, None, :, 2] * r["py"][j, c, None]
        assert np.abs(r["val"][j, c] - want).max() < 1e-6      # (the float32 pixels of the linear image round at 3e-8)


def test_a_nan_tap_removes_exactly_that_pair():
    case = MC.plates()
    clean = MC.evaluate(case, f32, images="random")
    x0, y0 = int(np.floor(clean["px"][0, 1] - 0.5)), int(np.floor(clean["py"][0, 1] - 0.5))
    for channel, value in ((0, np.nan), (2, np.inf)):
        img = case["random"].copy()
        img[1, y0 + 1, x0, channel] = value      # one of the 12 taps of (point 0, camera 1), one channel
        r = MC.evaluate(case, f32, images=img)
        assert clean["contributed"][0, 1] and not r["contributed"][0, 1]
        rest = np.ones_like(r["contributed"])
        rest[0, 1] = False
        lost = clean["contributed"] & ~r["contributed"] & rest      # other points whose taps include the poisoned pixel
        for i in range(len(case["points"])):
            if not lost[i].any() and i != 0:
                assert np.array_equal(_bits(r["acc"][i]), _bits(clean["acc"][i]))
        assert r["count"][0] == clean["count"][0] - 1 and np.isfinite(r["acc"]).all()
        only0 = MC.evaluate(case, f32, images=case["random"], cameras=[0])
        assert np.array_equal(_bits(r["acc"][0]), _bits(only0["acc"][0]))      # point 0 is left with camera 0 alone


# ---- order ------------------------------------------------------------------------------------------------------------------------
def test_batch_splits_equal_one_call():
    case = MC.many_cameras()
    whole = MC.evaluate(case, f32, images="random")
    for cuts in ((64,), (1, 2, 33), tuple(range(1, 65))):
        acc = count = None
        for a, b in zip((0,) + cuts, cuts + (65,)):
            r = MC.evaluate(case, f32, images="random", cameras=range(a, b), acc=acc, count=count)
            acc, count = r["acc"], r["count"]
        assert np.array_equal(_bits(acc), _bits(whole["acc"])) and np.array_equal(count, whole["count"]), cuts


def test_the_sums_depend_on_the_camera_order_as_defined():
    case = MC.many_cameras()
    a = MC.evaluate(case, f32, images="random")
    b = MC.evaluate(case, f32, images="random")
    assert np.array_equal(_bits(a["acc"]), _bits(b["acc"]))      # the same order: the same bits, always
    order = np.random.default_rng(3).permutation(65)
    p = MC.evaluate(case, f32, images="random", cameras=order)
    assert np.array_equal(p["count"], a["count"])
    differ = (_bits(p["acc"]) != _bits(a["acc"])).any(1)
    print(f"mesh_colors_reference many_cameras: a permuted camera order changes the float32 sums of {int(differ.sum())} of {len(differ)} rows")
    assert differ.any(), "65 float32 additions in another order and not one row differs: the order would not matter"
    err = np.abs(p["colors"].astype(f64) - a["colors"])[a["valid"]]
    assert err.max() <= (2 * 65 + 12) * MC.U * 2      # two roundings of the weighted mean's bound apart, on colours <= 1


def test_resolve_colors_arithmetic():
    acc = np.array([[1, 2, 3, 4], [0.3, 0.1, 0.2, 0.7], [5, 5, 5, 0], [1, 1, 1, -2], [1, 1, 1, np.nan], [0, 0, 0, 1e-30]], f32)
    colors, valid = MC.resolve(acc, (0.1, 0.2, 0.3))
    assert valid.tolist() == [True, True, False, False, False, True]
    assert np.array_equal(colors[0], np.array([0.25, 0.5, 0.75], f32))
    assert np.array_equal(_bits(colors[1]), _bits(acc[1, :3] / acc[1, 3]))
    assert np.array_equal(colors[2:5], np.tile(np.array([0.1, 0.2, 0.3], f32), (3, 1))) and not colors[5].any()


def test_round_trip_on_the_icosphere_reference_alone():
    """Render the coloured icosphere (mesh_render_reference, float32), project back with min_cos = 0.5: the deviation from the
    colours the mesh had is printed and recorded in DESIGN.md 4.25, not asserted against a number chosen in advance; the float32
    restatement stays within the derived bound of float64."""
    case = MC.round_trip()
    img, r64, r32 = MC.round_trip_reference()
    assert img.shape == (14, 48, 48, 3) and r64["valid"].all(), "a vertex of the sphere that no camera sees within 60 degrees of its normal"
    dev = np.abs(r64["colors"] - case["colors"].astype(f64))
    print(f"mesh_colors_reference round trip: {len(dev)} vertices, {int(r64['count'].min())}..{int(r64['count'].max())} cameras each, "
          f"|colour - original| mean {dev.mean():.4f} max {dev.max():.4f}")
    B, judged = MC.bound(r32, r64, img)
    assert judged.all() and (np.abs(r32["colors"].astype(f64) - r64["colors"]) <= B).all()


# ---- the second header ----------------------------------------------------------------------------------------------------------------
def test_new_entries_against_the_header_and_tool_prototypes():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    from test_mesh_visibility_cpu import TOOLS_HEADER, _prototypes
    hdr = _prototypes(TOOLS_HEADER)
    so = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert name in hdr and tuple(_capi.TOOL_PROTOTYPES[name]) == hdr[name], name
        assert hasattr(so, name), f"the library does not export {name}"
        assert name not in _capi.PROTOTYPES
    views, colors = _capi.TOOL_PROTOTYPES["scanerf_mesh_point_views"][1], _capi.TOOL_PROTOTYPES["scanerf_mesh_project_colors"][1]
    # points, [normals], N, [images], Ks, C2Ws, C, H, W, bias, near, far, [min_cos], the tracer's nine, then the outputs and the stream
    assert colors == "P" + "P" + "I" + "P" + views[2:10] + "F" + views[10:19] + "PPP"
    assert _capi.TOOL_PROTOTYPES["scanerf_mesh_project_colors_counted"][1] == colors + "P"
    assert _capi.TOOL_PROTOTYPES["scanerf_mesh_resolve_colors"] == ("I", "PIPPPP")
    with pytest.raises(TypeError, match="scanerf_mesh_project_colors"):
        _capi.tool("scanerf_mesh_project_colors")(1, 2)
    text = open(TOOLS_HEADER).read()
    for word in ("IN THIS ORDER", "x0 = clamp((int)x0f, 0, W-1)", "cosv = (-q) / (len * nl)", "all 12 taps are finite", "fill[3]: a HOST array"):
        assert word in text, word


# ---- the entries' refusals, before any launch ------------------------------------------------------------------------------------------
def _entry(counted=False, **over):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    a = dict(points=None, normals=None, N=4, images=None, Ks=None, C2Ws=None, C=2, H=8, W=8, bias=0.1, near=0.0, far=math.inf, min_cos=0.0,
             vertices=None, faces=None, tris=None, bitmask=None, rank=None, start_num=None, cell_faces=None, scene_info=None, log2dim=6,
             acc=None, count=None)
    if counted:
        a["counters"] = None
    a.update(over)
    name = "scanerf_mesh_project_colors" + ("_counted" if counted else "")
    status = _capi.tool(name)(*a.values(), None)
    return status, _capi.lib().scanerf_last_error()


def test_project_colors_refuses_before_any_launch():
    for over, text in (({}, b"null pointer"), ({"H": 0}, b"H=0"), ({"W": 0}, b"W=0"), ({"W": -2}, b"W=-2"), ({"log2dim": 3}, b"log2dim=3"),
                       ({"log2dim": 8}, b"log2dim=8"), ({"bias": 0.0}, b"bias=0"), ({"bias": -1.0}, b"bias=-1"), ({"bias": math.inf}, b"bias=inf"),
                       ({"bias": math.nan}, b"bias="), ({"near": -0.5}, b"near=-0.5"), ({"near": math.nan}, b"near="), ({"far": 0.0}, b"far=0"),
                       ({"far": -2.0}, b"far=-2"), ({"far": math.nan}, b"far="), ({"N": -1}, b"N=-1"), ({"C": -1}, b"C=-1"),
                       ({"min_cos": -0.1}, b"min_cos=-0.1"), ({"min_cos": 1.0}, b"min_cos=1"), ({"min_cos": math.nan}, b"min_cos=")):
        status, msg = _entry(**over)
        assert status != 0 and text in msg and b"mesh_project_colors" in msg, (over, msg)
    assert _entry(N=0)[0] == 0 and _entry(N=0, H=0, log2dim=3, min_cos=7.0)[0] == 0      # a no-op, whatever else is passed
    buf = ctypes.create_string_buffer(512)
    p = ctypes.addressof(buf)
    p += -p % 16
    for missing in ("points", "acc", "count"):
        given = dict(points=p, acc=p, count=p)
        given[missing] = None
        status, msg = _entry(**given)
        assert status != 0 and b"null pointer" in msg, missing
    status, msg = _entry(points=p, acc=p + 4, count=p)
    assert status != 0 and b"16-byte aligned" in msg
    assert _entry(points=p, acc=p, count=p, C=0)[0] == 0       # no camera: nothing is launched, nothing else is looked at
    status, msg = _entry(points=p, acc=p, count=p)
    assert status != 0 and b"null pointer" in msg               # the images, the cameras and the grid, C > 0
    rest = dict(points=p, acc=p, count=p, Ks=p, C2Ws=p, bitmask=p, rank=p, start_num=p, scene_info=p)
    status, msg = _entry(**rest)
    assert status != 0 and b"null pointer" in msg               # images
    status, msg = _entry(images=p, **rest)
    assert status != 0 and b"neither triangles nor an indexed mesh" in msg
    status, msg = _entry(images=p, vertices=p, faces=p, **rest)
    assert status != 0 and b"neither triangles nor an indexed mesh" in msg
    status, msg = _entry(counted=True, images=p, tris=p, **rest)
    assert status != 0 and b"mesh_project_colors_counted: null pointer" in msg      # counters


def test_resolve_colors_refuses_before_any_launch():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    fn = _capi.tool("scanerf_mesh_resolve_colors")
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    p += -p % 16
    fill = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert fn(None, 0, None, None, None, None) == 0
    assert fn(p, -1, fill, p, p, None) != 0 and b"N=-1" in _capi.lib().scanerf_last_error()
    for args in ((None, 3, fill, p, p), (p, 3, None, p, p), (p, 3, fill, None, p), (p, 3, fill, p, None)):
        assert fn(*args, None) != 0 and b"mesh_resolve_colors: null pointer" in _capi.lib().scanerf_last_error()
    assert fn(p + 8, 3, fill, p, p, None) != 0 and b"16-byte aligned" in _capi.lib().scanerf_last_error()


# ---- the Python level -----------------------------------------------------------------------------------------------------------------
def _unbuilt():
    from scanerf_amd.fastmesh import FastMesh
    return FastMesh.__new__(FastMesh)


def test_project_colors_python_refusals():
    import scanerf_amd  # noqa: F401
    fm = _unbuilt()
    pts, img = torch.zeros(5, 3), torch.zeros(1, 4, 4, 3)
    ks, c2ws = torch.eye(3)[None], torch.eye(4)[None, :3]
    with pytest.raises(ValueError, match="route"):
        fm.project_colors(pts, img, ks, c2ws, 0.1, route="grid")
    for bias in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="bias"):
            fm.project_colors(pts, img, ks, c2ws, bias)
    for kw, word in ((dict(near=-0.1), "near"), (dict(near=math.nan), "near"), (dict(far=0.0), "far"), (dict(far=math.nan), "far"),
                     (dict(min_cos=-0.1), "min_cos"), (dict(min_cos=1.0), "min_cos"), (dict(min_cos=math.nan), "min_cos")):
        with pytest.raises(ValueError, match=word):
            fm.project_colors(pts, img, ks, c2ws, 0.1, **kw)
    with pytest.raises(ValueError, match="both or neither"):
        fm.project_colors(pts, img, ks, c2ws, 0.1, acc=torch.zeros(5, 4))
    for bad in (torch.zeros(5, 2), torch.zeros(5, 3, dtype=torch.float64), np.zeros((5, 3), f32)):
        with pytest.raises(RuntimeError, match="points must be"):
            fm.project_colors(bad, img, ks, c2ws, 0.1)
    for bad in (torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="images must be"):
            fm.project_colors(pts, bad, ks, c2ws, 0.1)
    with pytest.raises(RuntimeError, match="normals must be"):
        fm.project_colors(pts, img, ks, c2ws, 0.1, normals=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="acc must be"):
        fm.project_colors(pts, img, ks, c2ws, 0.1, acc=torch.zeros(5, 3), count=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="count must be"):
        fm.project_colors(pts, img, ks, c2ws, 0.1, acc=torch.zeros(5, 4), count=torch.zeros(5))
    for route in ("fused", "composed"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fm.project_colors(pts, img, ks, c2ws, 0.1, route=route)


def test_meshing_and_renderer_refusals():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import meshing, renderer
    V = torch.arange(21, dtype=torch.float32).reshape(7, 3)
    mesh = meshing.Mesh(V, torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32), None, None, None)
    ks, c2ws, img = torch.eye(3)[None], torch.eye(4)[None, :3], torch.zeros(1, 4, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU path|must live on the GPU"):
        meshing.color_from_views(mesh, img, ks, c2ws, 0.1)
    for kw, word in ((dict(route="dense"), "route"), (dict(min_cos=1.0), "min_cos"), (dict(fill=(1, 2)), "fill"), (dict(fill=(0, math.nan, 0)), "fill"),
                     (dict(views_per_batch=0), "views_per_batch"), (dict(views_per_batch=True), "views_per_batch"), (dict(normals="face"), "normals")):
        with pytest.raises(RuntimeError, match=word):
            meshing.color_from_views(mesh, img, ks, c2ws, 0.1, **kw)
    with pytest.raises(RuntimeError, match="images must be"):
        meshing.color_from_views(mesh, torch.zeros(2, 4, 4, 3), ks, c2ws, 0.1)
    with pytest.raises(RuntimeError, match="acc must be"):
        meshing.resolve_colors(torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        meshing.resolve_colors(torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match="fill"):
        meshing.resolve_colors(torch.zeros(5, 4), fill=(1, 2, 3, 4))
    assert meshing.default_edge_bias(mesh) == pytest.approx(0.5 * float(torch.linalg.norm(V[1] - V[0])) * (1 + 1 + 2) / 3)
    with pytest.raises(RuntimeError, match="colors must be None or a callable"):
        meshing.extract_scene_mesh(*[None] * 12, colors="diffuse")
    rnd = renderer.TileSetRenderer.__new__(renderer.TileSetRenderer)      # the checks come before anything of the scene is read
    with pytest.raises(RuntimeError, match="colors must be"):
        rnd.extract_mesh(1.0, colors="specular")
    with pytest.raises(RuntimeError, match="needs cameras"):
        rnd.extract_mesh(1.0, colors="diffuse")
    with pytest.raises(RuntimeError, match="only mean something with colors"):
        rnd.extract_mesh(1.0, color_scale=2)
    with pytest.raises(RuntimeError, match="which must be"):
        rnd.color_mesh(mesh, (ks, c2ws, 4, 4), which="specular")
    with pytest.raises(RuntimeError, match="needs cameras"):
        rnd.color_mesh(mesh, None)


# ---- the commands -----------------------------------------------------------------------------------------------------------------------
def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(f"tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_commands_arguments():
    tool = _tool("color_mesh")
    a = tool.parser().parse_args(["m.ply", "--cameras", "c.log", "--images", "i.npy"])
    assert (a.mesh, a.cameras, a.images, a.out, a.bias, a.min_cos, a.views_per_batch, a.no_normals, a.log2dim) == \
        ("m.ply", "c.log", "i.npy", None, None, 0.0, 8, False, 6) and tuple(a.fill) == (0.5, 0.5, 0.5) and a.far == math.inf
    a = tool.parser().parse_args(["m.ply", "--cameras", "c.log", "--images", "i.npy", "-o", "o.ply", "--min-cos", "0.25", "--bias", "0.1",
                                  "--fill", "0", "0", "1", "--no-normals", "--views-per-batch", "3", "--far", "9"])
    assert (a.out, a.min_cos, a.bias, a.fill, a.no_normals, a.views_per_batch, a.far) == ("o.ply", 0.25, 0.1, [0.0, 0.0, 1.0], True, 3, 9.0)
    for bad in (["m.ply", "--cameras", "c.log"], ["m.ply", "--images", "i.npy"], ["--cameras", "c.log", "--images", "i.npy"]):
        with pytest.raises(SystemExit):
            tool.parser().parse_args(bad)
    for bad in (["--min-cos", "1.0"], ["--min-cos", "-0.5"], ["--views-per-batch", "0"]):
        with pytest.raises(SystemExit):
            tool.main(["m.ply", "--cameras", "c.log", "--images", "i.npy", *bad])      # refused before a file is opened
    scene = _tool("extract_scene_mesh")
    a = scene.parser().parse_args(["t0", "--level", "3", "--out", "o.ply"])
    assert a.colors is None and a.color_scale == 1
    a = scene.parser().parse_args(["t0", "--level", "3", "--out", "o.ply", "--cameras", "c.log", "--colors", "rgb", "--color-scale", "2"])
    assert (a.colors, a.color_scale) == ("rgb", 2)
    with pytest.raises(SystemExit):
        scene.parser().parse_args(["t0", "--level", "3", "--out", "o.ply", "--colors", "specular"])
    with pytest.raises(SystemExit):
        scene.main(["t0", "--level", "3", "--out", "o.ply", "--colors", "diffuse"])      # --colors needs --cameras
