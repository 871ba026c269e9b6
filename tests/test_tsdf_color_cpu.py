"""The colour fusion without a GPU: the numpy reference's own facts (the cap on the flags, float32 against float64
within the derived bounds, the hand-built rows, batch splits, acc untouched by colour, the known answers on the sphere, the uniform
maps), the new entries of the second header against _capi.TOOL_PROTOTYPES, every refusal that happens before a launch, and the PLY
round trip with colours."""
import ctypes
import math

import numpy as np
import pytest
import torch

import tsdf_color_reference as CR
import tsdf_reference as TR

ENTRIES = ("scanerf_tsdf_integrate_color", "scanerf_tsdf_integrate_color_counted", "scanerf_tsdf_vertex_colors")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.SPHERES)
def test_flags_old_and_new_leave_out_at_most_ten_percent(name):
    c = CR.case(name)
    left_out = 1.0 - c["judged"].mean()
    new_only = (c["cref64"]["band"] & TR.case(name)["judged"]).mean()
    print(f"tsdf_color_reference {name}: {len(c['judged'])} points, flagged {100 * left_out:.2f} %, by the band flag alone {100 * new_only:.3f} %")
    assert left_out <= TR.CAP, (name, left_out)
    assert new_only <= 0.001
    free = int(c["cref64"]["acc"][:, 1].sum() - c["cref64"]["cacc"][:, 3].sum())
    print(f"tsdf_color_reference {name}: observed pairs {int(c['cref64']['acc'][:, 1].sum())}, of them not coloured {free}")
    assert c["cref64"]["cacc"][:, 3].max() >= 3 and free > 0      # several cameras colour a point; the band rule leaves pairs out


@pytest.mark.parametrize("name", CR.CASES)
def test_float32_restatement_against_float64(name):
    c = CR.case(name)
    a64, a32, j, bound = c["cref64"]["cacc"], c["cref32"]["cacc"], c["judged"], c["cref64"]["bound"]
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    err = np.abs(a32[:, :3].astype(np.float64) - a64[:, :3])
    worst = (err[j] / np.maximum(bound[j], 1e-300)).max() if j.any() else 0.0
    print(f"tsdf_color_reference {name}: Wc mismatches (all points) {int((a32[:, 3] != a64[:, 3]).sum())}, max |RGB32 - RGB64| judged "
          f"{err[j].max() if j.any() else 0.0:.2e}, max error / bound {worst:.3f}")
    assert np.array_equal(a32[j, 3], a64[j, 3])
    assert (err[j] <= bound[j]).all()
    assert (bound < 1e-3).all() and (bound[a64[:, 3] > 0].max(1) > 0).all()      # a bound, and a float32-sized one


def test_edges_color_rows_equal_their_hand_computed_answers():
    c = CR.case("edges")
    assert len(c["color_rows"]) >= 18 and len(c["ks"]) == 10
    for dtype in (np.float64, np.float32):
        r = CR.integrate(c, dtype, details=True)
        for cam, ijk, observed, coloured, added in c["color_rows"]:
            p = TR.point_index(c["n"], ijk)
            got = (bool(r["observed"][cam, p]), bool(r["coloured"][cam, p]), tuple(float(v) for v in r["added"][cam, p]))
            assert got == (observed, coloured, tuple(float(v) for v in added)), (dtype.__name__, cam, ijk, got)
        for ijk, want in c["color_points"]:
            assert tuple(r["cacc"][TR.point_index(c["n"], ijk)].tolist()) == want, (dtype.__name__, ijk)
        assert not r["coloured"][5].any() and not r["coloured"][6].any()      # looking away; the all-invalid map
        front = np.arange(r["acc"].shape[0]) % (c["n"][2] + 1) == 0           # the layer z = 1: one ulp above +trunc wherever camera 9 sees it
        assert r["observed"][9][front].any() and not r["coloured"][9][front].any() and r["coloured"][9][~front].any()
        p0 = TR.point_index(c["n"], (0, 0, 0))
        assert r["acc"][p0].tolist() == [3.0, 4.0]                            # cameras 0, 2, 8, 9: terms 0, 1, 1, 1
        # the geometry's own hand rows still hold with the tenth camera
        d = TR.integrate(c, dtype, details=True)
        for cam, ijk, inview, observed, term in c["geometry_rows"]:
            p = TR.point_index(c["n"], ijk)
            assert (bool(d["inview"][cam, p]), bool(d["observed"][cam, p]), float(d["term"][cam, p])) == (inview, observed, term)
    assert np.array_equal(c["cref32"]["cacc"].astype(np.float64), c["cref64"]["cacc"])      # every operand is exact
    finite = c["colors"][np.isfinite(c["colors"])]
    assert finite.size < c["colors"].size and finite.min() < 0 and finite.max() > 1


def test_planted_channels_do_work():
    c = CR.case("sphere40")
    assert len(c["planted"]) == CR.PLANTED and int(np.isnan(c["colors"]).sum()) >= 1 and int(np.isinf(c["colors"]).sum()) >= 2
    lost = c["coloured_before_planting"] - int(c["cref64"]["cacc"][:, 3].sum())
    print(f"tsdf_color_reference sphere40: {CR.PLANTED} planted channels take {lost} of {c['coloured_before_planting']} coloured pairs")
    assert lost >= len(set(c["planted"])) and np.isfinite(c["cref64"]["cacc"]).all() and np.isfinite(c["cref32"]["cacc"]).all()


@pytest.mark.parametrize("name", CR.CASES)
def test_batch_splits_give_equal_bits_and_acc_is_unaffected_by_colour(name):
    c = CR.case(name)
    C = len(c["ks"])
    for k in sorted({1, C - 1, C // 2}):
        first = CR.integrate(c, np.float32, cameras=range(0, k))
        both = CR.integrate(c, np.float32, acc=first["acc"], cacc=first["cacc"], cameras=range(k, C))
        for key in ("acc", "cacc"):
            assert both[key].dtype == np.float32 and np.array_equal(_bits(both[key]), _bits(c["cref32"][key])), (name, k, key)
    for dtype, key in ((np.float32, "cref32"), (np.float64, "cref64")):
        plain = TR.integrate(c, dtype)["acc"]
        assert np.array_equal(plain, c[key]["acc"]) and plain.dtype == c[key]["acc"].dtype
    if name != "edges":
        assert np.array_equal(_bits(c["cref32"]["acc"]), _bits(TR.case(name)["ref32"]["acc"]))
    assert (c["cref32"]["cacc"][:, 3] <= c["cref32"]["acc"][:, 1]).all()      # a coloured pair is an observed pair


@pytest.mark.parametrize("name", CR.SPHERES)
def test_vertex_colors_float32_against_float64_and_the_radial_known_answer(name):
    c = CR.case(name)
    raw, mesh = CR.reference_mesh(c)
    assert len(mesh.vertices) > 100
    for what, m in (("culled", mesh), ("raw", raw)):
        v64 = CR.vertex_colors(c["cref32"]["cacc"], c["n"], m.cells, m.lattice, np.float64)
        v32 = CR.vertex_colors(c["cref32"]["cacc"], c["n"], m.cells, m.lattice, np.float32)
        assert v32["rgb"].dtype == np.float32 and v32["weight"].dtype == np.float32 and v64["judged"].all()
        err = np.abs(v32["rgb"].astype(np.float64) - v64["rgb"])
        print(f"tsdf_color_reference {name} {what}: V {len(m.cells)}, max |rgb32 - rgb64| {err.max():.2e}, max error / bound "
              f"{(err / np.maximum(v64['bound'], 1e-300)).max():.3f}, max bound {v64['bound'].max():.2e}")
        assert (err <= v64["bound"]).all() and v64["bound"].max() < 1e-4
        assert (np.abs(v32["weight"].astype(np.float64) - v64["weight"]) <= v64["weight_bound"]).all()
    # every kept vertex (support 8) has a colour, although some kept cells have a corner nobody coloured
    v = CR.vertex_colors(c["cref32"]["cacc"], c["n"], mesh.cells, mesh.lattice, np.float64)
    ok, q = CR._rows(c["n"], mesh.cells)
    holes = int((c["cref32"]["cacc"][q, 3] == 0).any(1).sum())
    assert ok.all() and (v["weight"] > 0).all()
    err = np.abs(v["rgb"] - CR.radial_answer(mesh.vertices)).max(1)
    print(f"tsdf_color_reference {name}: {holes} kept cells with an uncoloured corner; radial colour error max {err.max():.4f} mean {err.mean():.4f} "
          f"(recorded max {CR.RADIAL_MAX[name]})")
    assert err.max() <= CR.RADIAL_MARGIN * CR.RADIAL_MAX[name]


def test_constant_map_gives_the_constant_at_every_coloured_vertex():
    c = CR.uniform("constant")
    cacc = c["cref32"]["cacc"]
    assert np.array_equal(cacc[:, :3], cacc[:, 3:] * np.asarray(CR.CONSTANT, np.float32))      # exact: small integers times binary fractions
    raw, mesh = CR.reference_mesh(c)
    for m in (mesh, raw):
        for dtype in (np.float32, np.float64):
            v = CR.vertex_colors(cacc, c["n"], m.cells, m.lattice, dtype)
            bound = CR.vertex_colors(cacc, c["n"], m.cells, m.lattice, np.float64)["bound"]
            has = v["weight"] > 0
            assert has.sum() > 100 and (np.abs(v["rgb"][has].astype(np.float64) - np.asarray(CR.CONSTANT)) <= bound[has]).all()
            assert (v["rgb"][~has] == 0).all()


def test_camera_index_map_gives_the_mean_index_of_the_colouring_cameras():
    c = CR.uniform("camera_index")
    for dtype in (np.float32, np.float64):
        r = CR.integrate(c, dtype, details=True)
        count = r["coloured"].sum(0)
        total = (r["coloured"] * np.arange(len(c["ks"]))[:, None]).sum(0)
        assert np.array_equal(r["cacc"][:, 3], count) and np.array_equal(r["cacc"][:, 0], total) and not r["cacc"][:, 1:3].any()
        has = count > 0
        mean = total[has] / count[has]      # R / Wc is the mean index of the cameras that coloured the point, to one rounding
        assert has.sum() > 1000 and (np.abs(r["cacc"][has, 0] / r["cacc"][has, 3] - mean) <= 2.0 ** -24 * mean).all()
        assert mean.min() >= 0 and mean.max() <= len(c["ks"]) - 1 and len(np.unique(mean)) > 100


def test_vertex_colors_statement_on_hand_built_cells():
    n = (2, 2, 2)
    cacc = np.zeros((27, 4), np.float32)
    cacc[TR.point_index(n, (0, 0, 0))] = (1.0, 2.0, 4.0, 2.0)
    cacc[TR.point_index(n, (1, 1, 1))] = (3.0, 0.0, -1.0, 1.0)
    cells = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1], [-1, 0, 0], [0, 2, 0], [0, 0, 0], [0, 0, 0]], np.int32)
    lattice = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1.5, 1.5, 1.5], [0.5, 0.5, 0.5], [0.5, 2.5, 0.5], [-3, 0, 0], [0, 7, np.nan]],
                       np.float32)
    for dtype in (np.float32, np.float64):
        v = CR.vertex_colors(cacc, n, cells, lattice, dtype)
        assert v["rgb"][0].tolist() == [0.5, 1.0, 2.0] and v["weight"][0] == 2.0      # t = 0 on every axis: corner 0 alone
        assert v["rgb"][1].tolist() == [3.0, 0.0, -1.0] and v["weight"][1] == 1.0     # t = 1: corner 7 alone
        third = [float(dtype(0.5) / dtype(0.375)), float(dtype(0.25) / dtype(0.375)), 1.0]      # (1 + 3) / 8 over (2 + 1) / 8, ...
        assert v["rgb"][2].tolist() == third and v["weight"][2] == 0.375
        assert v["rgb"][3].tolist() == [3.0, 0.0, -1.0] and v["weight"][3] == 0.125   # cell (1, 1, 1): its corner 0 is point (1, 1, 1)
        assert not v["rgb"][4:6].any() and not v["weight"][4:6].any()                 # outside the lattice
        assert v["rgb"][6].tolist() == [0.5, 1.0, 2.0]                                # t clamped to 0
        assert not v["rgb"][7].any() and v["weight"][7] == 0                          # t = (0, 1, NaN -> 0): corner (0, 1, 0), uncoloured


# ---- the second header ---------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_typed():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    from test_mesh_visibility_cpu import TOOLS_HEADER, _prototypes
    hdr = _prototypes(TOOLS_HEADER)
    so = ctypes.CDLL(_capi.LIB_PATH)
    for name in ENTRIES:
        assert name in hdr and name in _capi.TOOL_PROTOTYPES and tuple(_capi.TOOL_PROTOTYPES[name]) == hdr[name], name
        assert hasattr(so, name), name
    plain, color = _capi.TOOL_PROTOTYPES["scanerf_tsdf_integrate"][1], _capi.TOOL_PROTOTYPES["scanerf_tsdf_integrate_color"][1]
    assert color == "P" + plain[:-1] + "PP"      # colors after depths, cacc after acc


# ---- the entries' refusals, before any launch (host buffers: nothing reads them before the refusal) ----------------------------------------
def _aligned(buf):
    return (ctypes.addressof(buf) + 15) & ~15


def _integrate_color(counted=False, **over):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    buf = ctypes.create_string_buffer(256 + 16)
    p = _aligned(buf)
    o, s = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    a = dict(depths=p, colors=p, Ks=p, C2Ws=p, C=2, H=8, W=8, origin=o, spacing=s, nx=4, ny=4, nz=4, trunc=0.5, near=0.0, far=math.inf,
             acc=p, cacc=p)
    if counted:
        a["counters"] = p
    if over.pop("misaligned", False):
        a["cacc"] = p + 4
    a.update(over)
    name = "scanerf_tsdf_integrate_color" + ("_counted" if counted else "")
    status = _capi.tool(name)(*a.values(), None)
    return status, _capi.lib().scanerf_last_error(), buf.raw


def test_integrate_color_entries_refuse_before_any_launch():
    bad3 = lambda *v: (ctypes.c_float * 3)(*v)
    cases = [({"depths": None}, b"null pointer"), ({"colors": None}, b"null pointer"), ({"Ks": None}, b"null pointer"),
             ({"C2Ws": None}, b"null pointer"), ({"acc": None}, b"null pointer"), ({"cacc": None}, b"null pointer"),
             ({"origin": None}, b"null pointer"), ({"spacing": None}, b"null pointer"),
             ({"C": -1}, b"C=-1"), ({"H": 0}, b"H=0"), ({"W": 0}, b"W=0"), ({"nx": 0}, b"n=(0"), ({"ny": -2}, b"-2"),
             ({"nz": 0}, b"n=(4, 4, 0)"), ({"nx": 2047, "ny": 2047, "nz": 2047}, b"2^31"),
             ({"trunc": 0.0}, b"trunc=0"), ({"trunc": -1.0}, b"trunc=-1"), ({"trunc": math.inf}, b"trunc=inf"), ({"trunc": math.nan}, b"trunc="),
             ({"near": -0.5}, b"near=-0.5"), ({"near": math.nan}, b"near="), ({"near": 2.0, "far": 2.0}, b"far=2"), ({"far": math.nan}, b"far="),
             ({"spacing": bad3(1, 0, 1)}, b"spacing[1]=0"), ({"spacing": bad3(math.inf, 1, 1)}, b"spacing[0]=inf"),
             ({"origin": bad3(0, math.inf, 0)}, b"origin[1]=inf")]
    for counted in (False, True):
        tag = b"tsdf_integrate_color_counted" if counted else b"tsdf_integrate_color:"
        for over, text in cases:
            status, msg, raw = _integrate_color(counted, **over)
            assert status != 0 and text in msg and tag in msg, (counted, over, msg)
            assert raw == bytes(len(raw))
        status, msg, raw = _integrate_color(counted, misaligned=True)
        assert status != 0 and b"16-byte aligned" in msg and tag in msg
        assert _integrate_color(counted, C=0)[0] == 0                  # nothing to add: no launch (the buffers are host memory)
    status, msg, raw = _integrate_color(True, counters=None)
    assert status != 0 and b"tsdf_integrate_color_counted: null pointer" in msg


def test_vertex_colors_entry_refuses_before_any_launch():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    err = lambda: _capi.lib().scanerf_last_error()
    buf = ctypes.create_string_buffer(64 + 16)
    p = _aligned(buf)
    colors = _capi.tool("scanerf_tsdf_vertex_colors")
    for args, text in (((None, 4, 4, 4, p, p, 3, p, p), b"null pointer"), ((p, 4, 4, 4, None, p, 3, p, p), b"null pointer"),
                       ((p, 4, 4, 4, p, None, 3, p, p), b"null pointer"), ((p, 4, 4, 4, p, p, 3, None, p), b"null pointer"),
                       ((p, 4, 4, 4, p, p, 3, p, None), b"null pointer"), ((p, 4, 4, 4, p, p, -1, p, p), b"V=-1"),
                       ((p, 0, 4, 4, p, p, 3, p, p), b"n=(0"), ((p, 4, -1, 4, p, p, 3, p, p), b"n=(4, -1"), ((p, 4, 4, 0, p, p, 3, p, p), b"n=(4, 4, 0)"),
                       ((p, 2047, 2047, 2047, p, p, 3, p, p), b"2^31"), ((p + 8, 4, 4, 4, p, p, 3, p, p), b"16-byte aligned")):
        assert colors(*args, None) != 0 and text in err() and b"tsdf_vertex_colors" in err(), args
    assert colors(p, 4, 4, 4, p, p, 0, p, p, None) == 0      # V == 0: no launch
    assert buf.raw == bytes(len(buf.raw))


# ---- the Python level ----------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import fusion, meshing
    ok = dict(origin=[0, 0, 0], spacing=[1, 1, 1], n=[2, 2, 2], trunc=1.0, device="cpu")
    for bad in (1, "yes", None):
        with pytest.raises(RuntimeError, match="scanerf: color must be True or False"):
            fusion.TSDFVolume(**ok, color=bad)
    plain, vol = fusion.TSDFVolume(**ok), fusion.TSDFVolume(**ok, color=True)
    assert plain.cacc is None and vol.cacc.shape == (27, 4) and vol.cacc.dtype == torch.float32 and not vol.cacc.any()
    assert vol.acc.shape == (27, 2)      # a volume on the CPU can be described; nothing can be done with it
    depths, ks, c2ws = torch.zeros(2, 4, 4), torch.eye(3).repeat(2, 1, 1), torch.eye(4)[:3].repeat(2, 1, 1)
    colors = torch.zeros(2, 4, 4, 3)
    with pytest.raises(RuntimeError, match="needs colors="):
        vol.integrate(depths, ks, c2ws)
    with pytest.raises(RuntimeError, match="a volume without takes none"):
        plain.integrate(depths, ks, c2ws, colors=colors)
    for bad in (torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, 4), torch.zeros(1, 4, 4, 3), torch.zeros(2, 4, 5, 3),
                torch.zeros(2, 4, 4, 3, dtype=torch.float64), np.zeros((2, 4, 4, 3), np.float32)):
        with pytest.raises(RuntimeError, match="scanerf: colors must be a \\[2, 4, 4, 3\\] float32 tensor"):
            vol.integrate(depths, ks, c2ws, colors=bad)
    with pytest.raises(RuntimeError, match="depths"):
        vol.integrate(torch.zeros(2, 4), ks, c2ws, colors=colors)
    with pytest.raises(RuntimeError, match="route"):
        vol.integrate(depths, ks, c2ws, colors=colors, route="dense")
    for route in fusion.ROUTES:
        with pytest.raises(RuntimeError, match="no CPU path"):
            vol.integrate(depths, ks, c2ws, colors=colors, route=route)
    mesh = meshing.Mesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32), torch.zeros((4, 3), dtype=torch.int32), torch.zeros(4, 3), None)
    bare = meshing.Mesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32), None, None, None)
    with pytest.raises(RuntimeError, match="vertex_colors needs a volume with colour"):
        plain.vertex_colors(mesh)
    with pytest.raises(RuntimeError, match="needs mesh.cells and mesh.lattice"):
        vol.vertex_colors(bare)
    for bad in (math.nan, math.inf, None, "grey", True):
        with pytest.raises(RuntimeError, match="fill"):
            vol.vertex_colors(mesh, fill=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.vertex_colors(mesh)
    with pytest.raises(RuntimeError, match="needs a volume with colour"):
        plain.extract(colors=True)
    with pytest.raises(RuntimeError, match="colors must be True or False"):
        vol.extract(colors="rgb")
    with pytest.raises(RuntimeError, match="min_weight"):
        vol.extract(min_weight=0, colors=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.extract(colors=True)
    box = ([0, 0, 0], [1, 1, 1], [2, 2, 2])
    for bad in (torch.zeros(2, 4, 4), torch.zeros(1, 4, 4, 3), np.zeros((2, 4, 4, 3), np.float32)):
        with pytest.raises(RuntimeError, match="colors must be a \\[C,H,W,3\\] float32 tensor"):
            fusion.fuse_depth_maps(depths, ks, c2ws, *box, colors=bad)
    with pytest.raises(RuntimeError, match="colors must be a \\[2, 4, 4, 3\\] float32 tensor"):
        fusion.fuse_depth_maps(depths, ks, c2ws, *box, colors=torch.zeros(2, 4, 4, 3, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.fuse_depth_maps(depths, ks, c2ws, *box, colors=colors)
    img = fusion.clamped_image(torch.tensor([[-1.0, 0.25, 2.0]]), torch.tensor([[0.5, 0.5, math.nan]]))
    assert img[0, :2].tolist() == [0.0, 0.75] and math.isnan(float(img[0, 2]))
    assert fusion.clamped_image(torch.tensor([[-1.0, 0.25, 2.0]])).tolist() == [[0.0, 0.25, 1.0]]


def test_fuse_mesh_refuses_an_unknown_colour_source():
    import scanerf_amd  # noqa: F401
    from scanerf_amd.renderer import TileSetRenderer
    r = TileSetRenderer.__new__(TileSetRenderer)      # the check comes before anything of the renderer is read
    ks, c2ws = torch.eye(3)[None], torch.eye(4)[None, :3]
    for bad in ("specular", True, 1, "RGB"):
        with pytest.raises(RuntimeError, match="colors must be None, 'diffuse' or 'rgb'"):
            r.fuse_mesh((ks, c2ws, 8, 8), colors=bad)
    for good in ("diffuse", "rgb"):
        with pytest.raises(RuntimeError, match="needs cameras"):
            r.fuse_mesh(None, colors=good)


def test_the_command_knows_the_option():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuse_mesh.py")
    spec = importlib.util.spec_from_file_location("fuse_mesh_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.parser()
    head = ["tile", "--cameras", "camera.log", "--out", "x.ply"]
    assert ap.parse_args(head).colors is None
    assert ap.parse_args(head + ["--colors", "diffuse"]).colors == "diffuse" and ap.parse_args(head + ["--colors", "rgb"]).colors == "rgb"
    with pytest.raises(SystemExit):
        ap.parse_args(head + ["--colors", "specular"])


# ---- the PLY round trip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("with_normals", [False, True])
def test_ply_round_trip_with_colors(tmp_path, binary, with_normals):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import formats
    rng = np.random.default_rng(5)
    V, F = rng.normal(size=(7, 3)).astype(np.float32), rng.integers(0, 7, (4, 3)).astype(np.int32)
    N = rng.normal(size=(7, 3)).astype(np.float32) if with_normals else None
    C = np.array([[0.0, 1.0, 0.5], [-0.25, 1.5, 0.25], [0.1, 0.2, 0.3], [0.999, 0.001, 0.498], [1.0, 1.0, 1.0], [0.5 / 255, 1.5 / 255, 254.4 / 255],
                  [1e-9, 1 - 1e-9, 0.75]], np.float32)
    want = np.array([[0, 255, 128], [0, 255, 64], [26, 51, 77], [255, 0, 127], [255, 255, 255], [1, 2, 254], [0, 255, 191]], np.uint8)
    assert np.array_equal(want, np.floor(np.clip(C.astype(np.float64), 0, 1) * 255 + 0.5).astype(np.uint8))
    assert np.array_equal(formats.quantize_colors(C), want)
    path = str(tmp_path / "c.ply")
    formats.write_ply(path, V, F, binary=binary, normals=N, colors=C)
    header = open(path, "rb").read().split(b"end_header")[0].decode()
    props = [ln.split()[-1] for ln in header.splitlines() if ln.startswith("property") and "list" not in ln]
    assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + ["red", "green", "blue"]
    assert header.count("property uchar") == 3
    got = formats.read_ply(path, normals=with_normals, colors=True)
    assert len(got) == 3 + with_normals and got[-1].dtype == np.uint8 and np.array_equal(got[-1], want)
    assert np.array_equal(got[0], V) and np.array_equal(got[1], F)
    if with_normals:
        assert np.array_equal(got[2], N)
    plain = formats.read_ply(path, normals=with_normals)      # a reader that does not ask for the colours skips them
    assert len(plain) == 2 + with_normals and np.array_equal(plain[0], V) and np.array_equal(plain[1], F)
    # a torch tensor's numpy view, float64 input
    formats.write_ply(path, V, F, binary=binary, normals=N, colors=C.astype(np.float64))
    assert np.array_equal(formats.read_ply(path, colors=True)[-1], want)


def test_ply_color_refusals(tmp_path):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import formats
    V, F = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    path = str(tmp_path / "r.ply")
    for bad in (math.nan, math.inf, -math.inf):
        C = np.full((3, 3), 0.5)
        C[1, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            formats.write_ply(path, V, F, colors=C)
    import os
    assert not os.path.exists(path)      # refused before the file is opened
    with pytest.raises(ValueError, match="do not match vertices"):
        formats.write_ply(path, V, F, colors=np.zeros((2, 3)))
    for binary in (True, False):
        formats.write_ply(path, V, F, binary=binary, normals=np.ones((3, 3), np.float32))
        with pytest.raises(ValueError, match="lacks one of"):
            formats.read_ply(path, colors=True)
        with pytest.raises(ValueError, match="lacks one of"):
            formats.read_ply(path, normals=True, colors=True)
        formats.write_ply(path, V, F, binary=binary, colors=np.zeros((3, 3)))
        with pytest.raises(ValueError, match="lacks one of"):
            formats.read_ply(path, normals=True, colors=True)
