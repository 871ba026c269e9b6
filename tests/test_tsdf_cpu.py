"""The depth-map fusion without a GPU: the numpy reference's own facts (the cap on the flags, float32 against float64
within the derived bound, the hand-built rows, batch splits, camera order, the known answers on the sphere), the second header's new
entries against _capi.TOOL_PROTOTYPES, and every refusal that happens before a launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mesh_components_reference as MC
import surface_nets_reference as SN
import tsdf_reference as TR

SPHERES = ("sphere6", "sphere40", "sphere70")
ENTRIES = ("scanerf_tsdf_cameras_per_pass", "scanerf_tsdf_integrate", "scanerf_tsdf_integrate_counted", "scanerf_tsdf_values",
           "scanerf_tsdf_cell_support")


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SPHERES)
def test_flags_leave_out_at_most_ten_percent(name):
    c = TR.case(name)
    left_out = 1.0 - c["judged"].mean()
    print(f"tsdf_reference {name}: {len(c['judged'])} points, flagged {100 * left_out:.2f} %")
    assert left_out <= TR.CAP, (name, left_out)
    assert c["ref64"]["acc"][:, 1].max() >= 3      # the case observes something, several times


@pytest.mark.parametrize("name", TR.CASES)
def test_float32_restatement_against_float64(name):
    c = TR.case(name)
    a64, a32, j = c["ref64"]["acc"], c["ref32"]["acc"], c["judged"]
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    err = np.abs(a32[:, 0].astype(np.float64) - a64[:, 0])
    print(f"tsdf_reference {name}: Wt mismatches (all points) {int((a32[:, 1] != a64[:, 1]).sum())}, max |S32 - S64| judged "
          f"{err[j].max() if j.any() else 0.0:.2e}, max error / bound {(err[j] / np.maximum(c['ref64']['bound'][j], 1e-300)).max() if j.any() else 0.0:.3f}")
    assert np.array_equal(a32[j, 1], a64[j, 1])
    assert (err[j] <= c["ref64"]["bound"][j]).all()
    assert (c["ref64"]["bound"][a64[:, 1] > 0] > 0).all() and (c["ref64"]["bound"] < 1e-3).all()      # a bound, and a float32-sized one


def test_edges_rows_equal_their_hand_computed_answers():
    c = TR.case("edges")
    assert len(c["ks"]) > 0 and len(c["rows"]) >= 20
    for dtype in (np.float64, np.float32):
        r = TR.integrate(c, dtype, details=True)
        for cam, ijk, inview, observed, term in c["rows"]:
            p = TR.point_index(c["n"], ijk)
            got = (bool(r["inview"][cam, p]), bool(r["observed"][cam, p]), float(r["term"][cam, p]))
            assert got == (inview, observed, term), (dtype.__name__, cam, ijk, got)
        assert not r["inview"][5].any()               # the camera that looks away sees nothing
        assert r["inview"][6].any() and not r["observed"][6].any()      # the all-invalid map: in view, never observed
    # float32 and float64 agree in every bit of this case: every operand is exact
    assert np.array_equal(c["ref32"]["acc"].astype(np.float64), c["ref64"]["acc"])


@pytest.mark.parametrize("name", TR.CASES)
def test_batch_splits_give_equal_bits(name):
    c = TR.case(name)
    C = len(c["ks"])
    for k in sorted({1, C - 1, C // 2}):
        first = TR.integrate(c, np.float32, cameras=range(0, k))["acc"]
        both = TR.integrate(c, np.float32, acc=first, cameras=range(k, C))["acc"]
        assert both.dtype == np.float32 and np.array_equal(both.view(np.uint32), c["ref32"]["acc"].view(np.uint32)), (name, k)


@pytest.mark.parametrize("name", SPHERES)
def test_camera_order_matters_only_through_float_addition(name):
    c = TR.case(name)
    order = np.random.default_rng(1).permutation(len(c["ks"]))
    for dtype in (np.float32, np.float64):
        again = TR.integrate(c, dtype, cameras=order)["acc"]
        ref = c["ref32" if dtype is np.float32 else "ref64"]["acc"]
        assert np.array_equal(again[:, 1], ref[:, 1])                    # Wt: a count
        assert np.abs(again[:, 0] - ref[:, 0]).max() <= 2.0 * c["ref64"]["bound"].max()


def _fused_reference_mesh(c, min_weight=1.0):
    val, obs = TR.values(c["ref32"]["acc"], min_weight)
    shape = [m + 1 for m in c["n"]]
    raw = SN.surface_nets(val.reshape(shape), 0.5, c["origin"], c["spacing"], dtype=np.float64)
    support = TR.cell_support(obs.reshape(shape), c["n"], raw.cells)
    return raw, support, TR.support_cull(raw, support), obs.reshape(shape)


@pytest.mark.parametrize("name", SPHERES)
def test_known_answers_on_the_sphere(name):
    c = TR.case(name)
    raw, support, mesh, obs = _fused_reference_mesh(c)
    h = max(c["spacing"])
    assert len(mesh.vertices) > 100
    radial = np.abs(np.linalg.norm(mesh.vertices, axis=1) - TR.RADIUS) / h
    closed, chi, vol = SN.topology(mesh)
    n_comp = len(MC.components(mesh.faces, len(mesh.vertices)).label)
    print(f"tsdf_reference {name}: raw V {len(raw.vertices)} -> culled V {len(mesh.vertices)} F {len(mesh.faces)}, components {n_comp}, "
          f"closed {closed}, chi {chi}, volume {vol:.3f} (exact {4 / 3 * math.pi * TR.RADIUS ** 3:.3f}), max radial error {radial.max():.3f} spacings")
    assert radial.max() <= 1.0, "a vertex lies more than one lattice spacing from the sphere"
    if name != "sphere6":
        assert closed and chi == 2 and n_comp == 1
        assert abs(vol - 4 / 3 * math.pi * TR.RADIUS ** 3) < 0.1 * 4 / 3 * math.pi * TR.RADIUS ** 3
    else:
        assert not closed      # six cameras leave gaps: the cull keeps what is surrounded by observation only


@pytest.mark.parametrize("name", SPHERES)
def test_support_cull_removes_exactly_the_unsupported(name):
    c = TR.case(name)
    raw, support, mesh, obs = _fused_reference_mesh(c)
    assert support.min() >= 0 and support.max() == 8 and (support < 8).any()
    # every kept vertex has support 8: no kept cell touches an unobserved corner
    kept = TR.cell_support(obs, c["n"], mesh.cells)
    assert (kept == 8).all()
    # nothing else went: a face all of whose vertices have support 8 is kept, in order
    f = raw.faces.astype(np.int64)
    full = (support == 8)[f].all(1)
    assert len(mesh.faces) == int(full.sum())
    assert np.array_equal(mesh.vertices[mesh.faces], raw.vertices[f[full]])
    used = np.zeros(len(raw.vertices), bool)
    used[f[full].reshape(-1)] = True
    assert np.array_equal(mesh.cells, raw.cells[used])
    assert TR.cell_support(obs, c["n"], np.array([[-1, 0, 0], [0, c["n"][1], 0]])).tolist() == [0, 0]


def test_values_statement():
    acc = np.array([[0, 0], [1, 1], [-1, 1], [0.5, 2], [3, 4], [-2, 2]], np.float32)
    val, obs = TR.values(acc, 1)
    assert obs.tolist() == [False, True, True, True, True, True] and val.tolist() == [0.0, 0.0, 1.0, 0.375, 0.125, 1.0]
    val, obs = TR.values(acc, 2)
    assert obs.tolist() == [False, False, False, True, True, True] and val.tolist() == [0.0, 0.0, 0.0, 0.375, 0.125, 1.0]


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
    per_pass = _capi.tool("scanerf_tsdf_cameras_per_pass")()
    assert 1 <= per_pass < len(TR.case("sphere70")["ks"])      # the 70-camera case takes more than one pass


# ---- the entries' refusals, before any launch (host buffers: nothing reads them before the refusal) ----------------------------------------
def _integrate(**over):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    o, s = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    a = dict(depths=p, Ks=p, C2Ws=p, C=2, H=8, W=8, origin=o, spacing=s, nx=4, ny=4, nz=4, trunc=0.5, near=0.0, far=math.inf, acc=p)
    a.update(over)
    status = _capi.tool("scanerf_tsdf_integrate")(*a.values(), None)
    return status, _capi.lib().scanerf_last_error(), buf.raw


def test_integrate_entry_refuses_before_any_launch():
    bad3 = lambda *v: (ctypes.c_float * 3)(*v)
    for over, text in (({"depths": None}, b"null pointer"), ({"Ks": None}, b"null pointer"), ({"C2Ws": None}, b"null pointer"),
                       ({"acc": None}, b"null pointer"), ({"origin": None}, b"null pointer"), ({"spacing": None}, b"null pointer"),
                       ({"C": -1}, b"C=-1"), ({"H": 0}, b"H=0"), ({"W": 0}, b"W=0"), ({"nx": 0}, b"n=(0"), ({"ny": -2}, b"-2"),
                       ({"nz": 0}, b"n=(4, 4, 0)"), ({"nx": 2047, "ny": 2047, "nz": 2047}, b"2^31"),
                       ({"nx": 2 ** 31 - 1, "ny": 2 ** 31 - 1, "nz": 2 ** 31 - 1}, b"2^31"),
                       ({"trunc": 0.0}, b"trunc=0"), ({"trunc": -1.0}, b"trunc=-1"), ({"trunc": math.inf}, b"trunc=inf"),
                       ({"trunc": math.nan}, b"trunc="), ({"near": -0.5}, b"near=-0.5"), ({"near": math.nan}, b"near="),
                       ({"near": 2.0, "far": 2.0}, b"far=2"), ({"far": math.nan}, b"far="), ({"far": 0.0}, b"far=0"),
                       ({"spacing": bad3(1, 0, 1)}, b"spacing[1]=0"), ({"spacing": bad3(1, 1, -1)}, b"spacing[2]=-1"),
                       ({"spacing": bad3(math.inf, 1, 1)}, b"spacing[0]=inf"), ({"spacing": bad3(1, math.nan, 1)}, b"spacing[1]="),
                       ({"origin": bad3(0, math.inf, 0)}, b"origin[1]=inf")):
        status, msg, raw = _integrate(**over)
        assert status != 0 and text in msg and b"tsdf_integrate" in msg, (over, msg)
        assert raw == bytes(256)
    assert _integrate(C=0)[0] == 0                  # nothing to add: no launch (the buffers are host memory)


def test_other_entries_refuse_before_any_launch():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    err = lambda: _capi.lib().scanerf_last_error()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    o, s = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    counted = _capi.tool("scanerf_tsdf_integrate_counted")
    assert counted(p, p, p, 2, 8, 8, o, s, 4, 4, 4, 0.5, 0.0, 1.0, p, None, None) != 0 and b"tsdf_integrate_counted: null pointer" in err()
    values = _capi.tool("scanerf_tsdf_values")
    for args, text in (((None, 5, 1.0, p, p), b"null pointer"), ((p, 5, 1.0, None, p), b"null pointer"), ((p, 5, 1.0, p, None), b"null pointer"),
                       ((p, -1, 1.0, p, p), b"P=-1"), ((p, 5, 0.5, p, p), b"min_weight=0.5"), ((p, 5, 0.0, p, p), b"min_weight=0"),
                       ((p, 5, math.nan, p, p), b"min_weight=")):
        assert values(*args, None) != 0 and text in err() and b"tsdf_values" in err(), args
    assert values(p, 0, 1.0, p, p, None) == 0
    support = _capi.tool("scanerf_tsdf_cell_support")
    for args, text in (((None, 4, 4, 4, p, 3, p), b"null pointer"), ((p, 4, 4, 4, None, 3, p), b"null pointer"),
                       ((p, 4, 4, 4, p, 3, None), b"null pointer"), ((p, 4, 4, 4, p, -1, p), b"V=-1"), ((p, 0, 4, 4, p, 3, p), b"n=(0"),
                       ((p, 2047, 2047, 2047, p, 3, p), b"2^31")):
        assert support(*args, None) != 0 and text in err() and b"tsdf_cell_support" in err(), args
    assert support(p, 4, 4, 4, p, 0, p, None) == 0
    assert buf.raw == bytes(64)


# ---- the Python level ----------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import fusion, meshing
    ok = dict(origin=[0, 0, 0], spacing=[1, 1, 1], n=[2, 2, 2], trunc=1.0, device="cpu")
    for over, text in (({"n": [2, 2]}, "3 cell counts"), ({"n": [0, 2, 2]}, "n_k"), ({"n": [2047, 2047, 2047]}, "2\\^31"),
                       ({"spacing": [1, 0, 1]}, "spacing"), ({"spacing": [1, math.inf, 1]}, "spacing"), ({"spacing": [1, 1]}, "spacing"),
                       ({"origin": [0, math.nan, 0]}, "origin"), ({"trunc": 0.0}, "trunc"), ({"trunc": -1.0}, "trunc"),
                       ({"trunc": math.inf}, "trunc"), ({"trunc": math.nan}, "trunc")):
        with pytest.raises(RuntimeError, match="scanerf: .*" + text):
            fusion.TSDFVolume(**{**ok, **over})
    vol = fusion.TSDFVolume(**ok)      # a volume on the CPU can be described; nothing can be done with it
    assert vol.acc.shape == (27, 2) and not vol.acc.any() and vol.shape == (3, 3, 3)
    depths, ks, c2ws = torch.zeros(2, 4, 4), torch.eye(3).repeat(2, 1, 1), torch.eye(4)[:3].repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="route"):
        vol.integrate(depths, ks, c2ws, route="dense")
    for near in (-0.1, math.nan):
        with pytest.raises(RuntimeError, match="near"):
            vol.integrate(depths, ks, c2ws, near=near)
    for near, far in ((0.0, 0.0), (1.0, 0.5), (0.0, math.nan)):
        with pytest.raises(RuntimeError, match="far"):
            vol.integrate(depths, ks, c2ws, near=near, far=far)
    for bad in (torch.zeros(2, 4), torch.zeros(2, 4, 4, dtype=torch.float64), np.zeros((2, 4, 4), np.float32), torch.zeros(2, 0, 4)):
        with pytest.raises(RuntimeError, match="depths"):
            vol.integrate(bad, ks, c2ws)
    with pytest.raises(RuntimeError, match="2 depth maps but 1 cameras"):
        vol.integrate(depths, ks[:1], c2ws[:1])
    with pytest.raises(RuntimeError, match="ks must be"):
        vol.integrate(depths, torch.zeros(2, 9), c2ws)
    for route in fusion.ROUTES:
        with pytest.raises(RuntimeError, match="no CPU path"):
            vol.integrate(depths, ks, c2ws, route=route)
    for bad in (0, 0.5, -1, True, None, math.nan):
        with pytest.raises(RuntimeError, match="min_weight"):
            vol.values(bad)
        with pytest.raises(RuntimeError, match="min_weight"):
            vol.extract(min_weight=bad)
        with pytest.raises(RuntimeError, match="min_weight"):
            fusion.fuse_depth_maps(depths, ks, c2ws, [0, 0, 0], [1, 1, 1], [2, 2, 2], min_weight=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.values()
    with pytest.raises(RuntimeError, match="min_faces"):
        vol.extract(min_faces=-1)
    with pytest.raises(RuntimeError, match="keep_largest"):
        vol.extract(keep_largest=1.5)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(RuntimeError, match="views_per_batch"):
            fusion.fuse_depth_maps(depths, ks, c2ws, [0, 0, 0], [1, 1, 1], [2, 2, 2], views_per_batch=bad)
        with pytest.raises(RuntimeError, match="scale"):
            fusion.scale_cameras(ks, bad)
    with pytest.raises(RuntimeError, match="box_size"):
        fusion.fuse_depth_maps(depths, ks, c2ws, [0, 0, 0], [1, 0, 1], [2, 2, 2])
    with pytest.raises(RuntimeError, match="trunc"):
        fusion.fuse_depth_maps(depths, ks, c2ws, [0, 0, 0], [1, 1, 1], [2, 2, 2], trunc=0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.fuse_depth_maps(depths, ks, c2ws, [0, 0, 0], [1, 1, 1], [2, 2, 2])
    mesh = meshing.Mesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32), None, None, None)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(4), [8] * 4):
        with pytest.raises(RuntimeError, match="support must be an integer tensor"):
            fusion.support_cull(mesh, bad)
    assert fusion.default_trunc([0.5, 0.25, 1.0]) == 4.0
    k2 = fusion.scale_cameras(torch.tensor([[[30.0, 0, 16], [0, 60, 9], [0, 0, 1]]]), 3)
    assert torch.equal(k2, torch.tensor([[[10.0, 0, np.float32(16) / np.float32(3)], [0, 20, 3], [0, 0, 1]]]))


def test_support_cull_rule_on_a_hand_built_mesh():
    """torch on the CPU: the rule is not the hot path and runs wherever its tensors live."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd import fusion, meshing
    V = torch.arange(21, dtype=torch.float32).reshape(7, 3)
    F = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 5, 6], [1, 2, 3]], dtype=torch.int32)
    mesh = meshing.Mesh(V, F, (V * 2).to(torch.int32), V + 0.5, None)
    report = {}
    out = fusion.support_cull(mesh, torch.tensor([8, 8, 8, 8, 7, 8, 8], dtype=torch.int32), report)
    assert out.faces.tolist() == [[0, 1, 2], [1, 2, 3]] and torch.equal(out.vertices, V[:4]) and torch.equal(out.cells, mesh.cells[:4])
    assert torch.equal(out.lattice, mesh.lattice[:4]) and out.normals is None
    assert report == {"vertices": (7, 4), "faces": (4, 2), "support_histogram": [0, 0, 0, 0, 0, 0, 0, 1, 6]}
    out = fusion.support_cull(mesh, torch.full((7,), 8, dtype=torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(out[:4], mesh[:4]))
    out = fusion.support_cull(mesh, torch.zeros(7, dtype=torch.int32))
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3)
    # against the numpy statement
    rng = np.random.default_rng(3)
    Vn, Fn = rng.normal(size=(40, 3)).astype(np.float32), rng.integers(0, 40, (70, 3)).astype(np.int32)
    sup = rng.choice([6, 7, 8, 8, 8, 8, 8, 8], 40).astype(np.int32)
    ref = TR.support_cull(SN.Mesh(Vn, Fn, Vn.astype(np.int32), Vn), sup)
    out = fusion.support_cull(meshing.Mesh(torch.from_numpy(Vn), torch.from_numpy(Fn), None, None, None), torch.from_numpy(sup))
    assert np.array_equal(out.vertices.numpy(), ref.vertices) and np.array_equal(out.faces.numpy(), ref.faces)


def test_fuse_mesh_refusals():
    import scanerf_amd  # noqa: F401
    from scanerf_amd.renderer import TileSetRenderer
    r = TileSetRenderer.__new__(TileSetRenderer)      # the checks below come before anything of the renderer is read
    ks, c2ws = torch.eye(3)[None], torch.eye(4)[None, :3]
    with pytest.raises(RuntimeError, match="needs cameras"):
        r.fuse_mesh(None)
    with pytest.raises(RuntimeError, match="needs cameras"):
        r.fuse_mesh((ks, c2ws, 8))
    for bad in (0, 1.5, True):
        with pytest.raises(RuntimeError, match="scale"):
            r.fuse_mesh((ks, c2ws, 8, 8), scale=bad)
        with pytest.raises(RuntimeError, match="views_per_batch"):
            r.fuse_mesh((ks, c2ws, 8, 8), views_per_batch=bad)
    with pytest.raises(RuntimeError, match="leave no pixel"):
        r.fuse_mesh((ks, c2ws, 8, 8), scale=16)
    with pytest.raises(RuntimeError, match="max_transparency"):
        r.fuse_mesh((ks, c2ws, 8, 8), max_transparency=1.5)
    with pytest.raises(RuntimeError, match="min_weight"):
        r.fuse_mesh((ks, c2ws, 8, 8), min_weight=0)
    with pytest.raises(RuntimeError, match="min_extent"):
        r.fuse_mesh((ks, c2ws, 8, 8), min_extent=-1)
    with pytest.raises(RuntimeError, match="c2ws must be"):
        r.fuse_mesh((ks, torch.eye(4)[None, :2], 8, 8))
