"""The point-visibility op without a GPU: the float64 reference's own facts, the float32 restatement against it, the
cull rule, the second public header against _capi.TOOL_PROTOTYPES, and every refusal that happens before a launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_visibility_reference as MV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS_HEADER = os.path.join(ROOT, "include", "scanerf_mesh_tools_hip.h")
SAMPLE = slice(1, None, 4)      # the terrain rows that are recomputed here (625 of 2 497: ~3 s instead of ~10 s)

CASES = {"terrain": MV.terrain, "terrain_small_bias": lambda: MV.terrain(MV.SMALL_BIAS), "nested": MV.nested,
         "nested_extra": lambda: MV.nested(True), "edges": MV.edges, "many_cameras": MV.many_cameras}


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_terrain_facts():
    """The definition on the terrain, 2 497 vertices x 8 cameras at 102 x 134: the counts of the issue, at both biases."""
    for bias in (MV.TERRAIN_BIAS, MV.SMALL_BIAS):
        case = MV.terrain(bias)
        assert case["points"].shape == (2497, 3) and case["F"].shape == (4752, 3) and len(case["ks"]) == 8
        assert MV.census(case) == (19976, 9092, 4102, 4990, 19, 907), (bias, MV.census(case))


@pytest.mark.parametrize("name", sorted(CASES))
def test_ambiguous_pairs_are_at_most_one_percent_of_the_pairs_in_view(name):
    case = CASES[name]()
    pairs, inview, seen, hidden, ambiguous, _ = MV.census(case)
    print(f"mesh_visibility_reference {name}: pairs {pairs} in view {inview} seen {seen} hidden {hidden} ambiguous {ambiguous}")
    assert inview > 0 and seen > 0 and hidden > 0
    assert ambiguous <= 0.01 * inview, (name, ambiguous, inview)
    r = case["ref"]
    assert not (r["seen"] & ~r["inview"]).any() and (r["lo"] <= r["hi"]).all()


def test_recorded_reference_is_what_the_module_computes():
    """tests/golden/g23_mesh_visibility.npz holds the brute force's result for the large cases; a sample of the rows from scratch."""
    for case in (MV.terrain(), MV.terrain(MV.SMALL_BIAS)):
        assert str(MV._golden().get(case["name"] + ".digest")) == MV._digest(case), "the record is not this case's: run make_golden_mesh_visibility.py"
        rows = SAMPLE if case["bias"] == MV.TERRAIN_BIAS else slice(3, None, 16)
        again = MV.recompute(case, rows)
        for k in MV._KEYS:
            assert np.array_equal(again[k], case["ref"][k][rows]), (case["name"], k)
    many = MV.many_cameras()
    assert str(MV._golden().get("many_cameras.digest")) == MV._digest(many)
    again = MV.recompute(many, slice(0, None, 6))
    for k in MV._KEYS:
        assert np.array_equal(again[k], many["ref"][k][::6]), k
    assert many["ref"]["seen"].shape == (MV.MANY_POINTS, MV.MANY_CAMERAS) and MV.pack_mask(many["ref"]["seen"]).shape[1] == 3
    for c in (31, 32, 63, 64):      # the word seams carry both answers
        col = many["ref"]["seen"][:, c]
        assert col.any() and not col.all(), c


def _float32(case, rows=slice(None)):
    return MV.evaluate(case["points"][rows], case["ks"], case["c2ws"], case["H"], case["W"], case["bias"], case["V"], case["F"], case["near"],
                       case["far"], dtype=np.float32)


@pytest.mark.parametrize("name", ["terrain", "nested", "nested_extra", "edges"])
def test_float32_restatement_equals_float64_outside_the_ambiguous_set(name):
    """On these cases it equals float64 in EVERY pair (the terrain: on the sampled rows here, on all rows when the record was made)."""
    case = CASES[name]()
    rows = SAMPLE if name == "terrain" else slice(None)
    r32, r64 = _float32(case, rows), case["ref"]
    differ = r32["seen"] != r64["seen"][rows]
    assert not (differ & ~r64["ambiguous"][rows]).any()
    assert not differ.any()
    assert np.array_equal(r32["inview"], r64["inview"][rows])


def test_nested_facts():
    case = MV.nested()
    r, no = case["ref"], case["n_outer"]
    assert len(case["points"]) - no == MV.NESTED_INNER == 8 and len(case["F"]) - case["f_outer"] == 12 and len(case["ks"]) == 8
    assert not r["ambiguous"].any()
    assert (r["hi"][no:] == 0).all(), "an inner vertex is seen from outside"
    assert (r["lo"][:no] >= 1).all(), "an outer vertex no camera clearly sees"
    views = r["seen"].sum(1)
    V2, F2, _ = MV.cull(case["V"], case["F"], views, 1)
    assert np.array_equal(V2, case["V"][:no]) and np.array_equal(F2, case["F"][:case["f_outer"]])
    extra = MV.nested(True)
    r = extra["ref"]
    facing = extra["V"][no:, 0] == extra["V"][no:, 0].max()
    assert facing.sum() == 4 and np.array_equal(r["seen"][no:, 8], facing) and not r["seen"][no:, :8].any()
    assert not r["ambiguous"][no:].any()


def test_edges_reference_gives_the_answers_worked_out_by_hand():
    case = MV.edges()
    assert np.array_equal(case["ref"]["seen"], case["expected"])
    assert not case["ref"]["ambiguous"].any()
    assert case["expected"][:, 0].sum() == 2 and not np.isfinite(case["points"]).all()


def test_mask_packing():
    seen = np.zeros((3, 65), bool)
    seen[0, [0, 31, 32, 64]] = True
    seen[2, 63] = True
    m = MV.pack_mask(seen)
    assert m.dtype == np.uint32 and m.tolist() == [[0x80000001, 1, 1], [0, 0, 0], [0, 0x80000000, 0]]
    assert np.array_equal(MV.unpack_mask(m.view(np.int32), 65), seen)


# ---- the cull rule ------------------------------------------------------------------------------------------------------------------
def _hand_mesh():
    from scanerf_amd import meshing
    V = torch.arange(21, dtype=torch.float32).reshape(7, 3)
    F = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 5, 6], [1, 2, 3]], dtype=torch.int32)
    return meshing.Mesh(V, F, (V * 2).to(torch.int32), V + 0.5, -V)


def test_cull_rule_on_hand_built_views():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import meshing
    mesh = _hand_mesh()
    views = torch.tensor([0, 0, 0, 0, 0, 2, 1], dtype=torch.int32)
    report = {}
    out = meshing.cull_by_views(mesh, views, 1, report)
    # only face 2 = (4, 5, 6) has a vertex with a view; vertices 4, 5, 6 stay, in order, remapped to 0, 1, 2
    assert out.faces.dtype == torch.int32 and out.faces.tolist() == [[0, 1, 2]]
    for name in ("vertices", "cells", "lattice", "normals"):
        assert torch.equal(getattr(out, name), getattr(mesh, name)[4:7]), name
    assert report == {"vertices": (7, 3), "faces": (4, 1), "views_histogram": [5, 1, 1]}
    out = meshing.cull_by_views(mesh, views, 2)
    assert out.faces.tolist() == [[0, 1, 2]] and torch.equal(out.vertices, mesh.vertices[4:7])
    # one seen vertex keeps every face that uses it, and those faces keep their other vertices
    out = meshing.cull_by_views(mesh, torch.tensor([0, 0, 0, 5, 0, 0, 0]), 1)
    assert out.faces.tolist() == [[1, 2, 3], [0, 1, 2]] and torch.equal(out.vertices, mesh.vertices[1:5])
    assert torch.equal(out.cells, mesh.cells[1:5])
    out = meshing.cull_by_views(mesh, torch.zeros(7, dtype=torch.int32), 1)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.normals.shape == (0, 3)
    for k in (3, 6):
        got = meshing.cull_by_views(mesh, views + 3, k)
        if k == 3:
            assert all(torch.equal(a, b) for a, b in zip(got, mesh))
        else:
            assert got.faces.shape[0] == 0
    partial = mesh._replace(cells=None, normals=None)
    out = meshing.cull_by_views(partial, views, 1)
    assert out.cells is None and out.normals is None and torch.equal(out.lattice, mesh.lattice[4:7])
    # against the numpy statement of the rule
    rng = np.random.default_rng(5)
    Vn, Fn = rng.normal(size=(40, 3)).astype(np.float32), rng.integers(0, 40, (70, 3)).astype(np.int32)
    vw = rng.integers(0, 3, 40).astype(np.int32)
    for k in (1, 2, 3):
        V2, F2, _ = MV.cull(Vn, Fn, vw, k)
        out = meshing.cull_by_views(meshing.Mesh(torch.from_numpy(Vn), torch.from_numpy(Fn), None, None, None), torch.from_numpy(vw), k)
        assert np.array_equal(out.vertices.numpy(), V2) and np.array_equal(out.faces.numpy(), F2)


def test_min_views_zero_is_the_identity():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import meshing
    mesh = _hand_mesh()
    assert meshing.cull_by_views(mesh, torch.zeros(7, dtype=torch.int32), 0) is mesh
    assert meshing.cull_unseen(mesh, None, None, 4, 4, min_views=0, bias=0.1) is mesh      # no camera is looked at, nothing launched


# ---- the second header --------------------------------------------------------------------------------------------------------------
def _code(path):
    """test_capi_cpu._header_code's two substitutions on another file."""
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
    return re.sub(r"^\s*#.*$", "", hdr, flags=re.M)


def _prototypes(path):
    """test_capi_cpu._header_prototypes' expression and its _alias on another file: name -> (return letter, argument letters)."""
    from test_capi_cpu import _alias
    out = {}
    for ret, name, args in re.findall(r"([\w\s*]+?)\b(scanerf_\w+)\s*\(([^)]*)\)\s*;", _code(path)):
        args = [] if args.strip() in ("", "void") else args.split(",")
        out[name] = (_alias(ret), "".join(_alias(a) for a in args))
    return out


def test_tool_prototypes_match_the_second_header():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    from test_capi_cpu import _declared_symbols
    hdr = _prototypes(TOOLS_HEADER)
    text = re.sub(r"/\*.*?\*/", "", open(TOOLS_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(scanerf_[a-z0-9_]+)\s*\(", text)))
    assert len(hdr) == len(declared) >= 3
    assert set(hdr) == set(_capi.TOOL_PROTOTYPES), sorted(set(hdr) ^ set(_capi.TOOL_PROTOTYPES))
    bad = {n: (hdr[n], _capi.TOOL_PROTOTYPES[n]) for n in hdr if hdr[n] != tuple(_capi.TOOL_PROTOTYPES[n])}
    assert not bad, bad
    # the two headers (and the two tables) share no name: scanerf_hip.h's set is what ABI version 10 pins
    assert not set(hdr) & set(_declared_symbols())
    assert not set(_capi.TOOL_PROTOTYPES) & set(_capi.PROTOTYPES)
    assert not set(_capi.TOOL_PROTOTYPES) & (set(_capi.SYMBOLS) | set(_capi.OPTIONAL_SYMBOLS))
    so = ctypes.CDLL(_capi.LIB_PATH)
    missing = [n for n in hdr if not hasattr(so, n)]
    assert not missing, missing
    assert so.scanerf_abi_version() == 10
    # the stream comes last in every launching entry, as in the first header
    for n, (ret, args) in hdr.items():
        assert ret == "I" and (args == "" or args.endswith("P")), n
    per_pass = _capi.tool("scanerf_mesh_point_views_cameras_per_pass")()
    assert per_pass >= 32 and per_pass % 32 == 0 and per_pass < MV.MANY_CAMERAS      # the many-cameras case takes two passes
    with pytest.raises(TypeError, match="scanerf_mesh_point_views"):
        _capi.tool("scanerf_mesh_point_views")(1, 2)
    with pytest.raises(KeyError):
        _capi.tool("scanerf_mesh_first_hit")      # the first header's entries are lib()'s


def test_no_call_site_reaches_the_tools_through_lib():
    """Every use of a second-header entry in the package, tests/ and tools/ goes through _capi.tool(name): an attribute call
    `<x>.scanerf_mesh_point_views(...)` would be a name test_capi_cpu's call-site check cannot look up."""
    import ast
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    paths = []
    for top in (_capi._HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
        paths += [os.path.join(d, f) for d, _, fs in os.walk(top) for f in fs if f.endswith(".py")]
    used = 0
    for path in paths:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.Attribute) and node.attr in _capi.TOOL_PROTOTYPES:
                raise AssertionError(f"{os.path.relpath(path, ROOT)}:{node.lineno} reaches {node.attr} as an attribute")
            if (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "tool" or
                    isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "tool"):
                if node.args and isinstance(node.args[0], ast.Constant) and node.args[0].value in _capi.TOOL_PROTOTYPES:
                    used += 1
    assert used >= 3


# ---- the entry's refusals, before any launch ----------------------------------------------------------------------------------------
def _entry(**over):
    """scanerf_mesh_point_views on null pointers with valid scalars, one thing changed -> (status, message)."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    a = dict(points=None, N=4, Ks=None, C2Ws=None, C=2, H=8, W=8, bias=0.1, near=0.0, far=math.inf, vertices=None, faces=None, tris=None,
             bitmask=None, rank=None, start_num=None, cell_faces=None, scene_info=None, log2dim=6, views=None, mask=None)
    a.update(over)
    status = _capi.tool("scanerf_mesh_point_views")(*a.values(), None)
    return status, _capi.lib().scanerf_last_error()


def test_entry_refuses_before_any_launch():
    for over, text in (({}, b"null pointer"), ({"H": 0}, b"H=0"), ({"W": 0}, b"W=0"), ({"H": -3}, b"H=-3"), ({"log2dim": 3}, b"log2dim=3"),
                       ({"log2dim": 8}, b"log2dim=8"), ({"bias": 0.0}, b"bias=0"), ({"bias": -1.0}, b"bias=-1"), ({"bias": math.inf}, b"bias=inf"),
                       ({"bias": math.nan}, b"bias="), ({"near": -0.5}, b"near=-0.5"), ({"near": math.nan}, b"near="), ({"far": 0.0}, b"far=0"),
                       ({"far": -2.0}, b"far=-2"), ({"far": math.nan}, b"far="), ({"N": -1}, b"N=-1"), ({"C": -1}, b"C=-1")):
        status, msg = _entry(**over)
        assert status != 0 and text in msg and b"mesh_point_views" in msg, (over, msg)
    assert _entry(N=0)[0] == 0                                   # a no-op, whatever else is passed
    assert _entry(N=0, H=0, log2dim=3)[0] == 0
    # some pointers given (host buffers: nothing reads them before the refusal), others missing
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    status, msg = _entry(points=p)
    assert status != 0 and b"null pointer" in msg                # views
    status, msg = _entry(points=p, views=p)
    assert status != 0 and b"null pointer" in msg                # the cameras and the grid, C > 0
    status, msg = _entry(points=p, views=p, Ks=p, C2Ws=p, bitmask=p, rank=p, start_num=p, scene_info=p)
    assert status != 0 and b"neither triangles nor an indexed mesh" in msg
    status, msg = _entry(points=p, views=p, Ks=p, C2Ws=p, bitmask=p, rank=p, start_num=p, scene_info=p, vertices=p, faces=p)
    assert status != 0 and b"neither triangles nor an indexed mesh" in msg     # cell_faces names the faces of the indexed form
    from scanerf_amd import _capi
    counted = _capi.tool("scanerf_mesh_point_views_counted")
    args = [p, 4, p, p, 2, 8, 8, 0.1, 0.0, math.inf, None, None, p, p, p, p, None, p, 6, p, None]
    assert counted(*args, None, None) != 0 and b"mesh_point_views_counted: null pointer" in _capi.lib().scanerf_last_error()      # counters


# ---- the Python level ---------------------------------------------------------------------------------------------------------------
def _unbuilt():
    from scanerf_amd.fastmesh import FastMesh
    return FastMesh.__new__(FastMesh)      # the checks below come before anything of the tracer is read


def test_point_views_refusals():
    import scanerf_amd  # noqa: F401
    fm = _unbuilt()
    pts = torch.zeros(5, 3)
    ks, c2ws = torch.eye(3)[None], torch.eye(4)[None, :3]
    ok = dict(H=8, W=8, bias=0.1)
    with pytest.raises(ValueError, match="route"):
        fm.point_views(pts, ks, c2ws, route="grid", **ok)
    for bias in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="bias"):
            fm.point_views(pts, ks, c2ws, 8, 8, bias)
    for near in (-0.1, math.nan):
        with pytest.raises(ValueError, match="near"):
            fm.point_views(pts, ks, c2ws, near=near, **ok)
    for far in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="far"):
            fm.point_views(pts, ks, c2ws, far=far, **ok)
    for hw in ((0, 8), (8, 0), (8.5, 8), (True, 8)):
        with pytest.raises(ValueError, match="positive integer"):
            fm.point_views(pts, ks, c2ws, hw[0], hw[1], 0.1)
    for bad in (torch.zeros(5, 2), torch.zeros(5, 3, dtype=torch.float64), torch.zeros(15)):
        with pytest.raises(RuntimeError, match=r"points must be \[N,3\] float32"):
            fm.point_views(bad, ks, c2ws, **ok)
    for route in ("fused", "composed"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fm.point_views(pts, ks, c2ws, route=route, **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.point_views(np.zeros((5, 3), np.float32), ks, c2ws, **ok)


def test_meshing_refusals():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import meshing
    mesh = _hand_mesh()
    ks, c2ws = torch.eye(3)[None], torch.eye(4)[None, :3]
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.vertex_views(mesh, ks, c2ws, 8, 8, 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.cull_unseen(mesh, ks, c2ws, 8, 8, min_views=1, bias=0.1)
    with pytest.raises(RuntimeError, match="route"):
        meshing.vertex_views(mesh, ks, c2ws, 8, 8, 0.1, route="dense")
    with pytest.raises(RuntimeError, match="route"):
        meshing.cull_unseen(mesh, ks, c2ws, 8, 8, bias=0.1, route="brute")
    with pytest.raises(RuntimeError, match="needs bias"):
        meshing.cull_unseen(mesh, ks, c2ws, 8, 8)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(RuntimeError, match="min_views"):
            meshing.cull_unseen(mesh, ks, c2ws, 8, 8, min_views=bad, bias=0.1)
        with pytest.raises(RuntimeError, match="min_views"):
            meshing.cull_by_views(mesh, torch.zeros(7, dtype=torch.int32), bad)
    for bad in (torch.zeros(6, dtype=torch.int32), torch.zeros(7), [0] * 7):
        with pytest.raises(RuntimeError, match="views must be an integer tensor"):
            meshing.cull_by_views(mesh, bad, 1)
    # the extractors check the view rule with their other rules, before anything is read
    for fn, n_args in ((meshing.extract_mesh, 10), (meshing.extract_scene_mesh, 12)):
        args = [None] * n_args
        with pytest.raises(RuntimeError, match="needs cameras"):
            fn(*args, min_views=1)
        with pytest.raises(RuntimeError, match="needs cameras"):
            fn(*args, min_views=1, cameras=(ks, c2ws, 8))
        with pytest.raises(RuntimeError, match="min_views"):
            fn(*args, min_views=-1)
        with pytest.raises(RuntimeError, match="view_bias"):
            fn(*args, cameras=(ks, c2ws, 8, 8), min_views=1, view_bias=0.0)
        with pytest.raises(RuntimeError, match="view_far"):
            fn(*args, cameras=(ks, c2ws, 8, 8), min_views=1, view_far=-1.0)
    assert meshing.default_view_bias([4.0, 2.0, 8.0], [8, 8, 8]) == 0.125

