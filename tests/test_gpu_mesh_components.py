"""Mesh components and the filter by component on the GPU (csrc/mesh_components.hip; meshing.mesh_components / filter_mesh and the
extractors' rules).  Every quantity is an integer: the fused route equals the composed route and the numpy reference
(tests/mesh_components_reference.py) bit for bit -- labels, table and filtered mesh -- and a second fused run gives the same bits."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_components_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _same(got, want, what):
    """Two tuples of arrays / tensors / None: the same fields, dtypes, shapes and bits."""
    assert got._fields == want._fields
    for k in got._fields:
        a, b = getattr(got, k), getattr(want, k)
        a, b = (_np(a) if isinstance(a, torch.Tensor) else a), (_np(b) if isinstance(b, torch.Tensor) else b)
        if a is None or b is None:
            assert a is None and b is None, (what, k)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (what, k)


def _gpu(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV).contiguous()      # (a copy: the cases are read-only arrays)


@functools.lru_cache(maxsize=None)
def lattice_mesh(name):
    """The case extracted on the GPU through meshing.surface_nets, its host copy and the reference's components of THAT mesh --
    computed once per process, never written to."""
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    mesh = meshing.surface_nets(_gpu(R.lattice_cases()[name]), R.LEVEL)
    host = R.Mesh(_np(mesh.vertices), _np(mesh.faces), _np(mesh.cells), _np(mesh.lattice), None)
    return mesh, host, R.components(host.faces, len(host.vertices), host.cells)


# ---------------------------------------------------------------------------------------------------------------- lattice cases
@pytest.mark.parametrize("name", list(R.lattice_cases()))
def test_lattice_cases_fused_composed_and_reference_agree(name):
    from scanerf_amd import meshing
    mesh, host, want = lattice_mesh(name)
    V = len(host.vertices)
    ref_mesh, ref = R.lattice_reference(name)          # the numpy extraction: another vertex order, the same components
    assert V == len(ref_mesh.vertices) and sorted(want.n_faces.tolist()) == sorted(ref.n_faces.tolist())
    fused = meshing.mesh_components(mesh.faces, V, mesh.cells)
    _same(fused, want, name)
    _same(meshing.mesh_components(mesh.faces, V, mesh.cells, route="composed"), want, name + " composed")
    _same(meshing.mesh_components(mesh.faces, V, mesh.cells), fused, name + " again")
    bare = meshing.mesh_components(mesh.faces, V)
    assert bare.cell_min is None and bare.cell_max is None and torch.equal(bare.labels, fused.labels) and torch.equal(bare.n_faces, fused.n_faces)
    if len(host.faces):
        again = meshing.mesh_components(_gpu(R.permuted(host.faces, 5)), V, mesh.cells)
        _same(again, want, name + " permuted")
    for rules in R.RULES:
        want_mesh = R.filter_mesh(host, rules)
        got = meshing.filter_mesh(mesh, *rules)
        _same(got, want_mesh, (name, rules))
        _same(meshing.filter_mesh(mesh, *rules, route="composed"), want_mesh, (name, rules, "composed"))
        _same(meshing.filter_mesh(mesh, *rules), got, (name, rules, "again"))
    assert meshing.filter_mesh(mesh) is mesh           # the default rule: the input itself


def test_known_answers_on_the_gpu():
    from scanerf_amd import meshing
    mesh, host, _ = lattice_mesh("three")
    out = meshing.filter_mesh(mesh, keep_largest=2)
    closed, chi, _ = R.topology_of(R.Mesh(*(_np(t) for t in out)))
    assert closed and chi == 4 and out.faces.shape[0] == 1548 + 1540
    mesh, host, want = lattice_mesh("twin")
    out = meshing.filter_mesh(mesh, keep_largest=1)
    assert np.array_equal(_np(out.vertices), host.vertices[want.labels == want.label[0]]) and want.label[0] < want.label[1]
    mesh, host, _ = lattice_mesh("value-equals-level")
    out = meshing.filter_mesh(mesh, min_faces=1)
    assert out.vertices.shape[0] == len(host.vertices) - 9 and out.faces.shape[0] == len(host.faces)
    assert np.array_equal(_np(out.vertices)[_np(out.faces)], host.vertices[host.faces])


# ---------------------------------------------------------------------------------------------------------------- synthetic graphs
GRAPH_RULES = [R.Rules(keep_largest=1), R.Rules(min_faces=2), R.Rules(min_extent=40, keep_largest=3), R.Rules(min_faces=1)]


@pytest.mark.parametrize("name", list(R.graph_cases()))
def test_synthetic_graphs(name):
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    faces, V = R.graph_cases()[name]
    want = R.graph_reference(name)
    cells = R.graph_cells(V)
    f, c = _gpu(faces), _gpu(cells)
    fused = meshing.mesh_components(f, V, c)
    _same(fused, want, name)
    _same(meshing.mesh_components(f, V, c, route="composed"), want, name + " composed")
    _same(meshing.mesh_components(f, V, c), fused, name + " again")
    for seed in (1, 2):
        again = meshing.mesh_components(_gpu(R.permuted(faces, seed)), V, c)
        assert torch.equal(again.labels, fused.labels), (name, seed)
        _same(again, want, (name, "permuted", seed))
    # the filter with all four per-vertex arrays present
    rng = np.random.default_rng(23)
    host = R.Mesh(rng.uniform(size=(V, 3)).astype(np.float32), faces, cells, rng.uniform(size=(V, 3)).astype(np.float32),
                  rng.normal(size=(V, 3)).astype(np.float32))
    mesh = meshing.Mesh(*(_gpu(a) for a in host))
    for rules in GRAPH_RULES:
        want_mesh = R.filter_mesh(host, rules)
        _same(meshing.filter_mesh(mesh, *rules), want_mesh, (name, rules))
        _same(meshing.filter_mesh(mesh, *rules, route="composed"), want_mesh, (name, rules, "composed"))


def test_no_vertices():
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    faces = torch.empty((0, 3), dtype=torch.int32, device=DEV)
    for route in meshing.COMPONENT_ROUTES:
        c = meshing.mesh_components(faces, 0, route=route)
        assert c.labels.shape == (0,) and c.label.shape == (0,) and c.n_faces.shape == (0,) and c.cell_min is None and c.labels.dtype == torch.int32
        c = meshing.mesh_components(faces, 0, cells=torch.empty((0, 3), dtype=torch.int32, device=DEV), route=route)
        assert c.cell_min.shape == (0, 3) and c.cell_max.shape == (0, 3)
        e = torch.empty((0, 3), device=DEV)
        mesh = meshing.Mesh(e, faces, torch.empty((0, 3), dtype=torch.int32, device=DEV), e, None)
        out = meshing.filter_mesh(mesh, min_faces=1, keep_largest=1, route=route)
        assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.normals is None


def test_meshing_refuses_gpu_arguments_before_any_library_call(monkeypatch):
    import scanerf_amd  # noqa
    from scanerf_amd import meshing

    def refuse():
        raise AssertionError("the library was called before the arguments were refused")
    monkeypatch.setattr(meshing, "lib", refuse)
    faces = torch.tensor([[0, 1, 2], [2, 3, 9]], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="outside"):
        meshing.mesh_components(faces, 9)
    with pytest.raises(RuntimeError, match="outside"):
        meshing.mesh_components(faces - 1, 10)
    with pytest.raises(RuntimeError, match="dtype"):
        meshing.mesh_components(faces.to(torch.int64), 10)
    with pytest.raises(RuntimeError, match=r"\[F,3\]"):
        meshing.mesh_components(faces.reshape(-1), 10)
    with pytest.raises(RuntimeError, match="contiguous"):
        meshing.mesh_components(faces.t().contiguous().t(), 10)
    with pytest.raises(RuntimeError, match="cells must be"):
        meshing.mesh_components(faces, 10, cells=torch.zeros((9, 3), dtype=torch.int32, device=DEV))
    v = torch.zeros((10, 3), device=DEV)
    mesh = meshing.Mesh(v, faces, None, v, None)
    with pytest.raises(RuntimeError, match="min_extent needs"):
        meshing.filter_mesh(mesh, min_extent=2)
    with pytest.raises(RuntimeError, match="mesh.lattice"):
        meshing.filter_mesh(mesh._replace(lattice=v[:5]), min_faces=1)
    with pytest.raises(RuntimeError, match="outside"):
        meshing.filter_mesh(mesh._replace(vertices=v[:9], lattice=v[:9]), min_faces=1)
    with pytest.raises(RuntimeError, match="non-negative"):
        meshing.filter_mesh(mesh, keep_largest=-1)


# ---------------------------------------------------------------------------------------------------------------- the C entry points
def test_guard_regions_exact_rows_and_outputs_declared_too_small():
    """The C entry points on caller-owned buffers prefilled with a sentinel: labels, the table, and exactly V' / F' rows are written,
    nothing before or behind them and nothing outside the scratch; with V' or F' declared too small the call reports an error and
    writes nothing at all."""
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    lib = _capi.lib()
    mesh, host, want = lattice_mesh("sparse-noise")
    V, F = len(host.vertices), len(host.faces)
    G = 256
    nbytes = lib.scanerf_mesh_components_scratch_bytes(V, F)
    scratch = torch.full((nbytes + 2 * G,), 0x5A, dtype=torch.uint8, device=DEV)
    sp = scratch.data_ptr() + G
    scratch_guards = lambda: bool((scratch[:G] == 0x5A).all()) and bool((scratch[G + nbytes:] == 0x5A).all())

    def guarded(rows, width, fill, dtype):
        return torch.full((rows * width + 2 * G,), fill, dtype=dtype, device=DEV)
    body = lambda t: t[G:-G]
    inner = lambda t: t.data_ptr() + t.element_size() * G
    holds = lambda t, fill: bool((t[:G] == fill).all()) and bool((t[-G:] == fill).all())

    labels = guarded(V, 1, -7, torch.int32)
    _capi.check(lib.scanerf_mesh_components_label(mesh.faces.data_ptr(), V, F, inner(labels), sp, nbytes, _capi.stream()), "label")
    C = int(scratch[G:G + 8].view(torch.int64).item())
    assert C == len(want.label) and scratch_guards() and holds(labels, -7)
    assert np.array_equal(_np(body(labels)), want.labels)

    table = {k: guarded(C, w, -7, torch.int32) for k, w in (("label", 1), ("n_vertices", 1), ("n_faces", 1), ("cell_min", 3), ("cell_max", 3))}
    _capi.check(lib.scanerf_mesh_components_table(mesh.faces.data_ptr(), mesh.cells.data_ptr(), inner(labels), V, F, sp, nbytes, C,
                                                  *(inner(t) for t in table.values()), _capi.stream()), "table")
    assert scratch_guards() and all(holds(t, -7) for t in table.values())
    by_label = np.argsort(want.label)                   # the library's rows: ascending label
    for k, t in table.items():
        assert np.array_equal(_np(body(t)).reshape(getattr(want, k).shape), getattr(want, k)[by_label]), k

    rules = R.Rules(min_faces=2, keep_largest=40)
    keep_ranked = R.kept_rows(want, rules)
    keep = _gpu(keep_ranked[by_label].astype(np.uint8))
    expect = R.filter_mesh(host, rules)
    Vk, Fk = len(expect.vertices), len(expect.faces)
    assert 0 < Vk < V and 0 < Fk < F
    head = (mesh.faces.data_ptr(), inner(labels), keep.data_ptr(), V, F, C, sp, nbytes)
    _capi.check(lib.scanerf_mesh_filter_count(*head, _capi.stream()), "count")
    assert scratch[G + 8:G + 24].view(torch.int64).tolist() == [Vk, Fk] and scratch_guards()
    normals = torch.rand((V, 3), device=DEV)

    def buffers(Vo, Fo):
        return {"vertices": guarded(Vo, 3, 7.0, torch.float32), "faces": guarded(Fo, 3, -7, torch.int32), "cells": guarded(Vo, 3, -7, torch.int32),
                "lattice": guarded(Vo, 3, 7.0, torch.float32), "normals": guarded(Vo, 3, 7.0, torch.float32)}

    def emit(b, Vo, Fo):
        status = lib.scanerf_mesh_filter_emit(*head, mesh.vertices.data_ptr(), mesh.cells.data_ptr(), mesh.lattice.data_ptr(),
                                              normals.data_ptr(), inner(b["vertices"]), inner(b["faces"]), inner(b["cells"]),
                                              inner(b["lattice"]), inner(b["normals"]), Vo, Fo, _capi.stream())
        torch.cuda.synchronize()
        return status

    full = buffers(Vk, Fk)
    assert emit(full, Vk, Fk) == 0
    fill = lambda t: 7.0 if t.dtype == torch.float32 else -7
    assert scratch_guards() and all(holds(t, fill(t)) for t in full.values())
    expect = expect._replace(normals=_np(normals)[np.isin(want.labels, want.label[keep_ranked])])
    for k, t in full.items():
        assert np.array_equal(_np(body(t)).reshape(-1, 3).view(np.int32), getattr(expect, k).view(np.int32)), k     # every row written
    for Vo, Fo in ((Vk - 1, Fk), (Vk, Fk - 1), (Vk - 1, Fk - 1)):
        small = buffers(Vo, Fo)
        assert emit(small, Vo, Fo) != 0
        assert b"V'=" in lib.scanerf_last_error() and str(Vk).encode() in lib.scanerf_last_error()
        assert scratch_guards() and all(bool((t == fill(t)).all()) for t in small.values())            # nothing was written anywhere


# ---------------------------------------------------------------------------------------------------------------- integration
def _scene_args():
    import scene_mesh_reference as M
    from test_gpu_scene_mesh import _case_args
    return M, _case_args(M.CASES[0])


def test_the_scene_extraction_filters_before_its_normals():
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    M, args = _scene_args()
    plain = meshing.extract_scene_mesh(**args, normals=True)
    report = {}
    got = meshing.extract_scene_mesh(**args, normals=True, keep_largest=1, report=report)
    want = meshing.filter_mesh(plain, keep_largest=1)
    _same(got, want, "scene keep_largest=1")             # normals: the gathered rows of the unfiltered normals, bit for bit
    comps = meshing.mesh_components(plain.faces, plain.vertices.shape[0], plain.cells)
    assert report["components"] == comps.label.shape[0] and report["kept_components"] == 1
    assert report["vertices"] == (plain.vertices.shape[0], got.vertices.shape[0]) and report["faces"] == (plain.faces.shape[0], got.faces.shape[0])
    assert got.faces.shape[0] == int(comps.n_faces[0]) and got.vertices.shape[0] == int(comps.n_vertices[0])
    no_normals = meshing.extract_scene_mesh(**args, keep_largest=1)
    assert no_normals.normals is None and torch.equal(no_normals.faces, got.faces)
    same = meshing.extract_scene_mesh(**args, normals=True)
    _same(same, plain, "default rules")
    dense = meshing.extract_scene_mesh(**args, normals=False, keep_largest=1, route="dense")
    _same(dense, no_normals, "dense route, composed filter")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_commands_with_a_rule(tmp_path, capsys):
    """tools/extract_scene_mesh.py and tools/extract_mesh.py once each with a rule: the PLY read back is the library's filtered mesh,
    and the component count and the rows before and after are printed."""
    import render_scenes as RS
    from scanerf_amd import formats, renderer
    M, _ = _scene_args()
    sc = M.scene("G9")
    dirs = []
    for b, tile in enumerate(RS.renderer_tiles(sc)):
        path = str(tmp_path / f"tile-{b}")
        os.makedirs(path)
        t = torch.as_tensor
        renderer.write_feature_npz(path, t(tile["features"]), t(tile["occupied_grid"]), t(tile["block_corner"]), t(tile["block_size"]),
                                   t(tile["grid_log2dim"]), t(tile["resolution"]))
        torch.save(dict(M.O.unpack_blob(torch.from_numpy(tile["blob"]))), os.path.join(path, "decoder.pth"))
        dirs.append(path)
    level = M.reference(M.CASES[0])[6]
    rnd = renderer.TileSetRenderer(DEV, [renderer.load_tile(p) for p in dirs])
    out = str(tmp_path / "scene.ply")
    assert _tool("extract_scene_mesh").main([*dirs, "--level", repr(level), "--cells-per-axis", "20", "--out", out, "--keep-largest", "1",
                                             "--normals"]) == 0
    want = rnd.extract_mesh(level, cells_per_axis=20, keep_largest=1, normals=True)
    plain = rnd.extract_mesh(level, cells_per_axis=20)
    assert 0 < want.vertices.shape[0] <= plain.vertices.shape[0]
    ply = formats.read_ply(out)
    assert np.array_equal(np.asarray(ply[0], np.float32), _np(want.vertices)) and np.array_equal(np.asarray(ply[1], np.int32), _np(want.faces))
    printed = capsys.readouterr().out
    assert "components" in printed and f"vertices {plain.vertices.shape[0]} -> {want.vertices.shape[0]}" in printed
    assert f"faces {plain.faces.shape[0]} -> {want.faces.shape[0]}" in printed
    # one tile, unused vertices dropped
    tool = _tool("extract_mesh")
    assert tool.main([dirs[0], "--level", repr(level), "--cells-per-axis", "24", "--out", str(tmp_path / "out"), "--min-faces", "1"]) == 0
    tile = renderer.load_tile(dirs[0])
    plain = tool.extract_tile(tile, 24, level, DEV)
    want = tool.extract_tile(tile, 24, level, DEV, min_faces=1)
    assert plain.vertices.shape[0] > 0
    used = torch.zeros(plain.vertices.shape[0], dtype=torch.bool, device=DEV)
    used[plain.faces.reshape(-1).long()] = True
    assert want.vertices.shape[0] == int(used.sum()) and torch.equal(want.vertices, plain.vertices[used])
    tv, tf = formats.read_ply(str(tmp_path / "out" / "tile-0.ply"))[:2]
    assert np.array_equal(np.asarray(tv, np.float32), _np(want.vertices)) and np.array_equal(np.asarray(tf, np.int32), _np(want.faces))
    printed = capsys.readouterr().out
    assert "components" in printed and f"vertices {plain.vertices.shape[0]} -> {want.vertices.shape[0]}" in printed
