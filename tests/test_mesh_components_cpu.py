"""Mesh components and the filter by component without a GPU: the numpy reference of
tests/mesh_components_reference.py on cases that hold the condition each is named for, its known answers and invariances, and the
part of the library's surface that needs no device -- the prototypes, the C entry points' refusals, and meshing's refusals, every
one of them raised before a library call."""
import os

import numpy as np
import pytest
import torch

import mesh_components_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the cases hold
def test_three_spheres_give_three_components():
    mesh, c = R.lattice_reference("three")
    assert c.n_faces.tolist() == [1548, 1540, 72] and int(c.n_vertices.sum()) == len(mesh.vertices)
    assert c.label[0] == 0 and np.array_equal(c.labels[c.label], c.label)
    ext = (c.cell_max - c.cell_min + 1).max(1)
    assert ext.tolist() == [14, 14, 4]


def test_twin_spheres_tie():
    _, c = R.lattice_reference("twin")
    assert c.n_faces.tolist() == [1548, 1548] and c.label[0] < c.label[1]


def test_value_equals_level_has_nine_faceless_vertices():
    mesh, c = R.lattice_reference("value-equals-level")
    assert len(c.label) == 10 and int((c.n_faces == 0).sum()) == 9 and c.n_faces[0] == len(mesh.faces)
    assert c.n_vertices[1:].tolist() == [1] * 9 and np.all(np.diff(c.label[1:]) > 0)     # ties by label ascending


def test_thin_lattice_has_no_faces():
    mesh, c = R.lattice_reference("noise-65x1x1")
    assert len(mesh.vertices) == 64 and len(mesh.faces) == 0 and len(c.label) == 64
    assert np.array_equal(c.labels, np.arange(64)) and np.array_equal(c.label, np.arange(64))


def test_sparse_noise_has_many_components_faceless_ones_and_ties():
    _, c = R.lattice_reference("sparse-noise")
    assert len(c.label) >= 100
    assert int((c.n_faces == 0).sum()) >= 1
    with_faces = c.n_faces[c.n_faces > 0]
    assert len(with_faces) - len(np.unique(with_faces)) >= 1
    assert np.all(np.diff(c.n_faces.astype(np.int64)) <= 0)
    same = np.diff(c.n_faces) == 0
    assert np.all(np.diff(c.label.astype(np.int64))[same] > 0)


def test_graph_cases_are_what_they_are_named_for():
    g = R.graph_reference
    for name in ("chain-permuted", "chain-reversed", "fan-around-largest"):
        c = g(name)
        faces, V = R.graph_cases()[name]
        assert len(c.label) == 1 and c.label[0] == 0 and c.n_vertices[0] == V and c.n_faces[0] == len(faces), name
    assert int(R.graph_cases()["fan-around-largest"][0][:, 0].min()) == R.graph_cases()["fan-around-largest"][1] - 1
    c = g("disjoint-triangles")
    assert len(c.label) == 10000 and set(c.n_faces.tolist()) == {1} and set(c.n_vertices.tolist()) == {3}
    c = g("even-odd")
    assert c.label.tolist() == [0, 1] and np.array_equal(c.labels, np.arange(4099) % 2)
    c = g("degenerate-duplicate")
    assert c.labels.tolist() == [0, 0, 0, 3, 4, 4, 4, 7, 7, 7] + list(range(10, 20)) + [20, 20]
    assert c.label.tolist()[:5] == [0, 4, 7, 20, 3] and c.n_faces.tolist()[:5] == [3, 3, 2, 2, 1]
    c = g("no-faces")
    assert len(c.label) == 1000 and not c.n_faces.any()


# ---------------------------------------------------------------------------------------------------------------- known answers
def test_keep_largest_two_of_three_leaves_two_closed_manifolds():
    mesh, _ = R.lattice_reference("three")
    out = R.filter_mesh(mesh, R.Rules(keep_largest=2))
    assert len(out.faces) == 1548 + 1540
    closed, chi, volume = R.topology_of(out)
    assert closed and chi == 4 and volume > 0
    c = R.components(out.faces, len(out.vertices), out.cells)
    assert c.n_faces.tolist() == [1548, 1540]


def test_keep_largest_one_of_the_twins_keeps_the_lower_label():
    mesh, c = R.lattice_reference("twin")
    out = R.filter_mesh(mesh, R.Rules(keep_largest=1))
    first = c.labels == c.label[0]
    assert np.array_equal(out.vertices, mesh.vertices[first]) and len(out.faces) == 1548
    assert R.topology_of(out)[:2] == (True, 2)


def test_min_faces_one_removes_exactly_the_unused_vertices():
    mesh, _ = R.lattice_reference("value-equals-level")
    out = R.filter_mesh(mesh, R.Rules(min_faces=1))
    used = np.zeros(len(mesh.vertices), bool)
    used[mesh.faces.reshape(-1)] = True
    assert int((~used).sum()) == 9 and len(out.vertices) == len(mesh.vertices) - 9 and len(out.faces) == len(mesh.faces)
    assert np.array_equal(out.vertices, mesh.vertices[used]) and np.array_equal(out.cells, mesh.cells[used])
    assert np.array_equal(out.vertices[out.faces], mesh.vertices[mesh.faces])       # the same triangles, in the same order and winding


@pytest.mark.parametrize("name", list(R.lattice_cases()))
def test_default_rules_return_the_input(name):
    mesh, _ = R.lattice_reference(name)
    out = R.filter_mesh(mesh, R.Rules())
    for k in ("vertices", "faces", "cells", "lattice"):
        a, b = getattr(out, k), getattr(mesh, k)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), k


@pytest.mark.parametrize("name", list(R.lattice_cases()))
def test_filtered_meshes_keep_order_and_winding(name):
    mesh, c = R.lattice_reference(name)
    for rules in R.RULES:
        out = R.filter_mesh(mesh, rules)
        keep_rows = R.kept_rows(c, rules)
        assert len(out.faces) == int(c.n_faces[keep_rows].sum()) and len(out.vertices) == int(c.n_vertices[keep_rows].sum())
        if len(out.faces):
            assert out.faces.min() >= 0 and out.faces.max() < len(out.vertices)
            kept_faces = np.isin(c.labels[mesh.faces[:, 0]], c.label[keep_rows])
            assert np.array_equal(out.cells[out.faces], mesh.cells[mesh.faces[kept_faces]])


# ---------------------------------------------------------------------------------------------------------------- invariances
@pytest.mark.parametrize("name", ["three", "sparse-noise"])
def test_labels_do_not_depend_on_face_or_corner_order(name):
    mesh, c = R.lattice_reference(name)
    for seed in (1, 2):
        assert np.array_equal(R.labels_of(R.permuted(mesh.faces, seed), len(mesh.vertices)), c.labels)


@pytest.mark.parametrize("name", ["chain-permuted", "fan-around-largest", "degenerate-duplicate"])
def test_graph_labels_do_not_depend_on_face_order(name):
    faces, V = R.graph_cases()[name]
    assert np.array_equal(R.labels_of(R.permuted(faces, 3), V), R.graph_reference(name).labels)


# ---------------------------------------------------------------------------------------------------------------- library surface
NEW_EXPORTS = ("scanerf_mesh_components_scratch_bytes", "scanerf_mesh_components_label", "scanerf_mesh_components_table",
               "scanerf_mesh_filter_count", "scanerf_mesh_filter_emit")


def test_the_new_exports_are_in_the_prototype_table_and_the_header():
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "scanerf_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _capi.PROTOTYPES and _capi.PROTOTYPES[name][2] is _capi.REQ, name
        assert name + "(" in hdr, name
        assert hasattr(_capi.lib(), name), name
    assert _capi.PROTOTYPES["scanerf_mesh_components_scratch_bytes"][:2] == ("Z", "II")
    assert _capi.lib().scanerf_abi_version() == 10


def test_the_c_entry_points_refuse_before_any_launch():
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    lib = _capi.lib()
    null = None
    nbytes = lib.scanerf_mesh_components_scratch_bytes(1000, 2000)
    assert nbytes >= 64 + 2 * 4 * 1000 and nbytes % 16 == 0
    assert lib.scanerf_mesh_components_scratch_bytes(1000, 0) > 0
    for V, F in ((0, 0), (-1, 5), (5, -1), (2 ** 31 - 1, 0), (10, 2 ** 31 // 3)):
        assert lib.scanerf_mesh_components_scratch_bytes(V, F) == 0 and b"not supported" in lib.scanerf_last_error(), (V, F)
    label = lambda V, F, scratch, n: lib.scanerf_mesh_components_label(null, V, F, null, scratch, n, null)
    assert label(0, 0, null, 0) != 0 and b"not supported" in lib.scanerf_last_error()
    assert label(1000, 2000, null, nbytes) != 0 and b"scratch is null" in lib.scanerf_last_error()
    assert label(1000, 2000, 4096 + 8, nbytes) != 0 and b"aligned" in lib.scanerf_last_error()
    assert label(1000, 2000, 4096, nbytes - 1) != 0 and b"needs" in lib.scanerf_last_error()
    assert label(1000, 2000, 4096, nbytes) != 0 and b"null pointer" in lib.scanerf_last_error()
    table = lambda C: lib.scanerf_mesh_components_table(null, null, null, 1000, 2000, 4096, nbytes, C, null, null, null, null, null, null)
    assert table(0) != 0 and b"C=0" in lib.scanerf_last_error()
    assert table(1001) != 0 and b"C=1001" in lib.scanerf_last_error()
    assert table(5) != 0 and b"null pointer" in lib.scanerf_last_error()
    assert lib.scanerf_mesh_filter_count(null, null, null, 1000, 2000, 5, 4096, nbytes, null) != 0 and b"null pointer" in lib.scanerf_last_error()
    emit = lambda Vo, Fo, scratch=4096: lib.scanerf_mesh_filter_emit(null, null, null, 1000, 2000, 5, scratch, nbytes, null, null, null, null, null,
                                                                     null, null, null, null, Vo, Fo, null)
    assert emit(1, 1) != 0 and b"null pointer" in lib.scanerf_last_error()
    assert emit(1, 1, null) != 0 and b"scratch is null" in lib.scanerf_last_error()


def _no_library(monkeypatch):
    """Any library call from here on fails the test."""
    from scanerf_amd import meshing

    def refuse():
        raise AssertionError("the library was called before the arguments were refused")
    monkeypatch.setattr(meshing, "lib", refuse)


def test_meshing_refuses_before_any_library_call(monkeypatch):
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    _no_library(monkeypatch)
    faces = torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.mesh_components(faces, 10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.mesh_components(faces, 10, route="composed")
    with pytest.raises(RuntimeError, match="route"):
        meshing.mesh_components(faces, 10, route="dense")
    with pytest.raises(RuntimeError, match="n_vertices"):
        meshing.mesh_components(faces, -1)
    with pytest.raises(RuntimeError, match="n_vertices"):
        meshing.mesh_components(faces, 2.5)
    with pytest.raises(RuntimeError, match="must be a torch.Tensor"):
        meshing.mesh_components(np.zeros((4, 3), np.int32), 10)
    mesh = meshing.Mesh(torch.zeros((5, 3)), faces, torch.zeros((5, 3), dtype=torch.int32), torch.zeros((5, 3)), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.filter_mesh(mesh, min_faces=1)
    with pytest.raises(RuntimeError, match="mesh.vertices"):
        meshing.filter_mesh(mesh._replace(vertices=None), min_faces=1)
    # the rule's values are judged by the extractors before anything else, and by _rules for filter_mesh
    for bad in (dict(min_faces=-1), dict(min_extent=-2), dict(keep_largest=-1), dict(min_faces=1.5), dict(keep_largest=True)):
        with pytest.raises(RuntimeError, match="non-negative integer"):
            meshing._rules(**{"min_faces": 0, "min_extent": 0, "keep_largest": None, **bad}, have_cells=True)
        with pytest.raises(RuntimeError, match="non-negative integer"):
            meshing.extract_scene_mesh(*[None] * 10, (4, 4, 4), 1.0, **bad)
        with pytest.raises(RuntimeError, match="non-negative integer"):
            meshing.extract_mesh(*[None] * 8, (4, 4, 4), 1.0, **bad)
    with pytest.raises(RuntimeError, match="min_extent needs"):
        meshing._rules(0, 1, None, have_cells=False)
    assert meshing._rules(0, 0, None, False) == (0, 0, None, False) and meshing._rules(0, 0, 0, False)[3]
