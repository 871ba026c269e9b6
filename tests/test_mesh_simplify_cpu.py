"""Mesh simplification by vertex clustering without a GPU (tests/mesh_simplify_reference.py): the numpy reference of
the definition on the lattice cases with their known answers (counts, closed manifolds, the Euler characteristic, the identity
below the vertex spacing, the one-vertex collapse, the distance bound, the plate's stated limit), hand rows at the definition's
edges, invariance under face permutation and vertex renumbering, the bad vertices, every refusal that happens before a launch, the
new entries of the second header against _capi.TOOL_PROTOTYPES and the commands' options."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import mesh_simplify_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("scanerf_mesh_simplify_scratch_bytes", "scanerf_mesh_simplify_cluster", "scanerf_mesh_simplify_emit")
f32 = np.float32
EPS = 2.0 ** -24


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- the lattice cases: known answers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.LATTICE))
def test_lattice_case_counts_topology_and_distance(name):
    V, F, table, chi = R.LATTICE[name]
    v, faces, normals, colors = R.lattice_mesh(name)
    assert (v.shape[0], faces.shape[0]) == (V, F)
    assert R.closed_manifold(faces) and R.euler(V, faces) == chi
    for h, (Vk, Fk) in table.items():
        r = R.simplify(v, faces, h, normals=normals, colors=colors)
        assert (r.vertices.shape[0], r.faces.shape[0]) == (Vk, Fk), (name, h)
        assert R.closed_manifold(r.faces) and R.euler(Vk, r.faces) == chi, (name, h)
        assert int(r.counts.sum()) == V and r.counts.min() >= 1
        # Every member lies within h per axis of its cluster's vertex: in exact arithmetic both lie in the closed cell
        # [o + k h, o + (k + 1) h].  Allowance: the key (subtract, divide) and the output (convert M, add k, multiply, add o) are at
        # most six float32 roundings, each at most 2^-24 relative to a magnitude no larger than |v| + |o| + h; 8 covers the six and
        # their compounding.  (o = 0 here.)
        allow = 8 * EPS * (np.abs(v).astype(np.float64) + h)
        d = np.abs(r.vertices[r.row].astype(np.float64) - v.astype(np.float64))
        assert (d <= h + allow).all(), (name, h, float((d / h).max()))
        # unit normals in, unit normals out (a cluster's members point the same way on these shapes); colours stay in [0, 1]
        assert np.abs(np.linalg.norm(r.normals.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        assert r.colors.min() >= 0.0 and r.colors.max() <= 1.0


@pytest.mark.parametrize("name", sorted(R.LATTICE))
def test_a_cell_below_the_vertex_spacing_returns_the_input_bit_for_bit(name):
    v, faces, normals, colors = R.lattice_mesh(name)
    for h in R.IDENTITY_CELLS:
        r = R.simplify(v, faces, h, normals=normals, colors=colors)
        assert int(r.counts.max()) == 1, (name, h)          # the premise, before the identity is claimed
        assert R.same_bits(r.vertices, v) and R.same_bits(r.faces, faces) and R.same_bits(r.normals, normals) and R.same_bits(r.colors, colors)
        assert np.array_equal(r.row, np.arange(v.shape[0]))


@pytest.mark.parametrize("name", sorted(R.LATTICE))
def test_one_huge_cell_leaves_one_vertex_and_no_face(name):
    v, faces, normals, colors = R.lattice_mesh(name)
    r = R.simplify(v, faces, 100.0, normals=normals, colors=colors)
    assert r.vertices.shape == (1, 3) and r.faces.shape == (0, 3) and int(r.counts[0]) == v.shape[0]
    # against the float64 mean: q truncates (at most one unit of 2^-16 h per member, so at most one in the mean), M rounds (half a unit)
    assert np.abs(r.vertices[0].astype(np.float64) - v.mean(0, dtype=np.float64)).max() <= 2.0 * 100.0 * 2.0 ** -16


def test_the_plate_is_the_stated_limit():
    """Two sheets one cell apart collapse into each other at h = 4: edges with four faces, yet no duplicate triple (the sheets' quads
    are split along different diagonals); at h = 2 they stay apart."""
    V, F, table = R.PLATE
    v, faces, _, _ = R.lattice_mesh("plate")
    assert (v.shape[0], faces.shape[0]) == (V, F) and R.closed_manifold(faces)
    r = R.simplify(v, faces, 4.0)
    assert (r.vertices.shape[0], r.faces.shape[0]) == table[4.0]
    assert int((R.edge_counts(r.faces) != 2).sum()) == 40 and R.duplicate_triples(r.faces) == 0
    r = R.simplify(v, faces, 2.0)
    assert (r.vertices.shape[0], r.faces.shape[0]) == table[2.0] and R.closed_manifold(r.faces)


# ---- hand rows ---------------------------------------------------------------------------------------------------------------------
def test_a_vertex_exactly_on_a_cell_face_belongs_to_the_upper_cell():
    v = np.array([[2.0, 4.0, -6.0], [3.0, 5.0, -5.0], [1.999, 4.0, -6.0]], f32)
    k, q, good = R.key(v, (0, 0, 0), 2.0)
    assert good.all() and k.tolist() == [[1, 2, -3], [1, 2, -3], [0, 2, -3]] and q[0].tolist() == [0, 0, 0] and q[1].tolist() == [32768] * 3
    r = R.simplify(v, [[0, 1, 2]], 2.0)
    assert r.row.tolist() == [0, 0, 1] and r.faces.shape == (0, 3)
    assert r.vertices[0].tolist() == [2.5, 4.5, -5.5] and R.same_bits(r.vertices[1], v[2])
    # with an origin: the grid moves with it
    k, q, _ = R.key(np.array([[2.5, 0.5, -1.5]], f32), (0.5, 0.5, 0.5), 2.0)
    assert k.tolist() == [[1, 0, -1]] and q.tolist() == [[0, 0, 0]]


def test_negative_coordinates_floor_and_do_not_truncate():
    v = np.array([[-0.5, -1.0, -2.25], [-0.25, -0.75, -2.75]], f32)
    k, q, _ = R.key(v, (0, 0, 0), 1.0)
    assert k.tolist() == [[-1, -1, -3], [-1, -1, -3]]
    assert q.tolist() == [[32768, 0, 49152], [49152, 16384, 16384]]
    r = R.simplify(v, np.zeros((0, 3), np.int32), 1.0)
    assert r.vertices.tolist() == [[-0.375, -0.875, -2.5]]
    # a negative u too small for 1 + u to differ from 1: f rounds to 1, q = 65536, and the vertex comes out on the cell's upper face
    tiny = np.array([[-1e-10, 0.0, 0.0], [-0.5, 0.0, 0.0]], f32)
    k, q, good = R.key(tiny, (0, 0, 0), 1.0)
    assert good.all() and k[0, 0] == -1 and q[0, 0] == 65536
    assert R.simplify(tiny, np.zeros((0, 3), np.int32), 1.0).vertices[0, 0] == f32(-0.25)      # (65536 + 32768) / 2 -> -1 + 0.75


def test_the_mean_rounds_halves_up_for_both_signs():
    """M = floor((2 S + n) / (2 n)) where 2 S + n is a multiple of 2 n: S / n ends in .5, and M is the next integer ABOVE."""
    assert [int(R.rounded_mean(np.int64(S), np.int64(2))) for S in (1, 3, -1, -3, 0, 2, -2)] == [1, 2, 0, -1, 0, 1, -1]
    assert [int(R.rounded_mean(np.int64(S), np.int64(3))) for S in (4, 5, -4, -5, -3)] == [1, 2, -1, -2, -1]
    u = 2.0 ** -16
    v = np.array([[0.25, 0.25, 0.25], [0.75, 0.75, 0.75]], f32)
    c = np.array([[u, -u, -3 * u], [0.0, 0.0, 0.0]], f32)
    r = R.simplify(v, np.zeros((0, 3), np.int32), 1.0, colors=c)
    assert r.colors.tolist() == [[u, 0.0, -u]]
    # positions: q = 16384 and 16385 -> S = 32769, M = 16385 (16384.5 rounds up)
    v = np.array([[0.25, 0.5, 0.5], [0.25 + u, 0.5, 0.5]], f32)
    assert R.simplify(v, np.zeros((0, 3), np.int32), 1.0).vertices[0, 0] == f32(0.25 + u)


def test_attributes_are_clamped_at_32767():
    assert R.fixed(np.array([32767.0, 40000.0, -32767.0, -1e9, 0.5, 2.0 ** -17, 3 * 2.0 ** -17], f32)).tolist() == [
        32767 * 65536, 32767 * 65536, -32767 * 65536, -32767 * 65536, 32768, 0, 2]          # (halves round to even, as rintf)
    v = np.array([[0.25, 0.25, 0.25], [0.75, 0.75, 0.75]], f32)
    c = np.array([[40000.0, -1e9, 32767.0], [32767.0, -32767.0, 32766.0]], f32)
    r = R.simplify(v, np.zeros((0, 3), np.int32), 1.0, colors=c)
    assert r.colors.tolist() == [[32767.0, -32767.0, 32766.5]]
    # ... but a cluster of one member keeps its value, clamped or not
    assert R.simplify(v[:1], np.zeros((0, 3), np.int32), 1.0, colors=c[:1]).colors.tolist() == c[:1].tolist()


def test_opposite_normals_give_a_zero_normal():
    v = np.array([[0.25, 0.25, 0.25], [0.75, 0.75, 0.75], [1.5, 0.5, 0.5], [1.25, 0.5, 0.5]], f32)
    n = np.array([[0.0, 0.6, -0.8], [0.0, -0.6, 0.8], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], f32)
    r = R.simplify(v, np.zeros((0, 3), np.int32), 1.0, normals=n)
    assert r.normals[0].tolist() == [0.0, 0.0, 0.0]
    assert np.allclose(r.normals[1], [0.0, math.sqrt(0.5), math.sqrt(0.5)], atol=1e-6)
    z = R.simplify(v[:2], np.zeros((0, 3), np.int32), 1.0, normals=np.zeros((2, 3), f32))
    assert z.normals.tolist() == [[0.0, 0.0, 0.0]]


def test_faces_keep_order_and_winding_and_duplicates_stay():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.6, 0.6], [1.6, 0.6, 0.6], [9.5, 9.5, 9.5]], f32)
    faces = np.array([[4, 2, 0], [0, 1, 3], [3, 4, 2], [1, 2, 0], [5, 5, 1]], np.int32)
    r = R.simplify(v, faces, 1.0)
    assert r.row.tolist() == [0, 1, 2, 0, 1, 3]
    assert r.faces.tolist() == [[1, 2, 0], [0, 1, 2], [1, 2, 0]]          # the second face lost a corner; two equal triples stay
    assert r.vertices.shape[0] == 4                                      # cluster 3 ends with no face and stays a vertex


# ---- invariance --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [2.0, 3.0])
def test_invariance_under_face_permutation_and_vertex_renumbering(h):
    v, faces, normals, colors = R.lattice_mesh("sphere19")
    base = R.simplify(v, faces, h, normals=normals, colors=colors)
    rng = np.random.default_rng(3)
    # faces permuted: the vertices do not move; the kept faces are the permuted input's kept faces, in its order
    p = rng.permutation(faces.shape[0])
    r = R.simplify(v, faces[p], h, normals=normals, colors=colors)
    assert all(R.same_bits(a, b) for a, b in zip(r[:1] + r[2:4], base[:1] + base[2:4]))
    rf = base.row[faces[p]]
    assert np.array_equal(r.faces, rf[(rf[:, 0] != rf[:, 1]) & (rf[:, 0] != rf[:, 2]) & (rf[:, 1] != rf[:, 2])])
    # vertices renumbered: new vertex i is old vertex p[i].  The clusters are the same sets; their numbers follow the new order.
    p = rng.permutation(v.shape[0])
    inv = np.argsort(p)
    r = R.simplify(v[p], inv[faces].astype(np.int32), h, normals=normals[p], colors=colors[p])
    to_new = np.full(base.vertices.shape[0], -1)
    to_new[base.row] = r.row[inv]                                  # old cluster -> new cluster, through any member
    assert np.array_equal(to_new[base.row], r.row[inv]) and sorted(to_new.tolist()) == list(range(r.vertices.shape[0]))
    assert R.same_bits(r.vertices[to_new], base.vertices) and R.same_bits(r.normals[to_new], base.normals)
    assert R.same_bits(r.colors[to_new], base.colors) and np.array_equal(to_new[base.faces], r.faces)
    first = np.full(r.vertices.shape[0], v.shape[0])
    np.minimum.at(first, r.row, np.arange(v.shape[0]))
    assert (np.diff(first) > 0).all()                              # the induced order: ascending smallest member


# ---- bad vertices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.bad_cases()))
def test_bad_vertices_are_counted_and_refused(name):
    v, faces, normals, colors, n_bad = R.bad_cases()[name]
    assert R.count_bad(v, (0, 0, 0), 1.0, normals, colors) == n_bad
    with pytest.raises(R.BadVertices) as e:
        R.simplify(v, faces, 1.0, normals=normals, colors=colors)
    assert e.value.n_bad == n_bad


def test_the_largest_cells_that_are_not_bad():
    v, faces, normals, colors = R.extreme_keys()
    r = R.simplify(v, faces, 1.0, normals=normals, colors=colors)
    assert r.vertices.shape[0] == 5 and sorted(r.counts.tolist()) == [3] * 5
    assert np.abs(r.vertices).max() == f32(2 ** 20 - 1 + 0.25)
    assert R.count_bad(np.array([[2.0 ** 20, 0, 0]], f32), (0, 0, 0), 1.0) == 1
    assert R.count_bad(np.array([[-(2.0 ** 20), 0, 0]], f32), (0, 0, 0), 1.0) == 1
    assert R.count_bad(np.array([[-(2.0 ** 20) + 1.0, 0, 0]], f32), (0, 0, 0), 1.0) == 0
    assert R.count_bad(np.array([[3e38, 0, 0]], f32), (-3e38, 0, 0), 1.0) == 1          # v - o overflows: u is not finite


# ---- the header, the prototypes, the entries' refusals -------------------------------------------------------------------------------
def test_new_entries_match_the_second_header():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    from test_mesh_visibility_cpu import TOOLS_HEADER, _prototypes
    hdr = _prototypes(TOOLS_HEADER)
    for name in ENTRIES:
        assert name in hdr and name in _capi.TOOL_PROTOTYPES and tuple(_capi.TOOL_PROTOTYPES[name]) == hdr[name], name
        assert hdr[name][0] == "I" and hdr[name][1].endswith("P")
    assert _capi.TOOL_PROTOTYPES[ENTRIES[0]][1] == "IIP"
    cluster, emit = _capi.TOOL_PROTOTYPES[ENTRIES[1]][1], _capi.TOOL_PROTOTYPES[ENTRIES[2]][1]
    assert emit.startswith(cluster[:-1]) and emit[len(cluster) - 1:] == "PPPPPPIIP"      # the same head, then the emit pass's own
    text = open(TOOLS_HEADER).read()
    for words in ("floorf(u)", "(2 S_a + n) div (2 n)", "smallest member index", "Duplicate faces are kept", "n_bad"):
        assert words in text, words


def _scratch_bytes(V, F):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    n = ctypes.c_size_t(12345)
    status = _capi.tool(ENTRIES[0])(V, F, ctypes.addressof(n))
    return status, int(n.value)


def test_scratch_bytes_is_the_documented_formula():
    r16 = lambda x: (x + 15) // 16 * 16
    for V, F in ((1, 0), (31, 7), (32, 0), (33, 100), (6310, 12616), (65537, 65535), (2 ** 29, 5)):
        T = 64
        while T < 2 * V:
            T *= 2
        want = 64 + 12 * T + 2 * r16(4 * V) + r16(4 * ((V + 255) // 256 + 1)) + r16(4 * ((F + 255) // 256 + 1))
        assert _scratch_bytes(V, F) == (0, want), (V, F)
    for V, F in ((0, 0), (-1, 3), (2 ** 29 + 1, 0), (5, -1), (5, 2 ** 31 // 3)):
        status, n = _scratch_bytes(V, F)
        assert status != 0 and n == 0, (V, F)
    from scanerf_amd import _capi
    assert _capi.tool(ENTRIES[0])(4, 4, None) != 0 and b"null" in _capi.lib().scanerf_last_error()


def _entry(which, **over):
    """An entry on buffers that are valid HOST memory for everything the host side reads (origin) and placeholders elsewhere, one
    thing changed -> (status, message).  Every case here is refused before any launch."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    origin = (ctypes.c_float * 3)(*over.pop("origin_values", (0.0, 0.0, 0.0)))
    a = dict(vertices=16, faces=16, normals=None, colors=None, V=4, F=2, origin=ctypes.addressof(origin), cell=1.0, scratch=None,
             scratch_bytes=1 << 20)
    if which == "emit":
        a.update(sums=16, counts=16, out_vertices=16, out_faces=16, out_normals=None, out_colors=None, Vout=2, Fout=1)
    a.update(over)
    status = _capi.tool(ENTRIES[1] if which == "cluster" else ENTRIES[2])(*a.values(), None)
    return status, _capi.lib().scanerf_last_error()


@pytest.mark.parametrize("which", ["cluster", "emit"])
def test_entries_refuse_before_any_launch(which):
    for over, text in (({}, b"scratch is null"), ({"scratch": 24}, b"16-byte aligned"), ({"scratch": 32, "scratch_bytes": 100}, b"needs"),
                       ({"V": 0}, b"V=0"), ({"V": -2}, b"V=-2"), ({"V": 2 ** 29 + 1}, b"not supported"), ({"F": -1}, b"F=-1"),
                       ({"vertices": None}, b"null pointer"), ({"faces": None}, b"null pointer"), ({"origin": None}, b"null pointer"),
                       ({"cell": 0.0}, b"cell=0"), ({"cell": -1.0}, b"cell=-1"), ({"cell": math.inf}, b"cell=inf"), ({"cell": math.nan}, b"cell="),
                       ({"origin_values": (0.0, math.nan, 0.0)}, b"origin"), ({"origin_values": (math.inf, 0.0, 0.0)}, b"origin")):
        status, msg = _entry(which, **over)
        assert status != 0 and text in msg, (over, msg)


def test_emit_entry_refuses_its_own_arguments_before_any_launch():
    ok = {"scratch": 32}
    for over, text in (({"Vout": 0}, b"Vout=0"), ({"Vout": 5}, b"Vout=5"), ({"Fout": -1}, b"Fout=-1"), ({"Fout": 3}, b"Fout=3"),
                       ({"sums": None}, b"null pointer"), ({"counts": None}, b"null pointer"), ({"out_vertices": None}, b"null pointer"),
                       ({"out_faces": None}, b"null pointer"), ({"normals": 16}, b"go together"), ({"out_normals": 16}, b"go together"),
                       ({"colors": 16}, b"go together"), ({"out_colors": 16}, b"go together")):
        status, msg = _entry("emit", **ok, **over)
        assert status != 0 and text in msg, (over, msg)


# ---- the Python refusals -----------------------------------------------------------------------------------------------------------
def _cpu_mesh():
    from scanerf_amd import meshing
    return meshing.Mesh(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32), None, None, None)


def test_python_refusals_happen_before_any_library_call(monkeypatch):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi, fusion, meshing

    def no_call(name):
        raise AssertionError(f"{name} was reached")
    monkeypatch.setattr(_capi, "tool", no_call)
    mesh = _cpu_mesh()
    with pytest.raises(RuntimeError, match="route must be one of"):
        meshing.simplify_mesh(mesh, 1.0, route="dense")
    for cell in (0.0, -1.0, math.inf, math.nan, 1e-50, 1e39, "1", None, True):
        with pytest.raises(RuntimeError, match="cell must be"):
            meshing.simplify_mesh(mesh, cell)
    for origin in ((0.0, 0.0), (0.0, math.nan, 0.0), (math.inf, 0.0, 0.0)):
        with pytest.raises(RuntimeError, match="origin"):
            meshing.simplify_mesh(mesh, 1.0, origin=origin)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        meshing.simplify_mesh(mesh, 1.0)
    with pytest.raises(RuntimeError, match="must be a torch.Tensor"):
        meshing.simplify_mesh(meshing.Mesh(np.zeros((4, 3), f32), mesh.faces, None, None, None), 1.0)
    # the extractors check simplify= before they do anything else
    for bad in (0.0, -2.0, math.nan, "x"):
        with pytest.raises(RuntimeError, match="cell must be"):
            fusion.fuse_depth_maps(None, None, None, (0, 0, 0), (1, 1, 1), (4, 4, 4), simplify=bad)
        with pytest.raises(RuntimeError, match="cell must be"):
            meshing.extract_scene_mesh(*[None] * 8, (0, 0, 0), (1, 1, 1), (4, 4, 4), 1.0, simplify=bad)
    assert meshing._simplified(mesh, None, None, None) is mesh
    colors = torch.zeros((4, 3))
    got = meshing._simplified(mesh, None, colors, None)
    assert got[0] is mesh and got[1] is colors


# ---- the commands ------------------------------------------------------------------------------------------------------------------
def test_commands_take_the_new_options():
    args = _tool("simplify_mesh").parser().parse_args(["in.ply", "out.ply", "--cell", "0.5", "--origin", "1", "2", "-3"])
    assert (args.input, args.output, args.cell, list(args.origin)) == ("in.ply", "out.ply", 0.5, [1.0, 2.0, -3.0])
    assert list(_tool("simplify_mesh").parser().parse_args(["a", "b", "--cell", "2"]).origin) == [0.0, 0.0, 0.0]
    with pytest.raises(SystemExit):
        _tool("simplify_mesh").parser().parse_args(["in.ply", "out.ply"])
    fuse = _tool("fuse_mesh").parser()
    assert fuse.parse_args(["t", "--cameras", "c.log", "--out", "o.ply"]).simplify is None
    assert fuse.parse_args(["t", "--cameras", "c.log", "--out", "o.ply", "--simplify", "0.25"]).simplify == 0.25
    scene = _tool("extract_scene_mesh").parser()
    assert scene.parse_args(["t", "--level", "5", "--out", "o.ply"]).simplify is None
    assert scene.parse_args(["t", "--level", "5", "--out", "o.ply", "--simplify", "3"]).simplify == 3.0


def test_ply_vertex_properties_reads_the_header(tmp_path):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import formats
    v, faces, normals, colors = R.lattice_mesh("sphere19")
    plain, full = str(tmp_path / "plain.ply"), str(tmp_path / "full.ply")
    formats.write_ply(plain, v, faces)
    formats.write_ply(full, v, faces, normals=normals, colors=colors, binary=False)
    assert formats.ply_vertex_properties(plain) == ["x", "y", "z"]
    assert formats.ply_vertex_properties(full) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
