"""Mesh simplification by vertex clustering on the GPU (csrc/mesh_simplify.hip, scanerf_amd/meshing.py): the fused
route against the composed torch route against the numpy reference bit for bit -- vertices, faces, normals, colours, the report,
n_bad and a second run -- on the lattice cases and on synthetic inputs (vertex counts around a wavefront, one contended cluster,
65 537 one-member clusters, a block of distinct cells, the largest keys, bad vertices, F = 0, V = 0, degenerate faces); the C entries
on sentinel-filled buffers with guard regions; every refusal; a side stream; the extractors' simplify=; the commands and the PLY
round trip."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mesh_simplify_reference as R
import tsdf_reference as TR
from test_gpu_tsdf import DEV, GUARD, _guarded, _guards_intact, _icosphere, _np, _trace_depth, tile_scene  # noqa: F401

pytestmark = pytest.mark.gpu
ENTRIES = ("scanerf_mesh_simplify_scratch_bytes", "scanerf_mesh_simplify_cluster", "scanerf_mesh_simplify_emit")
SENTINEL = -7.25
ISENTINEL = -77


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV).contiguous()      # (a copy: the cases are read-only arrays)


def _mesh(v, faces, normals=None):
    from scanerf_amd import meshing
    return meshing.Mesh(_dev(v), _dev(faces), None, None, _dev(normals))


def _run(v, faces, normals, colors, h, origin=(0.0, 0.0, 0.0), route="fused", report=None):
    """-> (vertices, faces, normals, colors) as numpy arrays (None where not given)."""
    from scanerf_amd import meshing
    out = meshing.simplify_mesh(_mesh(v, faces, normals), h, origin=origin, colors=_dev(colors), route=route, report=report)
    mesh, rgb = out if colors is not None else (out, None)
    assert isinstance(mesh, meshing.Mesh) and mesh.cells is None and mesh.lattice is None and (mesh.normals is None) == (normals is None)
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32 and mesh.vertices.is_contiguous() and mesh.faces.is_contiguous()
    return tuple(None if t is None else _np(t) for t in (mesh.vertices, mesh.faces, mesh.normals, rgb))


def _agree(what, v, faces, normals, colors, h, origin=(0.0, 0.0, 0.0)):
    """fused == composed == numpy in every bit, the reports equal, a second fused run equal -> the reference's Result."""
    want = R.simplify(v, faces, h, origin, normals, colors)
    ref = (want.vertices, want.faces, want.normals, want.colors)
    rep = {}
    got = _run(v, faces, normals, colors, h, origin, "fused", rep)
    rep_c = {}
    witness = _run(v, faces, normals, colors, h, origin, "composed", rep_c)
    again = _run(v, faces, normals, colors, h, origin, "fused")
    names = ("vertices", "faces", "normals", "colors")
    for other, who in ((ref, "numpy"), (witness, "composed"), (again, "a second run")):
        for a, b, k in zip(got, other, names):
            assert (a is None) == (b is None), (what, who, k)
            if a is not None:
                assert a.shape == b.shape and a.dtype == b.dtype, (what, who, k, a.shape, b.shape)
                bad = np.flatnonzero((a.view(np.int32) != b.view(np.int32)).reshape(len(a), -1).any(1)) if len(a) else []
                assert len(bad) == 0, (what, f"fused != {who}", k, len(bad), bad[:5])
    V, F = len(v), len(faces)
    expect = dict(clusters=len(want.vertices), largest_cluster=int(want.counts.max()) if V else 0, vertices=(V, len(want.vertices)),
                  faces=(F, len(want.faces)))
    assert rep == expect and rep_c == expect, (what, rep, rep_c, expect)
    return want


# ---- the lattice cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.LATTICE))
def test_lattice_cases_fused_composed_and_numpy_agree_in_every_bit(name):
    V, F, table, _ = R.LATTICE[name]
    v, faces, normals, colors = R.lattice_mesh(name)
    for h, (Vk, Fk) in table.items():
        want = _agree(f"{name} h={h}", v, faces, normals, colors, h)
        assert (len(want.vertices), len(want.faces)) == (Vk, Fk)
    for h in R.IDENTITY_CELLS:          # every cluster has one member: the input comes back in every bit
        got = _run(v, faces, normals, colors, h)
        assert all(R.same_bits(a, b) for a, b in zip(got, (v, faces, normals, colors))), (name, h)
    one = _agree(f"{name} h=100", v, faces, normals, colors, 100.0)
    assert one.vertices.shape == (1, 3) and one.faces.shape == (0, 3)
    _agree(f"{name} h=2.5 origin", v, faces, None, None, 2.5, origin=(0.3, -1.7, 11.0))          # positions alone, another grid
    _agree(f"{name} h=3 colours", v, faces, None, colors, 3.0)
    _agree(f"{name} h=3 normals", v, faces, normals, None, 3.0)


def test_the_plate_collapses_as_stated():
    v, faces, normals, colors = R.lattice_mesh("plate")
    for h, (Vk, Fk) in R.PLATE[2].items():
        want = _agree(f"plate h={h}", v, faces, normals, colors, h)
        assert (len(want.vertices), len(want.faces)) == (Vk, Fk)


# ---- synthetic inputs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_vertex_counts_around_a_wavefront(V):
    v, faces, normals, colors = R.random_mesh(V, 2 * V + 3, 40 + V)
    for h in (0.5, 3.0, 20.0):
        _agree(f"V={V} h={h}", v, faces, normals, colors, h)


def test_one_cluster_of_6310_vertices():
    v, faces, normals, colors = R.one_cluster()
    want = _agree("one cluster", v, faces, normals, colors, 1.0)
    assert want.vertices.shape == (1, 3) and want.faces.shape == (0, 3) and int(want.counts[0]) == 6310


def test_65537_one_member_clusters_on_a_line():
    v, faces, normals, colors = R.line_of_singles()
    want = _agree("line", v, faces, normals, colors, 1.0)
    assert int(want.counts.max()) == 1 and R.same_bits(want.vertices, v) and R.same_bits(want.faces, faces)
    _agree("line h=7", v, faces, normals, colors, 7.0)


def test_a_block_of_distinct_cells_fills_the_table_to_its_documented_load():
    v, faces, normals, colors = R.block_of_cells()
    V = len(v)
    T = 64
    while T < 2 * V:
        T *= 2
    assert V == 64000 and T == 131072 and V / T > 0.48          # just below the documented 1/2
    want = _agree("block", v, faces, normals, colors, 1.0)
    assert len(want.vertices) == V
    _agree("block h=4", v, faces, normals, colors, 4.0)


def test_the_largest_keys():
    v, faces, normals, colors = R.extreme_keys()
    want = _agree("extreme keys", v, faces, normals, colors, 1.0)
    assert len(want.vertices) == 5


def test_no_faces_no_vertices_and_degenerate_faces():
    from scanerf_amd import meshing
    v, faces, normals, colors = R.random_mesh(300, 500, 7)
    _agree("F=0", v, faces[:0], normals, colors, 2.0)
    assert (faces[1, 0] == faces[1, 1]) and (faces[3] == faces[3, 0]).all()
    _agree("degenerate input faces", v, faces, normals, colors, 0.01)          # one member per cluster: only the input's own go
    for route in meshing.SIMPLIFY_ROUTES:
        rep = {}
        got = _run(v[:0], faces[:0], normals[:0], colors[:0], 1.0, route=route, report=rep)
        assert [a.shape for a in got] == [(0, 3)] * 4 and rep == dict(clusters=0, largest_cluster=0, vertices=(0, 0), faces=(0, 0))
        got = _run(v[:0], faces[:0], None, None, 1.0, route=route)
        assert got[2] is None and got[3] is None


# ---- bad vertices ------------------------------------------------------------------------------------------------------------------
def _scratch(V, F):
    from scanerf_amd import _capi
    n = ctypes.c_size_t(0)
    assert _capi.tool(ENTRIES[0])(V, F, ctypes.addressof(n)) == 0
    return int(n.value)


def _cluster(v, faces, normals, colors, h, origin=(0.0, 0.0, 0.0)):
    """The cluster entry on a guarded scratch -> (head for the emit entry, buf, scratch, (V', F', n_bad), the tensors kept alive)."""
    from scanerf_amd import _capi
    V, F = len(v), len(faces)
    nbytes = _scratch(V, F)
    buf, scratch = _guarded((nbytes // 4,), torch.int32, ISENTINEL)
    assert scratch.data_ptr() % 16 == 0
    keep = [_dev(v), _dev(faces), _dev(normals), _dev(colors), (ctypes.c_float * 3)(*origin)]
    ptr = lambda t: None if t is None else t.data_ptr()
    head = (ptr(keep[0]), ptr(keep[1]) if F else None, ptr(keep[2]), ptr(keep[3]), V, F, ctypes.addressof(keep[4]), float(h),
            scratch.data_ptr(), nbytes)
    assert _capi.tool(ENTRIES[1])(*head, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return head, buf, scratch, tuple(scratch[:6].view(torch.int64).tolist()), keep


@pytest.mark.parametrize("name", sorted(R.bad_cases()))
def test_bad_vertices_are_an_error_and_nothing_is_written(name):
    from scanerf_amd import _capi, meshing
    v, faces, normals, colors, n_bad = R.bad_cases()[name]
    for route in meshing.SIMPLIFY_ROUTES:
        with pytest.raises(RuntimeError, match=f"{n_bad} bad vertices"):
            meshing.simplify_mesh(_mesh(v, faces, normals), 1.0, colors=_dev(colors), route=route)
    head, buf, scratch, (Vk, Fk, bad), keep = _cluster(v, faces, normals, colors, 1.0)
    assert bad == n_bad and _guards_intact(buf, ISENTINEL)
    rows = max(Vk, 1)
    outs = [_guarded((rows, 9), torch.int64, ISENTINEL), _guarded((rows,), torch.int32, ISENTINEL), _guarded((rows, 3), torch.float32, SENTINEL),
            _guarded((max(Fk, 1), 3), torch.int32, ISENTINEL), _guarded((rows, 3), torch.float32, SENTINEL), _guarded((rows, 3), torch.float32, SENTINEL)]
    status = _capi.tool(ENTRIES[2])(*head, *(o[1].data_ptr() for o in outs), rows, max(Fk, 1), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status != 0 and b"bad vertices" in _capi.lib().scanerf_last_error()
    for (b, _), fill in zip(outs, (ISENTINEL, ISENTINEL, SENTINEL, ISENTINEL, SENTINEL, SENTINEL)):
        assert bool((b == fill).all()), "the emit entry wrote something for a mesh with bad vertices"


# ---- the C entries on guarded buffers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sphere19-h2", "random-257", "F=0"])
def test_entries_write_exactly_their_rows_and_nothing_else(case):
    from scanerf_amd import _capi
    if case == "sphere19-h2":
        (v, faces, normals, colors), h = R.lattice_mesh("sphere19"), 2.0
    else:
        (v, faces, normals, colors), h = R.random_mesh(257, 0 if case == "F=0" else 700, 5), 3.0
    want = R.simplify(v, faces, h, normals=normals, colors=colors)
    head, buf, scratch, (Vk, Fk, bad), keep = _cluster(v, faces, normals, colors, h)
    assert (Vk, Fk, bad) == (len(want.vertices), len(want.faces), 0)
    assert _guards_intact(buf, ISENTINEL), "the cluster entry wrote outside its scratch"
    before = scratch.clone()
    st = torch.cuda.current_stream().cuda_stream
    extra = 5          # rows behind the declared ones, inside the tensors: they must stay as they are too
    mk = lambda rows, cols, dt, fill: _guarded((rows + extra,) + cols, dt, fill)
    sums, counts = mk(Vk, (9,), torch.int64, ISENTINEL), mk(Vk, (), torch.int32, ISENTINEL)
    ov, of = mk(Vk, (3,), torch.float32, SENTINEL), mk(Fk, (3,), torch.int32, ISENTINEL)
    on, oc = mk(Vk, (3,), torch.float32, SENTINEL), mk(Vk, (3,), torch.float32, SENTINEL)
    ptrs = [t[1].data_ptr() for t in (sums, counts, ov, of, on, oc)]
    # outputs declared with other sizes: an error, and nothing written
    for dv, df in ((-1, 0), (1, 0), (0, 1), (0, -1)):
        if Vk + dv < 1 or Fk + df < 0 or Fk + df > len(faces):
            continue
        assert _capi.tool(ENTRIES[2])(*head, *ptrs, Vk + dv, Fk + df, st) != 0
        assert b"declared with" in _capi.lib().scanerf_last_error()
        torch.cuda.synchronize()
        for (b, _), fill in zip((sums, counts, ov, of, on, oc), (ISENTINEL, ISENTINEL, SENTINEL, ISENTINEL, SENTINEL, SENTINEL)):
            assert bool((b == fill).all()), (dv, df)
    assert _capi.tool(ENTRIES[2])(*head, *ptrs, Vk, Fk, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(scratch, before), "the emit entry wrote to the scratch"
    for (b, t), fill, rows in zip((sums, counts, ov, of, on, oc), (ISENTINEL, ISENTINEL, SENTINEL, ISENTINEL, SENTINEL, SENTINEL), (Vk, Vk, Vk, Fk, Vk, Vk)):
        assert _guards_intact(b, fill) and bool((t[rows:] == fill).all()), "rows behind the declared ones were written"
        if rows and t.dtype == torch.float32:
            assert not bool((t[:rows] == fill).any()), "a declared row was left unwritten"
    assert R.same_bits(_np(ov[1][:Vk]), want.vertices) and R.same_bits(_np(of[1][:Fk]), want.faces)
    assert R.same_bits(_np(on[1][:Vk]), want.normals) and R.same_bits(_np(oc[1][:Vk]), want.colors)
    assert np.array_equal(_np(counts[1][:Vk]), want.counts)
    q = R.key(v, (0, 0, 0), h)[1]
    S = np.zeros((Vk, 3), np.int64)
    np.add.at(S, want.row, q)
    assert np.array_equal(_np(sums[1][:Vk, :3]), S)
    # without attributes: their outputs are NULL, their sums stay zero
    head2, buf2, scratch2, totals2, keep2 = _cluster(v, faces, None, None, h)
    assert totals2 == (Vk, Fk, 0)
    ptrs2 = ptrs[:4] + [None, None]
    assert _capi.tool(ENTRIES[2])(*head2, *ptrs2, Vk, Fk, st) == 0
    torch.cuda.synchronize()
    assert R.same_bits(_np(ov[1][:Vk]), want.vertices) and not bool(sums[1][:Vk, 3:].any())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    from scanerf_amd import meshing
    v, faces, normals, colors = R.random_mesh(40, 60, 2)
    mesh = _mesh(v, faces, normals)
    bad = [(mesh._replace(vertices=mesh.vertices.double()), None, "dtype"), (mesh._replace(faces=mesh.faces.long()), None, "dtype"),
           (mesh._replace(vertices=mesh.vertices[:, :2].contiguous()), None, r"must be \[V,3\]"),
           (mesh._replace(vertices=mesh.vertices.t().contiguous().t()), None, "contiguous"),
           (mesh._replace(faces=mesh.faces.cpu()), None, "GPU"), (mesh._replace(normals=mesh.normals[:39]), None, "normals must be"),
           (mesh._replace(normals=mesh.normals.half()), None, "dtype"), (mesh, _dev(colors)[:39], "colors must be"),
           (mesh, _dev(colors).double(), "dtype"), (mesh, colors, "torch.Tensor"),
           (mesh._replace(faces=_dev(np.array([[0, 1, 40]], np.int32))), None, "outside"),
           (mesh._replace(faces=_dev(np.array([[0, -1, 3]], np.int32))), None, "outside"),
           (mesh._replace(faces=mesh.faces[:, :2].contiguous()), None, r"faces must be \[F,3\]")]
    for m, c, text in bad:
        with pytest.raises(RuntimeError, match=text):
            meshing.simplify_mesh(m, 1.0, colors=c)
    with pytest.raises(RuntimeError, match="route"):
        meshing.simplify_mesh(mesh, 1.0, route="dense")
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="cell must be"):
            meshing.simplify_mesh(mesh, cell)


# ---- the stream --------------------------------------------------------------------------------------------------------------------
def test_stream_both_passes_run_on_the_callers_stream(monkeypatch):
    import stream_cases as SC
    from scanerf_amd import _capi, meshing
    from test_gpu_stream_contract import Delay, same_bits

    def build(seed):
        v, faces, normals, colors = R.random_mesh(20000, 40000, 900 + seed, span=30.0)
        return {"vertices": torch.from_numpy(v), "normals": torch.from_numpy(normals), "colors": torch.from_numpy(colors)}

    faces = _dev(R.random_mesh(20000, 40000, 901, span=30.0)[1])

    def run_(state):
        i = state["in"]
        mesh, rgb = meshing.simplify_mesh(meshing.Mesh(i["vertices"], faces, None, None, i["normals"]), 2.0, colors=i["colors"])
        return mesh.vertices, mesh.faces, mesh.normals, rgb

    c = SC.Case("mesh_simplify", ENTRIES[1:], build, run_)
    X, Y = c.build(1), c.build(2)
    state = c.to_device(X)
    Xd, Yd = SC.stage(X), SC.stage(Y)
    handles = []
    for name in ENTRIES[1:]:
        real = _capi.tool(name)

        def recorded(*a, real=real):
            handles.append(int(a[-1] or 0))
            return real(*a)
        monkeypatch.setitem(_capi._tools, name, recorded)
    torch.cuda.synchronize()
    R_X = c.run(state)
    c.refill(state, Yd)
    R_Y = c.run(state)
    torch.cuda.synchronize()
    assert not same_bits(R_X[:1], R_Y[:1]), "the two seeds give the same answer: a stale read would not show"
    assert handles == [torch.cuda.current_stream().cuda_stream] * 4
    delay = Delay()
    s = torch.cuda.Stream()
    del handles[:]
    with torch.cuda.stream(s):
        delay(20.0)
        c.refill(state, Xd)           # queued behind the delay: a launch on any other stream reads Y
        got = c.run(state)            # (the op's one host read waits for the stream: that is its contract)
    s.synchronize()
    torch.cuda.synchronize()
    assert handles == [s.cuda_stream] * 2 and s.cuda_stream != 0, "a pass did not carry the caller's stream"
    assert same_bits(got, R_X), "under a side stream the op read stale inputs: a launch went to another stream"


# ---- the extractors ----------------------------------------------------------------------------------------------------------------
def _same_mesh(got, want, what):
    for k in ("vertices", "faces", "cells", "lattice", "normals"):
        a, b = getattr(got, k), getattr(want, k)
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, k)


@functools.lru_cache(maxsize=None)
def _icosphere_maps():
    from scanerf_amd.fastmesh import FastMesh
    from tsdf_color_reference import radial_colors
    c = TR.case("sphere40")
    V, F = _icosphere(TR.RADIUS, 3)
    depths = _trace_depth(FastMesh.from_arrays(V, F, DEV), c["ks"], c["c2ws"], *c["depths"].shape[1:])
    return c, depths, torch.from_numpy(radial_colors(c["ks"], c["c2ws"], _np(depths))).to(DEV)


def test_fuse_depth_maps_with_simplify_is_simplify_mesh_on_its_result_on_the_traced_icosphere():
    from scanerf_amd import fusion, meshing
    c, depths, colors = _icosphere_maps()
    args = (depths, c["ks"], c["c2ws"], c["origin"], [TR.BOX[1]] * 3, c["n"])
    kw = dict(trunc=TR.TRUNC, views_per_batch=7, near=TR.NEAR, far=TR.FAR)
    h = 3.0 * max(c["spacing"])
    mesh, rgb = fusion.fuse_depth_maps(*args, colors=colors, normals=True, **kw)
    assert mesh.vertices.shape[0] > 100 and mesh.normals is not None
    again, rgb2 = fusion.fuse_depth_maps(*args, colors=colors, normals=True, simplify=None, **kw)
    _same_mesh(again, mesh, "simplify=None")
    assert torch.equal(rgb2.view(torch.int32), rgb.view(torch.int32))
    report = {}
    got, got_rgb = fusion.fuse_depth_maps(*args, colors=colors, normals=True, simplify=h, report=report, **kw)
    want, want_rgb = meshing.simplify_mesh(mesh, h, colors=rgb)
    _same_mesh(got, want, "fuse_depth_maps(simplify=h)")
    assert torch.equal(got_rgb.view(torch.int32), want_rgb.view(torch.int32))
    assert got.cells is None and got.lattice is None and got.normals is not None
    assert report["simplify"]["vertices"] == (mesh.vertices.shape[0], got.vertices.shape[0]) and report["simplify"]["largest_cluster"] > 1
    assert got.vertices.shape[0] < mesh.vertices.shape[0] // 4          # cells of 3 spacings: about a ninth of the vertices
    # averaged outward normals still point outwards (the inputs' mean angle to the radial direction is a few degrees; a
    # cluster spans at most h sqrt(3) = 0.29 on a sphere of radius 0.8, some 20 degrees: cos(37 deg) = 0.8 leaves room for both); unit length
    v, n = _np(got.vertices).astype(np.float64), _np(got.normals).astype(np.float64)
    dots = (v * n).sum(1) / np.linalg.norm(v, axis=1)
    print(f"simplify end to end: V {mesh.vertices.shape[0]} -> {got.vertices.shape[0]}, F {mesh.faces.shape[0]} -> {got.faces.shape[0]}, closed "
          f"{R.closed_manifold(_np(got.faces))}, chi {R.euler(got.vertices.shape[0], _np(got.faces))}, mean n.r {dots.mean():.4f}, min {dots.min():.4f}")
    assert dots.mean() > 0.8 and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6
    assert float(got_rgb.min()) >= 0.0 and float(got_rgb.max()) <= 1.0
    # without colours and normals: the Mesh alone
    plain = fusion.fuse_depth_maps(*args, simplify=h, **kw)
    assert isinstance(plain, meshing.Mesh) and plain.normals is None
    assert torch.equal(plain.vertices.view(torch.int32), got.vertices.view(torch.int32)) and torch.equal(plain.faces, got.faces)


def test_fuse_mesh_and_extract_mesh_with_simplify_on_the_tile_fixture(tile_scene):  # noqa: F811
    from scanerf_amd import meshing
    rnd, cams = tile_scene["rnd"], tile_scene["cameras"]
    kw = dict(cells_per_axis=20, max_transparency=0.9, scale=2, views_per_batch=2, colors="diffuse", normals=True)
    mesh, rgb = rnd.fuse_mesh(cams, **kw)
    none, rgb_none = rnd.fuse_mesh(cams, simplify=None, **kw)
    _same_mesh(none, mesh, "fuse_mesh(simplify=None)")
    assert torch.equal(rgb_none.view(torch.int32), rgb.view(torch.int32))
    size = [float(s) for s in rnd.scene_box()[1]]
    h = 2.5 * max(size) / 20
    got, got_rgb = rnd.fuse_mesh(cams, simplify=h, **kw)
    want, want_rgb = meshing.simplify_mesh(mesh, h, colors=rgb)
    _same_mesh(got, want, "fuse_mesh(simplify=h)")
    assert torch.equal(got_rgb.view(torch.int32), want_rgb.view(torch.int32))
    # the level-set route, both of its routes
    level = 0.5          # (the fixture's density is low: 2 290 vertices at this level on 20 cells per axis, none at 2)
    for route in ("fused", "dense"):
        full = rnd.extract_mesh(level, 20, route=route, normals=True, min_faces=1)
        assert full.vertices.shape[0] > 0
        _same_mesh(rnd.extract_mesh(level, 20, route=route, normals=True, min_faces=1, simplify=None), full, f"extract_mesh {route} simplify=None")
        report = {}
        got = rnd.extract_mesh(level, 20, route=route, normals=True, min_faces=1, simplify=h, report=report)
        _same_mesh(got, meshing.simplify_mesh(full, h), f"extract_mesh {route} simplify=h")
        assert report["simplify"]["vertices"] == (full.vertices.shape[0], got.vertices.shape[0])
    print(f"simplify on the tile fixture: fused mesh V {mesh.vertices.shape[0]} -> {want.vertices.shape[0]}, level set V {full.vertices.shape[0]} -> "
          f"{got.vertices.shape[0]} at h = {h:.4f}")


# ---- the commands ------------------------------------------------------------------------------------------------------------------
def test_the_simplify_command_and_the_ply_round_trip(tmp_path, capsys):
    from scanerf_amd import formats, meshing
    from test_gpu_mesh_components import _tool
    v, faces, normals, colors = R.lattice_mesh("sphere19")
    src, out, same = str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), str(tmp_path / "same.ply")
    formats.write_ply(src, v, faces, normals=normals, colors=colors)
    assert _tool("simplify_mesh").main([src, out, "--cell", "2", "--origin", "0.5", "0", "-0.25"]) == 0
    assert "vertices 536 -> " in capsys.readouterr().out
    v_in, f_in, n_in, c_in = formats.read_ply(src, normals=True, colors=True)
    want, want_rgb = meshing.simplify_mesh(_mesh(v_in, f_in, n_in), 2.0, origin=(0.5, 0.0, -0.25), colors=_dev(c_in.astype(np.float32) / np.float32(255.0)))
    v_out, f_out, n_out, c_out = formats.read_ply(out, normals=True, colors=True)
    assert R.same_bits(v_out, _np(want.vertices)) and R.same_bits(f_out, _np(want.faces)) and R.same_bits(n_out, _np(want.normals))
    assert np.array_equal(c_out, formats.quantize_colors(_np(want_rgb)))
    # a cell below the vertex spacing: the file's arrays come back, the colours' bytes included
    assert _tool("simplify_mesh").main([src, same, "--cell", "0.25"]) == 0
    back = formats.read_ply(same, normals=True, colors=True)
    assert all(R.same_bits(a, b) for a, b in zip(back, (v_in, f_in, n_in, c_in)))
    # a file without attributes gets none
    bare, bare_out = str(tmp_path / "bare.ply"), str(tmp_path / "bare_out.ply")
    formats.write_ply(bare, v, faces)
    assert _tool("simplify_mesh").main([bare, bare_out, "--cell", "3"]) == 0
    assert formats.ply_vertex_properties(bare_out) == ["x", "y", "z"]
    assert formats.read_ply(bare_out)[0].shape == (R.LATTICE["sphere19"][2][3.0][0], 3)


def test_the_extraction_commands_take_simplify(tile_scene, tmp_path, capsys):  # noqa: F811
    from scanerf_amd import formats
    from test_gpu_mesh_components import _tool
    rnd = tile_scene["rnd"]
    size = [float(s) for s in rnd.scene_box()[1]]
    h = 2.5 * max(size) / 20
    out = str(tmp_path / "fused.ply")
    assert _tool("fuse_mesh").main([tile_scene["path"], "--cameras", tile_scene["log"], "--out", out, "--cells-per-axis", "20", "--scale", "2",
                                    "--max-transparency", "0.9", "--views-per-batch", "2", "--colors", "diffuse", "--normals", "--simplify", repr(h)]) == 0
    want, rgb = rnd.fuse_mesh(tile_scene["cameras"], cells_per_axis=20, max_transparency=0.9, scale=2, views_per_batch=2, colors="diffuse",
                              normals=True, simplify=h)
    v, f, n, c = formats.read_ply(out, normals=True, colors=True)
    assert R.same_bits(v, _np(want.vertices)) and R.same_bits(f, _np(want.faces)) and R.same_bits(n, _np(want.normals))
    assert np.array_equal(c, formats.quantize_colors(_np(rgb)))
    assert "simplified at cell" in capsys.readouterr().out
    out = str(tmp_path / "scene.ply")
    assert _tool("extract_scene_mesh").main([tile_scene["path"], "--level", "0.5", "--cells-per-axis", "20", "--out", out, "--normals", "--min-faces", "1",
                                             "--simplify", repr(h)]) == 0
    want = rnd.extract_mesh(0.5, 20, normals=True, min_faces=1, simplify=h)
    assert want.vertices.shape[0] > 0
    v, f, n = formats.read_ply(out, normals=True)
    assert R.same_bits(v, _np(want.vertices)) and R.same_bits(f, _np(want.faces)) and R.same_bits(n, _np(want.normals))
    assert "simplified at cell" in capsys.readouterr().out
