"""The scene mesh on the GPU (csrc/isosurface.hip's scene source; meshing.extract_scene_mesh, TileSetRenderer.extract_mesh,
tools/extract_scene_mesh.py): the fused route against the composed one bit for bit, against float64 (cells and faces
exactly outside the ambiguity band, vertices within K x the float32 yardstick's error; profiles/scene_mesh_error.md holds the figures),
determinism, guards, empty scenes, the renderer's method and the command."""
import ctypes
import os

import numpy as np
import pytest
import torch

import render_scenes as RS
import scene_mesh_reference as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def scene_args(sc, corner, size, n, level):
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV).contiguous()
    return dict(feature_tables=t(sc["tables"], torch.float16), resolutions=t(sc["res"], torch.int32), blobs=t(sc["params"], torch.float32),
                corners=t(sc["corners"], torch.float32), sizes=t(sc["sizes"], torch.float32), occupied_grid=t(sc["occ"], torch.bool),
                grid_starts=t(sc["starts"], torch.int64), log2dim=t(sc["l2d"], torch.int32), box_corner=[float(v) for v in corner],
                box_size=[float(v) for v in size], n=tuple(n), level=level)


def _case_args(c):
    sc, corner, size, _, _, _, level = M.reference(c)
    return scene_args(sc, corner, size, c.n, level)


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_fused_against_the_composed_route_and_float64(c):
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    sc, corner, size, b64, b32, live, level = M.reference(c)
    args = _case_args(c)
    fused = meshing.extract_scene_mesh(**args, route="fused")
    dense = meshing.extract_scene_mesh(**args, route="dense")
    again = meshing.extract_scene_mesh(**args, route="fused")
    assert fused.normals is None and fused.vertices.shape[0] > 0 and fused.faces.shape[0] > 0
    assert fused.vertices.dtype == torch.float32 and fused.faces.dtype == torch.int32 and fused.cells.dtype == torch.int32
    # the composed route: the same V and F, the same rows in the same order, bit for bit
    assert fused.vertices.shape == dense.vertices.shape and fused.faces.shape == dense.faces.shape
    for name in ("vertices", "faces", "cells", "lattice"):
        assert torch.equal(_bits(getattr(fused, name)), _bits(getattr(dense, name))), name
        assert torch.equal(_bits(getattr(fused, name)), _bits(getattr(again, name))), name      # two launches: equal bits
    # world positions: box_corner + L * (box_size / n), separately rounded
    step = torch.tensor([float(np.float32(s) / np.float32(m)) for s, m in zip(size, c.n)], dtype=torch.float32, device=DEV)
    world = torch.tensor(np.asarray(corner, np.float32), device=DEV) + fused.lattice * step
    assert torch.equal(_bits(fused.vertices), _bits(world))
    assert int(fused.faces.min()) >= 0 and int(fused.faces.max()) < fused.vertices.shape[0]
    # against float64
    amb, judged = M.judged(c)
    assert 1.0 - judged.mean() <= M.CAP and judged.sum() >= M.MIN_JUDGED
    r64, r32 = M.surface_nets(b64["v"], level), M.surface_nets(b32["v"], level, dtype=np.float32)
    bad = M.judge_mesh(M.case_id(c), fused, r64, r32, judged)
    assert not bad, bad


def test_guard_regions_and_outputs_smaller_than_the_scratch_says():
    """The C entry points on caller-owned buffers prefilled with a sentinel: exactly V / F rows are written, nothing before or behind
    them, nothing outside the scratch; with V or F declared too small the bricks that would not fit are left unwritten."""
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    lib = _capi.lib()
    c = M.CASES[0]
    a = _case_args(c)
    G = 256
    nbytes = lib.scanerf_isosurface_scratch_bytes(*c.n)
    scratch = torch.full((nbytes + 2 * G,), 0x5A, dtype=torch.uint8, device=DEV)
    f3 = lambda v: (ctypes.c_float * 3)(*v)
    head = (a["feature_tables"].data_ptr(), a["blobs"].data_ptr(), a["resolutions"].data_ptr(), a["occupied_grid"].data_ptr(),
            a["grid_starts"].data_ptr(), a["log2dim"].data_ptr(), a["corners"].data_ptr(), a["sizes"].data_ptr(),
            a["feature_tables"].shape[2], a["feature_tables"].shape[0], f3(a["box_corner"]), f3(a["box_size"]), *c.n, float(a["level"]))
    _capi.check(lib.scanerf_isosurface_count_tiles(*head, scratch.data_ptr() + G, nbytes, _capi.stream()), "count")
    V, F = scratch[G:G + 16].view(torch.int64).tolist()
    assert V > 0 and F > 0
    assert bool((scratch[:G] == 0x5A).all()) and bool((scratch[G + nbytes:] == 0x5A).all())

    def buffers(V, F):
        return {k: torch.full((rows * 3 + 2 * G,), fill, dtype=dt, device=DEV)
                for k, rows, fill, dt in (("vertices", V, 7.0, torch.float32), ("faces", F, -7, torch.int32), ("cells", V, -7, torch.int32),
                                          ("lattice", V, 7.0, torch.float32))}

    def emit(bufs, V, F):
        ptr = lambda k: bufs[k].data_ptr() + 4 * G
        _capi.check(lib.scanerf_isosurface_emit_tiles(*head, scratch.data_ptr() + G, nbytes, ptr("vertices"), ptr("faces"), ptr("cells"),
                                                      ptr("lattice"), V, F, _capi.stream()), "emit")
        torch.cuda.synchronize()

    def guards_hold(bufs):
        for k, b in bufs.items():
            fill = 7.0 if b.dtype == torch.float32 else -7
            assert bool((b[:G] == fill).all()) and bool((b[-G:] == fill).all()), k

    full = buffers(V, F)
    emit(full, V, F)
    guards_hold(full)
    for k, b in full.items():
        assert not bool((b[G:-G] == (7.0 if b.dtype == torch.float32 else -7)).any()), k     # every element between them was written
    vbase = scratch[G + 64 + 64 * 8:G + 64 + 64 * 8 + 4 * 9].view(torch.int32).tolist()        # 8 bricks: masks, then vbase [9]
    assert vbase[-1] == V and vbase[0] == 0
    # one vertex short: the last brick with a vertex does not fit and is left unwritten, the others are as before
    last = max(i for i in range(8) if vbase[i + 1] > vbase[i])
    small = buffers(V - 1, F)
    emit(small, V - 1, F)
    guards_hold(small)
    body = lambda bufs, k: bufs[k][G:-G]
    assert torch.equal(_bits(body(small, "vertices")[:3 * vbase[last]]), _bits(body(full, "vertices")[:3 * vbase[last]]))
    assert bool((body(small, "vertices")[3 * vbase[last]:] == 7.0).all())
    # two triangles short
    small = buffers(V, F - 2)
    emit(small, V, F - 2)
    guards_hold(small)
    assert bool((body(small, "faces") == -7).any())


def test_empty_scenes_give_valid_empty_meshes():
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    c = M.CASES[0]
    a = _case_args(c)
    b64 = M.reference(c)[3]
    above = float(b64["v"].max()) * 2.0 + 1.0
    clear = dict(a, occupied_grid=torch.zeros_like(a["occupied_grid"]))
    for args in (dict(a, level=above), clear):
        for route in ("fused", "dense"):
            m = meshing.extract_scene_mesh(**args, route=route)
            assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.cells.shape == (0, 3) and m.lattice.shape == (0, 3)
            assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.vertices.is_cuda


@pytest.fixture(scope="module")
def g9_renderer():
    import scanerf_amd  # noqa
    from scanerf_amd import renderer
    return renderer.TileSetRenderer(DEV, RS.renderer_tiles(M.scene("G9")))


def test_the_renderers_method_is_the_op_on_its_arrays(g9_renderer):
    from scanerf_amd import meshing
    rnd = g9_renderer
    level = M.reference(M.CASES[0])[6]
    corner, size = rnd.scene_box()
    lo, sz = M.scene_bound(M.scene("G9"))
    assert np.array_equal(np.float32(corner), lo) and np.array_equal(np.float32(size), sz)
    got = rnd.extract_mesh(level, cells_per_axis=20)
    n = meshing.cells_per_axis(size, 20)
    assert n == [20, 8, 20]
    want = meshing.extract_scene_mesh(rnd.feature_tables, rnd.resolution, rnd.params, rnd.block_corner, rnd.block_size, rnd.occupied_grid,
                                      rnd.grid_starts, rnd.grid_log2dim, corner, size, n, level)
    assert got.vertices.shape[0] > 0 and got.normals is None
    for name in ("vertices", "faces", "cells", "lattice"):
        assert torch.equal(_bits(getattr(got, name)), _bits(getattr(want, name))), name
    # a box of the caller's: the part of the scene inside it
    part = rnd.extract_mesh(level, cells_per_axis=12, box=([2.0, -1.0, 2.0], [5.0, 2.0, 5.0]))
    v = part.vertices
    assert v.shape[0] > 0 and bool((v >= torch.tensor([2.0, -1.0, 2.0], device=DEV)).all()) and bool((v <= torch.tensor([7.0, 1.0, 7.0], device=DEV)).all())


def test_the_command_round_trip(tmp_path, g9_renderer):
    """Tiles written as renderer.export_tile writes them -> tools/extract_scene_mesh.py -> formats.read_ply: the renderer's mesh."""
    import importlib.util
    from scanerf_amd import formats, network, renderer
    sc = M.scene("G9")
    dirs = []
    for b, tile in enumerate(RS.renderer_tiles(sc)):
        path = str(tmp_path / f"tile-{b}")
        os.makedirs(path)
        t = torch.as_tensor
        renderer.write_feature_npz(path, t(tile["features"]), t(tile["occupied_grid"]), t(tile["block_corner"]), t(tile["block_size"]),
                                   t(tile["grid_log2dim"]), t(tile["resolution"]))
        torch.save(dict(M.O.unpack_blob(torch.from_numpy(tile["blob"]))), os.path.join(path, "decoder.pth"))
        assert np.array_equal(renderer.load_tile(path)["blob"], tile["blob"])
        dirs.append(path)
    spec = importlib.util.spec_from_file_location("extract_scene_mesh_tool", os.path.join(ROOT, "tools", "extract_scene_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    level = M.reference(M.CASES[0])[6]
    out = str(tmp_path / "mesh" / "scene.ply")
    assert tool.main([*dirs, "--level", repr(level), "--cells-per-axis", "20", "--out", out]) == 0
    want = g9_renderer.extract_mesh(level, cells_per_axis=20)
    rv, rf = formats.read_ply(out)[:2]
    assert np.array_equal(np.asarray(rv, np.float32), want.vertices.cpu().numpy()) and np.array_equal(np.asarray(rf, np.int32), want.faces.cpu().numpy())
