"""The blended density's gradient on the GPU (csrc/scene_normals.hip; meshing.scene_sigma_normals_points, extract_scene_mesh(normals=True),
TileSetRenderer.extract_mesh, the two commands): sigma against the scene mesh's field and sigma / grad against the
composed route bit for bit, grad and normal against float64 within K x the float32 yardstick's error
(tests/scene_normals_reference.py; profiles/scene_normals_error.md holds the figures), point independence, the mesh ops and the files."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import render_scenes as RS
import scene_mesh_reference as SM
import scene_normals_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def tile_args(sc):
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV).contiguous()
    return dict(feature_tables=t(sc["tables"], torch.float16), resolutions=t(sc["res"], torch.int32), blobs=t(sc["params"], torch.float32),
                corners=t(sc["corners"], torch.float32), sizes=t(sc["sizes"], torch.float32), occupied_grid=t(sc["occ"], torch.bool),
                grid_starts=t(sc["starts"], torch.int64), log2dim=t(sc["l2d"], torch.int32))


def _op(sc, p, route="fused", want_grad=True):
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    pts = torch.from_numpy(np.array(p, np.float32)).to(DEV)
    return meshing.scene_sigma_normals_points(pts, **tile_args(sc), want_grad=want_grad, route=route)


def _against_witness_and_float64(name, sc, p, r64, r32, cap=True):
    """fused sigma and grad == the composed route bit for bit; grad and normal judged against float64 -> fused outputs."""
    sigma, grad, normal = _op(sc, p)
    ws, wg, _ = _op(sc, p, route="dense")
    assert sigma.shape == (len(p),) and grad.shape == (len(p), 3) and normal.shape == (len(p), 3)
    assert torch.equal(_bits(sigma), _bits(ws)), name
    assert torch.equal(_bits(grad), _bits(wg)), name
    idle = torch.as_tensor(r64["run"] == 0, device=DEV)
    assert not bool(_bits(sigma)[idle].any()) and not bool(_bits(grad)[idle].any()) and not bool(_bits(normal)[idle].any())   # +0.0
    bad = R.judge_points(name, grad, normal, r64, r32, cap=cap)
    assert not bad, bad
    return sigma, grad, normal


@pytest.mark.parametrize("c", R.LATTICE_CASES, ids=SM.case_id)
def test_lattice_points_field_bits_witness_bits_and_float64(c):
    """(a): at the lattice points sigma IS the scene mesh's field (meshing._scene_field_dense, whose bits the fused extraction has)."""
    from scanerf_amd import meshing
    sc = SM.scene(c.scene)
    p, r64, r32 = R.lattice_reference(c)
    sigma, _, _ = _against_witness_and_float64(SM.case_id(c), sc, p, r64, r32)
    corner, size = SM.case_box(c)
    a = tile_args(sc)
    field = meshing._scene_field_dense(a["feature_tables"], a["resolutions"], a["blobs"], a["corners"], a["sizes"], a["occupied_grid"],
                                       a["grid_starts"], a["log2dim"], [float(v) for v in corner], [float(v) for v in size], list(c.n))
    assert np.array_equal(sigma.cpu().numpy().view(np.int32), field.reshape(-1).view(np.int32))


@pytest.mark.parametrize("name", R.SCENES)
def test_random_points_witness_bits_and_float64(name):
    """(b), nb = 1 (single) and nb = 65 (G65) among them."""
    p, r64, r32 = R.random_reference(name)
    _against_witness_and_float64(f"{name}-random", SM.scene(name), p, r64, r32)


@pytest.mark.parametrize("name", ["G9", "G9-hole"])
def test_edge_points_witness_bits_and_float64(name):
    """(c): the weight's branches, its kink, faces, corners, W == 0, outside points, listed-but-idle tiles."""
    names, p, r64, r32 = R.edge_reference(name)
    sigma, grad, normal = _against_witness_and_float64(f"{name}-edges", SM.scene(name), p, r64, r32, cap=False)
    for i, nm in enumerate(names):
        print(f"  {nm}: p = {p[i].tolist()}, listed {int(r64['listed'][i])}, contributing {int(r64['run'][i])}, sigma = {float(sigma[i]):.6g}, "
              f"grad = {grad[i].tolist()}")


def _raw(a, pts, want_grad=True, fill=float("nan")):
    """The C entry point on caller-owned, prefilled buffers with guard rows on both sides -> (sigma, grad, normal) bodies."""
    from scanerf_amd import _capi
    N, G = int(pts.shape[0]), 64
    sigma = torch.full((N + 2 * G,), fill, dtype=torch.float32, device=DEV)
    grad = torch.full((3 * N + 2 * G,), fill, dtype=torch.float32, device=DEV)
    normal = torch.full((3 * N + 2 * G,), fill, dtype=torch.float32, device=DEV)
    _capi.check(_capi.lib().scanerf_scene_sigma_normals_points(
        pts.data_ptr(), a["feature_tables"].data_ptr(), a["blobs"].data_ptr(), a["resolutions"].data_ptr(), a["occupied_grid"].data_ptr(),
        a["grid_starts"].data_ptr(), a["log2dim"].data_ptr(), a["corners"].data_ptr(), a["sizes"].data_ptr(),
        int(a["feature_tables"].shape[2]), int(a["feature_tables"].shape[0]), sigma.data_ptr() + 4 * G,
        grad.data_ptr() + 4 * G if want_grad else None, normal.data_ptr() + 4 * G, N, _capi.stream()), "scene_sigma_normals_points")
    torch.cuda.synchronize()
    for t in (sigma, grad, normal):
        assert bool(torch.isnan(t[:G]).all()) and bool(torch.isnan(t[-G:]).all())      # nothing before or behind the outputs
    return sigma[G:-G], grad[G:-G].reshape(N, 3), normal[G:-G].reshape(N, 3)


def test_a_points_bits_depend_on_its_position_alone():
    """Permutation, a second launch, the prefixes (d), NaN-prefilled outputs, grad = null."""
    import scanerf_amd  # noqa
    sc = SM.scene("G9")
    p = R.random_reference("G9")[0]
    a = tile_args(sc)
    pts = torch.from_numpy(np.array(p, np.float32)).to(DEV)
    sigma, grad, normal = _raw(a, pts)
    for t in (sigma, grad, normal):
        assert not bool(torch.isnan(t).any())                                            # every element of every point is written
    ref = _op(sc, p)
    for got, want in zip((sigma, grad, normal), ref):
        assert torch.equal(_bits(got), _bits(want))                                      # two launches: equal bits
    perm = torch.as_tensor(np.random.default_rng(3).permutation(len(p))).to(DEV)
    for got, want in zip(_raw(a, pts[perm].contiguous()), (sigma, grad, normal)):
        assert torch.equal(_bits(got), _bits(want[perm]))
    for N in R.PREFIXES:
        if N == 0:
            s0, g0, n0 = _op(sc, p[:0])
            assert s0.shape == (0,) and g0.shape == (0, 3) and n0.shape == (0, 3) and s0.is_cuda
            continue
        for got, want in zip(_raw(a, pts[:N].contiguous()), (sigma, grad, normal)):
            assert torch.equal(_bits(got), _bits(want[:N])), N
    s1, g1, n1 = _raw(a, pts, want_grad=False)
    assert bool(torch.isnan(g1).all())                                                   # grad = null: not written
    assert torch.equal(_bits(s1), _bits(sigma)) and torch.equal(_bits(n1), _bits(normal))
    s2, g2, n2 = _op(sc, p, want_grad=False)
    assert g2 is None and torch.equal(_bits(s2), _bits(sigma)) and torch.equal(_bits(n2), _bits(normal))


# ---------------------------------------------------------------------------------------------------------------- mesh and commands
def _mesh_args(c):
    sc, corner, size, _, _, _, level = SM.reference(c)
    return dict(tile_args(sc), box_corner=[float(v) for v in corner], box_size=[float(v) for v in size], n=tuple(c.n), level=level)


@pytest.mark.parametrize("c", R.MESH_CASES, ids=SM.case_id)
def test_mesh_vertices_get_the_ops_normals_judged_against_float64(c):
    """extract_scene_mesh(normals=True): the same mesh, normals = the op at its vertices (off-lattice points in brick order); grad and
    normal there against float64 (the reference evaluates the vertices on the CPU)."""
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    args = _mesh_args(c)
    plain = meshing.extract_scene_mesh(**args)
    mesh = meshing.extract_scene_mesh(**args, normals=True)
    assert plain.normals is None and mesh.vertices.shape[0] > 64
    for name in ("vertices", "faces", "cells", "lattice"):
        assert torch.equal(_bits(getattr(mesh, name)), _bits(getattr(plain, name))), name
    sc = SM.scene(c.scene)
    v = mesh.vertices.cpu().numpy()
    sigma, grad, normal = _op(sc, v)
    assert mesh.normals.shape == mesh.vertices.shape and torch.equal(_bits(mesh.normals), _bits(normal))
    r64, r32 = R.reference_at(sc, v)
    bad = R.judge_points(SM.case_id(c) + " vertices", grad, normal, r64, r32)
    assert not bad, bad
    dense = meshing.extract_scene_mesh(**args, route="dense", normals=True)
    assert torch.equal(_bits(dense.vertices), _bits(mesh.vertices)) and dense.normals.shape == mesh.normals.shape


def test_an_empty_mesh_has_empty_normals():
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    c = SM.CASES[0]
    above = float(SM.reference(c)[3]["v"].max()) * 2.0 + 1.0
    for route in ("fused", "dense"):
        m = meshing.extract_scene_mesh(**dict(_mesh_args(c), level=above), route=route, normals=True)
        assert m.vertices.shape == (0, 3) and m.normals.shape == (0, 3) and m.normals.dtype == torch.float32 and m.normals.is_cuda


@pytest.fixture(scope="module")
def g9_renderer():
    import scanerf_amd  # noqa
    from scanerf_amd import renderer
    return renderer.TileSetRenderer(DEV, RS.renderer_tiles(SM.scene("G9")))


def test_the_renderers_method_returns_the_ops_normals(g9_renderer):
    from scanerf_amd import meshing
    rnd = g9_renderer
    level = SM.reference(SM.CASES[0])[6]
    plain = rnd.extract_mesh(level, cells_per_axis=20)
    mesh = rnd.extract_mesh(level, cells_per_axis=20, normals=True)
    assert plain.normals is None and mesh.vertices.shape[0] > 0 and torch.equal(_bits(mesh.vertices), _bits(plain.vertices))
    _, _, want = meshing.scene_sigma_normals_points(mesh.vertices, rnd.feature_tables, rnd.resolution, rnd.params, rnd.block_corner,
                                                    rnd.block_size, rnd.occupied_grid, rnd.grid_starts, rnd.grid_log2dim)
    assert torch.equal(_bits(mesh.normals), _bits(want))
    # unit length wherever a tile contributes; a vertex in a cell no tile occupies (the field is 0 there) has the zero normal
    sigma, _, _ = meshing.scene_sigma_normals_points(mesh.vertices, rnd.feature_tables, rnd.resolution, rnd.params, rnd.block_corner,
                                                     rnd.block_size, rnd.occupied_grid, rnd.grid_starts, rnd.grid_log2dim)
    length = mesh.normals.norm(dim=1)
    assert int((sigma > 0).sum()) > 64 and float((length[sigma > 0] - 1).abs().max()) < 1e-5 and not bool(mesh.normals[sigma == 0].any())


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _export(tmp_path, sc):
    from scanerf_amd import renderer
    dirs = []
    for b, tile in enumerate(RS.renderer_tiles(sc)):
        path = str(tmp_path / f"tile-{b}")
        os.makedirs(path)
        t = torch.as_tensor
        renderer.write_feature_npz(path, t(tile["features"]), t(tile["occupied_grid"]), t(tile["block_corner"]), t(tile["block_size"]),
                                   t(tile["grid_log2dim"]), t(tile["resolution"]))
        torch.save(dict(SM.O.unpack_blob(torch.from_numpy(tile["blob"]))), os.path.join(path, "decoder.pth"))
        dirs.append(path)
    return dirs


def test_the_commands_write_normals(tmp_path, g9_renderer):
    """tools/extract_scene_mesh.py --normals: the renderer's mesh and normals in one PLY; tools/extract_mesh.py --normals: per-tile
    PLYs with the tile density's normals."""
    from scanerf_amd import formats
    dirs = _export(tmp_path, SM.scene("G9"))
    level = SM.reference(SM.CASES[0])[6]
    out = str(tmp_path / "mesh" / "scene.ply")
    assert _tool("extract_scene_mesh").main([*dirs, "--level", repr(level), "--cells-per-axis", "20", "--normals", "--out", out]) == 0
    want = g9_renderer.extract_mesh(level, cells_per_axis=20, normals=True)
    rv, rf, rn = formats.read_ply(out, normals=True)
    assert np.array_equal(rv, want.vertices.cpu().numpy()) and np.array_equal(rf, want.faces.cpu().numpy())
    assert np.array_equal(rn.view(np.int32), want.normals.cpu().numpy().view(np.int32))
    # per tile
    tool = _tool("extract_mesh")
    outdir = str(tmp_path / "tiles")
    assert tool.main([*dirs[:2], "--level", repr(level), "--cells-per-axis", "16", "--normals", "--out", outdir]) == 0
    from scanerf_amd import renderer
    for path in dirs[:2]:
        m = tool.extract_tile(renderer.load_tile(path), 16, level, DEV, normals=True)
        rv, rf, rn = formats.read_ply(os.path.join(outdir, os.path.basename(path) + ".ply"), normals=True)
        assert m.vertices.shape[0] > 0 and np.array_equal(rv, m.vertices.cpu().numpy()) and np.array_equal(rf, m.faces.cpu().numpy())
        assert np.array_equal(rn.view(np.int32), m.normals.cpu().numpy().view(np.int32))
