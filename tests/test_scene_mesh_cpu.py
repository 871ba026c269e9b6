"""The scene mesh without a GPU: the float64 reference of tests/scene_mesh_reference.py holds the edges its cases are
named for and the condition the GPU judgement stands on, shows what the feature is for (one closed surface where the per-tile meshes
are open), reduces to the single tile's field, and the new entry points refuse bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import scene_mesh_reference as M
import surface_nets_reference as SR
from oracle import oracle as O

CASE = {M.case_id(c): c for c in M.CASES}


def test_every_case_holds_the_edge_it_is_named_for():
    run = lambda name: M.reference(CASE[name])[3]
    assert run("STACK6-n16x16x16-bound")["listed"].max() >= 5            # more tiles on a point than a slot list holds
    assert run("STACK6-n11x13x9-cut")["listed"].max() >= 5
    assert run("G9-n16x16x16-bound")["listed"].max() >= 2 and run("G9-n37x5x29-bound")["listed"].max() == 4
    assert run("single-n16x16x16-bound")["listed"].max() == 1
    for c in M.CASES:                                                    # points with W > 0 and no contributor
        b64 = M.reference(c)[3]
        assert ((b64["W"] > 0) & (b64["run"] == 0)).any(), M.case_id(c)
        assert (b64["v"][b64["run"] == 0] == 0).all() and (b64["v"] >= 0).all()
    # whole bricks that no tile's box reaches, and bricks a tile reaches where nothing contributes
    grown = run("G9-n88x5x88-grown")
    assert (~M.brick_has(grown["listed"] > 0)).sum() >= 20
    hole = run("G9-hole-n72x4x72-bound")
    assert (M.brick_has(hole["listed"] > 0) & ~M.brick_has(hole["run"] > 0)).sum() >= 1
    # the cleared tile leaves no hole in the field: its neighbours' margins contribute around its own 2 x 2
    h16, g16 = run("G9-hole-n16x16x16-bound"), run("G9-n16x16x16-bound")
    assert (h16["run"] < g16["run"]).any() and ((h16["run"] > 0) & (h16["run"] < g16["run"])).any()
    # a zeroed table is not an absent tile: it contributes its constant density
    z16 = run("G9-zero-n16x16x16-bound")
    assert np.array_equal(z16["run"], g16["run"]) and not np.array_equal(z16["v"], g16["v"])
    # more tiles than a wave has lanes, and the last of them contributes
    c = CASE["G65-n19x5x45-bound"]
    sc, corner, size = M.reference(c)[:3]
    assert sc["corners"].shape[0] == 65 and M.pinned_tiles(sc, corner, size, c.n)["tiles"][64]["run"].any()
    # ragged lattices: no axis a multiple of the brick; a lattice one cell thick
    assert all(m % M.BRICK for m in CASE["G9-n37x5x29-bound"].n) and CASE["G9-n70x1x9-bound"].n[1] == 1
    # the cutting box starts and ends inside tiles
    c = CASE["G9-n19x7x21-cut"]
    lo, size = M.scene_bound(M.scene(c.scene))
    corner, csize = M.case_box(c)
    assert (corner > lo).all() and (corner + csize < lo + size).all()


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_the_ambiguity_band_leaves_the_judgement_its_cells(c):
    """The condition that keeps the GPU judgement from hiding a failure: at most CAP of the cells are left out, at least MIN_JUDGED
    are judged, the level lies strictly between lattice values, and the float32 yardstick agrees with float64 on every judged cell."""
    sc, corner, size, b64, b32, live, level = M.reference(c)
    amb, judged = M.judged(c)
    assert level > 0 and not (b64["v"].astype(np.float32) == np.float32(level)).any()
    assert 1.0 - judged.mean() <= M.CAP and judged.sum() >= M.MIN_JUDGED, (1.0 - judged.mean(), judged.sum())
    r64, r32 = M.surface_nets(b64["v"], level), M.surface_nets(b32["v"], level, dtype=np.float32)
    assert len(r64.vertices) >= 100
    assert not M.judge_mesh(M.case_id(c), r32, r64, r32, judged)


def test_one_closed_surface_where_the_tile_meshes_are_open():
    """What the feature is for.  A ball of occupied cells around a four-tile corner, every tile's density a constant: the blended
    field's level set is ONE closed oriented manifold; the level sets of the four tiles that hold it, each over its own box as
    tools/extract_mesh.py extracts them, are open where the ball crosses their faces."""
    sc = M.blob_scene()
    corner, size = M.scene_bound(sc)
    pin = M.pinned_tiles(sc, corner, size, M.BLOB_N)
    b64 = M.blend(sc, pin, np.float64)
    sigma = [float(M.tile_sigma(sc, b, np.zeros((1, 3), np.float32), M.F64)[0]) for b in range(sc["corners"].shape[0])]
    level = 0.25 * min(sigma)
    assert level > 0
    holders = [b for b, t in enumerate(pin["tiles"]) if t["run"].any()]
    assert holders == [0, 1, 3, 4]                       # the four tiles of the corner (ix, iz) in {0, 1}^2
    mesh = M.surface_nets(b64["v"], level, corner, size / np.asarray(M.BLOB_N, np.float32))
    closed, chi, vol = M.topology(mesh)
    assert closed and chi == 2 and vol > 0
    ball = 4.0 / 3.0 * np.pi * M.BLOB_RADIUS ** 3
    assert ball < vol < 4.0 * ball                       # the occupied cells that hold the ball, no more than a cell around it
    for b in holders:
        G = tuple(2 ** int(k) for k in sc["l2d"][b])
        lo = int(sc["starts"][b])
        occ = np.asarray(sc["occ"][lo:lo + int(np.prod(G))]).reshape(G)
        tile = SR.surface_nets(np.where(SR.live_points((16, 16, 16), occ), sigma[b], 0.0), level)
        assert len(tile.faces) and not SR.topology(tile)[0], b


def test_the_blend_of_one_tile_is_that_tiles_field():
    """A scene of one tile on the tile's own box: where the tile is listed with a weight, w sigma / w is model_reference's sigma at the
    same lattice point.  The two routes reach the contracted position by different float32 expressions (2 ((corner + i step) - corner)
    / size - 1 against i (2 / n) - 1); the density moves by its gradient times that difference, so the bound per point is
    4 sum_k |d sigma / d x_k| |dx_k| (4: the gradient is piecewise, a point may change cell) + 2^-40 sigma for the float64 blend."""
    c = SR.MODEL_CASES[1]                                # base, f16 table, n = (17, 9, 5), full occupancy
    ins, live, s64, _, _ = SR.model_reference(c)
    assert c.pattern == "full" and live.all() and bool((SR.NR.case_mask(ins) == 1).all())
    sc = {"corners": ins["occ_corner"][None], "sizes": ins["occ_size"][None], "l2d": np.int32([c.log2dim]), "starts": np.zeros(1, np.int64),
          "occ": ins["occ"].reshape(-1), "tables": ins["table"].numpy()[None], "params": O.pack_blob(ins["sd"]).numpy()[None],
          "res": ins["res"].numpy()[None]}
    pin = M.pinned_tiles(sc, ins["occ_corner"], ins["occ_size"], c.n)
    t = pin["tiles"][0]
    assert t["listed"].all() and t["run"].all()
    b64 = M.blend(sc, pin, np.float64)
    x_model = SR.lattice_positions(c.n).reshape(-1, 3)
    dx = np.abs(t["x"].astype(np.float64) - x_model.astype(np.float64))
    assert dx.max() <= 2.0 ** -21                        # a few ulps of 1
    g = SR.NR.sigma_normals(x_model, np.ones(3, np.float32), ins["table"], ins["res"], ins["sd"], torch.ones(32), SR.NR.F64)["g"].abs().numpy()
    bound = (4.0 * (g * dx).sum(1) + 2.0 ** -40 * s64.reshape(-1)).reshape(s64.shape)
    weighted = b64["W"] > 0
    assert weighted.sum() >= 0.9 * weighted.size
    assert (np.abs(b64["v"] - s64)[weighted] <= bound[weighted]).all()
    assert (b64["v"][~weighted] == 0).all()             # the box's vertical edges: both distances are 0, the weight is 0


# ------------------------------------------------------------------------------------------------------------------- arguments
def _entries():
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    return _capi.lib(), _capi


def _err(lib):
    return lib.scanerf_last_error().decode()


def test_the_new_entries_validate_before_any_launch():
    lib, _capi = _entries()
    assert lib.scanerf_abi_version() == 10
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    p = 4096                                              # a non-null, 16-byte aligned address that is never dereferenced
    tiles = [p] * 8
    good = dict(T=1024, nb=9, corner=f3(0, 0, 0), size=f3(10, 4, 10), n=(16, 16, 16), level=1.0)

    def count(tiles=tiles, scratch=p, nbytes=None, **kw):
        a = dict(good, **kw)
        nbytes = lib.scanerf_isosurface_scratch_bytes(16, 16, 16) if nbytes is None else nbytes
        return lib.scanerf_isosurface_count_tiles(*tiles, a["T"], a["nb"], a["corner"], a["size"], *a["n"], a["level"], scratch, nbytes, None)

    def emit(tiles=tiles, scratch=p, out=(p, p, p, p), V=8, F=12, **kw):
        a = dict(good, **kw)
        nbytes = lib.scanerf_isosurface_scratch_bytes(16, 16, 16)
        return lib.scanerf_isosurface_emit_tiles(*tiles, a["T"], a["nb"], a["corner"], a["size"], *a["n"], a["level"], scratch, nbytes, *out, V, F,
                                                 None)

    for call, name in ((count, "isosurface_count_tiles"), (emit, "isosurface_emit_tiles")):
        for k in range(8):
            assert call(tiles=[None if i == k else p for i in range(8)]) != 0 and "null pointer" in _err(lib) and name in _err(lib)
        assert call(corner=None) != 0 and "box_corner" in _err(lib)
        assert call(size=None) != 0 and "box_size" in _err(lib)
        assert call(scratch=None) != 0 and "scratch" in _err(lib)
        assert call(nb=0) != 0 and "nb=0" in _err(lib)
        assert call(nb=-3) != 0 and "nb=-3" in _err(lib)
        assert call(T=1000) != 0 and "power of two" in _err(lib)
        assert call(T=1) != 0 and "power of two" in _err(lib)
        assert call(size=f3(10, 0, 10)) != 0 and "box_size[1]" in _err(lib)
        assert call(size=f3(-1, 4, 10)) != 0 and "box_size[0]" in _err(lib)
        assert call(size=f3(10, 4, float("inf"))) != 0 and "box_size[2]" in _err(lib)
        assert call(size=f3(10, 4, float("nan"))) != 0 and "box_size[2]" in _err(lib)
        assert call(level=0.0) != 0 and "level" in _err(lib)
        assert call(level=-1.0) != 0 and "level" in _err(lib)
        assert call(n=(0, 16, 16)) != 0 and "n_k" in _err(lib)
        assert call(n=(2048, 2048, 2048)) != 0 and "2^31" in _err(lib)
    assert count(nbytes=lib.scanerf_isosurface_scratch_bytes(16, 16, 16) - 1) != 0 and "scratch holds" in _err(lib)
    assert count(scratch=p + 4) != 0 and "aligned" in _err(lib)
    assert count(tiles=[p + 8] + [p] * 7) != 0 and "16-byte aligned" in _err(lib)
    assert emit(out=(None, p, p, p)) != 0 and "vertices" in _err(lib)
    assert emit(out=(p, None, p, p)) != 0 and "faces" in _err(lib)
    assert emit(F=11) != 0 and "F=11" in _err(lib)
    assert emit(V=-1) != 0
    assert emit(out=(None, None, None, None), V=0, F=0) == 0    # an empty mesh: a no-op, nothing is launched
    assert lib.scanerf_isosurface_scratch_bytes(16, 16, 16) == 72 * 8 + 72


def test_extract_scene_mesh_refuses_bad_arguments():
    _entries()
    from scanerf_amd import meshing, renderer
    nb, T = 2, 64
    a = dict(feature_tables=torch.zeros(nb, 16, T, 2, dtype=torch.float16), resolutions=torch.zeros(nb, 16, 3, dtype=torch.int32),
             blobs=torch.zeros(nb, 13994), corners=torch.zeros(nb, 3), sizes=torch.ones(nb, 3), occupied_grid=torch.zeros(2 * 512, dtype=torch.bool),
             grid_starts=torch.tensor([0, 512]), log2dim=torch.full((nb, 3), 3, dtype=torch.int32), box_corner=[0, 0, 0], box_size=[1, 1, 1],
             n=(8, 8, 8), level=1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.extract_scene_mesh(**a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.extract_scene_mesh(**a, route="dense")
    with pytest.raises(RuntimeError, match="route"):
        meshing.extract_scene_mesh(**a, route="welded")
    with pytest.raises(RuntimeError, match="3 cell counts"):
        meshing.extract_scene_mesh(**dict(a, n=(8, 8)))
    with pytest.raises(RuntimeError, match="is None"):
        meshing.extract_scene_mesh(**dict(a, feature_tables=None))
    assert callable(renderer.TileSetRenderer.extract_mesh) and callable(renderer.TileSetRenderer.scene_box)


def test_the_scene_tool_has_its_own_command_line():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("extract_scene_mesh_tool", os.path.join(root, "tools", "extract_scene_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ap = tool.parser()
    args = ap.parse_args(["a", "b", "--level", "2.5", "--box", "0", "1", "2", "3", "4", "5", "--out", "scene.ply"])
    assert args.tiles == ["a", "b"] and args.level == 2.5 and args.box == [0, 1, 2, 3, 4, 5] and args.cells_per_axis == 256
    assert args.route == "fused" and "ONE mesh" in ap.format_help()
    with pytest.raises(SystemExit):
        ap.parse_args(["a", "--level", "1"])             # --out is required
