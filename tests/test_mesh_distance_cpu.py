"""The closest-point query's definition, its numpy references and the evaluation's torch parts, without a GPU: closed-form answers of
tests/mesh_distance_reference.py, sample_surface's properties, the score arithmetic, the conditions the GPU case list stands on, the
prototypes, and every refusal that has to come before a library call."""
import math
import os
import re

import numpy as np
import pytest
import torch

import fastmesh_reference as FR
import mesh_distance_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRI_V = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float32)
TRI_F = np.array([[0, 1, 2]], np.int32)
# point, closest point, distance: the seven Voronoi regions, then a vertex, two edges and the inside (d = 0)
TRI_CASES = [
    ((-1, -1, 1), (0, 0, 0), math.sqrt(3)),      # vertex A
    ((3, -1, 0), (2, 0, 0), math.sqrt(2)),       # vertex B
    ((-1, 3, 0), (0, 2, 0), math.sqrt(2)),       # vertex C
    ((1, -1, 2), (1, 0, 0), math.sqrt(5)),       # edge AB
    ((-1, 1, 0), (0, 1, 0), 1.0),                # edge AC
    ((2, 2, 0), (1, 1, 0), math.sqrt(2)),        # edge BC
    ((0.5, 0.5, 3), (0.5, 0.5, 0), 3.0),         # interior
    ((2, 0, 0), (2, 0, 0), 0.0), ((1, 0, 0), (1, 0, 0), 0.0), ((1, 1, 0), (1, 1, 0), 0.0), ((0.5, 0.5, 0), (0.5, 0.5, 0), 0.0),
]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_triangle_every_voronoi_region(dtype):
    P = np.array([c[0] for c in TRI_CASES], np.float32)
    d2, face, q = R.closest(P, TRI_V, TRI_F, dtype)
    assert d2.dtype == dtype and (face == 0).all()
    np.testing.assert_allclose(np.sqrt(d2.astype(np.float64)), [c[2] for c in TRI_CASES], rtol=0, atol=1e-6 if dtype == np.float32 else 1e-14)
    np.testing.assert_allclose(q, [c[1] for c in TRI_CASES], rtol=0, atol=1e-6 if dtype == np.float32 else 1e-14)
    assert (d2[7:] == 0).all()


def test_unit_cube_against_the_box_distance():
    V, F = FR._CUBE.astype(np.float32), np.array(FR._CUBE_FACES, np.int32)
    rng = np.random.default_rng(1)
    P = np.concatenate([rng.uniform(0, 1, (200, 3)), rng.uniform(-2, 3, (300, 3))]).astype(np.float32)
    p = P.astype(np.float64)
    outside = np.linalg.norm(np.maximum(np.maximum(-p, p - 1), 0), axis=1)
    inside = np.minimum(p, 1 - p).min(1)
    want = np.where(outside > 0, outside, inside)      # |signed box distance|
    d2, face, q = R.closest(P, V, F)
    np.testing.assert_allclose(np.sqrt(d2), want, rtol=0, atol=1e-14)
    assert (face >= 0).all()
    np.testing.assert_allclose(np.linalg.norm(p - q, axis=1), want, rtol=0, atol=1e-14)


def test_permuting_faces_and_corners_leaves_the_distance():
    V, F, _ = FR.terrain_fixture()
    P = R.terrain_points()[::16]
    d2, _, _ = R.closest(P, V, F)
    rng = np.random.default_rng(2)
    Fp = F[rng.permutation(len(F))]
    Fp = np.stack([np.roll(f, k) for f, k in zip(Fp, rng.integers(0, 3, len(Fp)))]).astype(np.int32)
    e2, _, _ = R.closest(P, V, Fp)
    np.testing.assert_allclose(np.sqrt(e2), np.sqrt(d2), rtol=0, atol=1e-12)


def test_dead_faces_are_ignored():
    Vd = R.dead_vertices()
    assert not R.live32(Vd, np.array([[0, 1, 2]], np.int32)).any()             # collinear
    assert not R.live32(TRI_V, np.array([[1, 1, 2]], np.int32)).any()          # two equal indices
    V = np.concatenate([Vd, TRI_V + np.float32(5)])
    F = np.array([[0, 1, 2], [4, 4, 5], [3, 4, 5]], np.int32)
    P = np.array([[0.5, 0.5, 0.5], [5, 5, 5]], np.float32)                     # the first ON the dead collinear face
    for dtype in (np.float64, np.float32):
        d2, face, _ = R.closest(P, V, F, dtype)
        assert (face == 2).all() and d2[1] == 0 and d2[0] > 1
        d2, face, q = R.closest(P, V, F[:2], dtype)                            # only dead faces
        assert np.isinf(d2).all() and (face == -1).all() and np.array_equal(q, P.astype(dtype))


def test_empty_mesh_and_non_finite_points():
    P = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0.2, 0.2, 1]], np.float32)
    d2, face, q = R.closest(P, TRI_V, np.zeros((0, 3), np.int32))
    assert np.isinf(d2).all() and (face == -1).all()
    d2, face, q = R.closest(P, TRI_V, TRI_F)
    assert np.isinf(d2[1:3]).all() and (face[1:3] == -1).all() and (face[[0, 3]] == 0).all()
    assert d2[0] == 0 and d2[3] == 1 and np.array_equal(q[1:3], P[1:3].astype(np.float64), equal_nan=True)
    bad = np.array([[0, 1, 7], [0, 1, 2]], np.int32)                            # a vertex index outside [0, V): left out by the build
    assert R.registered32(TRI_V, bad).tolist() == [False, True]
    assert R.closest(P[:1], TRI_V, bad)[1][0] == 1


# ---- sample_surface ---------------------------------------------------------------------------------------------------------------
def _two_triangles():
    """areas 1 : 3, a zero-area face between them"""
    V = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 5], [3, 0, 5], [0, 2, 5.0]], dtype=torch.float32)
    F = torch.tensor([[0, 1, 2], [1, 1, 2], [3, 4, 5]], dtype=torch.int32)
    return V, F


def test_sample_surface_properties():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation
    V, F = _two_triangles()
    n, seed = 1001, 5
    pts, face = evaluation.sample_surface(V, F, n, seed)
    assert pts.shape == (n, 3) and pts.dtype == torch.float32 and face.shape == (n,) and face.dtype == torch.int64
    assert not (face == 1).any()                                                # the zero-area face is never chosen
    # in the face's plane with non-negative barycentrics (solved in float64 from the float32 points: their rounding is the tolerance)
    tri = V.double()[F.long()[face]]
    A, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    sol = torch.linalg.lstsq(torch.stack([ab, ac], -1), (pts.double() - A)[..., None]).solution[:, :, 0]
    back = A + sol[:, :1] * ab + sol[:, 1:] * ac
    assert (back - pts.double()).abs().max() < 1e-6
    assert sol.min() > -1e-6 and (sol.sum(1) < 1 + 1e-6).all()
    # the prefix-sum bracket of u_i = (i + xi_i) / n * total, xi = the first column of the documented draw
    r = torch.rand(n, 3, dtype=torch.float64, generator=torch.Generator(device="cpu").manual_seed(seed))
    area = torch.tensor([1.0, 0.0, 3.0], dtype=torch.float64)
    cum = torch.cumsum(area, 0)
    u = (torch.arange(n, dtype=torch.float64) + r[:, 0]) / n * cum[-1]
    lo = torch.cat([torch.zeros(1, dtype=torch.float64), cum[:-1]])[face]
    assert ((lo <= u) & (u < cum[face])).all()
    # stratification: each face's count within 1 of n area / total
    for f_, a in ((0, 1.0), (2, 3.0)):
        assert abs(int((face == f_).sum()) - n * a / 4.0) <= 1.0
    # the same seed gives the same bits; another seed does not
    pts2, face2 = evaluation.sample_surface(V, F, n, seed)
    assert torch.equal(pts, pts2) and torch.equal(face, face2)
    assert not torch.equal(evaluation.sample_surface(V, F, n, seed + 1)[0], pts)
    with pytest.raises(ValueError, match="no area"):
        evaluation.sample_surface(V, F[1:2], 10, 0)


def test_score_arithmetic_on_hand_made_distances():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation
    inf = float("inf")
    a = torch.tensor([0.0, 1.0, 2.0, 3.0, inf])        # pred -> gt: 4 of 5 found
    b = torch.tensor([0.5, 0.5, 4.0, inf, inf, inf, 1.5, 0.25])
    s = evaluation.summarize(a, b, [1.0, 2.5])
    pg, gp = s["pred_to_gt"], s["gt_to_pred"]
    assert pg["n"] == 5 and pg["not_found"] == pytest.approx(0.2) and pg["mean"] == pytest.approx(1.5)
    assert pg["median"] == pytest.approx(1.0) and pg["rms"] == pytest.approx(math.sqrt(14 / 4))
    assert gp["n"] == 8 and gp["not_found"] == pytest.approx(3 / 8) and gp["mean"] == pytest.approx(6.75 / 5)
    assert gp["median"] == pytest.approx(0.5)
    assert s["precision"] == {1.0: pytest.approx(0.4), 2.5: pytest.approx(0.6)}
    assert s["recall"] == {1.0: pytest.approx(3 / 8), 2.5: pytest.approx(4 / 8)}
    assert s["fscore"][1.0] == pytest.approx(2 * 0.4 * 0.375 / 0.775) and s["fscore"][2.5] == pytest.approx(2 * 0.6 * 0.5 / 1.1)
    assert s["chamfer"] == pytest.approx(0.5 * (1.5 + 1.35))
    z = evaluation.summarize(torch.tensor([inf]), torch.tensor([inf]), [1.0])
    assert z["fscore"][1.0] == 0.0 and math.isnan(z["chamfer"]) and z["pred_to_gt"]["not_found"] == 1.0
    import json
    line = json.loads(evaluation.json_line(dict(s, distances="dropped")))
    assert "distances" not in line and line["precision"]["1.0"] == pytest.approx(0.4)


# ---- the case list's own conditions -------------------------------------------------------------------------------------------------
def test_case_list_conditions():
    cases = R.cases()
    V, F, P = cases["terrain"]
    assert V.shape == (2497, 3) and F.shape == (4752, 3) and P.shape == (1792, 3) and P.dtype == np.float32
    ref = R.reference("terrain")
    d = ref["d64"]
    assert np.isfinite(d).all()
    # the max_dist cuts: at most 1 % of the points within 1e-4 max_dist of a cut, and every cut splits the set
    for md in R.MAX_DISTS:
        assert (np.abs(d - md) <= R.BAND * md).mean() <= 0.01
        assert 0.2 < (d <= md).mean() < 0.8
    # ties at the float32 minimum are the rule, not the exception: the lowest-index rule is exercised
    assert R.ties32(P[::4], V, F) > 0.3
    # the yardstick: a correct float32 answer is off by about one rounding of the largest coordinate
    M = float(max(np.abs(V).max(), np.abs(P).max()))
    assert 0.1 * 2.0 ** -24 * M < R.yardstick_error("terrain") < 4 * 2.0 ** -24 * M
    # points outside the grid cube exist on the terrain case; every engineered case says what its name says
    assert (np.abs(P[1024:1280]).max(1) > 10).all()
    Vc, Fc, Pc = cases["corner_cluster"]
    side = 128
    cell = (Vc.max(0) - Vc.min(0)).max() / side
    assert Vc[Fc].max() / cell < 5                                             # the cluster: the first cells of the grid
    assert (np.clip(np.floor((Pc - Vc.min(0)) / cell), 0, side - 1).max(1) >= side - 8).all()   # the shells cross > 110 cells
    assert sum(((Pc < 0) | (Pc > 10)).any(1)) == 6
    Vp, Fp, Pp = cases["cell_planes"]
    for L in (4, 5, 6, 7):
        c = 8.0 / (1 << L)
        assert np.array_equal(Vp / c, np.round(Vp / c))
    assert np.array_equal(Pp / 0.0625, np.round(Pp / 0.0625))
    assert (R.reference("cell_planes")["d64"][:578 + 192] == 0).all()           # vertices and edge midpoints: d = 0 exactly
    assert R.reference("on_surface")["d64"].max() < 1e-6
    Vd, Fd, _ = cases["dead_mixed"]
    assert (~R.live32(Vd, Fd)).sum() == 4 and not R.live32(Vd, Fd)[:2].any()
    assert not R.live32(*cases["dead_only"][:2]).any() and R.registered32(*cases["dead_only"][:2]).all()
    assert np.isinf(R.reference("dead_only")["d64"]).all()
    nf = cases["non_finite"][2]
    assert (~np.isfinite(nf).all(1)).sum() == 4 and np.isinf(R.reference("non_finite")["d64"]).sum() == 4
    assert [len(cases[f"n{n}"][2]) for n in (1, 63, 64, 65)] == [1, 63, 64, 65]
    # the sloping plane: its two large faces are registered in every cell of the slab their box covers (z in [-4, 4] of the cube's
    # 20: 7 of 16 layers), far from their surface, and every such cell's box is the faces' whole box: cell_box prunes nothing
    g = FR.build_grid(*cases["sloping_plane"][:2], 4)
    assert len(g["cells"]) == 16 * 16 * 7 and all(c >= 2 for c in g["start_num"][:, 1])
    assert (g["cell_box"][:, :3] == [-10, -10, -4]).all() and (g["cell_box"][:, 3:] == [10, 10, 4]).all()


# ---- the prototypes and the refusals ------------------------------------------------------------------------------------------------
def test_prototypes_and_header():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    assert _capi.PROTOTYPES["scanerf_mesh_closest_point"] == ("I", "PIPPPPPPPPPIFPPPP", True)
    assert _capi.PROTOTYPES["scanerf_mesh_closest_point_brute"] == ("I", "PIPPIIPIFPPPP", True)
    assert _capi.PROTOTYPES["scanerf_mesh_closest_point_counted"][2] is False
    hdr = open(os.path.join(ROOT, "include", "scanerf_hip.h")).read()
    for name in ("scanerf_mesh_closest_point", "scanerf_mesh_closest_point_brute"):
        assert re.search(rf"\bint {name}\(const float \*points, int N,", hdr)
    lib = _capi.lib()
    assert lib.scanerf_abi_version() == 10


def test_c_entries_refuse_before_any_launch():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    lib = _capi.lib()
    x = 0x1000      # a non-null pointer that must never be dereferenced: every call below is refused (or a no-op) before a launch
    grid = lambda N=4, L=6, md=1.0, points=x, tris=x, cell_box=x, dist2=x: lib.scanerf_mesh_closest_point(
        points, N, None, None, tris, x, x, x, x, cell_box, x, L, md, dist2, x, None, None)
    brute = lambda N=4, L=6, md=1.0, V=3, F=1, faces=x: lib.scanerf_mesh_closest_point_brute(x, N, x, faces, V, F, x, L, md, x, x, None, None)
    assert grid(N=0) == 0 and brute(N=0) == 0
    for call, what in ((grid, b"mesh_closest_point"), (brute, b"mesh_closest_point_brute")):
        assert call(N=-1) != 0 and b"N=-1" in lib.scanerf_last_error() and what in lib.scanerf_last_error()
        assert call(L=3) != 0 and call(L=8) != 0 and b"log2dim=8" in lib.scanerf_last_error()
        assert call(md=-0.5) != 0 and b"max_dist" in lib.scanerf_last_error()
        assert call(md=float("nan")) != 0 and b"max_dist" in lib.scanerf_last_error()
    assert grid(points=None) != 0 and b"null" in lib.scanerf_last_error()
    assert grid(dist2=None) != 0 and grid(cell_box=None) != 0 and b"null" in lib.scanerf_last_error()
    assert grid(tris=None) != 0 and b"neither triangles nor an indexed mesh" in lib.scanerf_last_error()
    assert brute(faces=None) != 0 and b"null" in lib.scanerf_last_error()
    assert brute(V=-1) != 0 and brute(F=-1) != 0 and b"F=-1" in lib.scanerf_last_error()


def test_python_refusals_come_before_any_library_call(monkeypatch):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation, fastmesh

    def no_call():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(fastmesh, "lib", no_call)
    mesh = fastmesh.FastMesh.__new__(fastmesh.FastMesh)      # no structure: a refusal must not need one
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.closest_point(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.closest_point(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="route"):
        mesh.closest_point(torch.zeros(4, 3), route="bvh")
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            mesh.closest_point(torch.zeros(4, 3), max_dist=bad)
    for bad in (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 2), torch.zeros(12)):
        with pytest.raises(RuntimeError, match=r"\[N,3\] float32"):
            mesh.closest_point(bad)
    with pytest.raises(ValueError, match="max_dist"):
        evaluation.compare_meshes((TRI_V, TRI_F), (TRI_V, TRI_F), 10, [0.1], max_dist=-1.0, device="cpu")
    with pytest.raises(ValueError, match="max_dist"):
        evaluation.compare_meshes((TRI_V, TRI_F), (TRI_V, TRI_F), 10, [0.1], max_dist=float("nan"), device="cpu")
    with pytest.raises(ValueError, match="n_samples"):
        evaluation.compare_meshes((TRI_V, TRI_F), (TRI_V, TRI_F), 0, [0.1], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluation.compare_meshes((TRI_V, TRI_F), (TRI_V, TRI_F), 10, [0.1], device="cpu")
