"""The fused mesh's normals without a GPU (tests/tsdf_normals_reference.py): the definition on linear and quadratic
fields with exact answers, which branch a stencil takes, the zeros, the sphere cases (float32 restatement against float64 within
the derived bound, the radial known answer, unit length, agreement with the faces), the score arithmetic of normal consistency, the
new entry's declaration and refusals, the Python refusals, the commands' options and the PLY round trip."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import tsdf_normals_reference as NR
import tsdf_reference as TR

ENTRY = "scanerf_tsdf_vertex_normals"
DTYPES = (np.float32, np.float64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- linear fields: exact ------------------------------------------------------------------------------------------------------------
def _dyadic_vertices(n, V, seed):
    rng = np.random.default_rng(seed)
    cells = np.stack([rng.integers(0, m, V) for m in n], 1).astype(np.int32)
    return cells, (cells + rng.integers(0, 9, (V, 3)) / 8.0).astype(np.float32)      # t in {0, 1/8, .., 1}: every weight exact


@pytest.mark.parametrize("n,spacing,coeffs", [((5, 4, 6), (0.5, 0.25, 2.0), (0.25, -0.5, 1.0)), ((1, 1, 1), (1.0, 0.125, 4.0), (2.0, 0.375, -0.75)),
                                              ((2, 7, 3), (0.0625, 1.0, 0.5), (-1.5, 0.0, 0.125))])
def test_linear_field_gives_its_gradient_exactly_whatever_is_unobserved(n, spacing, coeffs):
    val = NR.linear_field(n, coeffs, 0.375)
    want = [coeffs[a] / spacing[a] for a in range(3)]
    rng = np.random.default_rng(sum(n))
    cells, lattice = _dyadic_vertices(n, 200, 3)
    for share in (0.0, 0.1, 0.3):
        obs = rng.uniform(size=len(val)) >= share
        for T in DTYPES:
            g, branch = NR.lattice_gradient(val, obs, n, spacing, T)
            for a in range(3):      # every stencil that keeps a neighbour: central and one-sided differences agree
                kept = branch[:, a] != NR.NEITHER
                assert kept.any() and (g[kept, a] == T(want[a])).all() and not g[~kept, a].any()
            r = NR.vertex_normals(val, obs, n, spacing, cells, lattice, T)
            ev = r["evaluated"]
            assert (ev.all() if share == 0.0 else True) and r["grad"].dtype == T
            assert (r["grad"][ev] == np.asarray(want, T)).all() and not r["grad"][~ev].any() and not r["normal"][~ev].any()
            assert (r["branches"][ev] != NR.NEITHER).all()      # all eight corners observed: each has a neighbour inside the cell
        if share == 0.1 and n == (5, 4, 6):      # the pattern does work: some cells lose a corner, some kept stencils are one-sided
            assert ev.any() and (~ev).any() and (r["branches"][ev] != NR.BOTH).any()


# ---- which branch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_quadratic_field_pins_the_branch_taken(axis):
    n, spacing = (4, 4, 4), (0.5, 0.25, 2.0)
    h = spacing[axis]
    val = NR.quadratic_field(n, axis, 0.5)
    ijk = NR.lattice_indices(n)
    i = ijk[:, axis]
    at = lambda *p: TR.point_index(n, p)
    step = np.eye(3, dtype=int)[axis]
    for T in DTYPES:
        obs = np.ones(len(val), bool)
        g, branch = NR.lattice_gradient(val, obs, n, spacing, T)
        # everything observed: the first index has has+ alone, the last has- alone, the rest both
        assert (branch[i == 0, axis] == NR.PLUS_ONLY).all() and (branch[i == n[axis], axis] == NR.MINUS_ONLY).all()
        assert (branch[(i > 0) & (i < n[axis]), axis] == NR.BOTH).all()
        assert (g[i == 0, axis] == T(0.5 / h)).all()                                   # (1 - 0) s / h
        assert (g[i == n[axis], axis] == T(0.5 * (2 * n[axis] - 1) / h)).all()         # (n^2 - (n - 1)^2) s / h
        for k in range(1, n[axis]):
            assert (g[i == k, axis] == T(0.5 * 2 * k / h)).all()                       # ((k + 1)^2 - (k - 1)^2) s / (2 h)
        other = [a for a in range(3) if a != axis]
        assert not g[:, other].any()
        # an interior point q = 2 along the axis with its neighbours switched off in turn
        q = np.array([1, 1, 1])
        q[axis] = 2
        p, plus, minus = at(*q), at(*(q + step)), at(*(q - step))
        for off, code, answer in (((minus,), NR.PLUS_ONLY, 0.5 * 5 / h), ((plus,), NR.MINUS_ONLY, 0.5 * 3 / h), ((plus, minus), NR.NEITHER, 0.0)):
            obs = np.ones(len(val), bool)
            obs[list(off)] = False
            g, branch = NR.lattice_gradient(val, obs, n, spacing, T)
            assert branch[p, axis] == code and g[p, axis] == T(answer), (off, code)
            # q itself being unobserved changes nothing at q: the definition asks for the neighbours
            obs[p] = False
            g2, branch2 = NR.lattice_gradient(val, obs, n, spacing, T)
            assert branch2[p, axis] == code and g2[p, axis] == T(answer)
        # at the first and last index a lone unobserved neighbour leaves "neither"
        for end, nb in ((0, 1), (n[axis], n[axis] - 1)):
            q = np.array([2, 2, 2])
            q[axis] = end
            r = q.copy()
            r[axis] = nb
            obs = np.ones(len(val), bool)
            obs[at(*r)] = False
            g, branch = NR.lattice_gradient(val, obs, n, spacing, T)
            assert branch[at(*q), axis] == NR.NEITHER and g[at(*q), axis] == 0
        # and at vertices: a cell at the low border, in the middle, at the high border (t = 0: corner 0 alone carries the weight)
        obs = np.ones(len(val), bool)
        for c0, code0, code1 in ((0, NR.PLUS_ONLY, NR.BOTH), (1, NR.BOTH, NR.BOTH), (n[axis] - 1, NR.BOTH, NR.MINUS_ONLY)):
            cell = np.array([[1, 1, 1]], np.int32)
            cell[0, axis] = c0
            r = NR.vertex_normals(val, obs, n, spacing, cell, cell.astype(np.float32), T)
            d_hi = 4 >> axis
            assert r["branches"][0, 0, axis] == code0 and r["branches"][0, d_hi, axis] == code1
            want = 0.5 / h if c0 == 0 else 0.5 * 2 * c0 / h
            assert r["grad"][0, axis] == T(want) and r["normal"][0, axis] == T(-1.0) * (T(want) / (T(want) + T(NR.EPS)))


def test_the_unit_lattice_has_its_hand_worked_answer():
    n, spacing, val, obs = NR.unit_lattice()
    cells = np.zeros((3, 3), np.int32)
    lattice = np.array([[0.5, 0.5, 0.5], [0, 0, 0], [1, 1, 1]], np.float32)
    for T in DTYPES:
        g, branch = NR.lattice_gradient(val, obs, n, spacing, T)
        ijk = NR.lattice_indices(n)
        assert (branch[ijk == 0] == NR.PLUS_ONLY).all() and (branch[ijk == 1] == NR.MINUS_ONLY).all()      # every stencil one-sided
        i, j, k = ijk.T
        # val = 0.5 i + 0.25 j + 2 k + i j k, h = (0.5, 0.25, 2): g = (1 + 2 j k, 1 + 4 i k, 1 + 0.5 i j) at both ends of each edge
        assert np.array_equal(g, np.stack([1 + 2 * j * k, 1 + 4 * i * k, 1 + 0.5 * i * j], 1).astype(T))
        r = NR.vertex_normals(val, obs, n, spacing, cells, lattice, T)
        assert r["grad"].tolist() == [[1.5, 2.0, 1.125], [1.0, 1.0, 1.0], [3.0, 5.0, 1.5]]       # centre: the mean of the 8 corners
        length = np.sqrt(T(7.515625))                                                           # 2.25 + 4 + 1.265625
        assert np.array_equal(r["normal"][0], -np.asarray([1.5, 2.0, 1.125], T) / (length + T(NR.EPS)))
        assert r["evaluated"].all()


# ---- zeros and clamps -------------------------------------------------------------------------------------------------------------------
def test_zeros_and_clamps():
    n, spacing = (3, 3, 3), (0.5, 0.5, 0.5)
    val = NR.linear_field(n, (0.25, 0.5, -0.125), 1.0)
    obs = np.ones(len(val), bool)
    obs[TR.point_index(n, (2, 2, 2))] = False
    cells = np.array([[1, 1, 1], [2, 1, 1], [-1, 0, 0], [0, 3, 0], [0, 0, 3], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.int32)
    lattice = np.array([[1.5, 1.5, 1.5], [2.5, 1.5, 1.5], [-0.5, 0.5, 0.5], [0.5, 3.5, 0.5], [0.5, 0.5, 3.5], [-3, 0.5, 0.5], [0.5, 7, 0.5],
                        [np.nan, 0.5, np.nan]], np.float32)
    for T in DTYPES:
        r = NR.vertex_normals(val, obs, n, spacing, cells, lattice, T)
        assert r["evaluated"].tolist() == [False, False, False, False, False, True, True, True]
        assert not r["grad"][:5].any() and not r["normal"][:5].any()      # a corner unobserved (twice), a cell outside (three times)
        assert not np.signbit(r["grad"][:5]).any() and not np.signbit(r["normal"][:5]).any()      # +0 by rule
        assert (r["grad"][5:] == np.asarray([0.5, 1.0, -0.25], T)).all()  # t clamped to 0, to 1, NaN -> 0: still the linear answer
        assert np.isfinite(r["normal"]).all()
    # the clamp itself, on a field where t matters: val = i^2 along x
    val = NR.quadratic_field(n, 0, 1.0)
    obs[:] = True
    cells = np.array([[1, 0, 0]] * 4, np.int32)
    lattice = np.array([[1.0, 0, 0], [-5.0, 0, 0], [np.nan, 0, 0], [9.0, 0, 0]], np.float32)
    r = NR.vertex_normals(val, obs, n, spacing, cells, lattice, np.float32)
    assert r["grad"][:, 0].tolist() == [4.0, 4.0, 4.0, 8.0]              # corner i = 1: (4 - 0) / 1; corner i = 2: (9 - 1) / 1
    # a zero gradient gives a zero normal
    for T in DTYPES:
        r = NR.vertex_normals(np.full(len(val), 0.5, np.float32), obs, n, spacing, cells, lattice, T)
        assert r["evaluated"].all() and not r["grad"].any() and not r["normal"].any()


# ---- the sphere cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NR.SPHERES)
def test_float32_restatement_against_float64_and_the_radial_known_answer(name):
    s = NR.sphere(name)
    r64, r32 = s["ref64"], s["ref32"]
    j, ev = r64["judged"], r64["evaluated"]
    assert r32["grad"].dtype == np.float32 and r32["normal"].dtype == np.float32
    assert ev.all(), "after the support cull every vertex's cell has eight observed corners"
    assert (r64["branches"] != NR.NEITHER).all()
    gerr = np.abs(r32["grad"].astype(np.float64) - r64["grad"])
    nerr = np.abs(r32["normal"].astype(np.float64) - r64["normal"]).max(1)
    noncentral = r64["branches"] != NR.BOTH
    unit = np.abs(np.linalg.norm(r32["normal"].astype(np.float64), axis=1) - 1.0)
    print(f"tsdf normals {name}: V {len(j)}, judged {j.mean():.4f}; max grad error / bound {(gerr[j] / np.maximum(r64['grad_bound'][j], 1e-300)).max():.3f}, "
          f"max normal error / bound {(nerr[j] / r64['normal_bound'][j]).max():.3f}; radial mean {s['radial_deg'].mean():.2f} p95 "
          f"{np.percentile(s['radial_deg'], 95):.1f} max {s['radial_deg'].max():.1f} deg; face average mean {s['face_deg'].mean():.2f} deg; stencils not "
          f"central {noncentral.mean():.4f}, vertices with one {noncentral.any((1, 2)).mean():.3f}; max | |n| - 1 | {unit.max():.2e}")
    assert j.mean() >= NR.JUDGED_SHARE
    assert (gerr[j] <= r64["grad_bound"][j]).all() and (nerr[j] <= r64["normal_bound"][j]).all()
    assert s["radial_deg"].mean() <= NR.RADIAL_MARGIN * NR.RADIAL_MEAN_DEG[name]
    assert abs(s["radial_deg"].mean() - NR.RADIAL_MEAN_DEG[name]) < 0.01 and abs(s["face_deg"].mean() - NR.FACE_AVERAGE_MEAN_DEG[name]) < 0.01
    assert unit.max() <= 1e-6 and np.abs(np.linalg.norm(r64["normal"], axis=1) - 1.0).max() <= 1e-6
    assert noncentral.any(), "the case exercises no one-sided stencil"


@pytest.mark.parametrize("name", ["sphere40", "sphere70"])
def test_normals_agree_with_the_faces_winding(name):
    s = NR.sphere(name)
    dots = (s["ref64"]["normal"] * s["face_normals"]).sum(1)
    out = (s["ref64"]["normal"] * np.asarray(s["mesh"].vertices, np.float64)).sum(1)
    print(f"tsdf normals {name}: min normal . face average {dots.min():.3f}, min normal . radial {out.min():.3f}")
    assert (dots > 0).all() and (out > 0).all()


def test_the_hand_lattice_holds_what_it_is_for():
    h = NR.hand()
    r = h["ref64"]
    ev, br = r["evaluated"], r["branches"]
    assert len(ev) == 257 and h["n"][2] + 1 > 64
    assert ev.sum() >= 60 and (~ev).sum() >= 60
    for code in (NR.MINUS_ONLY, NR.PLUS_ONLY, NR.BOTH):
        for a in range(3):
            assert (br[ev][:, :, a] == code).any(), (code, a)
    assert (br[ev] != NR.NEITHER).all()
    cells = h["cells"]
    outside = ((cells < 0) | (cells >= np.asarray(h["n"]))).any(1)
    assert outside.any() and (~outside & ~ev).any()      # both kinds of zero
    assert r["judged"].all()
    g32 = h["ref32"]
    assert (np.abs(g32["grad"].astype(np.float64) - r["grad"]) <= r["grad_bound"]).all()
    assert (np.abs(g32["normal"].astype(np.float64) - r["normal"]).max(1) <= r["normal_bound"]).all()
    crossing = ev & (cells[:, 2] >= 62) & (cells[:, 2] <= 64)
    assert crossing.any(), "no evaluated stencil crosses the 64-row boundary"


# ---- normal consistency: the score arithmetic ---------------------------------------------------------------------------------------------
def _tri(*faces):
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0]], dtype=torch.float32)
    return v, torch.tensor(faces, dtype=torch.int32)


def test_normal_consistency_arithmetic_on_hand_arrays():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation as E
    v, f = _tri((0, 1, 2), (0, 2, 1), (0, 1, 3), (0, 1, 4), (0, 3, 2))      # +z, -z, -y, zero area (collinear), -x
    n, area = E.face_normals(v, f)
    assert n.dtype == torch.float64 and n.tolist() == [[0, 0, 1], [0, 0, -1], [0, -1, 0], [0, 0, 0], [-1, 0, 0]]
    assert area.tolist() == [True, True, True, False, True]
    inf = math.inf
    dist = torch.tensor([0.1, 0.2, inf, 0.0, 0.3, 0.1])
    sample = torch.tensor([0, 0, 0, 3, 1, 2])
    nearest = torch.tensor([0, 1, 0, 0, 3, 0])
    # c = +1, -1, (not found), (sampled face without area), (nearest face without area), 0
    r = E._consistency(dist, sample, nearest, n, area, n, area)
    assert r == {"mean": 0.0, "mean_abs": 2.0 / 3.0, "skipped": 0.5}
    same = E._consistency(torch.zeros(4), torch.tensor([0, 1, 2, 4]), torch.tensor([0, 1, 2, 4]), n, area, n, area)
    assert same == {"mean": 1.0, "mean_abs": 1.0, "skipped": 0.0}
    flipped = E._consistency(torch.zeros(2), torch.tensor([0, 1]), torch.tensor([1, 0]), n, area, n, area)
    assert flipped == {"mean": -1.0, "mean_abs": 1.0, "skipped": 0.0}
    none = E._consistency(torch.tensor([inf, inf]), torch.tensor([0, 1]), torch.tensor([-1, -1]), n, area, n, area)
    assert math.isnan(none["mean"]) and math.isnan(none["mean_abs"]) and none["skipped"] == 1.0
    # the two directions and their mean; an oblique pair
    v2 = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 1]], dtype=torch.float32)      # normal (0, -1, 1) / sqrt 2
    f2 = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    zero1, face0 = torch.zeros(1), torch.zeros(1, dtype=torch.int64)
    out = E.normal_consistency((v, f[:1]), (v2, f2), (zero1, face0, face0), (zero1, face0, face0))
    assert out["pred_to_gt"]["mean"] == out["gt_to_pred"]["mean"] == out["mean"] and abs(out["mean"] - 2.0 ** -0.5) < 1e-15


def test_compare_meshes_and_the_commands_know_the_option():
    import argparse
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation as E
    from scanerf_amd.renderer import TileSetRenderer
    v, f = _tri((0, 1, 2))
    for bad in (1, "yes", None, np.True_):
        with pytest.raises(ValueError, match="normals must be True or False"):
            E.compare_meshes((v, f), (v, f), 10, [0.1], normals=bad)
        with pytest.raises(ValueError, match="normals must be True or False"):
            TileSetRenderer.__new__(TileSetRenderer).evaluate_mesh((v, f), 10.0, normals=bad)
    ap = argparse.ArgumentParser()
    E.add_score_arguments(ap, required=False)
    assert ap.parse_args([]).normal_consistency is False and ap.parse_args(["--normal-consistency"]).normal_consistency is True
    for name, head in (("fuse_mesh", ["tile", "--cameras", "camera.log", "--out", "x.ply"]), ("compare_meshes", ["a.ply", "b.ply", "--samples", "10", "--threshold", "0.1"])):
        ap = _tool(name).parser()
        assert ap.parse_args(head).normal_consistency is False and ap.parse_args(head + ["--normal-consistency"]).normal_consistency is True
        assert "--normal-consistency" in ap.format_help() and "--normal-consistency" in _tool(name).__doc__
    ap = _tool("fuse_mesh").parser()
    head = ["tile", "--cameras", "camera.log", "--out", "x.ply"]
    assert ap.parse_args(head).normals is False and ap.parse_args(head + ["--normals", "--colors", "rgb"]).normals is True
    assert "--normals" in ap.format_help() and "--normals" in _tool("fuse_mesh").__doc__


# ---- the entry ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_and_typed():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    from test_mesh_visibility_cpu import TOOLS_HEADER, _prototypes
    hdr = _prototypes(TOOLS_HEADER)
    assert ENTRY in hdr and tuple(_capi.TOOL_PROTOTYPES[ENTRY]) == hdr[ENTRY]
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), ENTRY)
    assert _capi.TOOL_PROTOTYPES[ENTRY][1] == "PPIIIPPPIPPP"


def test_the_entry_refuses_before_any_launch():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    err = lambda: _capi.lib().scanerf_last_error()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    s3 = lambda *v: (ctypes.c_float * 3)(*v)
    fn = _capi.tool(ENTRY)
    ok = dict(values=p, observed=p, nx=4, ny=4, nz=4, spacing=s3(1, 1, 1), cells=p, lattice=p, V=3, normal=p, grad=p)
    cases = [({k: None}, b"null pointer") for k in ("values", "observed", "spacing", "cells", "lattice", "normal", "grad")]
    cases += [({"V": -1}, b"V=-1"), ({"nx": 0}, b"n=(0"), ({"ny": -1}, b"n=(4, -1"), ({"nz": 0}, b"n=(4, 4, 0)"),
              ({"nx": 2047, "ny": 2047, "nz": 2047}, b"2^31"), ({"spacing": s3(1, 0, 1)}, b"spacing[1]=0"), ({"spacing": s3(-1, 1, 1)}, b"spacing[0]=-1"),
              ({"spacing": s3(1, 1, math.inf)}, b"spacing[2]=inf"), ({"spacing": s3(math.nan, 1, 1)}, b"spacing[0]=")]
    for over, text in cases:
        for V in (3, 0):      # a refusal comes before the empty call's return
            a = {**ok, "V": V, **over}
            assert fn(*a.values(), None) != 0 and text in err() and b"tsdf_vertex_normals" in err(), (over, err())
    assert fn(*{**ok, "V": 0}.values(), None) == 0      # V == 0: no launch (the buffers are host memory)
    assert buf.raw == bytes(len(buf.raw))


# ---- the Python level -------------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import fusion, meshing
    from scanerf_amd.renderer import TileSetRenderer
    ok = dict(origin=[0, 0, 0], spacing=[1, 1, 1], n=[2, 2, 2], trunc=1.0, device="cpu")
    vol, col = fusion.TSDFVolume(**ok), fusion.TSDFVolume(**ok, color=True)
    i32 = torch.int32
    mesh = meshing.Mesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=i32), torch.zeros((4, 3), dtype=i32), torch.zeros(4, 3), None)
    bare = meshing.Mesh(torch.zeros(4, 3), torch.zeros((2, 3), dtype=i32), None, None, None)
    values, observed = torch.zeros(3, 3, 3), torch.zeros(3, 3, 3, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="route"):
        vol.vertex_normals(mesh, route="dense")
    for bad in (0, -1, None, True, math.nan):
        with pytest.raises(RuntimeError, match="min_weight"):
            vol.vertex_normals(mesh, min_weight=bad)
    with pytest.raises(RuntimeError, match="vertex_normals needs mesh.cells and mesh.lattice"):
        vol.vertex_normals(bare)
    with pytest.raises(RuntimeError, match="values and observed together"):
        vol.vertex_normals(mesh, values=values)
    with pytest.raises(RuntimeError, match="values and observed together"):
        vol.vertex_normals(mesh, observed=observed)
    with pytest.raises(RuntimeError, match=r"values and observed must be \[3, 3, 3\]"):
        vol.vertex_normals(mesh, values=torch.zeros(27), observed=observed)
    with pytest.raises(RuntimeError, match=r"values and observed must be \[3, 3, 3\]"):
        vol.vertex_normals(mesh, values=values, observed=torch.zeros(3, 3, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="values must be a torch.Tensor"):
        vol.vertex_normals(mesh, values=np.zeros((3, 3, 3), np.float32), observed=observed)
    for cells, lattice in ((torch.zeros((4, 2), dtype=i32), torch.zeros(4, 3)), (torch.zeros((4, 3), dtype=i32), torch.zeros(5, 3)),
                           (torch.zeros(12, dtype=i32), torch.zeros(4, 3))):
        with pytest.raises(RuntimeError, match=r"cells and lattice must be \[V,3\]"):
            vol.vertex_normals(meshing.Mesh(mesh.vertices, mesh.faces, cells, lattice, None))
    for route in fusion.ROUTES:
        with pytest.raises(RuntimeError, match="no CPU path"):
            vol.vertex_normals(mesh, route=route)
        with pytest.raises(RuntimeError, match="no CPU path"):
            vol.vertex_normals(mesh, values=values, observed=observed, route=route)
    for v in (vol, col):
        for bad in (1, "yes", None):
            with pytest.raises(RuntimeError, match="normals must be True or False"):
                v.extract(normals=bad)
        with pytest.raises(RuntimeError, match="min_weight"):
            v.extract(min_weight=0, normals=True)
        with pytest.raises(RuntimeError, match="no CPU path"):
            v.extract(normals=True)
    with pytest.raises(RuntimeError, match="needs a volume with colour"):
        vol.extract(colors=True, normals=True)
    depths, ks, c2ws = torch.zeros(2, 4, 4), torch.eye(3).repeat(2, 1, 1), torch.eye(4)[:3].repeat(2, 1, 1)
    box = ([0, 0, 0], [1, 1, 1], [2, 2, 2])
    for bad in (1, "yes", None):
        with pytest.raises(RuntimeError, match="normals must be True or False"):
            fusion.fuse_depth_maps(depths, ks, c2ws, *box, normals=bad)
        with pytest.raises(RuntimeError, match="normals must be True or False"):
            TileSetRenderer.__new__(TileSetRenderer).fuse_mesh((ks, c2ws, 8, 8), normals=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.fuse_depth_maps(depths, ks, c2ws, *box, normals=True)
    with pytest.raises(RuntimeError, match="needs cameras"):
        TileSetRenderer.__new__(TileSetRenderer).fuse_mesh(None, normals=True)


# ---- the PLY round trip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip_with_normals_and_colours_together(tmp_path, binary):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import formats
    s = NR.sphere("sphere70")
    V, F = np.asarray(s["mesh"].vertices, np.float32), np.asarray(s["mesh"].faces, np.int32)
    N = s["ref32"]["normal"]
    C = (0.5 + 0.5 * N).astype(np.float32)
    path = str(tmp_path / "nc.ply")
    formats.write_ply(path, V, F, binary=binary, normals=N, colors=C)
    header = open(path, "rb").read().split(b"end_header")[0].decode()
    props = [ln.split()[-1] for ln in header.splitlines() if ln.startswith("property") and "list" not in ln]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    v, f, nrm, col = formats.read_ply(path, normals=True, colors=True)
    assert np.array_equal(v, V) and np.array_equal(f, F) and col.dtype == np.uint8 and np.array_equal(col, formats.quantize_colors(C))
    assert nrm.dtype == np.float32 and np.array_equal(nrm.view(np.int32), N.view(np.int32))      # the normals' bits survive both encodings
