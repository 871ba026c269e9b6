"""The mesh extraction's yardstick on its own (tests/surface_nets_reference.py): known answers, topology, the integer liveness rule, the
share of cells the float64 judgement leaves out on every model case, and the new entry points' argument validation -- no GPU."""
import ctypes

import numpy as np
import pytest

import surface_nets_reference as SR


def test_lone_inside_point_in_a_2x2x2_lattice():
    v = np.zeros((3, 3, 3), np.float32)
    v[1, 1, 1] = 2.0
    for dt in (np.float64, np.float32):
        m = SR.surface_nets(v, 1.0, dtype=dt)
        assert len(m.vertices) == 8 and len(m.faces) == 12
        closed, chi, vol = SR.topology(m)
        assert closed and chi == 2 and vol > 0
        # every crossing sits at t = 1/2 from the centre point: the vertices are the corners of the cube [0.75, 1.25]^3 ... per cell, the
        # mean of three crossings (1, 1, 0.5)-like points: 1 -/+ 1/6 per coordinate
        want = np.where(m.cells == 0, 1.0 - 1.0 / 6.0, 1.0 + 1.0 / 6.0)
        np.testing.assert_allclose(m.lattice, want, rtol=0, atol=1e-6)


def test_single_cell():
    v = np.zeros((2, 2, 2), np.float32)
    v[0, 0, 0] = 3.0
    m = SR.surface_nets(v, 1.0, origin=(10.0, 20.0, 30.0), spacing=(2.0, 2.0, 2.0))
    assert len(m.vertices) == 1 and len(m.faces) == 0 and m.cells.tolist() == [[0, 0, 0]]
    # three crossings at t = 2/3 on the edges from the corner: mean = (2/9, 2/9, 2/9)
    np.testing.assert_allclose(m.lattice[0], [2.0 / 9.0] * 3, rtol=1e-12)
    np.testing.assert_allclose(m.vertices[0], [10.0 + 4.0 / 9.0, 20.0 + 4.0 / 9.0, 30.0 + 4.0 / 9.0], rtol=1e-12)


@pytest.mark.parametrize("n, kind, chi_want", [((9, 8, 7), "sphere", 2), ((17, 5, 3), "sphere", 2), ((16, 16, 16), "sphere", 2),
                                               ((20, 20, 10), "torus", 0)])
def test_closed_oriented_surfaces(n, kind, chi_want):
    centre = [m / 2.0 + 0.13 for m in n]
    if kind == "sphere":
        v = SR.sphere_values(n, centre, 0.37 * min(n))
    else:
        v = SR.torus_values(n, centre, 6.1, 2.4)
    for dt in (np.float64, np.float32):
        m = SR.surface_nets(v, 1.0, dtype=dt)
        closed, chi, vol = SR.topology(m)
        assert len(m.faces) > 0 and closed and chi == chi_want and vol > 0, (closed, chi, vol)
        assert (m.lattice >= m.cells).all() and (m.lattice <= m.cells + 1).all()     # every vertex in its own closed cell
        assert m.faces.min() >= 0 and m.faces.max() < len(m.vertices)


def test_value_equal_to_the_level_is_outside():
    v = np.full((3, 3, 3), 1.0, np.float32)
    assert len(SR.surface_nets(v, 1.0).vertices) == 0
    v[1, 1, 1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert len(SR.surface_nets(v, 1.0).vertices) == 8
    v[1, 1, 1] = 1.0
    v[0, 0, 0] = 0.5
    assert len(SR.surface_nets(v, 1.0).vertices) == 0     # nothing is inside: 1.0 is not


def test_canonical_ignores_the_order():
    v, level = SR.dense_cases()["sphere-on-brick-corner"]
    m = SR.surface_nets(v, level)
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(m.vertices))
    inv = np.argsort(perm)
    f = inv[m.faces][rng.permutation(len(m.faces))]
    f = np.stack([np.roll(r, s) for r, s in zip(f, rng.integers(0, 3, len(f)))])
    m2 = SR.Mesh(m.vertices[perm], f.astype(np.int32), m.cells[perm], m.lattice[perm])
    a, b = SR.canonical(m), SR.canonical(m2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    flipped = SR.Mesh(m.vertices, m.faces[:, ::-1].copy(), m.cells, m.lattice)
    assert not np.array_equal(SR.canonical(flipped)["faces"], a["faces"])


def _live_brute(n, occ):
    """The rule in rationals: point i lies in closed cell c iff c / G <= i / n <= (c + 1) / G."""
    from fractions import Fraction as Fr
    G = occ.shape
    out = np.zeros(tuple(m + 1 for m in n), bool)
    per_axis = [[[c for c in range(G[k]) if Fr(c, G[k]) <= Fr(i, n[k]) <= Fr(c + 1, G[k])] for i in range(n[k] + 1)] for k in range(3)]
    for i in range(n[0] + 1):
        for j in range(n[1] + 1):
            for k in range(n[2] + 1):
                out[i, j, k] = any(occ[a, b, c] for a in per_axis[0][i] for b in per_axis[1][j] for c in per_axis[2][k])
    return out


@pytest.mark.parametrize("n, log2dim", [((32, 16, 48), (4, 4, 4)), ((4, 8, 2), (4, 4, 4)), ((12, 12, 12), (4, 4, 4)), ((40, 12, 5), (4, 3, 2))])
def test_liveness_rule(n, log2dim):
    for pattern in ("corner", "opposite", "ell", "checker", "none", "full"):
        occ = SR.occupancy(pattern, log2dim)
        live = SR.live_points(n, occ)
        assert np.array_equal(live, _live_brute(n, occ)), pattern
    m = SR.axis_membership(n[0], 2 ** log2dim[0])
    assert m.sum(1).min() >= 1 and m.sum(1).max() <= 2               # at most two cells per axis
    assert m[0].tolist() == [True] + [False] * (m.shape[1] - 1) and m[-1, -1] and m[-1].sum() == 1
    corner = SR.live_points(n, SR.occupancy("corner", log2dim))
    assert corner[0, 0, 0] and not corner[-1, -1, -1]
    # the corner cell's closed extent: points with i G <= n per axis
    want = [int(np.floor(n[k] / 2 ** log2dim[k])) + 1 for k in range(3)]
    assert corner.sum() == int(np.prod(want))
    assert SR.live_points(n, SR.occupancy("opposite", log2dim))[-1, -1, -1]


def test_lattice_positions_are_float32_and_span_the_box():
    x = SR.lattice_positions((12, 10, 7))
    assert x.dtype == np.float32 and x.shape == (13, 11, 8, 3)
    assert x[0, 0, 0].tolist() == [-1.0, -1.0, -1.0] and abs(float(x[-1, -1, -1, 2]) - 1.0) < 2e-7
    h = np.float32(2.0) / np.float32(7)
    assert x[3, 2, 5, 2] == np.float32(np.float32(5) * h) - np.float32(1.0)


@pytest.mark.parametrize("c", SR.MODEL_CASES, ids=SR.model_id)
def test_share_of_cells_left_out_stays_within_the_cap(c):
    """On the float64 / float32 yardsticks alone: few lattice points are ambiguous, enough cells are judged, and the float32 yardstick
    agrees with float64 on every judged cell."""
    ins, live, s64, s32, level = SR.model_reference(c)
    assert level > 0
    amb = SR.ambiguous_points(s64, s32, live, level)
    judged = SR.judged_cells(amb)
    left_out = 1.0 - judged.mean()
    print(f"{SR.model_id(c)}: level {level:.6g}, {int(amb.sum())} ambiguous of {int(live.sum())} live points, {left_out:.4%} of cells left out")
    assert left_out <= SR.CAP
    assert judged.sum() >= SR.MIN_JUDGED
    r64, r32 = SR.surface_nets(s64, level), SR.surface_nets(s32, level, dtype=np.float32)
    if c.family == "empty":
        assert len(r64.vertices) == 0 and len(r64.faces) == 0
    else:
        assert len(r64.vertices) > 0
    assert not SR.judge_mesh(SR.model_id(c) + " yardstick", r32, r64, r32, judged)


@pytest.mark.parametrize("c", SR.OPAQUE_CASES, ids=SR.model_id)
def test_opaque_cases_follow_from_the_integer_rule(c):
    ins, live, _, _, level = SR.model_reference(c)
    m = SR.surface_nets(np.where(live, 8.0, 0.0), level)
    if c.pattern == "none":
        assert len(m.vertices) == 0
    else:
        assert len(m.vertices) > 0 and (m.lattice >= m.cells).all() and (m.lattice <= m.cells + 1).all()


def test_abi_version_and_argument_validation():
    """The new entry points refuse bad arguments with a message before any launch (no GPU needed); the ABI version stays."""
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    lib = _capi.lib()
    assert lib.scanerf_abi_version() == 10
    null = None
    err = lambda: lib.scanerf_last_error()
    assert lib.scanerf_isosurface_scratch_bytes(256, 256, 256) == 64 + 72 * 32 ** 3 + 8
    assert lib.scanerf_isosurface_scratch_bytes(256, 256, 256) <= 256 ** 3 + 1024       # at most 1 byte per cell plus a constant
    assert lib.scanerf_isosurface_scratch_bytes(1, 1, 1) == 64 + 72 + 8
    assert lib.scanerf_isosurface_scratch_bytes(0, 4, 4) == 0 and b"n_k" in err()
    assert lib.scanerf_isosurface_scratch_bytes(2048, 1024, 1024) == 0 and b"2^31 cells" in err()
    assert lib.scanerf_isosurface_scratch_bytes(2 ** 31 - 2, 1, 1) == 0 and b"points" in err()

    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    dense_c = lambda n=(4, 4, 4), level=1.0: lib.scanerf_isosurface_count_dense(null, *n, level, null, 0, null)
    dense_e = lambda n=(4, 4, 4), level=1.0, V=3, F=2: lib.scanerf_isosurface_emit_dense(null, *n, level, f3, f3, null, 0, null, null, null, null, V, F, null)
    for fn in (dense_c, dense_e):
        assert fn() == 2 and b"null" in err()
        assert fn(level=0.0) == 2 and b"level" in err()
        assert fn(level=-1.0) == 2 and b"level" in err()
        assert fn(level=float("nan")) == 2 and b"level" in err()
        assert fn(n=(4, 0, 4)) == 2 and b"n_k" in err()
        assert fn(n=(2048, 2048, 512)) == 2 and b"2^31" in err()

    l2d = (ctypes.c_int32 * 3)(4, 4, 4)
    fused_c = lambda n=(4, 4, 4), level=1.0, T=4096, dt=_capi.F32, l2=l2d, cells=4096: lib.scanerf_isosurface_count(
        null, dt, null, null, null, T, null, l2, cells, *n, level, null, 0, null)
    fused_e = lambda n=(4, 4, 4), level=1.0, T=4096, dt=_capi.F32, l2=l2d, cells=4096: lib.scanerf_isosurface_emit(
        null, dt, null, null, null, T, null, l2, cells, *n, level, f3, f3, null, 0, null, null, null, null, 3, 2, null)
    for fn in (fused_c, fused_e):
        assert fn() == 2 and b"null" in err()
        assert fn(level=0.0) == 2 and b"level" in err()
        assert fn(n=(0, 1, 1)) == 2 and b"n_k" in err()
        assert fn(n=(1024, 2048, 1024)) == 2 and b"2^31" in err()
        assert fn(T=1000) == 2 and b"power of two" in err()
        assert fn(dt=_capi.BF16) == 2 and b"feat_dtype" in err()
        assert fn(cells=4095) == 2 and b"log2dim" in err()
        assert fn(l2=(ctypes.c_int32 * 3)(4, 3, 4)) == 2 and b"log2dim" in err()
        assert fn(l2=null) == 2 and b"null" in err()


def test_python_surface_has_no_cpu_path():
    import torch
    import scanerf_amd  # noqa
    from scanerf_amd import meshing
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.surface_nets(torch.zeros(3, 3, 3), 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshing.extract_mesh(torch.zeros(16, 1024, 2), torch.ones(16, 3, dtype=torch.int32), torch.zeros(13994), torch.ones(32),
                             torch.ones(2, 2, 2, dtype=torch.bool), [1, 1, 1], [0, 0, 0], [1, 1, 1], (4, 4, 4), 1.0)
    assert meshing.cells_per_axis([8.0, 2.0, 4.0], 64) == [64, 16, 32] and meshing.cells_per_axis([1.0, 1e-3, 1.0], 10) == [10, 1, 10]
