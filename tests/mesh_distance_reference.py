"""Independent yardsticks for the closest-point query (scanerf_amd.fastmesh.FastMesh.closest_point, csrc/mesh_distance.hip), numpy
only, written from the definition in include/scanerf_hip.h and not from the kernel:

  closest(P, V, F, dtype)   brute force over EVERY face: per (point, face) the closest point of the closed triangle by Voronoi regions
                            (vertices A, B, C; edges AB, AC, BC; interior) from (A, B - A, C - A); the minimum, the lowest face index
                            attaining it, that face's closest point.  dtype=float64: the judge.  dtype=float32: the YARDSTICK -- the
                            same formulas rounded to float32 after every operation (numpy never contracts), i.e. what a correct
                            float32 implementation gives;
  live32 / registered32     which faces may answer: n . n != 0 in float32, and the build's registration rule (csrc/mesh.hip);
  cases()                   the case list of tests/test_gpu_mesh_distance.py, with the conditions test_mesh_distance_cpu.py asserts.
"""
import functools

import numpy as np

import fastmesh_reference as FR

MAX_DISTS = (0.5, 1.0, 2.0)     # the cuts of the max_dist test on the terrain case
BAND = 1e-4                     # relative half-width of the band around a cut in which float32 may decide either way


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def operands(V, F, dtype):
    """(A, B - A, C - A) [F,3] each in `dtype`, from float32 vertices (float32: the subtraction rounds, as the build's does)."""
    V = np.asarray(V, np.float32).astype(dtype)
    A = V[F[:, 0]]
    return A, V[F[:, 1]] - A, V[F[:, 2]] - A


def live32(V, F):
    """The float32 liveness rule: n . n != 0, n = (B - A) x (C - A), every operation rounded to float32."""
    _, ab, ac = operands(V, F, np.float32)
    n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                  ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], -1)
    return _dot(n, n) != 0


def registered32(V, F, log2dim=6):
    """The faces the build registers (csrc/mesh.hip face_cells): indices in [0, V) and the box not wholly outside the grid cube."""
    V = np.asarray(V, np.float32)
    ok = ((F >= 0) & (F < len(V))).all(1)
    tri = V[np.clip(F, 0, len(V) - 1)]
    mn, mx = V.min(0), V.max(0)
    cell = np.float32((mx - mn).max() / np.float32(1 << log2dim))
    gmax = mn + np.float32(1 << log2dim) * cell
    out = ((tri.max(1) < mn) | (tri.min(1) > gmax)).any(1)
    return ok & ~out & (cell > 0)


def point_triangle(p, A, ab, ac):
    """p [b,1,3]; A, ab, ac [1,F,3], all of one dtype -> q [b,F,3], d2 [b,F] in that dtype (every operation rounds to it)."""
    one, zero = p.dtype.type(1), p.dtype.type(0)
    ap = p - A
    bp, cp = ap - ab, ap - ac
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = one / ((va + vb) + vc)
        regions = [   # (condition, v, w), the first that holds is taken; then edge BC; then the interior
            ((d1 <= 0) & (d2 <= 0), zero, zero),
            ((d3 >= 0) & (d4 <= d3), one, zero),
            ((d6 >= 0) & (d5 <= d6), zero, one),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),
        ]
        bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = vb * inv, vc * inv
    taken = np.zeros(d1.shape, bool)
    vv, ww = np.array(v), np.array(w)
    for cond, rv, rw in regions:
        m = cond & ~taken
        vv = np.where(m, rv, vv)
        ww = np.where(m, rw, ww)
        taken |= cond
    bc &= ~taken
    ww = np.where(bc, wbc, ww)
    q = np.where(bc[..., None], (A + ab) + ww[..., None] * (ac - ab), (A + vv[..., None] * ab) + ww[..., None] * ac)
    e = p - q
    return q, _dot(e, e)


def closest(P, V, F, dtype=np.float64, log2dim=6, chunk=64):
    """-> d2 [N] (dtype; +inf = no live face or a non-finite point), face [N] (lowest index at the minimum; -1), q [N,3]."""
    P = np.asarray(P, np.float32)
    N = len(P)
    d2 = np.full(N, np.inf, dtype)
    face = np.full(N, -1, np.int64)
    q = P.astype(dtype).copy()
    if len(F) == 0:
        return d2, face, q
    ok = registered32(V, F, log2dim)
    F = np.where(ok[:, None], F, 0)           # (faces the build leaves out are never dereferenced)
    ok &= live32(V, F)
    A, ab, ac = (a[None] for a in operands(V, F, dtype))
    finite = np.isfinite(P).all(1)
    idx = np.flatnonzero(finite)
    for s in range(0, len(idx), chunk):
        ii = idx[s:s + chunk]
        qq, dd = point_triangle(P[ii, None].astype(dtype), A, ab, ac)
        dd = np.where(ok[None] & ~np.isnan(dd), dd, np.inf)
        j = dd.argmin(1)                      # (the first index at the minimum)
        r = np.arange(len(ii))
        hit = np.isfinite(dd[r, j])
        d2[ii] = np.where(hit, dd[r, j], np.inf)
        face[ii] = np.where(hit, j, -1)
        q[ii] = np.where(hit[:, None], qq[r, j], q[ii])
    return d2, face, q


def dist_to_face64(P, V, F, face):
    """float64 distance of each point to ONE given face (face [N] >= 0)."""
    A, ab, ac = operands(V, F[face], np.float64)
    _, d2 = point_triangle(np.asarray(P, np.float32).astype(np.float64)[:, None], A[:, None], ab[:, None], ac[:, None])
    # (point i against its own face only: the diagonal of a [N,1] broadcast)
    return np.sqrt(d2[:, 0])


def ties32(P, V, F):
    """Share of the points at which two or more faces attain the float32 minimum."""
    ok = live32(V, F) & registered32(V, F)
    A, ab, ac = (a[None] for a in operands(V, F, np.float32))
    n = 0
    for s in range(0, len(P), 64):
        _, dd = point_triangle(np.asarray(P[s:s + 64], np.float32)[:, None], A, ab, ac)
        dd = np.where(ok[None], dd, np.inf)
        n += int(((dd == dd.min(1, keepdims=True)).sum(1) >= 2).sum())
    return n / len(P)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
DEAD_FACES = np.array([[5, 5, 9], [0, 1, 2]], np.int32)   # with dead_vertices(): two equal indices; three collinear points


def dead_vertices():
    """(0,0,0), (1,1,1), (2,2,2): collinear, n . n exactly 0 under any rounding or contraction (every product pair is equal)."""
    return np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)


def terrain_points():
    """The 1 792 query points of the terrain case: 1 024 ray origins above the terrain, 256 origins outside the grid cube at radius
    25..40, 512 vertices jittered by sigma = 0.05."""
    V, F, rays = FR.terrain_fixture()
    rng = np.random.default_rng(23)
    jit = V[rng.choice(len(V), 512, replace=False)] + rng.normal(size=(512, 3)) * 0.05
    return np.concatenate([rays["inside"][0][:1024], rays["outside"][0][:256], jit]).astype(np.float32)


def _plane_mesh():
    """Vertices on multiples of 0.5 in the cube [0,8]^3 (cell = 0.5 .. 0.0625 at log2dim 4 .. 7: every vertex on a cell plane): the
    plane z = 4 and the wall x = 4, 16 x 16 quads each, plus the two unused corner vertices that fix the grid cube."""
    ts = np.arange(17) * 0.5
    X, Y = np.meshgrid(ts, ts, indexing="ij")
    V = [np.stack([X, Y, np.full_like(X, 4.0)], -1).reshape(-1, 3), np.stack([np.full_like(X, 4.0), X, Y], -1).reshape(-1, 3)]
    F = []
    for base in (0, 289):
        for i in range(16):
            for j in range(16):
                a = base + i * 17 + j
                F += [[a, a + 17, a + 18], [a, a + 18, a + 1]]
    V.append(np.array([[0, 0, 0], [8, 8, 8]], float))
    return np.concatenate(V).astype(np.float32), np.array(F, np.int32)


def _corner_cluster():
    """A small cube in the corner of the grid cube [0,10]^3 (an unused vertex at (10,10,10) fixes the cube); queries from the opposite
    corner and from outside the cube on each of its six sides: the shells cross the whole grid."""
    V = np.concatenate([FR._CUBE * 0.3 + 0.05, [[0, 0, 0], [10, 10, 10]]]).astype(np.float32)
    F = np.array(FR._CUBE_FACES, np.int32)
    P = [[9.97, 9.95, 9.99], [9.0, 9.5, 8.0]]
    for a in range(3):
        for s in (-7.0, 17.0):
            p = [9.6, 9.7, 9.8]
            p[a] = s
            P.append(p)
    return V, F, np.array(P, np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (V [V,3] f32, F [F,3] i32, P [N,3] f32).  The references are computed once per session by the users of this list."""
    out = {}
    V, F, _ = FR.terrain_fixture()
    P = terrain_points()
    out["terrain"] = (V, F, P)
    # the sloping plane: two faces registered in every cell (cell_box prunes nothing) and a small box above it
    Vs, Fs, (o, _), _ = FR.sloping_plane_fixture()
    rng = np.random.default_rng(5)
    near = rng.uniform(-10, 10, (256, 3))
    near[:, 2] = 0.4 * near[:, 1] + rng.uniform(-3, 3, 256)        # within 3 of the plane: the walk through cells that nothing prunes
    out["sloping_plane"] = (Vs, Fs, np.concatenate([o, near]).astype(np.float32))   # stays short (corner_cluster crosses a whole grid)
    out["corner_cluster"] = _corner_cluster()
    # vertices AND points on cell planes; the first 578 points are the vertices themselves (d = 0 exactly), then the edge midpoints of
    # the first 64 faces (exact in float32: d = 0), then a lattice of multiples of the cell size
    Vp, Fp = _plane_mesh()
    tri = Vp[Fp[:64]]
    mid = np.concatenate([(tri[:, 0] + tri[:, 1]) / 2, (tri[:, 1] + tri[:, 2]) / 2, (tri[:, 0] + tri[:, 2]) / 2])
    g = np.arange(9, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32(0.0625) * np.float32(3)
    lattice2 = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[::3]
    out["cell_planes"] = (Vp, Fp, np.concatenate([Vp[:578], mid, lattice, lattice2]).astype(np.float32))
    # points on vertices, in edges and in faces of the terrain (d = 0 up to the rounding of the point itself)
    t = V[F[::19]]
    out["on_surface"] = (V, F, np.concatenate([V[::9], (t[:, 0] + t[:, 1]) / 2, t.mean(1)]).astype(np.float32))
    # dead faces FIRST (the lowest indices: they would win every tie) in front of the terrain's
    Vd = np.concatenate([dead_vertices(), V])
    Fd = np.concatenate([DEAD_FACES, F + 3, DEAD_FACES]).astype(np.int32)
    out["dead_mixed"] = (Vd, Fd, P[::4])
    # (an unused vertex makes the grid cube 64 wide: the dead faces fill a few cells, the walk crosses all the empty ones)
    out["dead_only"] = (np.concatenate([dead_vertices(), [[64, 0, 1]]]).astype(np.float32), DEAD_FACES[[1, 1, 1]], P[:65])
    nf = P[:130].copy()
    nf[3, 0], nf[64, 1], nf[65, 2], nf[129] = np.nan, np.inf, -np.inf, np.nan
    out["non_finite"] = (V, F, nf)
    for n in (1, 63, 64, 65):                 # (points above the terrain: the far ones, which walk a whole grid, stay in "terrain")
        out[f"n{n}"] = (V, F, P[512:512 + n])
    return out


@functools.lru_cache(maxsize=None)
def reference(name, log2dim=6):
    """-> dict of the float64 judge (d64, face64) and the float32 yardstick (d32, face32, q32) of a case; computed once."""
    V, F, P = cases()[name]
    d2, f64, q64 = closest(P, V, F, np.float64, log2dim)
    e2, f32, q32 = closest(P, V, F, np.float32, log2dim)
    return {"d64": np.sqrt(d2), "face64": f64, "q64": q64, "d2_32": e2, "d32": np.sqrt(e2.astype(np.float64)), "face32": f32, "q32": q32}


def yardstick_error(name):
    """The largest |d32 - d64| of the float32 yardstick on a case's finite answers: what a correct float32 result may be off by."""
    r = reference(name)
    ok = np.isfinite(r["d64"])
    return float(np.abs(r["d32"][ok] - r["d64"][ok]).max()) if ok.any() else 0.0
