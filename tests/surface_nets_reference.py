"""Yardstick and case list of the level-set mesh extraction (csrc/isosurface.hip; test infrastructure, CPU only, no GPU import).

The definition of include/scanerf_hip.h in numpy, from a value array, in a dtype of the caller's choice (float64 = the reference,
float32 = the yardstick for how much rounding the problem allows), the integer liveness rule, a canonical form of a mesh (vertices
sorted by cell, faces as a sorted set of oriented triangles named by their cells), the model cases of tests/test_gpu_mesh_extract.py
and their float64 / float32 density fields (tests/normals_reference.py's closed form at the float32-pinned lattice positions).

Judgement of the fused route against float64 (per_ray_reference.judge's rule: a bound is K x the float32 yardstick's own error):
  * a lattice point is AMBIGUOUS when |sigma64 - level| <= K max(e32, 2^-24 level), e32 = the case's largest |sigma32 - sigma64|;
    a cell with an ambiguous corner is left out (at most CAP = 2 % of the cells of a case); every other cell must be active exactly
    when the float64 reference says so;
  * a triangle of the reference all of whose quad's four cells are judged must exist, with its orientation; a triangle of the mesh
    whose three cells are judged must be one of the reference's;
  * the vertices of the judged active cells, in lattice steps: median, 99th percentile, maximum and pooled error against K x the
    error of the float32 yardstick (the definition in float32 on the float32 field), its figures taken as at least FLOOR.
K: the largest ratio (kernel's figure / max(yardstick's figure, FLOOR)) over all cases of the first MI355X run of the finished tests,
doubled and rounded up to a power of two (profiles/mesh_extract_error.md holds the run)."""
import collections
import functools

import numpy as np
import torch

import normals_reference as NR
from per_ray_reference import figures, judge  # noqa: F401  (figures: re-exported for the profile tool)

# That run: 2.19 (pooled) and 5.63 (maximum), both on base-f32-n12x10x8.  K_MAX is also the K of the ambiguity band.
K_QUANTILE = 8.0   # median, 99th percentile, pooled
K_MAX = 16.0       # maximum
K = (K_QUANTILE, K_MAX)
FLOOR = NR.FLOOR
CAP = 0.02
MIN_JUDGED = 200

Mesh = collections.namedtuple("Mesh", "vertices faces cells lattice")


# ------------------------------------------------------------------------------------------------------------------- the definition
def _shift(a, d, n):
    """a[(i + d0, j + d1, k + d2)] for the cells 0 <= i < n0 etc. of a point array [n0+1, n1+1, n2+1]."""
    return a[d[0]:d[0] + n[0], d[1]:d[1] + n[1], d[2]:d[2] + n[2]]


def surface_nets(values, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), dtype=np.float64):
    """values [nx+1, ny+1, nz+1] -> Mesh (vertices, lattice in `dtype`; vertices ordered by cell, faces by axis then edge)."""
    v = np.asarray(values).astype(dtype)
    level = dtype(level)
    n = tuple(s - 1 for s in v.shape)
    assert min(n) >= 1
    inside = v > level
    corners = [_shift(inside, ((q >> 2) & 1, (q >> 1) & 1, q & 1), n) for q in range(8)]
    cnt_in = sum(c.astype(np.int32) for c in corners)
    active = (cnt_in > 0) & (cnt_in < 8)
    idx = np.stack(np.meshgrid(*[np.arange(m) for m in n], indexing="ij"), -1)          # [nx,ny,nz,3] cell coordinates
    total = np.zeros(n + (3,), dtype)
    count = np.zeros(n, np.int32)
    for a in range(3):
        o1, o2 = (a + 1) % 3, (a + 2) % 3
        for d1, d2 in ((0, 0), (1, 0), (0, 1), (1, 1)):
            q = [0, 0, 0]
            q[o1], q[o2] = d1, d2
            e = list(q)
            e[a] = 1
            va, vb = _shift(v, q, n), _shift(v, e, n)
            cross = _shift(inside, q, n) != _shift(inside, e, n)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (level - va) / (vb - va)
            pt = (idx + np.asarray(q)).astype(dtype)
            pt[..., a] = pt[..., a] + np.where(cross, t, dtype(0))
            total = total + np.where(cross[..., None], pt, dtype(0))     # (adding 0 is exact: the sum is the sequential one)
            count += cross
    cells = np.argwhere(active).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = (total / count[..., None].astype(dtype))[active]
    vertices = np.asarray(origin, dtype) + L * np.asarray(spacing, dtype)
    vid = np.full(n, -1, np.int64)
    vid[active] = np.arange(len(cells))
    faces = []
    for a in range(3):
        o1, o2 = (a + 1) % 3, (a + 2) % 3
        lo, hi = [0, 0, 0], list(n)
        lo[o1] = lo[o2] = 1                       # interior: 1 <= p_o <= n_o - 1; 0 <= p_a <= n_a - 1
        sl = tuple(slice(lo[k], hi[k]) for k in range(3))
        e = [0, 0, 0]
        e[a] = 1
        sle = tuple(slice(lo[k] + e[k], hi[k] + e[k]) for k in range(3))
        ia, ib = inside[sl], inside[sle]
        p = np.argwhere(ia != ib) + np.asarray(lo)
        if not len(p):
            continue
        quad = []
        for d1, d2 in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            c = p.copy()
            c[:, o1] += d1
            c[:, o2] += d2
            quad.append(vid[c[:, 0], c[:, 1], c[:, 2]])
        quad = np.stack(quad, 1)
        assert (quad >= 0).all()
        p_in = inside[p[:, 0], p[:, 1], p[:, 2]]
        quad = np.where(p_in[:, None], quad, quad[:, ::-1])
        faces.append(np.stack([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]], 1).reshape(-1, 3))
    faces = np.concatenate(faces).astype(np.int32) if faces else np.zeros((0, 3), np.int32)
    return Mesh(vertices, faces, cells, L)


# ------------------------------------------------------------------------------------------------------------------- liveness
def axis_membership(n, G):
    """[n + 1, G] bool: lattice point i lies in the closed sampler cell c of an axis iff c n <= i G <= (c + 1) n (integers)."""
    iG = np.arange(n + 1, dtype=np.int64)[:, None] * G
    c = np.arange(G, dtype=np.int64)[None, :]
    return (c * n <= iG) & (iG <= (c + 1) * n)


def live_points(n, occ):
    """[nx+1, ny+1, nz+1] bool: the points in the closed extent of some occupied cell of occ [Gx,Gy,Gz] bool."""
    occ = np.asarray(occ).astype(np.int64)
    m = [axis_membership(n[k], occ.shape[k]).astype(np.int64) for k in range(3)]
    return np.einsum("ia,jb,kc,abc->ijk", *m, occ) > 0


def lattice_positions(n):
    """[nx+1, ny+1, nz+1, 3] float32: x = float32(i) * (2 / n) - 1, the multiply and the subtract separately rounded."""
    ax = [np.arange(n[k] + 1, dtype=np.float32) * (np.float32(2.0) / np.float32(n[k])) - np.float32(1.0) for k in range(3)]
    assert all(a.dtype == np.float32 for a in ax)
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


# ------------------------------------------------------------------------------------------------------------------- canonical form
def canonical(mesh):
    """-> {"cells" [V,3] sorted, "vertices", "lattice" in that order, "faces": sorted [F,3,3] of oriented triangles named by their
    vertices' cells, rotated so that the smallest cell comes first}.  Accepts tensors or arrays."""
    arr = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    cells, vertices, lattice, faces = arr(mesh.cells), arr(mesh.vertices), arr(mesh.lattice), arr(mesh.faces)
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0])) if len(cells) else np.zeros(0, np.int64)
    tri = cells[faces.astype(np.int64)].astype(np.int64) if len(faces) else np.zeros((0, 3, 3), np.int64)   # [F,3 corners,3]
    if len(tri):
        key = (tri[..., 0] << 42) | (tri[..., 1] << 21) | tri[..., 2]
        first = key.argmin(1)
        rot = (first[:, None] + np.arange(3)[None, :]) % 3
        tri = np.take_along_axis(tri, rot[..., None], 1)
        key = np.take_along_axis(key, rot, 1)
        tri = tri[np.lexsort((key[:, 2], key[:, 1], key[:, 0]))]
    return {"cells": cells[order], "vertices": vertices[order], "lattice": None if lattice is None else lattice[order], "faces": tri}


def face_keys(tri):
    """Oriented, rotated triangles [F,3,3] -> set of tuples."""
    return set(map(tuple, np.asarray(tri).reshape(len(tri), 9).tolist()))


# ------------------------------------------------------------------------------------------------------------------- topology checks
def topology(mesh):
    """(closed oriented 2-manifold?, Euler characteristic, signed volume) of a mesh."""
    f = np.asarray(mesh.faces, np.int64)
    v = np.asarray(mesh.vertices, np.float64)
    half = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    keys = set(map(tuple, half.tolist()))
    closed = len(keys) == len(half) and all((b, a) in keys for a, b in keys)
    E = len(keys) // 2
    chi = len(v) - E + len(f)
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
    return closed, chi, vol


# ------------------------------------------------------------------------------------------------------------------- cases
OCC_PATTERNS = ("full", "corner", "opposite", "ell", "checker", "none", "half")


def occupancy(pattern, log2dim):
    G = tuple(2 ** k for k in log2dim)
    occ = np.zeros(G, bool)
    if pattern == "full":
        occ[:] = True
    elif pattern == "corner":
        occ[0, 0, 0] = True
    elif pattern == "opposite":
        occ[-1, -1, -1] = True
    elif pattern == "ell":
        occ[: max(1, G[0] // 2), 0, 0] = True
        occ[0, : max(1, G[1] // 2), 0] = True
    elif pattern == "checker":
        i, j, k = np.meshgrid(*[np.arange(g) for g in G], indexing="ij")
        occ[:] = (i + j + k) % 2 == 0
    elif pattern == "half":
        i, j, k = np.meshgrid(*[np.arange(g) for g in G], indexing="ij")
        occ[:] = (i // 2 + j // 2 + k // 2) % 3 == 0
    else:
        assert pattern == "none"
    return occ


ModelCase = collections.namedtuple("ModelCase", "family half n log2dim pattern quantile seed")


def model_id(c):
    return f"{c.family}-{'f16' if c.half else 'f32'}-n{'x'.join(map(str, c.n))}-G{''.join(map(str, c.log2dim))}-{c.pattern}"


# level: the `quantile` of the live lattice values (between two of them); None: the family's fixed level (opaque 1, empty 0.1)
MODEL_CASES = [
    ModelCase("base", False, (12, 10, 8), (4, 4, 4), "full", 0.5, 700),
    ModelCase("base", True, (17, 9, 5), (4, 4, 4), "full", 0.4, 701),
    ModelCase("base", False, (40, 40, 40), (4, 4, 4), "half", 0.5, 702),
    ModelCase("aniso", False, (17, 9, 5), (3, 2, 4), "full", 0.5, 703),
    ModelCase("aniso", True, (12, 10, 8), (3, 2, 4), "checker", 0.6, 704),
    ModelCase("mask", False, (12, 10, 8), (4, 4, 4), "full", 0.5, 705),
    ModelCase("scaled", False, (17, 9, 5), (4, 4, 4), "full", 0.5, 706),
    ModelCase("scaled", True, (12, 10, 8), (4, 4, 4), "ell", 0.5, 707),
    ModelCase("empty", False, (12, 10, 8), (4, 4, 4), "full", None, 708),
]
OPAQUE_CASES = [ModelCase("opaque", i & 1 == 1, n, (4, 4, 4), p, None, 720 + i)
                for i, (n, p) in enumerate([((12, 10, 8), "corner"), ((17, 9, 5), "opposite"), ((40, 40, 40), "ell"),
                                            ((40, 40, 40), "checker"), ((12, 10, 8), "none"), ((17, 9, 5), "checker")])]
FIXED_LEVEL = {"opaque": 1.0, "empty": 0.1}
LOG2_T = 12


def model_inputs(c):
    """normals_reference.case_inputs of the case's family and table dtype (T = 2^12), its occupancy and the tile box: the inner half
    of the hash grid's 2x box -- occ_corner = mn + sz / 4, occ_size = sz / 2, [-1,1]^3 in contracted coordinates."""
    ins = NR.case_inputs(NR.Case(c.family, 1, 1, LOG2_T, False, c.half, "all", c.seed))
    ins = dict(ins)
    ins["occ"] = occupancy(c.pattern, c.log2dim)
    ins["occ_corner"] = (ins["mn"] + ins["sz"] / 4).numpy().astype(np.float32)
    ins["occ_size"] = (ins["sz"] / 2).numpy().astype(np.float32)
    return ins


def _sigma(ins, x, dtype, chunk=4096):
    out = []
    mask = NR.case_mask(ins)
    for i in range(0, len(x), chunk):
        out.append(NR.sigma_normals(x[i:i + chunk], NR.ascale_of(ins["sz"]), ins["table"], ins["res"], ins["sd"], mask, dtype)["sigma"].to(torch.float64))
    return torch.cat(out).numpy() if out else np.zeros(0)


@functools.lru_cache(maxsize=None)
def model_reference(c):
    """(inputs, live [points] bool, sigma64, sigma32 [points] as float64 arrays with 0 at dead points, level) -- computed once per
    process, shared, never written to.  Under "opaque" the density is not evaluated: live points are inside, whatever the table."""
    ins = model_inputs(c)
    live = live_points(c.n, ins["occ"])
    s64 = np.zeros(live.shape)
    s32 = np.zeros(live.shape)
    if c.family != "opaque":
        x = lattice_positions(c.n)[live]
        s64[live] = _sigma(ins, x, NR.F64)
        s32[live] = _sigma(ins, x, NR.F32)
        level = FIXED_LEVEL.get(c.family)
        if level is None:
            vals = np.sort(np.unique(s64[live].astype(np.float32)))
            i = min(max(int(c.quantile * len(vals)), 0), len(vals) - 2)
            level = float(np.float32((np.float64(vals[i]) + np.float64(vals[i + 1])) / 2))    # between two lattice values
    else:
        level = FIXED_LEVEL["opaque"]
    for a in (live, s64, s32):
        a.setflags(write=False)
    return ins, live, s64, s32, level


def ambiguous_points(s64, s32, live, level, k=K_MAX):
    e32 = float(np.abs(s32 - s64)[live].max()) if live.any() else 0.0
    return live & (np.abs(s64 - level) <= k * max(e32, 2.0 ** -24 * level))


def judged_cells(amb):
    """[nx,ny,nz] bool: the cells none of whose 8 corners is ambiguous."""
    n = tuple(s - 1 for s in amb.shape)
    bad = np.zeros(n, bool)
    for q in range(8):
        bad |= _shift(amb, ((q >> 2) & 1, (q >> 1) & 1, q & 1), n)
    return ~bad


def judge_mesh(name, got, ref64, ref32, judged, k=K):
    """got (any mesh with cells / faces / lattice), the float64 reference and the float32 yardstick, judged [nx,ny,nz] bool ->
    list of violations: activity and faces exactly, vertices (lattice steps) against k x the yardstick's error."""
    g, r, y = canonical(got), canonical(ref64), canonical(ref32)
    bad = []
    keep = lambda m: m["cells"][judged[m["cells"][:, 0], m["cells"][:, 1], m["cells"][:, 2]]] if len(m["cells"]) else m["cells"]
    gc, rc, yc = keep(g), keep(r), keep(y)
    if gc.shape != rc.shape or not np.array_equal(gc, rc):
        bad.append(f"{name}: active judged cells differ from the float64 reference ({len(gc)} vs {len(rc)})")
        return bad
    assert np.array_equal(yc, rc), "the float32 yardstick disagrees with float64 on a judged cell: the ambiguity band is too narrow"
    jd = lambda tri: judged[tri[..., 0], tri[..., 1], tri[..., 2]].all(1) if len(tri) else np.zeros(0, bool)
    gf, rf = face_keys(g["faces"]), face_keys(r["faces"])
    # reference triangles whose whole QUAD is judged: both triangles of a quad share its four cells; a triangle names three of them
    # and the fourth is the remaining corner of the 2 x 2 block they span
    def quad_judged(tri):
        lo, hi = tri.min(1), tri.max(1)
        ok = np.ones(len(tri), bool)
        for dx in range(2):
            for dy in range(2):
                for dz in range(2):
                    c = np.where(np.asarray([dx, dy, dz], bool), hi, lo)
                    ok &= judged[c[:, 0], c[:, 1], c[:, 2]]
        return ok
    must = face_keys(r["faces"][quad_judged(r["faces"])]) if len(r["faces"]) else set()
    missing = must - gf
    extra = face_keys(g["faces"][jd(g["faces"])]) - rf if len(g["faces"]) else set()
    if missing:
        bad.append(f"{name}: {len(missing)} judged faces of the reference are missing or flipped, e.g. {sorted(missing)[0]}")
    if extra:
        bad.append(f"{name}: {len(extra)} faces among judged cells are not the reference's, e.g. {sorted(extra)[0]}")
    if len(rc):
        sel = lambda m: m["lattice"][judged[m["cells"][:, 0], m["cells"][:, 1], m["cells"][:, 2]]]
        only = ("median", "p99", "max", "pooled") if len(rc) >= 16 else ("max", "pooled")
        bad += judge(name + " vertex", sel(g), sel(r), sel(y), k, scale=torch.ones(len(rc), dtype=torch.float64), only=only, floor=FLOOR)
    return bad


# ------------------------------------------------------------------------------------------------------------------- dense cases
BRICK = 8


def sphere_values(n, centre, radius):
    """A float32 lattice that is > 1 inside a sphere (lattice coordinates) and < 1 outside: 1 + radius - distance."""
    p = np.stack(np.meshgrid(*[np.arange(m + 1, dtype=np.float64) for m in n], indexing="ij"), -1)
    return (1.0 + radius - np.linalg.norm(p - np.asarray(centre, np.float64), axis=-1)).astype(np.float32)


def torus_values(n, centre, R, r):
    p = np.stack(np.meshgrid(*[np.arange(m + 1, dtype=np.float64) for m in n], indexing="ij"), -1) - np.asarray(centre, np.float64)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R
    return (1.0 + r - np.sqrt(q ** 2 + p[..., 2] ** 2)).astype(np.float32)


def dense_cases():
    """name -> (values float32, level): sizes around the brick, tiny and thin lattices, a sphere centred on a brick corner (its quads
    join four bricks), a plane exactly between bricks, values equal to the level, all inside, all outside."""
    rng = np.random.default_rng(5)
    noise = lambda n: rng.uniform(0.5, 1.5, tuple(m + 1 for m in n)).astype(np.float32)
    cases = {f"noise-{'x'.join(map(str, n))}": (noise(n), 1.0)
             for n in ((BRICK - 1, BRICK, BRICK + 1), (BRICK + 1, BRICK - 1, BRICK), (BRICK, BRICK + 1, BRICK - 1), (1, 1, 1), (2, 2, 2), (65, 1, 1),
                       (2 * BRICK + 1, BRICK, 3))}
    cases["sphere-on-brick-corner"] = (sphere_values((19, 18, 17), (8.0, 8.0, 8.0), 5.3), 1.0)
    plane = np.full((18, 12, 11), 0.5, np.float32)
    plane[:9] = 1.5                                  # inside up to point 8 = the last point of the first brick: crossings in brick 2
    cases["plane-between-bricks"] = (plane, 1.0)
    plane2 = np.full((18, 12, 11), 0.5, np.float32)
    plane2[:8] = 1.5                                 # crossings on the first brick's last cell layer
    cases["plane-before-brick-face"] = (plane2, 1.0)
    eq = noise((9, 9, 9))
    eq[rng.uniform(size=eq.shape) < 0.3] = 1.0       # value == level: outside
    cases["value-equals-level"] = (eq, 1.0)
    cases["all-inside"] = (np.full((10, 9, 11), 2.0, np.float32), 1.0)
    cases["all-outside"] = (np.full((10, 9, 11), 0.5, np.float32), 1.0)
    lone = np.zeros((3, 3, 3), np.float32)
    lone[1, 1, 1] = 2.0
    cases["lone-point"] = (lone, 1.0)
    return cases
