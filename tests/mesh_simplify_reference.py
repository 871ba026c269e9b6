"""numpy reference of mesh simplification by vertex clustering, written from the comment of
include/scanerf_mesh_tools_hip.h (scanerf_mesh_simplify_cluster), not from the kernel: float32 operation by operation for the key and
the output, Python / numpy integers for everything that is summed.  Also the lattice cases, the synthetic inputs the GPU tests share
and the topology helpers of the known answers."""
import collections
import functools

import numpy as np

import surface_nets_reference as SN

f32 = np.float32
CELL_LIMIT = 2 ** 20
Result = collections.namedtuple("Result", "vertices faces normals colors counts row n_bad")


class BadVertices(ValueError):
    """simplify() met bad vertices; n_bad is their number."""
    def __init__(self, n_bad):
        super().__init__(f"{n_bad} bad vertices")
        self.n_bad = n_bad


def key(vertices, origin, h):
    """-> (k [V,3] float32, q [V,3] int64, good [V] bool by the coordinates).  u = (v - o) / h; k = floorf(u); f = u - k;
    q = (int)(f * 65536): four float32 operations, one rounding each."""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    o, h = np.asarray(origin, f32), f32(h)
    with np.errstate(all="ignore"):
        u = ((v - o).astype(f32) / h).astype(f32)
        k = np.floor(u).astype(f32)
        f = (u - k).astype(f32)
        good = (np.isfinite(v) & (np.abs(k) < f32(CELL_LIMIT))).all(1)
        q = np.where(good[:, None], (f * f32(65536.0)).astype(f32), f32(0)).astype(np.int64)
    return k, q, good


def fixed(a):
    """t = rintf(fminf(fmaxf(a, -32767), 32767) * 65536) as int64 (np.rint rounds halves to even, as rintf does)."""
    a = np.asarray(a, f32)
    return np.rint((np.minimum(np.maximum(a, f32(-32767.0)), f32(32767.0)) * f32(65536.0)).astype(f32)).astype(np.int64)


def rounded_mean(S, n):
    """M = floor((2 S + n) / (2 n)): numpy's // on int64 is the floor division, for negative values too."""
    return (2 * S + n) // (2 * n)


def count_bad(vertices, origin, h, normals=None, colors=None):
    good = key(vertices, origin, h)[2]
    for a in (normals, colors):
        if a is not None:
            good = good & np.isfinite(np.asarray(a, f32)).all(1)
    return int((~good).sum())


def simplify(vertices, faces, h, origin=(0.0, 0.0, 0.0), normals=None, colors=None):
    """The definition -> Result(vertices [V',3] f32, faces [F',3] i32, normals, colors (None where not given), counts [V'] (the
    members of every cluster), row [V] (the output vertex of every input vertex), n_bad = 0).  Bad vertices raise BadVertices."""
    v = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V = v.shape[0]
    n_bad = count_bad(v, origin, h, normals, colors)
    if n_bad:
        raise BadVertices(n_bad)
    k, q, _ = key(v, origin, h)
    ki = k.astype(np.int64)
    label = np.empty(V, np.int64)
    first = {}
    for i, cell in enumerate(map(tuple, ki.tolist())):          # in ascending index: the first member met is the smallest
        label[i] = first.setdefault(cell, i)
    roots = np.flatnonzero(label == np.arange(V))
    number = np.full(V, -1, np.int64)
    number[roots] = np.arange(roots.shape[0])
    row = number[label]
    Vk = roots.shape[0]
    counts = np.bincount(row, minlength=Vk).astype(np.int64)
    n = counts[:, None]
    single = counts == 1

    def mean(t):
        S = np.zeros((Vk, 3), np.int64)
        np.add.at(S, row, t)
        return (rounded_mean(S, n).astype(f32) * f32(2.0 ** -16)).astype(f32)

    o, hh = np.asarray(origin, f32), f32(h)
    out_v = (o + ((k[roots] + mean(q)).astype(f32) * hh).astype(f32)).astype(f32)
    out_v[single] = v[roots[single]]
    out_n = out_c = None
    if normals is not None:
        nn = np.asarray(normals, f32)
        m = mean(fixed(nn))
        sq = lambda a: (a * a).astype(f32)
        length = (np.sqrt(((sq(m[:, 0]) + sq(m[:, 1])).astype(f32) + sq(m[:, 2])).astype(f32)).astype(f32) + f32(1e-8)).astype(f32)
        out_n = (m / length[:, None]).astype(f32)
        out_n[single] = nn[roots[single]]
    if colors is not None:
        cc = np.asarray(colors, f32)
        out_c = mean(fixed(cc))
        out_c[single] = cc[roots[single]]
    rf = row[faces.astype(np.int64)].reshape(-1, 3)
    keep = (rf[:, 0] != rf[:, 1]) & (rf[:, 0] != rf[:, 2]) & (rf[:, 1] != rf[:, 2])
    return Result(out_v, rf[keep].astype(np.int32), out_n, out_c, counts, row, 0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- topology of the known answers --------------------------------------------------------------------------------------------------
def edge_counts(faces):
    """-> the number of faces at every undirected edge (an int array over the distinct edges)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(1)
    return np.unique(e, axis=0, return_counts=True)[1] if e.shape[0] else np.zeros(0, np.int64)


def closed_manifold(faces):
    c = edge_counts(faces)
    return c.shape[0] > 0 and bool((c == 2).all())


def euler(n_vertices, faces):
    return int(n_vertices) - int(edge_counts(faces).shape[0]) + int(np.asarray(faces).reshape(-1, 3).shape[0])


def duplicate_triples(faces):
    """The faces that repeat an earlier face's vertex set."""
    f = np.sort(np.asarray(faces, np.int64).reshape(-1, 3), 1)
    return int(f.shape[0] - np.unique(f, axis=0).shape[0]) if f.shape[0] else 0


# ---- the lattice cases (float32 vertices, origin 0, spacing 1) -----------------------------------------------------------------------
# name -> (V, F, {h: (V', F')}, Euler characteristic): the known answers of DESIGN.md 4.23
LATTICE = {
    "sphere48": (6310, 12616, {2.0: (1578, 3152), 3.0: (698, 1392), 4.0: (412, 820)}, 2),
    "torus48": (4070, 8140, {2.0: (1018, 2036), 3.0: (442, 884), 4.0: (276, 552)}, 0),
    "sphere19": (536, 1068, {2.0: (128, 252), 3.0: (62, 120), 4.0: (32, 60)}, 2),
}
IDENTITY_CELLS = (0.25, 1.0)
PLATE = (716, 1428, {4.0: (36, 100), 2.0: (200, 396)})


def _values(name):
    if name == "sphere48":
        return SN.sphere_values((48, 48, 48), (23.7, 24.1, 24.4), 18.3)
    if name == "torus48":
        return SN.torus_values((48, 48, 24), (24.2, 23.9, 12.3), 14.0, 5.2)
    if name == "sphere19":
        return SN.sphere_values((19, 18, 17), (8.0, 8.0, 8.0), 5.3)
    assert name == "plate"
    v = np.full((26, 26, 26), 0.5, np.float32)          # a 25^3 lattice
    v[10:12, 4:21, 4:21] = 1.5
    return v


@functools.lru_cache(maxsize=None)
def lattice_mesh(name):
    """-> (vertices [V,3] f32, faces [F,3] i32, normals [V,3] f32, colors [V,3] f32) of a lattice case; the attributes are smooth
    functions of the position (unit radial normals about the lattice's middle, colours in [0, 1]).  Shared: do not write to them."""
    m = SN.surface_nets(_values(name), 1.0, dtype=np.float32)
    v = np.ascontiguousarray(m.vertices, np.float32)
    faces = np.ascontiguousarray(m.faces, np.int32)
    d = v - v.mean(0, dtype=np.float64).astype(np.float32)
    normals = (d / (np.linalg.norm(d, axis=1, keepdims=True) + np.float32(1e-8))).astype(np.float32)
    colors = (0.5 + 0.5 * np.sin(v * np.float32(0.37) + np.array([0.0, 1.0, 2.0], np.float32))).astype(np.float32)
    for a in (v, faces, normals, colors):
        a.setflags(write=False)
    return v, faces, normals, colors


# ---- synthetic inputs -----------------------------------------------------------------------------------------------------------------
def _attributes(rng, V):
    n = rng.normal(size=(V, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    return n, rng.uniform(0, 1, (V, 3)).astype(np.float32)


def random_mesh(V, F, seed, span=6.0):
    """V random vertices in [-span, span)^3, F random faces (some degenerate in the input already), attributes."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-span, span, (V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32) if V else np.zeros((0, 3), np.int32)
    if F >= 4:
        faces[1, 1] = faces[1, 0]          # degenerate input faces: two and three equal corners
        faces[3] = faces[3, 0]
    return (v, faces) + _attributes(rng, V)


def one_cluster(V=6310, seed=11):
    """Every vertex in the cell [0, 1)^3 of h = 1: the most contended row."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.01, 0.99, (V, 3)).astype(np.float32)
    return (v, rng.integers(0, V, (2 * V, 3)).astype(np.int32)) + _attributes(rng, V)


def line_of_singles(V=65537, seed=12):
    """V one-member clusters on a line at h = 1, the vertex ids permuted; faces join neighbours on the line."""
    rng = np.random.default_rng(seed)
    x = rng.permutation(V).astype(np.float32) - np.float32(V // 2)
    v = np.stack([x + rng.uniform(0.1, 0.9, V).astype(np.float32), np.full(V, 0.3, np.float32), np.full(V, -0.7, np.float32)], 1)
    order = np.argsort(x).astype(np.int32)
    faces = np.stack([order[:-2], order[1:-1], order[2:]], 1)
    return (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(faces)) + _attributes(rng, V)


def block_of_cells(side=40, seed=13):
    """side^3 vertices in side^3 distinct cells of h = 1 (the table at its documented load: V keys in the smallest power of two
    >= 2 V slots), ids permuted."""
    rng = np.random.default_rng(seed)
    c = np.stack(np.meshgrid(*[np.arange(side) - side // 2] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(side ** 3)]
    v = (c + rng.uniform(0.1, 0.9, c.shape)).astype(np.float32)
    V = v.shape[0]
    return (v, rng.integers(0, V, (V, 3)).astype(np.int32)) + _attributes(rng, V)


def extreme_keys(seed=14):
    """Cells at +-(2^20 - 1) on every axis (h = 1; the largest keys that are not bad), a few members each, and cells near 0."""
    rng = np.random.default_rng(seed)
    big = float(CELL_LIMIT - 1)
    base = np.array([[big, big, big], [-big, -big, -big], [big, -big, 0.0], [0.0, big, -big], [-1.0, 0.0, 1.0]], np.float32)
    v = np.repeat(base, 3, 0) + np.tile(np.array([[0.0], [0.25], [0.5]], np.float32), (5, 3))
    v = np.ascontiguousarray(v[rng.permutation(v.shape[0])], np.float32)
    V = v.shape[0]
    return (v, rng.integers(0, V, (24, 3)).astype(np.int32)) + _attributes(rng, V)


def bad_cases():
    """name -> (vertices, faces, normals, colors, n_bad): one bad vertex of each kind in a small random mesh."""
    out = {}
    for name, where, value in (("nan-coordinate", "v", np.nan), ("inf-coordinate", "v", np.inf), ("cell-2^20", "v", float(CELL_LIMIT)),
                               ("cell-minus-2^20-1", "v", -float(CELL_LIMIT) - 1.0), ("nan-normal", "n", np.nan), ("inf-colour", "c", -np.inf)):
        v, f, n, c = (a.copy() for a in random_mesh(70, 90, 21))
        {"v": v, "n": n, "c": c}[where][37, 1] = value
        out[name] = (v, f, n, c, 1)
    v, f, n, c = (a.copy() for a in random_mesh(70, 90, 22))
    v[3, 0] = np.nan
    n[3, 2] = np.inf          # one vertex, bad twice: counted once
    c[64, 0] = np.nan
    out["several"] = (v, f, n, c, 2)
    return out
