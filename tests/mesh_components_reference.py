"""Yardstick and case list of the mesh components and the filter by component (csrc/mesh_components.hip; test
infrastructure, CPU only, no GPU import).

The definition of include/scanerf_hip.h in numpy: a sequential union-find over the faces, the per-component table in rank order, the
keep rule and the filtered mesh.  Every quantity is an integer, so every comparison against this module is an equality.

Cases: dense value lattices (tests/surface_nets_reference.py's spheres and dense_cases) whose level set at 1.0 holds the condition
each is named for, and synthetic face lists at the smallest sizes at which the union-find, the aggregated sums and the
order-preserving compaction can still go wrong."""
import collections
import functools

import numpy as np

import surface_nets_reference as SN

Components = collections.namedtuple("Components", "labels label n_vertices n_faces cell_min cell_max")
Mesh = collections.namedtuple("Mesh", "vertices faces cells lattice normals")
Rules = collections.namedtuple("Rules", "min_faces min_extent keep_largest", defaults=(0, 0, None))


# ------------------------------------------------------------------------------------------------------------------- the definition
def labels_of(faces, V):
    """labels [V] int32: the smallest vertex index of every vertex's component (union-find with the smaller root on top)."""
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    return np.asarray([find(v) for v in range(V)], np.int32).reshape(V)


def components(faces, V, cells=None):
    """-> Components, the table in rank order: n_faces descending, ties by label ascending."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    labels = labels_of(faces, V)
    label = np.flatnonzero(labels == np.arange(V)).astype(np.int32)
    nv = np.bincount(labels, minlength=V)[label].astype(np.int32)
    nf = np.bincount(labels[faces[:, 0]], minlength=V)[label].astype(np.int32) if len(faces) else np.zeros(len(label), np.int32)
    cmin = cmax = None
    if cells is not None:
        cells = np.asarray(cells, np.int32).reshape(V, 3)
        cmin = np.full((V, 3), np.iinfo(np.int32).max, np.int32)
        cmax = np.full((V, 3), np.iinfo(np.int32).min, np.int32)
        np.minimum.at(cmin, labels, cells)
        np.maximum.at(cmax, labels, cells)
        cmin, cmax = cmin[label], cmax[label]
    order = np.lexsort((label, -nf.astype(np.int64)))
    pick = lambda a: None if a is None else np.ascontiguousarray(a[order])
    return Components(labels, pick(label), pick(nv), pick(nf), pick(cmin), pick(cmax))


def kept_rows(comps, rules):
    """[C] bool in rank order: the keep rule, its three conditions joined."""
    rules = Rules(*rules)
    C = len(comps.label)
    keep = comps.n_faces >= rules.min_faces
    if rules.min_extent > 0:
        assert comps.cell_min is not None, "min_extent needs cells"
        keep &= (comps.cell_max.astype(np.int64) - comps.cell_min + 1).max(1) >= rules.min_extent
    if rules.keep_largest is not None:
        keep &= np.arange(C) < rules.keep_largest
    return keep


def filter_mesh(mesh, rules):
    """mesh: anything with vertices / faces / cells / lattice / normals (arrays or None) -> Mesh of numpy arrays by the definition."""
    arr = lambda a: None if a is None else np.asarray(a)
    vertices, faces = arr(mesh.vertices), np.asarray(mesh.faces, np.int32).reshape(-1, 3)
    cells, lattice, normals = arr(mesh.cells), arr(mesh.lattice), arr(getattr(mesh, "normals", None))
    V = len(vertices)
    comps = components(faces, V, cells)
    kept = np.zeros(V, bool)
    kept[comps.label[kept_rows(comps, rules)]] = True
    kv = kept[comps.labels] if V else np.zeros(0, bool)
    kf = kv[faces[:, 0]] if len(faces) else np.zeros(0, bool)
    new_index = np.cumsum(kv) - 1
    pick = lambda a: None if a is None else np.ascontiguousarray(a[kv])
    return Mesh(pick(vertices), new_index[faces[kf]].astype(np.int32).reshape(-1, 3), pick(cells), pick(lattice), pick(normals))


# ------------------------------------------------------------------------------------------------------------------- lattice cases
N3 = (40, 24, 24)
LEVEL = 1.0


def _spheres(n, *balls):
    return np.maximum.reduce([SN.sphere_values(n, c, r) for c, r in balls])


def sparse_noise():
    """24^3 cells of uniform(0, 1.08): a few hundred small components, faceless ones and many ties in n_faces (seed 11, the
    generator's second draw)."""
    rng = np.random.default_rng(11)
    rng.uniform(size=4)
    return rng.uniform(0.0, 1.08, (25, 25, 25)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lattice_cases():
    """name -> values [nx+1, ny+1, nz+1] float32 (read-only), all cut at LEVEL."""
    dense = SN.dense_cases()
    cases = {
        "three": _spheres(N3, ((9.3, 12.1, 11.7), 6.4), ((30.6, 12.0, 12.2), 6.4), ((20.2, 5.1, 19.9), 1.3)),
        "twin": _spheres(N3, ((10.0, 12.0, 12.0), 6.4), ((30.0, 12.0, 12.0), 6.4)),
        "value-equals-level": dense["value-equals-level"][0],
        "noise-65x1x1": dense["noise-65x1x1"][0],
        "sparse-noise": sparse_noise(),
    }
    for v in cases.values():
        v.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def lattice_reference(name):
    """(the numpy surface nets mesh of the case in float32, its Components) -- computed once per process, never written to."""
    m = SN.surface_nets(lattice_cases()[name], LEVEL, dtype=np.float32)
    mesh = Mesh(m.vertices.astype(np.float32), m.faces, m.cells, m.lattice.astype(np.float32), None)
    return mesh, components(mesh.faces, len(mesh.vertices), mesh.cells)


# the rule combinations every lattice case is filtered by: each condition alone, ties under keep_largest, all three joined
RULES = [Rules(), Rules(min_faces=1), Rules(min_faces=100), Rules(min_extent=3), Rules(keep_largest=1), Rules(keep_largest=2),
         Rules(keep_largest=0), Rules(min_faces=2, min_extent=2, keep_largest=5), Rules(min_faces=10 ** 6)]


# ------------------------------------------------------------------------------------------------------------------- synthetic graphs
CHAIN = 65537


def _chain(ids):
    """A chain over the vertices ids[0] - ids[1] - ... as triangles (ids[i], ids[i+1], ids[i+1])."""
    ids = np.asarray(ids, np.int32)
    return np.stack([ids[:-1], ids[1:], ids[1:]], 1)


@functools.lru_cache(maxsize=None)
def graph_cases():
    """name -> (faces [F,3] int32, V)."""
    rng = np.random.default_rng(17)
    cases = {
        "chain-permuted": (_chain(rng.permutation(CHAIN)), CHAIN),
        "chain-reversed": (_chain(np.arange(CHAIN)[::-1]), CHAIN),
    }
    # a fan of 20 000 faces around the vertex with the LARGEST index: every hook moves the root, one label takes all the sums
    nf = 20000
    rim = np.arange(nf + 1, dtype=np.int32)
    cases["fan-around-largest"] = (np.stack([np.full(nf, nf + 1, np.int32), rim[:-1], rim[1:]], 1), nf + 2)
    cases["disjoint-triangles"] = (rng.permutation(30000).astype(np.int32).reshape(10000, 3), 30000)
    # two components interleaved on even and odd indices (strips (i, i+2, i+4)), V not a multiple of the wave
    V = 4099
    i = np.arange(V - 4, dtype=np.int32)
    cases["even-odd"] = (np.stack([i, i + 2, i + 4], 1), V)
    # degenerate faces (two or three equal indices) and duplicates; vertices 10..19 unused
    cases["degenerate-duplicate"] = (np.asarray([[0, 0, 1], [1, 2, 2], [3, 3, 3], [4, 5, 6], [4, 5, 6], [6, 5, 4], [7, 8, 7], [9, 8, 8],
                                                 [0, 0, 1], [20, 21, 21], [21, 20, 20]], np.int32), 22)
    cases["no-faces"] = (np.zeros((0, 3), np.int32), 1000)
    for f, _ in cases.values():
        f.setflags(write=False)
    return cases


def graph_cells(V):
    """Cells for a synthetic graph: distinct, not monotone in the index."""
    v = np.arange(V, dtype=np.int64)
    return np.stack([(v * 7919) % 1013, v // 256, (v * 31) % 97], 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def graph_reference(name):
    faces, V = graph_cases()[name]
    return components(faces, V, graph_cells(V))


def permuted(faces, seed):
    """The same faces in another order, each with its corners permuted."""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces)[rng.permutation(len(faces))]
    corners = np.argsort(rng.uniform(size=f.shape), 1)
    return np.ascontiguousarray(np.take_along_axis(f, corners, 1))


def topology_of(mesh):
    return SN.topology(SN.Mesh(mesh.vertices, mesh.faces, mesh.cells, mesh.lattice))
