"""Yardstick and case list of the fused mesh's normals (csrc/tsdf.hip, scanerf_tsdf_vertex_normals; test infrastructure,
numpy only, no GPU import), written from the comment of include/scanerf_mesh_tools_hip.h, not from the kernel.  It builds on
tsdf_reference and tsdf_color_reference (the sphere cases, their float32 acc and their culled reference meshes), which it imports and
does not change.

    lattice_gradient(values, observed, n, spacing, dtype)    g_a(q) at EVERY lattice point with all four branches, and which was taken
    vertex_normals(values, observed, n, spacing, cells, lattice, dtype)
                                                             the definition in float64 (the reference: adds the bounds and `judged`)
                                                             or float32 (the restatement: the kernel's and the composed torch route's
                                                             IEEE operations, so equal bits are expected of all three)
    sphere(name)                                             values / observed of the case's float32 acc, the culled reference mesh,
                                                             both results, the radial and the face-average figures; computed once
    linear_field / quadratic_field / HAND_*                  hand lattices with exact answers
    face_average_normals(vertices, faces)                    the area-weighted face-normal average (the alternative, for the record)

THE DEFINITION.  Per lattice point q and axis a (h = spacing[a]): has+ iff q + e_a is inside the lattice and observed, has- likewise;
g_a(q) = (val[q+] - val[q-]) / (h + h) with both, (val[q+] - val[q]) / h with has+ alone, (val[q] - val[q-]) / h with has- alone, 0
with neither.  At a vertex: t_a = fmin(fmax(lattice_a - cell_a, 0), 1), corner d = (d >> 2, (d >> 1) & 1, d & 1) with the weight
w_d = (wx wy) wz, G_a = sum_d w_d g_a(q_d) in ascending d from the d = 0 product; len = sqrt((Gx Gx + Gy Gy) + Gz Gz);
normal = (-G) / (len + 1e-8f); grad = G.  A cell outside the lattice or with an unobserved corner: zeros.

THE BOUND FOR grad (u = 2^-24, absolute errors, float64 on the float32 inputs taken as exact; h + h is exact in both precisions).
  g_d = fl(fl(a - b) / den): the difference carries u |a - b|, the quotient u |g_d|: dg_d <= 2 u |g_d| (0 in the "neither" branch).
  The axis weights carry an absolute error <= u each (tsdf_color_reference's analysis), so
  dw_d <= u (wy wz + wx wz + wx wy) + 2 u w_d.
  G = sum_d w_d g_d in ascending d: dG <= sum_d (dw_d |g_d| + w_d dg_d + u |w_d g_d|) + u sum_{j=1..7} |partial_j|,
  times (1 + 2^-10) for the higher orders: "grad_bound" [V,3].  Which branch a stencil takes depends on `observed` alone: the two
  precisions cannot disagree on it.
THE BOUND FOR normal.  With b = |grad_bound|_2: len' differs from len by at most b (the norm is 1-Lipschitz) and by its own roundings
  (three squares and two additions of positive terms: 3 u relative under the root, 1.5 u after it, u for the root), the denominator by
  one more u, the quotient by u: 4.5 u relative, rounded up to 5 u, on components of magnitude <= 1.  Propagated:
  |dn_a| <= (dG_a + |n_a| b) / (den - b) <= (max_a dG_a + b) / (den - b).
  "normal_bound" [V] = ((max_a grad_bound_a + b) / (den - b) + 5 u) (1 + 2^-10), the bound over len the issue names.
JUDGED.  A vertex is judged iff b <= FRACTION len (FRACTION = 2^-10: the direction is then known to about 0.1 degree, thirty times
  below the method's own error on the spheres), or the definition gives it zeros by rule (nothing is computed).  A vertex with
  G = 0 exactly in float64 but evaluated is judged iff its bound is 0 too."""
import functools

import numpy as np

import tsdf_color_reference as CR
import tsdf_reference as TR

U, f32 = TR.U, np.float32
HIGHER = CR.HIGHER
FRACTION = 2.0 ** -10
EPS = f32(1e-8)
NEITHER, MINUS_ONLY, PLUS_ONLY, BOTH = 0, 1, 2, 3       # lattice_gradient's branch codes: 2 has+ + has-


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def lattice_gradient(values, observed, n, spacing, dtype=np.float64):
    """g [P,3] in `dtype` and branch [P,3] (the codes above) at every lattice point; values [P] float32, observed [P] (non-zero = yes)."""
    T = dtype
    shape = [m + 1 for m in n]
    val = np.asarray(values, f32).reshape(shape).astype(T)
    obs = np.asarray(observed).reshape(shape) != 0
    g, branch = np.zeros((*shape, 3), T), np.zeros((*shape, 3), np.int8)
    with np.errstate(all="ignore"):
        for a in range(3):
            h = T(f32(spacing[a]))
            h2 = h + h
            vp, vm, hp, hm = np.roll(val, -1, a), np.roll(val, 1, a), np.roll(obs, -1, a), np.roll(obs, 1, a)
            last, first = [slice(None)] * 3, [slice(None)] * 3
            last[a], first[a] = -1, 0
            hp[tuple(last)] = False          # q + e_a is outside the lattice (the rolled value wrapped round: never used)
            hm[tuple(first)] = False
            both, plus, minus = (vp - vm) / h2, (vp - val) / h, (val - vm) / h
            assert both.dtype == T and plus.dtype == T and minus.dtype == T
            g[..., a] = np.where(hp & hm, both, np.where(hp, plus, np.where(hm, minus, T(0))))
            branch[..., a] = 2 * hp + hm
    return g.reshape(-1, 3), branch.reshape(-1, 3)


def vertex_normals(values, observed, n, spacing, cells, lattice, dtype=np.float64):
    """The header's scanerf_tsdf_vertex_normals, every operation in `dtype`.  -> {"normal" [V,3], "grad" [V,3], "evaluated" [V] (False:
    zeros by rule), "branches" [V,8,3]}; float64 adds "grad_bound" [V,3], "normal_bound" [V] and "judged" [V] (see the module text)."""
    T = dtype
    lattice = np.asarray(lattice, f32).reshape(-1, 3).astype(T)
    inside, q = CR._rows(n, cells)
    obs = np.asarray(observed).reshape(-1) != 0
    ok = inside & obs[q].all(1)
    cell = np.asarray(cells, np.int64).reshape(-1, 3).astype(T)
    g, branch = lattice_gradient(values, observed, n, spacing, T)
    V = len(q)
    with np.errstate(all="ignore"):
        t = np.fmin(np.fmax(lattice - cell, T(0)), T(1))           # fmaxf / fminf: a NaN becomes 0
        w = np.stack([T(1) - t, t], -1)                             # [V,3,2]
        assert w.dtype == T
        G = None
        dG, partial = np.zeros((V, 3)), np.zeros((V, 3))
        for d in range(8):
            i, j, k = d >> 2, (d >> 1) & 1, d & 1
            wd = (w[:, 0, i] * w[:, 1, j]) * w[:, 2, k]
            gd = g[q[:, d]]
            prod = wd[:, None] * gd
            G = prod if d == 0 else G + prod
            assert G.dtype == T
            if T is np.float64:
                dw = U * (w[:, 1, j] * w[:, 2, k] + w[:, 0, i] * w[:, 2, k] + w[:, 0, i] * w[:, 1, j]) + 2.0 * U * wd
                dG += dw[:, None] * np.abs(gd) + wd[:, None] * (2.0 * U * np.abs(gd)) + U * np.abs(prod)
                if d:
                    partial += np.abs(G)
        length = np.sqrt((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2])
        den = length + T(EPS)
        normal = (-G) / den[:, None]
        assert normal.dtype == T and length.dtype == T
    zero = np.zeros((V, 3), T)
    res = {"normal": np.where(ok[:, None], normal, zero), "grad": np.where(ok[:, None], G, zero), "evaluated": ok,
           "branches": branch[q]}
    if T is np.float64:
        gb = np.where(ok[:, None], (dG + U * partial) * HIGHER, 0.0)
        b = np.linalg.norm(gb, axis=1)
        judged = ~ok | (b <= FRACTION * length)
        with np.errstate(all="ignore"):
            nb = ((gb.max(1) + b) / (den - b) + 5.0 * U) * HIGHER
        res["grad_bound"] = gb
        res["normal_bound"] = np.where(ok & judged, nb, 0.0)
        res["judged"] = judged
    return res


# ---- figures ---------------------------------------------------------------------------------------------------------------------------
def angles_deg(a, b):
    """The angle between the rows of a and b, degrees, float64; NaN where one is zero."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        c = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def face_average_normals(vertices, faces):
    """[V,3] float64: the sum of cross(b - a, c - a) (twice the area times the unit normal) over the faces at each vertex, normalised."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, f[:, k], fn)
    with np.errstate(all="ignore"):
        return out / np.linalg.norm(out, axis=1, keepdims=True)


SPHERES = CR.SPHERES
# the mean angle (degrees) between the float64 normal and the radial direction at the vertices of the culled reference mesh, as
# this module computes it, and tsdf_color_reference's margin for choices that move the culled mesh's vertex set
RADIAL_MEAN_DEG = {"sphere6": 6.27, "sphere40": 3.82, "sphere70": 3.50}
# the same for the area-weighted face-normal average: recorded, not a bound on anything the library computes
FACE_AVERAGE_MEAN_DEG = {"sphere6": 5.81, "sphere40": 2.99, "sphere70": 2.96}
RADIAL_MARGIN = CR.RADIAL_MARGIN
JUDGED_SHARE = 0.95


@functools.lru_cache(maxsize=None)
def field(name, min_weight=1.0):
    """Any of tsdf_reference's four cases -> {"n", "spacing", "values" [P] f32, "observed" [P] bool, "raw", "mesh" (the culled
    reference mesh), "ref64", "ref32" (vertex_normals on the culled mesh)}; computed once and shared (treat as read-only)."""
    c = CR.case(name)
    val, obs = TR.values(c["cref32"]["acc"], min_weight)
    raw, mesh = CR.reference_mesh(c, min_weight)
    out = {"name": name, "n": c["n"], "spacing": c["spacing"], "values": val, "observed": obs, "raw": raw, "mesh": mesh}
    for key, T in (("ref64", np.float64), ("ref32", np.float32)):
        out[key] = vertex_normals(val, obs, c["n"], c["spacing"], mesh.cells, mesh.lattice, T)
    return out


def sphere(name):
    """field(name) of a sphere case plus "radial_deg" [V] (float64 normal against the radial direction) and "face_deg" [V] (the
    face-normal average against it)."""
    s = dict(field(name))
    v = np.asarray(s["mesh"].vertices, np.float64)
    s["radial_deg"] = angles_deg(s["ref64"]["normal"], v)
    s["face_normals"] = face_average_normals(v, s["mesh"].faces)
    s["face_deg"] = angles_deg(s["face_normals"], v)
    return s


# ---- hand lattices -----------------------------------------------------------------------------------------------------------------------
def lattice_indices(n):
    """[P,3] int: (i, j, k) of every lattice point, z fastest."""
    return np.stack(np.meshgrid(*[np.arange(m + 1) for m in n], indexing="ij"), -1).reshape(-1, 3)


def linear_field(n, coeffs, offset):
    """val = a i + b j + c k + d at every lattice point, float32 (exact for dyadic coefficients of moderate size)."""
    ijk = lattice_indices(n).astype(np.float64)
    val = ijk @ np.asarray(coeffs, np.float64) + offset
    assert np.array_equal(val.astype(f32).astype(np.float64), val), "the field is not exact in float32"
    return val.astype(f32)


def quadratic_field(n, axis, scale=1.0):
    """val = scale * i_axis^2: central difference at i is 2 i scale / h, forward (2 i + 1) scale / h, backward (2 i - 1) scale / h."""
    i = lattice_indices(n)[:, axis].astype(np.float64)
    return (scale * i * i).astype(f32)


def random_vertices(n, V, seed, outside=False):
    """cells [V,3] int32 inside the lattice (outside=True: some one step out on either side) and lattice positions in them."""
    rng = np.random.default_rng(seed)
    lo, hi = (-1, 1) if outside else (0, 0)
    cells = np.stack([rng.integers(lo, m + hi, V) for m in n], 1).astype(np.int32)
    return cells, (cells + rng.uniform(0.0, 1.0, (V, 3))).astype(f32)


def unit_lattice():
    """n = (1, 1, 1): eight points, every stencil one-sided on every axis.  val(i, j, k) = 0.5 i + 0.25 j + 2 k + i j k with
    spacing (0.5, 0.25, 2): at the cell centre the hand answer is worked in the test."""
    n, spacing = (1, 1, 1), (0.5, 0.25, 2.0)
    ijk = lattice_indices(n).astype(np.float64)
    val = (0.5 * ijk[:, 0] + 0.25 * ijk[:, 1] + 2.0 * ijk[:, 2] + ijk[:, 0] * ijk[:, 1] * ijk[:, 2]).astype(f32)
    return n, spacing, val, np.ones(8, bool)


HAND_N = (3, 4, 65)          # n_z = 65: 66 points a row, so stencils cross a 64-row boundary
HAND_SPACING = (0.5, 0.25, 0.125)


@functools.lru_cache(maxsize=None)
def hand():
    """A lattice with a smooth non-linear field and a pattern of unobserved points: every branch of the lattice gradient occurs at
    the corners of evaluated cells but "neither" (which an evaluated cell cannot have), and cells with an unobserved corner and
    cells outside the lattice are among the vertices.  -> dict like field()'s, vertices 257."""
    n, spacing = HAND_N, HAND_SPACING
    ijk = lattice_indices(n).astype(np.float64)
    val = (0.5 + 0.05 * np.sin(0.7 * ijk[:, 0] + 0.3 * ijk[:, 2]) + 0.01 * ijk[:, 1] * ijk[:, 1] - 0.004 * ijk[:, 2]).astype(f32)
    rng = np.random.default_rng(65)
    obs = rng.uniform(size=len(val)) > 0.03
    cells, lattice = random_vertices(n, 257, 66, outside=True)
    lattice[3] = cells[3]                       # t = 0 on every axis
    lattice[4] = cells[4] + 1                   # t = 1
    lattice[5] = (np.nan, cells[5, 1] - 3.0, cells[5, 2] + 7.0)      # NaN -> 0, below 0 -> 0, above 1 -> 1
    out = {"name": "hand", "n": list(n), "spacing": list(spacing), "values": val, "observed": obs, "cells": cells, "lattice": lattice}
    for key, T in (("ref64", np.float64), ("ref32", np.float32)):
        out[key] = vertex_normals(val, obs, n, spacing, cells, lattice, T)
    return out
