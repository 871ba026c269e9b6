"""Yardstick for the hit record and the rendered mesh (scanerf_amd.fastmesh trace / render_views, csrc/mesh_render.hip), numpy only,
written from the header comment of include/scanerf_mesh_tools_hip.h and not from the kernels.  Every piece exists twice: dtype =
np.float64 is the yardstick, dtype = np.float32 the restatement -- the same formula with every operation rounded to float32 in the
order the header gives, which the kernels must match bit for bit:

  pixel_rays     the ray of every pixel of a camera (scanerf_compute_ray_forward's formula);
  moller_trumbore (t, u, v, hit) of rays against faces, two-sided, edges inclusive, |det| <= 1e-12 dead;
  nearest        the (t, face) rule over ALL faces, no grid: smallest t, then lowest index; miss = (0, -1, 0, 0);
  on_face        (t, u, v) of each ray on ONE given face (what a returned face must reproduce);
  interpolate / face_normal / unit    the attribute rules;
  render         all of it per camera -> depth, face, normal, color.
The fixtures and the `grazing` flag (a ray that passes within 1e-4 barycentric of an edge near its hit) are fastmesh_reference's."""
import numpy as np

from fastmesh_reference import camera_rays, look_at, nearest_hit, shell_fixture, sloping_plane_fixture, terrain_fixture  # noqa: F401


def pixel_rays(K, M, H, W, dtype=np.float64):
    """K [9] or [3,3], M [12] or [3,4] float32 -> o, d [H*W,3] in `dtype`, row-major pixels:
    x = (1 px + 0.5 - K[2]) / K[0], y = (1 py + 0.5 - K[5]) / K[4], d_a = (M[4a] x + M[4a+1] y) + M[4a+2], o = (M[3], M[7], M[11])."""
    K, M = np.asarray(K, np.float32).reshape(9).astype(dtype), np.asarray(M, np.float32).reshape(-1)[:12].astype(dtype)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = (dtype(1.0) * px.astype(dtype) + dtype(0.5) - K[2]) / K[0]
    y = (dtype(1.0) * py.astype(dtype) + dtype(0.5) - K[5]) / K[4]
    d = np.stack([(M[4 * a] * x + M[4 * a + 1] * y) + M[4 * a + 2] for a in range(3)], -1).reshape(-1, 3)
    o = np.broadcast_to(np.array([M[3], M[7], M[11]], dtype), d.shape).copy()
    return o.astype(dtype), d.astype(dtype)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def moller_trumbore(o, d, A, E1, E2, dtype=np.float64):
    """o, d, A, E1, E2: arrays [...,3] of `dtype` that broadcast -> t, u, v, hit; every operation in `dtype`, in the header's order."""
    c = lambda x: [np.asarray(x[..., k], dtype) for k in range(3)]
    o, d, A, E1, E2 = c(o), c(d), c(A), c(E1), c(E2)
    with np.errstate(all="ignore"):
        p = _cross(d, E2)
        det = _dot(E1, p)
        ok = np.abs(det) > dtype(1e-12)
        inv = dtype(1.0) / np.where(ok, det, dtype(1.0))
        w = [o[k] - A[k] for k in range(3)]
        u = _dot(w, p) * inv
        q = _cross(w, E1)
        v = _dot(d, q) * inv
        t = _dot(E2, q) * inv
        hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return t, u, v, hit


def triangles(V, F, dtype=np.float64):
    """(A, B - A, C - A) [F,3] each, the subtraction in `dtype` from the float32 vertices."""
    V = np.asarray(V, np.float32).astype(dtype)
    A = V[F[:, 0]]
    return A, V[F[:, 1]] - A, V[F[:, 2]] - A


def nearest(o, d, V, F, dtype=np.float64, chunk=128):
    """-> t [B], face [B] i32, u, v [B]: over ALL faces the smallest t, among equal t the lowest index; a miss is (0, -1, 0, 0)."""
    A, E1, E2 = (x[None] for x in triangles(V, F, dtype))
    o, d = np.asarray(o, dtype), np.asarray(d, dtype)
    B = len(o)
    T, FA, U, W = np.zeros(B, dtype), np.full(B, -1, np.int32), np.zeros(B, dtype), np.zeros(B, dtype)
    for s in range(0, B, chunk):
        t, u, v, hit = moller_trumbore(o[s:s + chunk, None], d[s:s + chunk, None], A, E1, E2, dtype)
        t = np.where(hit, t, np.inf)
        f = t.argmin(1)                     # the first index of the minimum: the lowest face among equal t
        r = np.arange(len(f))
        found = np.isfinite(t[r, f])
        T[s:s + chunk] = np.where(found, t[r, f], 0)
        FA[s:s + chunk] = np.where(found, f, -1)
        U[s:s + chunk] = np.where(found, u[r, f], 0)
        W[s:s + chunk] = np.where(found, v[r, f], 0)
    return T, FA, U, W


def on_face(o, d, V, F, face, dtype=np.float32):
    """(t, u, v, hit) of ray i on face[i] (face >= 0), in `dtype`."""
    A, E1, E2 = triangles(V, F, dtype)
    return moller_trumbore(np.asarray(o, dtype), np.asarray(d, dtype), A[face], E1[face], E2[face], dtype)


def interpolate(attr, F, face, u, v, dtype=np.float64):
    """w0 = (1 - u) - v; a = (w0 a[ia] + u a[ib]) + v a[ic] per component; rows with face < 0 are 0."""
    a = np.asarray(attr).astype(dtype)          # (the kernels' attributes are float32; a float64 yardstick may pass finer ones)
    f = np.maximum(face, 0)
    u, v = np.asarray(u, dtype)[:, None], np.asarray(v, dtype)[:, None]
    w0 = (dtype(1.0) - u) - v
    out = (w0 * a[F[f, 0]] + u * a[F[f, 1]]) + v * a[F[f, 2]]
    return np.where((face >= 0)[:, None], out, dtype(0)).astype(dtype)


def face_normal(V, F, face, dtype=np.float64):
    """e1 x e2 of face[i] as wound (not normalised); rows with face < 0 are 0."""
    A, E1, E2 = triangles(V, F, dtype)
    f = np.maximum(face, 0)
    n = np.stack(_cross([E1[f, k] for k in range(3)], [E2[f, k] for k in range(3)]), -1)
    return np.where((face >= 0)[:, None], n, dtype(0)).astype(dtype)


def unit(n, dtype=np.float64):
    """n / (sqrt((nx nx + ny ny) + nz nz) + 1e-8)."""
    n = np.asarray(n, dtype)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(dtype) + dtype(1e-8)
    return (n / length[:, None]).astype(dtype)


def render(Ks, C2Ws, H, W, V, F, normals=None, colors=None, face_normals=False, dtype=np.float64):
    """The header's render_views over all faces -> {"depth" [C,H,W], "face" [C,H,W] i32, "normal", "color" [C,H,W,3]}."""
    out = {"depth": [], "face": [], "normal": [], "color": []}
    for K, M in zip(np.asarray(Ks), np.asarray(C2Ws)):
        o, d = pixel_rays(K, M, H, W, dtype)
        t, f, u, v = nearest(o, d, V, F, dtype)
        out["depth"].append(t.reshape(H, W))
        out["face"].append(f.reshape(H, W))
        if normals is not None or face_normals:
            n = interpolate(normals, F, f, u, v, dtype) if normals is not None else face_normal(V, F, f, dtype)
            out["normal"].append(unit(n, dtype).reshape(H, W, 3))
        if colors is not None:
            out["color"].append(interpolate(colors, F, f, u, v, dtype).reshape(H, W, 3))
    return {k: np.stack(v) for k, v in out.items() if v}


def grazing_rays(o, d, V, F):
    """fastmesh_reference's flag for a ray set."""
    return nearest_hit(np.asarray(o, np.float32), np.asarray(d, np.float32), V, F)[1]


def terrain_cameras(H=24, W=32):
    """Three cameras over the terrain fixture (two above it looking down at it, one low inside it looking along it), focal = W."""
    eyes = [((14.0, -12.0, 9.0), (0.0, 0.0, 0.0)), ((-3.0, 2.0, 12.0), (1.0, -1.0, 0.0)), ((0.5, 0.3, 2.2), (8.0, 7.0, 0.0))]
    cams = [look_at(e, t, H, W, float(W)) for e, t in eyes]
    return np.stack([k for _, k in cams]), np.stack([m for m, _ in cams])
