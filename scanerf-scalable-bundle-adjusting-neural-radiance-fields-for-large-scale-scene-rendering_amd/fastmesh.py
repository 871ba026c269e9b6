"""`FastMesh`: the reference's ray / mesh tracer module (fastMesh/__init__.py:9-133) with its method names and return
conventions, on the HIP tracer of csrc/mesh.hip.

The acceleration structure -- a uniform grid of 2^log2dim cells per axis with a bitmask, a per-word rank, per-cell face
lists and per-cell boxes -- is built on the device from the [V,3] float32 / [F,3] int32 arrays of formats.read_ply (the
reference builds it in a host loop, fastMesh/include/tile_structure.h:13-106).  The build uses no atomics on floats and no
data-dependent order: two builds of one mesh give the same arrays bit for bit.

Two deliberate differences from the reference's kernels:
  * rays are clipped to the grid cube first, so origins outside the mesh bounds are traced correctly;
  * first_hit carries its nearest candidate across cells; the reference returns at the first cell with any hit, even one that
    lies beyond that cell, which hides nearer surfaces behind large triangles.
closest_point (csrc/mesh_distance.hip) has no counterpart in the reference: the exact nearest triangle per query
point on the same structure, for the geometric evaluation of evaluation.py.  Neither has point_views (csrc/mesh_visibility.hip;
DESIGN.md 4.19): which cameras see which points, the mesh occluding -- what meshing.cull_unseen drops unseen surface by.
trace and render_views (csrc/mesh_render.hip) keep first_hit's hit record -- which face, where on it -- and render the
mesh with its vertex normals and colours through a set of cameras in one launch: what evaluation.render_mesh / compare_renders score.
project_colors (csrc/mesh_colors.hip) goes the other way: points projected into posed images, the cameras that see them
sampled and blended -- vertex colours for any mesh (meshing.color_from_views, TileSetRenderer.color_mesh).
There is no CPU path: CPU tensors raise.
"""
import torch

from . import formats
from ._capi import check, dev_ptr, lib, stream
from .cuda import background_sampling_cuda, ray_aabb_intersection

_f32, _i32, _i64 = torch.float32, torch.int32, torch.int64

CHUNK = 1 << 20            # rays per launch of the composite methods: their temporaries stay at a few MB for any frame size
PREGATHER_MAX_BYTES = 256 << 20   # pre-gathered triangles (36 B per face-list entry) are kept up to this size


def _require_gpu(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"scanerf: {name} must live on the GPU (no CPU path exists); got "
                           f"{t.device if isinstance(t, torch.Tensor) else type(t).__name__}")


class FastMesh:
    """FastMesh(path): read a PLY mesh and build the tracer on the current GPU (or `device`)."""

    def __init__(self, path, device=None, log2dim=6, pregather=None):
        vertices, faces = formats.read_ply(path)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._build(torch.from_numpy(vertices).to(device), torch.from_numpy(faces).to(device), log2dim, pregather)

    @classmethod
    def from_arrays(cls, vertices, faces, device, log2dim=6, pregather=None):
        """vertices [V,3] float32, faces [F,3] int32 (numpy arrays or tensors) -> FastMesh on `device`.
        pregather: keep (A, B - A, C - A) per face-list entry for first_hit (36 B per entry); None = when they fit in
        PREGATHER_MAX_BYTES; False = the indexed form (12 B per face and per vertex)."""
        self = cls.__new__(cls)
        self._build(torch.as_tensor(vertices).to(device), torch.as_tensor(faces).to(device), log2dim, pregather)
        return self

    # ---- structure ------------------------------------------------------------------------------------------------------------
    def _build(self, vertices, faces, log2dim, pregather):
        _require_gpu(vertices, "vertices")
        _require_gpu(faces, "faces")
        if not 4 <= int(log2dim) <= 7:
            raise ValueError(f"scanerf: FastMesh log2dim must be 4..7, got {log2dim}")
        v = vertices.to(_f32).reshape(-1, 3).contiguous()
        f = faces.to(_i32).reshape(-1, 3).contiguous()
        if v.shape[0] == 0 or f.shape[0] == 0:
            raise ValueError("scanerf: FastMesh needs a mesh with vertices and faces")
        dev, L = v.device, int(log2dim)
        side = 1 << L
        mn, mx = v.amin(0), v.amax(0)
        cell = (mx - mn).amax() / side
        self.device, self.log2dim = dev, L
        self.vertices, self.faces = v, f
        self.scene_info = torch.cat([mn, cell[None]]).contiguous()      # (min_corner, cell): what the kernels read
        self.scene_bound = torch.cat([mn, mx]).contiguous()             # getSceneBound(): min and max corner of the vertices
        V, F = v.shape[0], f.shape[0]
        l = lib()
        counts = torch.empty(F, dtype=_i32, device=dev)
        check(l.scanerf_mesh_count_cells(dev_ptr(v, _f32, "vertices"), dev_ptr(f, _i32, "faces"), V, F, L,
                                         dev_ptr(self.scene_info, _f32, "scene_info"), dev_ptr(counts, _i32, "counts"), stream()),
              "mesh_count_cells")
        ends = torch.cumsum(counts, 0, dtype=_i64)
        total = int(ends[-1])
        if total <= 0:
            raise ValueError("scanerf: FastMesh: no face lies inside the vertex bounds (degenerate mesh or bad indices)")
        if total >= 1 << 31:
            raise ValueError(f"scanerf: FastMesh: {total} (face, cell) pairs do not fit 31 bits; use a smaller log2dim")
        offsets = (ends - counts).contiguous()
        keys = torch.empty(total, dtype=_i64, device=dev)
        check(l.scanerf_mesh_emit_keys(dev_ptr(v, _f32, "vertices"), dev_ptr(f, _i32, "faces"), V, F, L,
                                       dev_ptr(self.scene_info, _f32, "scene_info"), dev_ptr(offsets, _i64, "offsets"),
                                       dev_ptr(keys, _i64, "keys"), total, stream()), "mesh_emit_keys")
        keys = torch.sort(keys)[0]            # distinct keys: the order does not depend on the sort's stability
        cells = keys >> 32
        self.cell_faces = (keys & 0xFFFFFFFF).to(_i32).contiguous()
        occupied, per_cell = torch.unique_consecutive(cells, return_counts=True)
        starts = torch.cumsum(per_cell, 0) - per_cell
        self.start_num = torch.stack([starts, per_cell], 1).to(_i32).contiguous()
        n_words = (side ** 3) // 64
        word, bit = occupied >> 6, occupied & 63
        # distinct bits of one word add up to their OR; integer adds are exact in any order
        self.bitmask = torch.zeros(n_words, dtype=_i64, device=dev).index_add_(0, word, torch.ones_like(bit) << bit)
        per_word = torch.zeros(n_words, dtype=_i64, device=dev).index_add_(0, word, torch.ones_like(bit))
        self.rank = (torch.cumsum(per_word, 0) - per_word).to(_i32).contiguous()
        self.num_cells = int(occupied.shape[0])
        self.cell_box = torch.empty(self.num_cells, 6, dtype=_f32, device=dev)
        check(l.scanerf_mesh_cell_boxes(dev_ptr(v, _f32, "vertices"), dev_ptr(f, _i32, "faces"),
                                        dev_ptr(self.start_num, _i32, "start_num"), dev_ptr(self.cell_faces, _i32, "cell_faces"),
                                        self.num_cells, dev_ptr(self.cell_box, _f32, "cell_box"), stream()), "mesh_cell_boxes")
        self.tris = None
        if pregather is None:
            pregather = total * 36 <= PREGATHER_MAX_BYTES
        if pregather:
            self.tris = torch.empty(total, 9, dtype=_f32, device=dev)
            check(l.scanerf_mesh_gather_triangles(dev_ptr(v, _f32, "vertices"), dev_ptr(f, _i32, "faces"),
                                                  dev_ptr(self.cell_faces, _i32, "cell_faces"), total,
                                                  dev_ptr(self.tris, _f32, "tris"), stream()), "mesh_gather_triangles")
        self.lds = False          # stage bitmask + rank into the LDS (log2dim <= 6): measured slower on frames (DESIGN.md 4.10 of the
                                  # current document); the switch stays for measurement
        self.bbox_center = self.bbox_size = None

    def set(self, bbox_center, bbox_size):
        """The tile box render_mask / compute_bgdepth* test against (tile.py: fmesh.set(center, size); full side lengths)."""
        self.bbox_center = torch.as_tensor(bbox_center, dtype=_f32).to(self.device).contiguous()
        self.bbox_size = torch.as_tensor(bbox_size, dtype=_f32).to(self.device).contiguous()

    def get_sceneinfo(self):
        """getSceneBound(): [6] = min corner, max corner of the vertices."""
        return self.scene_bound

    # ---- the two traces -----------------------------------------------------------------------------------------------------
    def _rays(self, rays_o, rays_d):
        _require_gpu(rays_o, "rays_o")
        _require_gpu(rays_d, "rays_d")
        o, d = rays_o.detach().to(_f32).contiguous(), rays_d.detach().to(_f32).contiguous()
        if o.dim() != 2 or o.shape[1] != 3 or o.shape != d.shape:
            raise RuntimeError(f"scanerf: rays must be [B,3], got {tuple(o.shape)} and {tuple(d.shape)}")
        return o, d

    def first_hit(self, rays_o, rays_d, out=None):
        """[B] distance (in units of |rays_d|) to the nearest triangle along each ray, two-sided, t > 0; 0 where none."""
        o, d = self._rays(rays_o, rays_d)
        B = o.shape[0]
        if out is None:
            out = torch.empty(B, dtype=_f32, device=o.device)
        pre = self.tris is not None
        check(lib().scanerf_mesh_first_hit(
            dev_ptr(o, _f32, "rays_o"), dev_ptr(d, _f32, "rays_d"), B, dev_ptr(self.vertices, _f32, "vertices"),
            dev_ptr(self.faces, _i32, "faces"), dev_ptr(self.tris, _f32, "tris") if pre else None,
            dev_ptr(self.bitmask, _i64, "bitmask"), dev_ptr(self.rank, _i32, "rank"), dev_ptr(self.start_num, _i32, "start_num"),
            dev_ptr(self.cell_faces, _i32, "cell_faces"), dev_ptr(self.scene_info, _f32, "scene_info"), self.log2dim,
            int(self.lds), dev_ptr(out, _f32, "out"), stream()), "mesh_first_hit")
        return out

    def first_enter(self, rays_o, rays_d, out=None):
        """[B] the reference's conservative occluder distance: entry of the ray into the box of the first occupied cell (in ray
        order) whose box it hits.  The entry is clamped at 0, so a ray that STARTS inside that box returns 0.0 = "nothing",
        exactly as a ray that meets no cell: render_mask relies on depth == 0 meaning visible (fastMesh_kernel.cu:181-191)."""
        o, d = self._rays(rays_o, rays_d)
        B = o.shape[0]
        if out is None:
            out = torch.empty(B, dtype=_f32, device=o.device)
        check(lib().scanerf_mesh_first_enter(
            dev_ptr(o, _f32, "rays_o"), dev_ptr(d, _f32, "rays_d"), B, dev_ptr(self.bitmask, _i64, "bitmask"),
            dev_ptr(self.rank, _i32, "rank"), dev_ptr(self.start_num, _i32, "start_num"), dev_ptr(self.cell_box, _f32, "cell_box"),
            dev_ptr(self.scene_info, _f32, "scene_info"), self.log2dim, int(self.lds), dev_ptr(out, _f32, "out"), stream()),
              "mesh_first_enter")
        return out

    # ---- closest point (csrc/mesh_distance.hip) ------------------------------------------------------------------
    @torch.no_grad()
    def closest_point(self, points, max_dist=float("inf"), route="grid", want_closest=True):
        """points [N,3] float32 on the GPU -> (dist [N] f32, face [N] i32, closest [N,3] f32 or None): the exact distance to the
        nearest live triangle, the lowest face index that attains it, and the closest point on that face (include/scanerf_hip.h is
        the definition).  Where nothing lies within max_dist (or the point is not finite): dist = +inf, face = -1, closest = the
        point.  route: "grid" (shells of the tracer's grid) or "brute" (every face; the witness, same bits)."""
        if route not in ("grid", "brute"):
            raise ValueError(f"scanerf: closest_point route must be 'grid' or 'brute', got {route!r}")
        max_dist = float(max_dist)
        if not max_dist >= 0.0:
            raise ValueError(f"scanerf: closest_point max_dist must be >= 0 (inf for no cut), got {max_dist}")
        if isinstance(points, torch.Tensor) and (points.dtype != _f32 or points.dim() != 2 or points.shape[1] != 3):
            raise RuntimeError(f"scanerf: points must be [N,3] float32, got {tuple(points.shape)} {points.dtype}")
        _require_gpu(points, "points")
        p = points.detach().contiguous()
        N = p.shape[0]
        dist2 = torch.empty(N, dtype=_f32, device=p.device)
        face = torch.empty(N, dtype=_i32, device=p.device)
        closest = torch.empty(N, 3, dtype=_f32, device=p.device) if want_closest else None
        out = (dev_ptr(dist2, _f32, "dist2"), dev_ptr(face, _i32, "face"), dev_ptr(closest, _f32, "closest", allow_none=True))
        if route == "grid":
            check(lib().scanerf_mesh_closest_point(
                dev_ptr(p, _f32, "points"), N, dev_ptr(self.vertices, _f32, "vertices"), dev_ptr(self.faces, _i32, "faces"),
                dev_ptr(self.tris, _f32, "tris", allow_none=True), dev_ptr(self.bitmask, _i64, "bitmask"),
                dev_ptr(self.rank, _i32, "rank"), dev_ptr(self.start_num, _i32, "start_num"),
                dev_ptr(self.cell_faces, _i32, "cell_faces"), dev_ptr(self.cell_box, _f32, "cell_box"),
                dev_ptr(self.scene_info, _f32, "scene_info"), self.log2dim, max_dist, *out, stream()), "mesh_closest_point")
        else:
            check(lib().scanerf_mesh_closest_point_brute(
                dev_ptr(p, _f32, "points"), N, dev_ptr(self.vertices, _f32, "vertices"), dev_ptr(self.faces, _i32, "faces"),
                self.vertices.shape[0], self.faces.shape[0], dev_ptr(self.scene_info, _f32, "scene_info"), self.log2dim, max_dist,
                *out, stream()), "mesh_closest_point_brute")
        return torch.sqrt(dist2), face, closest

    # ---- which cameras see which points (csrc/mesh_visibility.hip) ----------------------------------------------
    @torch.no_grad()
    def point_views(self, points, ks, c2ws, H, W, bias, near=0.0, far=float("inf"), want_mask=False, route="fused"):
        """points [N,3] float32 on the GPU, cameras ks [C,3,3] / c2ws [C,3,4] (arrays or tensors, moved to the points' device), the
        image size -> (views [N] i32: the number of cameras that see each point, mask [N, ceil(C/32)] i32 or None: bit c & 31 of word
        c >> 5 is "camera c sees the point").  Seen = inside the image, nearer than `far`, beyond `near` along the optical axis, and
        the segment from the point (moved `bias` towards the eye) to the eye meets no face; include/scanerf_mesh_tools_hip.h is the
        definition.  route="fused": one launch for all pairs; route="composed": the witness, per camera the same operands as separate
        torch elementwise ops, first_hit on the pairs in view, 0 < h < 1 (same bits where torch's division and square root are
        correctly rounded)."""
        if route not in ("fused", "composed"):
            raise ValueError(f"scanerf: point_views route must be 'fused' or 'composed', got {route!r}")
        bias, near, far = float(bias), float(near), float(far)
        if not (0.0 < bias < float("inf")):
            raise ValueError(f"scanerf: point_views bias must be > 0 and finite, got {bias}")
        if not near >= 0.0:
            raise ValueError(f"scanerf: point_views near must be >= 0, got {near}")
        if not far > 0.0:
            raise ValueError(f"scanerf: point_views far must be > 0 (inf for no limit), got {far}")
        for name, v in (("H", H), ("W", W)):
            if isinstance(v, bool) or int(v) != v or v < 1:
                raise ValueError(f"scanerf: point_views {name} must be a positive integer, got {v!r}")
        H, W = int(H), int(W)
        if isinstance(points, torch.Tensor) and (points.dtype != _f32 or points.dim() != 2 or points.shape[1] != 3):
            raise RuntimeError(f"scanerf: points must be [N,3] float32, got {tuple(points.shape)} {points.dtype}")
        _require_gpu(points, "points")
        from .allocation import _cameras
        p = points.detach().contiguous()
        k9, c12 = _cameras(ks, c2ws, p.device)
        N, C = p.shape[0], k9.shape[0]
        nw = (C + 31) // 32
        if route == "composed":
            return self._point_views_composed(p, k9, c12, H, W, bias, near, far, want_mask)
        views = torch.empty(N, dtype=_i32, device=p.device)
        mask = torch.empty((N, nw), dtype=_i32, device=p.device) if want_mask else None
        if N == 0:
            return views, mask
        from ._capi import tool
        check(tool("scanerf_mesh_point_views")(
            dev_ptr(p, _f32, "points"), N, dev_ptr(k9, _f32, "ks"), dev_ptr(c12, _f32, "c2ws"), C, H, W, bias, near, far,
            dev_ptr(self.vertices, _f32, "vertices"), dev_ptr(self.faces, _i32, "faces"),
            dev_ptr(self.tris, _f32, "tris", allow_none=True), dev_ptr(self.bitmask, _i64, "bitmask"),
            dev_ptr(self.rank, _i32, "rank"), dev_ptr(self.start_num, _i32, "start_num"),
            dev_ptr(self.cell_faces, _i32, "cell_faces"), dev_ptr(self.scene_info, _f32, "scene_info"), self.log2dim,
            dev_ptr(views, _i32, "views"), dev_ptr(mask, _i32, "mask", allow_none=True), stream()), "mesh_point_views")
        return views, mask

    def _seen_composed(self, p, finite, K, T, bias, near, far, Hf, Wf):
        """One camera of the composed routes: the definition's operands as separate torch elementwise ops, first_hit on the pairs in
        view -> (indices of the points the camera sees, w [N,3], len [N], px [N], py [N])."""
        E = torch.stack([T[3], T[7], T[11]])
        w = p - E
        w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
        xc = (w0 * T[0] + w1 * T[4]) + w2 * T[8]
        yc = (w0 * T[1] + w1 * T[5]) + w2 * T[9]
        zc = (w0 * T[2] + w1 * T[6]) + w2 * T[10]
        length = torch.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
        px = K[0] * (xc / zc) + K[2]
        py = K[4] * (yc / zc) + K[5]
        inview = finite & (zc > near) & (length <= far) & (length > bias) & (px >= 0) & (px < Wf) & (py >= 0) & (py < Hf)
        idx = torch.nonzero(inview).reshape(-1)
        if idx.shape[0] == 0:
            return idx, w, length, px, py
        pi, wi = p[idx], w[idx]
        s = bias / length[idx]
        P = pi - s[:, None] * wi
        d = E - P
        h = self.first_hit(P.contiguous(), d.contiguous())
        return idx[~((h > 0) & (h < 1))], w, length, px, py

    def _point_views_composed(self, p, k9, c12, H, W, bias, near, far, want_mask):
        dev = p.device
        N, C = p.shape[0], k9.shape[0]
        scalar = lambda v: torch.tensor(v, dtype=_f32, device=dev)
        bias, near, far, Hf, Wf = scalar(bias), scalar(near), scalar(far), scalar(float(H)), scalar(float(W))
        finite = torch.isfinite(p).all(1)
        views = torch.zeros(N, dtype=_i32, device=dev)
        words = torch.zeros((N, (C + 31) // 32), dtype=_i64, device=dev)
        for c in range(C):
            seen = self._seen_composed(p, finite, k9[c], c12[c], bias, near, far, Hf, Wf)[0]
            views[seen] += 1
            words[seen, c >> 5] |= 1 << (c & 31)
        return views, (words.to(_i32) if want_mask else None)

    # ---- colours from posed images (csrc/mesh_colors.hip) ----------------------------------------------------------
    @torch.no_grad()
    def project_colors(self, points, images, ks, c2ws, bias, normals=None, near=0.0, far=float("inf"), min_cos=0.0, acc=None,
                       count=None, route="fused"):
        """points [N,3] float32 on the GPU, images [C,H,W,3] float32 on the same device, cameras ks [C,3,3] / c2ws [C,3,4] (arrays or
        tensors, moved to the points' device) -> (acc [N,4] f32 = the sums (R, G, B, Wt), count [N] i32 = the cameras that
        contributed).  Every camera that sees a point (point_views' rule, this mesh occluding) is sampled bilinearly where the point
        projects and added with the weight cos(normal, direction to the eye) when `normals` [N,3] are given (only cosines above
        min_cos count), else 1; a sample with a non-finite tap is left out.  include/scanerf_mesh_tools_hip.h is the definition.
        acc / count: the sums of earlier batches of cameras, continued IN PLACE (both or neither; None: zeros); consecutive batches
        give the bits of one call.  route="fused": one launch; route="composed": the witness, per camera _point_views_composed's seen
        rule, then the sample and the blend as one eager float32 torch op per operation in the same order (the same bits)."""
        if route not in ("fused", "composed"):
            raise ValueError(f"scanerf: project_colors route must be 'fused' or 'composed', got {route!r}")
        bias, near, far, min_cos = float(bias), float(near), float(far), float(min_cos)
        if not (0.0 < bias < float("inf")):
            raise ValueError(f"scanerf: project_colors bias must be > 0 and finite, got {bias}")
        if not near >= 0.0:
            raise ValueError(f"scanerf: project_colors near must be >= 0, got {near}")
        if not far > 0.0:
            raise ValueError(f"scanerf: project_colors far must be > 0 (inf for no limit), got {far}")
        if not 0.0 <= min_cos < 1.0:
            raise ValueError(f"scanerf: project_colors min_cos must lie in [0, 1), got {min_cos}")
        if (acc is None) != (count is None):
            raise ValueError("scanerf: project_colors continues acc and count together: pass both or neither")
        p = self._strict(points, "points", (None, 3))
        N = p.shape[0]
        img = self._strict(images, "images", (None, None, None, 3))
        C, H, W = (int(v) for v in img.shape[:3])
        if H < 1 or W < 1:
            raise ValueError(f"scanerf: project_colors images must have at least one pixel, got {H} x {W}")
        nrm = None if normals is None else self._strict(normals, "normals", (N, 3))
        if acc is not None:
            acc = self._strict(acc, "acc", (N, 4))
            count = self._strict(count, "count", (N,), _i32)
        for name, t in (("points", p), ("images", img), ("normals", nrm), ("acc", acc), ("count", count)):
            if t is not None:
                _require_gpu(t, name)
        from .allocation import _cameras
        k9, c12 = _cameras(ks, c2ws, p.device)
        if k9.shape[0] != C:
            raise ValueError(f"scanerf: project_colors got {C} images and {k9.shape[0]} cameras")
        if acc is None:
            acc = torch.zeros(N, 4, dtype=_f32, device=p.device)
            count = torch.zeros(N, dtype=_i32, device=p.device)
        if N == 0 or C == 0:
            return acc, count
        if route == "composed":
            return self._project_colors_composed(p, nrm, img, k9, c12, bias, near, far, min_cos, acc, count)
        from ._capi import tool
        check(tool("scanerf_mesh_project_colors")(
            dev_ptr(p, _f32, "points"), dev_ptr(nrm, _f32, "normals", allow_none=True), N, dev_ptr(img, _f32, "images"),
            dev_ptr(k9, _f32, "ks"), dev_ptr(c12, _f32, "c2ws"), C, H, W, bias, near, far, min_cos, *self._tracer_args(),
            dev_ptr(acc, _f32, "acc"), dev_ptr(count, _i32, "count"), stream()), "mesh_project_colors")
        return acc, count

    def _project_colors_composed(self, p, nrm, img, k9, c12, bias, near, far, min_cos, acc, count):
        dev = p.device
        C, H, W = (int(v) for v in img.shape[:3])
        scalar = lambda v: torch.tensor(v, dtype=_f32, device=dev)
        bias, near, far, Hf, Wf, min_cos = scalar(bias), scalar(near), scalar(far), scalar(float(H)), scalar(float(W)), scalar(min_cos)
        finite = torch.isfinite(p).all(1)
        for c in range(C):
            idx, w, length, px, py = self._seen_composed(p, finite, k9[c], c12[c], bias, near, far, Hf, Wf)
            if idx.shape[0] == 0:
                continue
            if nrm is not None:
                n, wi = nrm[idx], w[idx]
                nl = torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
                q = (n[:, 0] * wi[:, 0] + n[:, 1] * wi[:, 1]) + n[:, 2] * wi[:, 2]
                wt = (-q) / (length[idx] * nl)
                facing = wt > min_cos
                idx, wt = idx[facing], wt[facing]
            else:
                wt = torch.ones(idx.shape[0], dtype=_f32, device=dev)
            u, v = px[idx] - 0.5, py[idx] - 0.5
            x0f, y0f = torch.floor(u), torch.floor(v)
            ax, ay = (u - x0f)[:, None], (v - y0f)[:, None]
            xi, yi = x0f.to(_i64), y0f.to(_i64)
            x0, x1 = xi.clamp(0, W - 1), (xi + 1).clamp(0, W - 1)
            y0, y1 = yi.clamp(0, H - 1), (yi + 1).clamp(0, H - 1)
            I = img[c]
            a, b, cc, d = I[y0, x0], I[y0, x1], I[y1, x0], I[y1, x1]
            ok = torch.isfinite(a).all(1) & torch.isfinite(b).all(1) & torch.isfinite(cc).all(1) & torch.isfinite(d).all(1)
            top = (1.0 - ax) * a + ax * b
            bot = (1.0 - ax) * cc + ax * d
            val = (1.0 - ay) * top + ay * bot
            idx, wt, val = idx[ok], wt[ok], val[ok]
            acc[idx, :3] = acc[idx, :3] + wt[:, None] * val      # (idx holds a point once: no accumulation inside the assignment)
            acc[idx, 3] = acc[idx, 3] + wt
            count[idx] += 1
        return acc, count

    # ---- the hit record and the rendered mesh (csrc/mesh_render.hip) ----------------------------------------------
    def _tracer_args(self):
        """vertices .. log2dim as scanerf_mesh_trace and scanerf_mesh_render_views take them."""
        return (dev_ptr(self.vertices, _f32, "vertices"), dev_ptr(self.faces, _i32, "faces"),
                dev_ptr(self.tris, _f32, "tris", allow_none=True), dev_ptr(self.bitmask, _i64, "bitmask"),
                dev_ptr(self.rank, _i32, "rank"), dev_ptr(self.start_num, _i32, "start_num"),
                dev_ptr(self.cell_faces, _i32, "cell_faces"), dev_ptr(self.scene_info, _f32, "scene_info"), self.log2dim)

    @staticmethod
    def _strict(t, name, tail, dtype=_f32):
        """A contiguous tensor of `dtype` and shape `tail` (None = any length), or an error: nothing is converted.  The device is
        the caller's next check (_require_gpu), after every argument's shape."""
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"scanerf: {name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != dtype or t.dim() != len(tail) or any(w is not None and s != w for s, w in zip(t.shape, tail)):
            want = "[" + ",".join("N" if w is None else str(w) for w in tail) + "]"
            raise RuntimeError(f"scanerf: {name} must be {want} {dtype}, got {tuple(t.shape)} {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"scanerf: {name} must be contiguous")
        return t.detach()

    @torch.no_grad()
    def trace(self, rays_o, rays_d, route="grid"):
        """rays_o, rays_d [B,3] float32 on the GPU -> (t [B] f32, face [B] i32, bary [B,2] f32): first_hit's distance with its bits,
        the lowest index of the faces the walk tested that attains it, and Moeller-Trumbore's (u, v) on that face: the hit point is
        A + u (B - A) + v (C - A).  A miss: t = 0, face = -1, bary = 0.  include/scanerf_mesh_tools_hip.h is the definition.
        route: "grid" (the tracer's walk) or "brute" (every face in order; the witness)."""
        if route not in ("grid", "brute"):
            raise ValueError(f"scanerf: trace route must be 'grid' or 'brute', got {route!r}")
        o = self._strict(rays_o, "rays_o", (None, 3))
        d = self._strict(rays_d, "rays_d", (o.shape[0], 3))
        _require_gpu(o, "rays_o")
        _require_gpu(d, "rays_d")
        B = o.shape[0]
        t = torch.empty(B, dtype=_f32, device=o.device)
        face = torch.empty(B, dtype=_i32, device=o.device)
        bary = torch.empty(B, 2, dtype=_f32, device=o.device)
        if B == 0:
            return t, face, bary
        from ._capi import tool
        out = (dev_ptr(t, _f32, "t"), dev_ptr(face, _i32, "face"), dev_ptr(bary, _f32, "bary"))
        if route == "grid":
            check(tool("scanerf_mesh_trace")(dev_ptr(o, _f32, "rays_o"), dev_ptr(d, _f32, "rays_d"), B, *self._tracer_args(), *out,
                                             stream()), "mesh_trace")
        else:
            check(tool("scanerf_mesh_trace_brute")(
                dev_ptr(o, _f32, "rays_o"), dev_ptr(d, _f32, "rays_d"), B, dev_ptr(self.vertices, _f32, "vertices"),
                dev_ptr(self.faces, _i32, "faces"), self.vertices.shape[0], self.faces.shape[0],
                dev_ptr(self.scene_info, _f32, "scene_info"), self.log2dim, *out, stream()), "mesh_trace_brute")
        return t, face, bary

    @torch.no_grad()
    def render_views(self, ks, c2ws, H, W, normals=None, colors=None, want_normals=False, route="fused"):
        """The mesh seen through cameras ks [C,3,3] / c2ws [C,3,4] (arrays or tensors, moved to the mesh's device) at H x W pixels ->
        {"depth": [C,H,W] f32 z-depth (0 = nothing), "face": [C,H,W] i32 (-1 = nothing)} and, when asked for, "normal" [C,H,W,3] (unit:
        the interpolated `normals` [V,3] when given, else with want_normals=True the face normal as wound) and "color" [C,H,W,3]
        (with `colors` [V,3]: interpolated).  Pixel (px, py)'s ray is compute_ray_forward's; include/scanerf_mesh_tools_hip.h is the
        definition.  route="fused": one launch for all cameras; route="composed": the witness -- compute_ray_forward on a locs grid,
        trace, then the interpolation as one eager float32 torch op per operation (the same bits)."""
        if route not in ("fused", "composed"):
            raise ValueError(f"scanerf: render_views route must be 'fused' or 'composed', got {route!r}")
        if not isinstance(want_normals, bool):
            raise ValueError(f"scanerf: want_normals must be True or False, got {want_normals!r}")
        for name, v in (("H", H), ("W", W)):
            if isinstance(v, bool) or int(v) != v or v < 1:
                raise ValueError(f"scanerf: render_views {name} must be a positive integer, got {v!r}")
        H, W = int(H), int(W)
        V = self.vertices.shape[0]
        vn = None if normals is None else self._strict(normals, "normals", (V, 3))
        vc = None if colors is None else self._strict(colors, "colors", (V, 3))
        want_normals = want_normals or vn is not None
        for name, a in (("normals", vn), ("colors", vc)):
            if a is not None:
                _require_gpu(a, name)
        from .allocation import _cameras
        dev = self.vertices.device
        k9, c12 = _cameras(ks, c2ws, dev)
        C = k9.shape[0]
        if C * H * W >= 1 << 31:
            raise ValueError(f"scanerf: render_views: {C} x {H} x {W} pixels do not fit 31 bits; render fewer views per call")
        if route == "composed":
            return self._render_views_composed(k9, c12, H, W, vn, vc, want_normals)
        out = {"depth": torch.empty(C, H, W, dtype=_f32, device=dev), "face": torch.empty(C, H, W, dtype=_i32, device=dev)}
        if want_normals:
            out["normal"] = torch.empty(C, H, W, 3, dtype=_f32, device=dev)
        if vc is not None:
            out["color"] = torch.empty(C, H, W, 3, dtype=_f32, device=dev)
        if C == 0:
            return out
        from ._capi import tool
        check(tool("scanerf_mesh_render_views")(
            dev_ptr(k9, _f32, "ks"), dev_ptr(c12, _f32, "c2ws"), C, H, W, *self._tracer_args(),
            dev_ptr(vn, _f32, "normals", allow_none=True), dev_ptr(vc, _f32, "colors", allow_none=True),
            dev_ptr(out["depth"], _f32, "depth"), dev_ptr(out["face"], _i32, "face"),
            dev_ptr(out.get("normal"), _f32, "normal", allow_none=True), dev_ptr(out.get("color"), _f32, "color", allow_none=True),
            stream()), "mesh_render_views")
        return out

    def _render_views_composed(self, k9, c12, H, W, vn, vc, want_normals):
        from .cuda.lib.CUDA_EXT import compute_ray_forward
        dev = k9.device
        C = k9.shape[0]
        n = C * H * W
        cam = torch.arange(C, device=dev, dtype=_i32)[:, None, None].expand(C, H, W)
        py = torch.arange(H, device=dev, dtype=_i32)[None, :, None].expand(C, H, W)
        px = torch.arange(W, device=dev, dtype=_i32)[None, None, :].expand(C, H, W)
        locs = torch.stack([cam, px, py], -1).reshape(-1, 3).contiguous()
        o = torch.empty(n, 3, dtype=_f32, device=dev)
        d = torch.empty(n, 3, dtype=_f32, device=dev)
        if n:
            compute_ray_forward(o, d, k9, c12, locs)
        t, face, bary = self.trace(o, d)
        out = {"depth": t.reshape(C, H, W), "face": face.reshape(C, H, W)}
        if not want_normals and vc is None:
            return out
        hit = face >= 0
        idx = self.faces[face.clamp(min=0).to(_i64)].to(_i64)            # [n,3]; row 0 stands in for a miss and is masked below
        ia, ib, ic = idx[:, 0], idx[:, 1], idx[:, 2]
        u, v = bary[:, 0:1], bary[:, 1:2]
        w0 = (1.0 - u) - v
        interp = lambda a: (w0 * a[ia] + u * a[ib]) + v * a[ic]
        zero = torch.zeros((), dtype=_f32, device=dev)
        if want_normals:
            if vn is not None:
                nrm = interp(vn)
            else:
                A = self.vertices[ia]
                e1, e2 = self.vertices[ib] - A, self.vertices[ic] - A
                nrm = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            sq = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
            length = torch.sqrt(sq) + 1e-8
            out["normal"] = torch.where(hit[:, None], nrm / length[:, None], zero).reshape(C, H, W, 3)
        if vc is not None:
            out["color"] = torch.where(hit[:, None], interp(vc), zero).reshape(C, H, W, 3)
        return out

    # ---- the reference's methods --------------------------------------------------------------------------------------------
    def _box(self):
        if self.bbox_center is None:
            raise RuntimeError("scanerf: FastMesh.set(bbox_center, bbox_size) first")
        return self.bbox_center, self.bbox_size

    def _bounds(self, o, d):
        center, size = self._box()
        bounds = torch.full((o.shape[0], 2), -1.0, dtype=_f32, device=o.device)
        ray_aabb_intersection(o, d, center, size, bounds)
        return bounds

    @torch.no_grad()
    def render_depth(self, rays_o, rays_d):
        """[B,1] first_hit depth."""
        return self.first_hit(rays_o, rays_d)[:, None]

    @torch.no_grad()
    def render_mask(self, rays_o, rays_d, trust_mesh=False):
        """[B,1] bool, True = the tile box is visible along the ray: the occluder (first_enter, or first_hit with trust_mesh)
        lies beyond the ray's entry into the box, or there is none (depth == 0), or the origin is inside the box."""
        o, d = self._rays(rays_o, rays_d)
        center, size = self._box()
        mask = torch.empty(o.shape[0], 1, dtype=torch.bool, device=o.device)
        for i in range(0, o.shape[0], CHUNK):
            oc, dc = o[i:i + CHUNK], d[i:i + CHUNK]
            depth = (self.first_hit if trust_mesh else self.first_enter)(oc, dc)[:, None]
            near = self._bounds(oc, dc)[:, :1]
            inside = torch.all(torch.abs(oc - center) < (size / 2.0), dim=-1, keepdim=True)
            mask[i:i + CHUNK] = ((depth > near) & (near != -1)) | (depth == 0) | inside
        return mask

    def _bgdepth(self, o, d):
        """-> exit bounds [b,2], valid = the ray meets the box, first_hit from the box exit [b,1]."""
        bounds = self._bounds(o, d)
        valid = bounds[:, 1] != -1
        start = torch.where(valid[:, None], o + bounds[:, 1:] * d, o)
        return bounds, valid, self.first_hit(start, d)[:, None]

    @torch.no_grad()
    def compute_bgdepth_batch(self, rays_o, rays_d):
        """-> bg_z [B,1], has_bg [B], bounds [B,2]: the first mesh hit BEHIND the tile box, measured from the ray origin
        (box exit distance + first_hit from the exit point); 1000 + exit for rays whose own first_hit finds nothing ("no
        background").  Unlike the reference (which moves the caller's rays_o to the exit points in place and is therefore
        called on a clone, fastMesh/__init__.py:64,80) the inputs are left alone."""
        o, d = self._rays(rays_o, rays_d)
        B = o.shape[0]
        bg_z = torch.empty(B, 1, dtype=_f32, device=o.device)
        has_bg = torch.empty(B, dtype=torch.bool, device=o.device)
        bounds = torch.empty(B, 2, dtype=_f32, device=o.device)
        for i in range(0, B, CHUNK):
            oc, dc = o[i:i + CHUNK], d[i:i + CHUNK]
            depth_z = self.first_hit(oc, dc)[:, None]
            b, valid, z = self._bgdepth(oc, dc)
            z = torch.where(depth_z == 0, torch.full_like(z, 1000.0), z)
            has_bg[i:i + CHUNK] = (z[:, 0] > 0) & valid
            bg_z[i:i + CHUNK] = torch.where(valid[:, None], z + b[:, 1:], z)
            bounds[i:i + CHUNK] = b
        return bg_z, has_bg, bounds

    @torch.no_grad()
    def background_sampling(self, rays_o, rays_d, num_sample, sample_range):
        """-> z_vals [B,num_sample], valid [B]: background_sampling_cuda between the box exit and the background depth."""
        o, d = self._rays(rays_o, rays_d)
        bg_z, valid, bounds = self.compute_bgdepth_batch(o, d)
        z_vals = torch.full((o.shape[0], num_sample), -1.0, dtype=_f32, device=o.device)
        background_sampling_cuda(o, d, bounds[:, 1:].contiguous(), bg_z, z_vals, num_sample, float(sample_range))
        return z_vals, valid

    @torch.no_grad()
    def compute_bgdepth(self, poses, H, W):
        """poses: cameras.CameraSet -> [N_cam,H,W] background depth per pixel (0 = no background), one camera at a time."""
        dev = poses.device
        n = poses.num_camera
        out = torch.zeros(n, H, W, dtype=_f32, device=dev)
        px = torch.arange(W, device=dev, dtype=_i32)[None, :].expand(H, W)
        py = torch.arange(H, device=dev, dtype=_i32)[:, None].expand(H, W)
        for idx in range(n):
            locs = torch.stack([torch.full_like(px, idx), px, py], -1).reshape(-1, 3).contiguous()
            o, d = poses.get_rays(locs)
            o, d = self._rays(o, d)
            for i in range(0, H * W, CHUNK):
                b, valid, z = self._bgdepth(o[i:i + CHUNK], d[i:i + CHUNK])
                no_bg = z <= 0
                z = torch.where(valid[:, None], z + b[:, 1:], z)
                out[idx].view(-1)[i:i + CHUNK] = torch.where(no_bg, torch.zeros_like(z), z)[:, 0]
        return out

    def sample_points(self, rays_o, rays_d, start, num_sample):
        """fastMesh_kernel.cu:23-122 has no live caller in the reference (its only user, background_sampling_v2, is commented
        out, fastMesh/__init__.py:88-94); the surface exists, the op does not."""
        raise NotImplementedError("FastMesh.sample_points is dead code in the reference (no caller); use background_sampling")


class fastMesh:
    """The reference's pybind class (fastMesh/binding.cpp:7-20: build, fisrtHit [sic], firstEnter, getSceneBound, sample_points)
    on FastMesh, for a checkout that keeps its own fastMesh/__init__.py: `from scanerf_amd.fastmesh import fastMesh` in place of
    `from .lib.fastMesh import fastMesh`.  depth [B,1] float32 is written in place, as the reference's kernels do."""

    def __init__(self):
        self.mesh = None

    def build(self, path):
        self.mesh = FastMesh(path)

    def _depth(self, depth, B):
        if not isinstance(depth, torch.Tensor) or depth.numel() != B:
            raise RuntimeError(f"scanerf: depth must be a [B,1] float32 tensor with B={B}")
        dev_ptr(depth, _f32, "depth")
        return depth.view(-1)

    def fisrtHit(self, rays_o, rays_d, depth):
        self.mesh.first_hit(rays_o, rays_d, out=self._depth(depth, rays_o.shape[0]))

    def firstEnter(self, rays_o, rays_d, depth):
        self.mesh.first_enter(rays_o, rays_d, out=self._depth(depth, rays_o.shape[0]))

    def getSceneBound(self):
        return self.mesh.get_sceneinfo()

    def sample_points(self, rays_o, rays_d, start, z_vals):
        self.mesh.sample_points(rays_o, rays_d, start, z_vals.shape[-1])
