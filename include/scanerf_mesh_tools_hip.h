/*
 * scanerf_mesh_tools_hip.h -- the second public header of libscanerf_hip.so: post-processing ops on extracted meshes that came after
 * ABI version 10 was pinned.  The same library and the same conventions as scanerf_hip.h (int status, scanerf_last_error(), device
 * pointers, contiguous row-major arrays, the stream last, no allocation, no state, no environment variable); scanerf_stream_t is
 * the first header's.  The entries live here, and not in scanerf_hip.h, because that header's set of declarations is pinned by the
 * ABI version and by the stream-contract registry (tests/test_capi_cpu.py, tests/stream_cases.py); an op added here leaves both as
 * they are and brings its own checks (tests/test_mesh_visibility_cpu.py, tests/test_gpu_mesh_visibility.py).  The Python side
 * types these entries from _capi.TOOL_PROTOTYPES and calls them through _capi.tool(name).
 */
#ifndef SCANERF_MESH_TOOLS_HIP_H_
#define SCANERF_MESH_TOOLS_HIP_H_

#include "scanerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- point visibility from a set of cameras (csrc/mesh_visibility.hip): for every point and every camera, is the
 *   point inside the camera's image and is the segment between them free of the mesh?  What "cull the parts of an extracted mesh
 *   that no training camera saw" needs.  The reference has no counterpart; the definition is this comment.
 *   Inputs: points [N,3] f32 (any points, typically a mesh's vertices); Ks [C,9], C2Ws [C,12] f32 row-major, as scanerf_view_coverage
 *     takes them; the image size H, W; bias > 0 and finite; near >= 0; far > 0 (+inf allowed); the tracer's arrays exactly as
 *     scanerf_mesh_first_hit takes them (tris != NULL: pre-gathered triangles, else vertices / faces / cell_faces); log2dim 4..7.
 *   Everything below is float32, operation by operation, without FMA contraction.  For point p and camera c:
 *     fx = K[0], cx = K[2], fy = K[4], cy = K[5] (skew is ignored, as scanerf_compute_ray_forward ignores it); column k of R is
 *     (C2W[k], C2W[4 + k], C2W[8 + k]); the eye is E = (C2W[3], C2W[7], C2W[11]).
 *     w = p - E;  xc = (w0 R00 + w1 R10) + w2 R20, yc and zc likewise with columns 1 and 2;  len = sqrtf((w0 w0 + w1 w1) + w2 w2).
 *   IN VIEW iff p is finite and zc > near and len <= far and len > bias and 0 <= fx (xc / zc) + cx < (float)W and
 *     0 <= fy (yc / zc) + cy < (float)H.  Pixel px covers [px, px + 1): the +0.5 convention of scanerf_compute_ray_forward.
 *   SEGMENT: s = bias / len, P = p - s w, d = E - P: it starts `bias` towards the eye, so that the point's own faces do not hide it.
 *   HIDDEN iff the first-hit walk of scanerf_mesh_first_hit on the ray (P, d) would return h with 0 < h < 1.  The kernel does not
 *     finish that walk: it stops at the first triangle with 0 < t < 1, and after the first cell whose exit t1 >= 1; it uses the same
 *     grid walk, the same ray / triangle test (two-sided, edges inclusive, |det| <= 1e-12 is a dead face that hides nothing) and the
 *     same operands (A, B - A, C - A).  An occluder behind the eye does not count.
 *   SEEN = in view and not hidden.
 *   Outputs: views [N] i32 = the number of cameras that see the point (every element written; 0 for a non-finite point);
 *     mask [N, ceil(C / 32)] u32 (may be NULL: not written): bit c & 31 of word c >> 5 is seen(p, c), the unused high bits are 0.
 *   Integer outputs only, every element written exactly once by a plain store, nothing else written: two launches give equal bits,
 *     both triangle forms give equal bits, every log2dim gives equal bits.
 *   N == 0 launches nothing.  C == 0 writes zeros to views (mask has no columns; the camera and tracer arrays are not read).
 *   Refused before any launch (nothing written): N < 0 or C < 0, null pointers (but tris, mask), H or W < 1, log2dim outside 4..7,
 *     bias not in (0, inf), near negative or NaN, far not > 0.  No allocation, no host synchronisation; every launch on `stream`.
 *   scanerf_mesh_point_views_cameras_per_pass: the cameras a wavefront takes per pass over its 64 points (its on-chip mask words); a
 *     larger C takes several passes.
 *   scanerf_mesh_point_views_counted (measurement): also adds to counters [3] u64, which the caller zeroes: the pairs in view (the
 *     segments walked), the occupied cells looked at, the ray / triangle tests. */
int scanerf_mesh_point_views_cameras_per_pass(void);
int scanerf_mesh_point_views(const float *points, int N, const float *Ks, const float *C2Ws, int C, int H, int W, float bias,
                             float near, float far, const float *vertices, const int32_t *faces, const float *tris,
                             const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces,
                             const float *scene_info, int log2dim, int32_t *views, uint32_t *mask, scanerf_stream_t stream);
int scanerf_mesh_point_views_counted(const float *points, int N, const float *Ks, const float *C2Ws, int C, int H, int W, float bias,
                                     float near, float far, const float *vertices, const int32_t *faces, const float *tris,
                                     const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                                     const int32_t *cell_faces, const float *scene_info, int log2dim, int32_t *views, uint32_t *mask,
                                     uint64_t *counters, scanerf_stream_t stream);

/* ---- depth-map fusion into a truncated signed distance volume (csrc/tsdf.hip): every lattice point against every
 *   camera's depth map.  What "mesh what the cameras saw, not the density" needs; the zero set is then cut by
 *   scanerf_isosurface_*_dense.  The reference has no counterpart; the definition is this comment.
 *   Inputs: depths [C,H,W] f32, z-depth (what scanerf_compute_ray_forward's rays measure: their camera-z component is 1); Ks [C,9],
 *     C2Ws [C,12] f32 row-major, read as scanerf_mesh_point_views reads them (fx = K[0], cx = K[2], fy = K[4], cy = K[5]; column k of R
 *     is (C2W[k], C2W[4 + k], C2W[8 + k]); E = (C2W[3], C2W[7], C2W[11])); origin[3], spacing[3]: HOST arrays; the lattice has
 *     (nx+1)(ny+1)(nz+1) points, point (i, j, k) at row p = (i (ny+1) + j)(nz+1) + k; trunc in (0, inf); near >= 0; far > near
 *     (+inf allowed); acc [P,2] f32, interleaved (S, Wt), read AND written.
 *   Everything below is float32, operation by operation, without FMA contraction.  Lattice point (i0, i1, i2) has the world position
 *     P_a = origin_a + (float)i_a * spacing_a (two roundings: the dense surface-nets op's vertex placement).
 *   For camera c = 0 .. C-1, IN THIS ORDER:
 *     w = P - E;  xc = (w0 R00 + w1 R10) + w2 R20, yc and zc likewise with columns 1 and 2;
 *     u = fx (xc / zc) + cx,  v = fy (yc / zc) + cy;
 *     IN VIEW iff zc > near and 0 <= u < (float)W and 0 <= v < (float)H;  px = (int)u, py = (int)v (pixel px covers [px, px + 1));
 *     D = depths[c][py][px];  VALID iff D is finite and near < D <= far;  sdf = D - zc;
 *     OBSERVED iff in view and valid and sdf >= -trunc;  term = fminf(1, sdf / trunc);
 *     for an observed pair: S <- S + term, Wt <- Wt + 1.
 *   The sums START FROM THE VALUES IN acc: cameras may be fed in batches, and a split into batches gives the bits of one call.
 *   Each point is owned by one thread; no atomics; acc[p] is read once and written once per call, only for a point some camera
 *     observed (an unobserved point's row is not written: it would receive the bits it holds); nothing else is written.  Whole
 *     (block of points, camera) pairs are skipped when the block's bounding sphere lies behind `near` or outside the frustum by a
 *     margin that covers the float32 rounding of the test above: the skip never changes a bit.
 *   C == 0 launches nothing.  Refused before any launch (nothing written): null pointers, C < 0, H or W < 1, an n_k < 1, 2^31 or more
 *     lattice points, trunc not in (0, inf), near negative or NaN, far not > near, a spacing not positive and finite, an origin not
 *     finite.  No allocation, no host synchronisation; every launch on `stream`.
 *   scanerf_tsdf_cameras_per_pass: the cameras a workgroup stages on chip per pass; a larger C takes several passes.
 *   scanerf_tsdf_integrate_counted (measurement): also adds to counters [3] u64, which the caller zeroes: the (point, camera) pairs
 *     evaluated, the (block, camera) pairs skipped, the updates (observed pairs: the sum of the Wt increments).
 *   scanerf_tsdf_values: for p < P (P >= 0; 0 launches nothing; min_weight >= 1): observed[p] (u8) = Wt >= min_weight;
 *     values[p] = observed ? 0.5f - 0.5f * (S / Wt) : 0.  In [0, 1] for sums this op formed; inside iff > 0.5: the level of the
 *     surface-nets op is 0.5 and its strict `values > level` makes an unobserved point outside.  Every element of both written once.
 *   scanerf_tsdf_cell_support: cells [V,3] i32 (Mesh.cells: cell (a, b, c) has the corners (a + da, b + db, c + dc), d in {0, 1});
 *     support[v] (i32) = the number of its 8 corners with observed != 0; a cell outside [0, n_k) on an axis gets 0 and reads nothing.
 *     V == 0 launches nothing; V < 0, an n_k < 1, 2^31 or more points and null pointers are refused.
 *   COLOUR.  scanerf_tsdf_integrate_color: the above, every word of it, and beside it colors [C,H,W,3] f32 (the
 *     cameras' images, pixel for pixel with depths) and cacc [P,4] f32, interleaved (R, G, B, Wc), read AND written, 16-byte aligned;
 *     row p of cacc is row p of acc.  For camera c, in order, for a pair that is OBSERVED by the rule above:
 *       COLOURED iff sdf <= trunc and the three channels of colors[c][py][px] are finite;
 *       for a coloured pair: R <- R + r, G <- G + g, B <- B + b, Wc <- Wc + 1.
 *     The channels are summed as they are (no clamp).  An observed pair with sdf > trunc is free space in front of whatever the
 *     pixel shows: its colour belongs to a surface further away and is left out.  The sums start from the values in cacc (a batch
 *     split gives the bits of one call); one thread owns the point, no atomics; cacc[p] is loaded once as one 16-byte word and
 *     stored once, only for a point some camera coloured; acc receives exactly the bits scanerf_tsdf_integrate gives it.  A skipped
 *     (block, camera) pair is not in view, so the skip never changes a bit of cacc either.  Refused before any launch as above,
 *     and: a null colors or cacc, a cacc that is not 16-byte aligned.  C == 0 launches nothing.
 *   scanerf_tsdf_integrate_color_counted (measurement): counters [4] u64; the first three as scanerf_tsdf_integrate_counted's, the
 *     fourth the coloured pairs (the sum of the Wc increments).
 *   scanerf_tsdf_vertex_colors: the colour of mesh vertices from cacc.  cells [V,3] i32 (Mesh.cells), lattice [V,3] f32 (Mesh.lattice:
 *     the vertex in lattice units), rgb [V,3] f32 and weight [V] f32 written, every element once.  float32, operation by operation:
 *       t_a = fminf(fmaxf(lattice_a - (float)cell_a, 0), 1);  per axis the corner weights (1 - t_a, t_a);
 *       corner d = 0 .. 7 has the offsets (d >> 2, (d >> 1) & 1, d & 1) (scanerf_tsdf_cell_support's order), the row q_d and the
 *       weight w_d = (wx * wy) * wz;  num_k and den = the sums of w_d * cacc[q_d][k] for k = R, G, B and Wc, accumulated in ascending
 *       d starting from the d = 0 product;  weight[v] = den;  rgb[v][k] = den > 0 ? num_k / den : 0.
 *     Sums and weight are interpolated, then divided: a corner nobody coloured drops out by itself.  A cell outside [0, n_k) on an
 *     axis gets rgb = 0, weight = 0 and reads nothing.  V == 0 launches nothing; V < 0, an n_k < 1, 2^31 or more points, null
 *     pointers and a cacc that is not 16-byte aligned are refused.
 *   NORMALS.  scanerf_tsdf_vertex_normals: the volume's own gradient at mesh vertices.  values [P] f32 and
 *     observed [P] u8: what scanerf_tsdf_values wrote (min_weight is already in observed); spacing[3]: a HOST array; cells [V,3] i32,
 *     lattice [V,3] f32 as scanerf_tsdf_vertex_colors takes them; normal [V,3] f32 and grad [V,3] f32 written, every element once.
 *     float32, operation by operation, without FMA contraction; division and sqrtf correctly rounded.
 *     THE GRADIENT AT A LATTICE POINT q, per axis a with h_a = spacing[a] and e_a the unit step of the axis:
 *       has+ iff q + e_a is inside the lattice and observed;  has- iff q - e_a is inside the lattice and observed;
 *       g_a(q) = (val[q + e_a] - val[q - e_a]) / (h_a + h_a)   with both,
 *                (val[q + e_a] - val[q]) / h_a                 with has+ alone,
 *                (val[q] - val[q - e_a]) / h_a                 with has- alone,
 *                0                                             with neither.
 *     AT A VERTEX: t_a, the corner order and the corner weights w_d = (wx * wy) * wz exactly as scanerf_tsdf_vertex_colors forms them;
 *       G_a = the sum of w_d * g_a(q_d), accumulated in ascending d starting from the d = 0 product, each component by itself;
 *       len = sqrtf((Gx * Gx + Gy * Gy) + Gz * Gz);  normal_a = (-G_a) / (len + 1e-8f);  grad_a = G_a.
 *     Values are higher inside, so -G points out, as the faces of the surface-nets op are wound (the convention of
 *     scanerf_scene_sigma_normals_points).  A zero G gives the normal (-0) / 1e-8f = -0 in every component.
 *     A vertex whose cell lies outside [0, n_k) on an axis, or whose cell has a corner with observed == 0, gets normal = grad = +0:
 *     an out-of-range cell reads nothing, an unobserved corner's value is a placeholder, not a distance.  (Where all 8 corners are
 *     observed every corner has a neighbour inside the cell on every axis, so no evaluated stencil takes the "neither" branch.)
 *     One thread owns one vertex; the 32 distinct lattice points of a cell's stencil (8 corners, 8 more beyond them per axis) are
 *     loaded once each; neither values nor observed is written.  Refused before any launch (nothing written): null pointers, V < 0,
 *     an n_k < 1, 2^31 or more lattice points, a spacing not positive and finite.  V == 0 (with valid pointers) launches nothing.
 *     No allocation, no host synchronisation; the launch goes on `stream`. */
int scanerf_tsdf_cameras_per_pass(void);
int scanerf_tsdf_integrate(const float *depths, const float *Ks, const float *C2Ws, int C, int H, int W, const float *origin,
                           const float *spacing, int nx, int ny, int nz, float trunc, float near, float far, float *acc,
                           scanerf_stream_t stream);
int scanerf_tsdf_integrate_counted(const float *depths, const float *Ks, const float *C2Ws, int C, int H, int W, const float *origin,
                                   const float *spacing, int nx, int ny, int nz, float trunc, float near, float far, float *acc,
                                   uint64_t *counters, scanerf_stream_t stream);
int scanerf_tsdf_values(const float *acc, int P, float min_weight, float *values, uint8_t *observed, scanerf_stream_t stream);
int scanerf_tsdf_cell_support(const uint8_t *observed, int nx, int ny, int nz, const int32_t *cells, int V, int32_t *support,
                              scanerf_stream_t stream);
int scanerf_tsdf_integrate_color(const float *depths, const float *colors, const float *Ks, const float *C2Ws, int C, int H, int W,
                                 const float *origin, const float *spacing, int nx, int ny, int nz, float trunc, float near, float far,
                                 float *acc, float *cacc, scanerf_stream_t stream);
int scanerf_tsdf_integrate_color_counted(const float *depths, const float *colors, const float *Ks, const float *C2Ws, int C, int H,
                                         int W, const float *origin, const float *spacing, int nx, int ny, int nz, float trunc,
                                         float near, float far, float *acc, float *cacc, uint64_t *counters,
                                         scanerf_stream_t stream);
int scanerf_tsdf_vertex_colors(const float *cacc, int nx, int ny, int nz, const int32_t *cells, const float *lattice, int V,
                               float *rgb, float *weight, scanerf_stream_t stream);
int scanerf_tsdf_vertex_normals(const float *values, const uint8_t *observed, int nx, int ny, int nz, const float *spacing,
                                const int32_t *cells, const float *lattice, int V, float *normal, float *grad,
                                scanerf_stream_t stream);

/* ---- mesh simplification by vertex clustering (csrc/mesh_simplify.hip): the vertices that fall into one cell of a
 *   world-aligned grid of cubic cells become one vertex (Rossignac-Borrel).  What "hand out the fused mesh at the resolution the
 *   consumer wants" needs.  The reference has no counterpart; the definition is this comment.
 *   Inputs: vertices [V,3] f32; faces [F,3] i32; normals [V,3] f32 and colors [V,3] f32 (each may be NULL); origin[3]: a HOST array,
 *     finite (the grid is the world's: meshes simplified separately cluster alike); cell = h, finite and > 0.
 *   KEY, per axis a, in float32, one IEEE operation each, without FMA contraction, the division correctly rounded:
 *     u = (v_a - o_a) / h;  k = floorf(u);  f = u - k;  q = (int)(f * 65536).
 *     0 <= f <= 1.  The subtraction is exact except for -1/2 < u < 0 (k = -1, and u carries bits below the result's last place): there
 *     it is one rounding like the others, and a u above -2^-25 gives f = 1, q = 65536.  Nothing below needs exactness or q < 65536.
 *     f * 65536 is an exact scaling.
 *   A vertex is BAD iff a coordinate is not finite, or not |k| < 2^20 on some axis, or one of its normal / colour values is not
 *     finite.  A bad vertex belongs to no cluster and a face with a bad corner counts for nothing; n_bad is their number.
 *   CLUSTERS: the sets of (good) vertices with equal (kx, ky, kz).  A cluster's label is its smallest member index; clusters are
 *     numbered by ascending label, and that number is the output vertex index (the output follows the input's order).
 *   POSITION: n members, S_a = the sum of q_a (an integer), M_a = (2 S_a + n) div (2 n);
 *     out_a = o_a + ((float)k_a + (float)M_a * 2^-16) * h, in float32 in that order.
 *   ATTRIBUTES, per value a: t = rintf(fminf(fmaxf(a, -32767), 32767) * 65536) as an integer; S = the sum of t in int64;
 *     M = floor((2 S + n) / (2 n)) (floor division for negative values too); m = (float)M * 2^-16.
 *     Colours are m.  Normals are m_a / (sqrtf((mx mx + my my) + mz mz) + 1e-8f): zero sums give a zero normal.
 *   A cluster of ONE member copies its vertex, normal and colour bit for bit: a cell below the vertex spacing returns the input.
 *   FACES: each corner goes to its cluster's number; a face with two equal corners is dropped; kept faces stay in order and keep
 *     their winding.  A cluster that ends with no face stays a vertex.  Duplicate faces are kept.
 *   Everything that decides the result is an integer or a single-rounded float32 operation: the output does not depend on thread
 *     order, launch geometry or timing.
 *   scanerf_mesh_simplify_scratch_bytes: *bytes = the scratch both passes need, for 1 <= V <= 2^29 and 0 <= F < 2^31 / 3 (otherwise
 *     refused, *bytes = 0).  With T = the smallest power of two >= max(64, 2 V) (the lookup table's slots: its load is at most 1/2)
 *     and r16(x) = x rounded up to a multiple of 16:
 *     bytes = 64 + 12 T + 2 r16(4 V) + r16(4 (ceil(V / 256) + 1)) + r16(4 (ceil(F / 256) + 1)).
 *   scanerf_mesh_simplify_cluster: the table, labels, numbers and per-vertex rows, the counts of kept faces and their scan, all on
 *     `stream`, no host synchronisation.  Afterwards the scratch starts with int64 (V', F', n_bad): the caller's one host read.
 *     Writes the scratch only.  scratch: 16-byte aligned, scratch_bytes >= the formula.
 *   scanerf_mesh_simplify_emit: the same vertices, faces, normals, colors, V, F, origin, cell and scratch as the cluster call.
 *     sums [V',9] i64 and counts [V'] i32: work arrays the caller allocates after its read; the entry zeroes them (per row: the
 *     sums of q, of the normals' t, of the colours' t).  out_vertices [V',3] f32, out_faces [F',3] i32 (may be NULL when F' == 0),
 *     out_normals / out_colors [V',3] f32 iff normals / colors are given.  The entry reads (V', F', n_bad) back from the scratch (one
 *     24-byte read, one synchronisation of `stream`) and REFUSES, writing nothing, when n_bad != 0 or when Vout / Fout are not V' / F'.
 *     Every row of every output is written exactly once by a plain store.
 *   Refused before any launch (nothing written): V or F outside the ranges above, null pointers (but faces with F == 0, normals,
 *     colors), a cell not finite and positive, an origin not finite, a scratch that is null, unaligned or too small; in the emit
 *     entry also Vout outside [1, V], Fout outside [0, F], an attribute input without its output or the reverse.  A face index
 *     outside [0, V) is never dereferenced: such a face is dropped.  No allocation, no environment variable. */
int scanerf_mesh_simplify_scratch_bytes(int V, int F, size_t *bytes);
int scanerf_mesh_simplify_cluster(const float *vertices, const int32_t *faces, const float *normals, const float *colors, int V, int F,
                                  const float *origin, float cell, void *scratch, size_t scratch_bytes, scanerf_stream_t stream);
int scanerf_mesh_simplify_emit(const float *vertices, const int32_t *faces, const float *normals, const float *colors, int V, int F,
                               const float *origin, float cell, const void *scratch, size_t scratch_bytes, int64_t *sums,
                               int32_t *counts, float *out_vertices, int32_t *out_faces, float *out_normals, float *out_colors,
                               int Vout, int Fout, scanerf_stream_t stream);

/* ---- the hit record of the tracer, and a mesh rendered with its vertex attributes through a set of cameras (csrc/mesh_render.hip;
 *   DESIGN.md 4.24).  What "look at the coloured mesh from the capture's cameras" needs.  The reference has no counterpart; the
 *   definition is this comment.  Everything below is float32, operation by operation, without FMA contraction.
 *   The tracer's arrays are taken as scanerf_mesh_first_hit takes them (tris != NULL: pre-gathered triangles, else vertices / faces),
 *     but cell_faces is ALWAYS required: it names the faces.  log2dim 4..7.
 *   scanerf_mesh_trace: rays_o, rays_d [B,3] -> t [B] f32, face [B] i32, bary [B,2] f32 = (u, v).
 *     The walk is scanerf_mesh_first_hit's: the same cells in the same order, the same ray / triangle test (Moeller-Trumbore,
 *     two-sided, edges inclusive, |det| <= 1e-12 is a dead face that is never returned, t > 0) on the same operands
 *     (A, B - A, C - A), the same stop rule (the walk ends after the first cell whose exit t1 >= the candidate's t).  t has the bits
 *     scanerf_mesh_first_hit writes for the ray, at every log2dim and in both triangle forms.
 *     Candidates are compared as (t, face index): a later face, or a later cell, replaces the candidate only with a smaller t, or an
 *     equal t and a lower index.  face is therefore the lowest index, AMONG THE FACES THE WALK TESTED, that attains t: a face that
 *     ties the answer exactly at the exit of the cell the walk stops in, and is registered only in cells beyond it, goes untested.
 *     u, v are Moeller-Trumbore's for that face: with p = d x e2, w = o - A, q = w x e1, inv = 1 / (e1 . p) (dot products summed
 *     left to right, each cross component two products and one subtraction): u = (w . p) inv, v = (d . q) inv, t = (e2 . q) inv.
 *     The hit point is A + u e1 + v e2.
 *     A MISS gives t = 0, face = -1, u = v = 0: no face hit, a ray that misses the grid cube, non-finite input (its walk ends at
 *     the step cap).
 *   scanerf_mesh_trace_brute (the witness): the same outputs from the same device function over the faces 0 .. F-1 in order, no
 *     grid.  A face answers iff the build registers it (indices in [0, V), box not outside the cube, cell > 0); a ray answers iff
 *     it meets the grid cube (the first-hit walk's clip).  It tests every face, so its face is the lowest index over ALL faces.
 *   scanerf_mesh_render_views: C cameras in one launch.  Ks [C,9], C2Ws [C,12] f32 row-major; the image size H, W; vertices and
 *     faces are required here (the attributes are gathered by vertex index); vertex_normals [V,3], vertex_colors [V,3] f32 or NULL.
 *     The ray of pixel (px, py) of camera c, K = Ks[c], M = C2Ws[c], is scanerf_compute_ray_forward's, operation for operation:
 *       x = (1.0f px + 0.5f - K[2]) / K[0];  y = (1.0f py + 0.5f - K[5]) / K[4];
 *       d_a = (M[4a] x + M[4a+1] y) + M[4a+2], a = 0, 1, 2;  o = (M[3], M[7], M[11]).
 *     The camera-z component of d is 1, so t is z-depth: what scanerf_tsdf_integrate reads.  No ray is stored.
 *     The hit is scanerf_mesh_trace's.  With (ia, ib, ic) = the face's vertex indices and w0 = (1 - u) - v, a vertex attribute a
 *     becomes a = (w0 a[ia] + u a[ib]) + v a[ic] per component.
 *     Outputs: depth [C,H,W] f32 = t; face [C,H,W] i32; normal [C,H,W,3] f32 or NULL (not written); color [C,H,W,3] f32 or NULL
 *       (not written; a non-NULL color needs vertex_colors).
 *     normal: n = the interpolated vertex normal, or with vertex_normals == NULL the face normal e1 x e2 (each component two
 *       products and one subtraction; its orientation follows the winding); then n_a / (sqrtf((nx nx + ny ny) + nz nz) + 1e-8f).
 *     color: the interpolated vertex colour, as it is.
 *     A miss writes depth 0, face -1, normal 0, colour 0.
 *     A wavefront owns an 8 x 8 pixel block of one camera (partial blocks at the right and bottom borders are masked); the output
 *       bits do not depend on that mapping.
 *   Every element of every output is written exactly once by a plain store and nothing else is written: two launches give equal bits.
 *   B == 0 and C == 0 launch nothing.  Refused before any launch (nothing written): B < 0 or B > 2^29; null pointers (but tris,
 *     and vertices / faces where tris is given, in scanerf_mesh_trace; tris, vertex_normals, vertex_colors, normal, color in
 *     scanerf_mesh_render_views; vertices / faces with F == 0 in the brute entry); V or F < 0; C < 0; H or W < 1; C H W >= 2^31;
 *     log2dim outside 4..7; a color output without vertex_colors.
 *   No allocation, no host synchronisation, no atomics, no scratch; every launch on `stream`. */
int scanerf_mesh_trace(const float *rays_o, const float *rays_d, int B, const float *vertices, const int32_t *faces, const float *tris,
                       const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces,
                       const float *scene_info, int log2dim, float *t, int32_t *face, float *bary, scanerf_stream_t stream);
int scanerf_mesh_trace_brute(const float *rays_o, const float *rays_d, int B, const float *vertices, const int32_t *faces, int V, int F,
                             const float *scene_info, int log2dim, float *t, int32_t *face, float *bary, scanerf_stream_t stream);
int scanerf_mesh_render_views(const float *Ks, const float *C2Ws, int C, int H, int W, const float *vertices, const int32_t *faces,
                              const float *tris, const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                              const int32_t *cell_faces, const float *scene_info, int log2dim, const float *vertex_normals,
                              const float *vertex_colors, float *depth, int32_t *face, float *normal, float *color,
                              scanerf_stream_t stream);

/* ---- vertex colours for any mesh from posed images (csrc/mesh_colors.hip): every point is projected into every
 *   camera, the cameras that see it are sampled bilinearly there and blended.  What "colour an extracted, simplified or foreign mesh
 *   from the field's renders or the capture's photographs" needs.  The reference has no counterpart; the definition is this comment.
 *   Everything below is float32, operation by operation, without FMA contraction; division and sqrtf correctly rounded.
 *   scanerf_mesh_project_colors.  Inputs: points [N,3] f32; normals [N,3] f32 or NULL; images [C,H,W,3] f32, any values; Ks [C,9],
 *     C2Ws [C,12], H, W, bias, near, far and the tracer's arrays with log2dim exactly as scanerf_mesh_point_views takes them; min_cos in
 *     [0, 1); acc [N,4] f32, interleaved (R, G, B, Wt), 16-byte aligned, read AND written; count [N] i32, read and written.
 *   For point p and camera c = 0 .. C-1, IN THIS ORDER:
 *     IN VIEW, SEGMENT, HIDDEN, SEEN: w, xc, yc, zc, len, px = fx (xc / zc) + cx, py = fy (yc / zc) + cy and the three rules are exactly
 *       scanerf_mesh_point_views': the same operands, the same walk, the same early ends.
 *     FACING (only with normals != NULL; n = the point's normal):
 *       nl = sqrtf((n0 n0 + n1 n1) + n2 n2);  q = (n0 w0 + n1 w1) + n2 w2;  cosv = (-q) / (len * nl);
 *       the pair faces the camera iff cosv > min_cos (false for a NaN: a zero or non-finite normal contributes nothing); wt = cosv.
 *       With normals == NULL every pair faces and wt = 1.
 *     SAMPLE (pixel j covers [j, j + 1), its centre is at j + 0.5):
 *       u = px - 0.5f, v = py - 0.5f;  x0f = floorf(u), ax = u - x0f;  y0f = floorf(v), ay = v - y0f;
 *       x0 = clamp((int)x0f, 0, W-1), x1 = clamp((int)x0f + 1, 0, W-1);  y0, y1 likewise with H;
 *       per channel k, I = images[c]:  top = (1 - ax) * I[y0][x0][k] + ax * I[y0][x1][k];  bot the same on row y1;
 *       val_k = (1 - ay) * top + ay * bot.
 *     The pair CONTRIBUTES iff it is seen, faces the camera, and all 12 taps are finite.  Then
 *       R <- R + wt * val_0, G <- G + wt * val_1, B <- B + wt * val_2, Wt <- Wt + wt, count <- count + 1.
 *   The sums START FROM THE VALUES IN acc / count and run in ascending camera order: consecutive batches of cameras give the bits
 *     of one call.  The order does not depend on which lane walked which segment: two launches give equal bits, both triangle forms
 *     and every log2dim give equal bits.  One lane owns a point; no atomics on floats, no global atomics; every row of acc (one 16-byte
 *     load, one 16-byte store) and of count is read once and written once per call by plain stores; nothing else is written.
 *   N == 0 launches nothing.  C == 0 launches nothing: acc and count stay as they are (the image, camera and tracer arrays are not
 *     read).  Refused before any launch (nothing written): N < 0 or C < 0, null pointers (but normals, tris), H or W < 1, log2dim
 *     outside 4..7, bias not in (0, inf), near negative or NaN, far not > 0, min_cos outside [0, 1) or NaN, an acc that is not 16-byte
 *     aligned.  No allocation, no host synchronisation; the launch goes on `stream`.
 *   scanerf_mesh_project_colors_counted (measurement): also adds to counters [4] u64, which the caller zeroes: the pairs in view (the
 *     segments walked), the occupied cells looked at, the ray / triangle tests, the pairs that contributed.
 *   scanerf_mesh_resolve_colors: fill[3]: a HOST array.  For p < N: valid[p] (u8) = Wt > 0; colors[p][k] = valid ? acc[p][k] / Wt :
 *     fill[k].  One launch, every element of colors [N,3] f32 and valid [N] written once.  N == 0 launches nothing; N < 0, null
 *     pointers and an acc that is not 16-byte aligned are refused. */
int scanerf_mesh_project_colors(const float *points, const float *normals, int N, const float *images, const float *Ks,
                                const float *C2Ws, int C, int H, int W, float bias, float near, float far, float min_cos,
                                const float *vertices, const int32_t *faces, const float *tris, const uint64_t *bitmask,
                                const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces, const float *scene_info,
                                int log2dim, float *acc, int32_t *count, scanerf_stream_t stream);
int scanerf_mesh_project_colors_counted(const float *points, const float *normals, int N, const float *images, const float *Ks,
                                        const float *C2Ws, int C, int H, int W, float bias, float near, float far, float min_cos,
                                        const float *vertices, const int32_t *faces, const float *tris, const uint64_t *bitmask,
                                        const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces,
                                        const float *scene_info, int log2dim, float *acc, int32_t *count, uint64_t *counters,
                                        scanerf_stream_t stream);
int scanerf_mesh_resolve_colors(const float *acc, int N, const float *fill, float *colors, uint8_t *valid, scanerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCANERF_MESH_TOOLS_HIP_H_ */
