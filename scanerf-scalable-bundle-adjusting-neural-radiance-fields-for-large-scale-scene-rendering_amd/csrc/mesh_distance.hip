// mesh_distance.hip -- exact closest point of a triangle mesh for many query points: the geometric half of the mesh
// evaluation (accuracy / completeness / chamfer / F-score of an extracted mesh against the scan).  The reference has no counterpart;
// the definition is the comment in include/scanerf_hip.h.  The structure is the tracer's (mesh.hip), read as it is.
//
// One point per lane.  closest_on_triangle() is the ONLY place where a closest point and its squared distance are computed: the
// grid route (pre-gathered or indexed triangles) and the brute-force route call it with the same operands (A, B - A, C - A), and the
// unit is built without FMA contraction, so one (point, face) pair gives the same bits on every route.  Candidates are compared as
// (d2, face index), so the answer does not depend on the order in which faces are met, nor on log2dim.
//
// The grid search visits the cells in Chebyshev shells r = 0, 1, ... around the (clamped) cell of p.  After shell r every face not
// yet seen is registered in no cell of the cube K_r of visited cells, i.e. on some axis a its cell range lies wholly beyond one side
// of K_r -- a side that is not the grid's boundary, because registration clamps into the grid.  Say its lowest cell is >= t, the
// first cell plane beyond K_r.  The build truncates fl(fl(min_a - g_a) / cell) (mesh.hip face_cells), two roundings, so
//     min_a >= g_a + t cell - 2.01 u E,            u = 2^-24, E = 2^L cell >= t cell,
// and every point of the face has coordinate a >= min_a.  The kernel forms d~ = fl(fl(g_a + fl(t cell)) - p_a), three roundings of
// quantities of magnitude <= H = E + max|g| + max|p|: the face's true distance is >= d~ - 5.01 u H.  What the search compares with
// is not the true distance but the float32 d2 of closest_on_triangle: its point q~ lies within ~20 u H of the triangle's box (the
// roundings of ap, the dots, the two quotients and A + v ab + w ac, each of magnitude <= H) and the sum of squares adds a relative
// 4 u, so sqrt(d2_f) >= d~ - 40 u H.  THE MARGIN is m = 2^-18 H = 64 u H: shell r ends the search when
//     min(best d2, max_dist^2) < (max(0, min over the open sides of K_r of d~ - m))^2,         strictly,
// so an unseen face can neither beat nor tie the answer.  The per-cell pruning uses the same margin per axis of the distance from p
// to cell_box (exact min / max of the cell's vertices) and skips only on db2 > best.  tests/test_gpu_mesh_distance.py holds both:
// the grid route equals the brute-force route bit for bit at log2dim 4..7, also with vertices and points on cell planes.
// The loop over r always ends: when no side of K_r is open, K_r is the whole grid.
//
// Empty space: per x-slab of a shell one rank difference over the slab's words tells that no cell of its columns is occupied (three
// loads); otherwise a column is one bitmask word at log2dim 6 (two at 7), scanned by its set bits.
// No atomics, no allocation, no host synchronisation; every output element is written exactly once; two launches give equal bits.
#include <climits>

#include "mesh_device.h"

namespace {

constexpr float kMargin = 3.814697265625e-06f;   // 2^-18 (times H: see above)

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Closest point q of the closed triangle (A, A + ab, A + ac) to p and d2 = |p - q|^2, by Voronoi regions: the three vertex regions,
// then the three edge regions, then the interior.  false (nothing written) for a dead face: n . n == 0 in float32, n = ab x ac.
__device__ __forceinline__ bool closest_on_triangle(const float p[3], const float A[3], const float ab[3], const float ac[3],
                                                    float q[3], float &d2)
{
    const float n[3] = { ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0] };
    if (dot3(n, n) == 0.0f) return false;
    const float ap[3] = { p[0] - A[0], p[1] - A[1], p[2] - A[2] };
    const float bp[3] = { ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2] };
    const float cp[3] = { ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2] };
    const float d1 = dot3(ab, ap), d2_ = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    float v, w;   // q = A + v ab + w ac
    bool bc = false;
    if (d1 <= 0.0f && d2_ <= 0.0f) { v = 0.0f; w = 0.0f; }
    else if (d3 >= 0.0f && d4 <= d3) { v = 1.0f; w = 0.0f; }
    else if (d6 >= 0.0f && d5 <= d6) { v = 0.0f; w = 1.0f; }
    else {
        const float vc = d1 * d4 - d3 * d2_, vb = d5 * d2_ - d1 * d6, va = d3 * d6 - d5 * d4;
        if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / (d1 - d3); w = 0.0f; }
        else if (vb <= 0.0f && d2_ >= 0.0f && d6 <= 0.0f) { v = 0.0f; w = d2_ / (d2_ - d6); }
        else if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) { bc = true; v = 0.0f; w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); }
        else {
            const float inv = 1.0f / ((va + vb) + vc);
            v = vb * inv;
            w = vc * inv;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = bc ? (A[a] + ab[a]) + w * (ac[a] - ab[a]) : (A[a] + v * ab[a]) + w * ac[a];
    const float e[3] = { p[0] - q[0], p[1] - q[1], p[2] - q[2] };
    d2 = dot3(e, e);
    return true;
}

struct Best {
    float d2;
    int face;
    float q[3];
    __device__ __forceinline__ void offer(const float p[3], const float A[3], const float ab[3], const float ac[3], int f)
    {
        float c[3], c2;
        if (!closest_on_triangle(p, A, ab, ac, c, c2)) return;
        if (c2 < d2 || (c2 == d2 && f < face)) {   // (a NaN is never taken)
            d2 = c2;
            face = f;
            q[0] = c[0]; q[1] = c[1]; q[2] = c[2];
        }
    }
};

__device__ __forceinline__ bool finite3(const float p[3])
{
    return fabsf(p[0]) < __builtin_huge_valf() && fabsf(p[1]) < __builtin_huge_valf() && fabsf(p[2]) < __builtin_huge_valf();
}

__device__ __forceinline__ void write_out(size_t i, const float p[3], const Best &b, float md2, float *__restrict__ dist2,
                                          int32_t *__restrict__ face, float *__restrict__ closest)
{
    const bool found = b.face != INT_MAX && b.d2 <= md2 && b.d2 < __builtin_huge_valf();
    dist2[i] = found ? b.d2 : __builtin_huge_valf();
    face[i] = found ? b.face : -1;
    if (closest) {
#pragma unroll
        for (int a = 0; a < 3; ++a) closest[3 * i + a] = found ? b.q[a] : p[a];
    }
}

// COUNT: counters [N,2] i32 = occupied cells whose box was looked at, face tests (the bench's census; the product entry has none)
template <bool PRE, bool COUNT>
__global__ void __launch_bounds__(256) k_closest_grid(const float *__restrict__ points, int N, Grid g, const float *__restrict__ cell_box,
                                                      const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                      const int32_t *__restrict__ cell_faces, const float *__restrict__ tris,
                                                      float max_dist, float *__restrict__ dist2, int32_t *__restrict__ face,
                                                      float *__restrict__ closest, int32_t *__restrict__ counters)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float p[3] = { points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2] };
    const float md2 = max_dist * max_dist;
    Best best = { __builtin_huge_valf(), INT_MAX, { p[0], p[1], p[2] } };
    int n_cells = 0, n_tests = 0;
    if (finite3(p)) {
        const int L = g.L, S = 1 << L;
        const float g0[3] = { g.scene_info[0], g.scene_info[1], g.scene_info[2] };
        const float cs = g.scene_info[3];
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float t = (p[a] - g0[a]) / cs;
            c[a] = !(t > 0.0f) ? 0 : (t >= (float)S ? S - 1 : (int)t);
        }
        const float H = (float)S * cs + fmaxf(fmaxf(fabsf(g0[0]), fabsf(g0[1])), fabsf(g0[2])) +
                        fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2]));
        const float m = H * kMargin;

        auto visit = [&](int ord) {   // one occupied cell
            if (COUNT) ++n_cells;
            const float *b = cell_box + 6 * (size_t)ord;
            float db[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) db[a] = fmaxf(fmaxf(b[a] - p[a], p[a] - b[3 + a]) - m, 0.0f);
            if (dot3(db, db) > best.d2) return;
            const int start = g.start_num[2 * ord], num = g.start_num[2 * ord + 1];
            for (int k = 0; k < num; ++k) {
                const int f = cell_faces[start + k];
                float A[3], ab[3], ac[3];
                if (PRE) {
                    const float *t = tris + 9 * (size_t)(start + k);
#pragma unroll
                    for (int a = 0; a < 3; ++a) { A[a] = t[a]; ab[a] = t[3 + a]; ac[a] = t[6 + a]; }
                } else {
                    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        A[a] = vertices[3 * (size_t)ia + a];
                        ab[a] = vertices[3 * (size_t)ib + a] - A[a];
                        ac[a] = vertices[3 * (size_t)ic + a] - A[a];
                    }
                }
                if (COUNT) ++n_tests;
                best.offer(p, A, ab, ac, f);
            }
        };
        auto segment = [&](uint32_t n0, uint32_t n1) {   // the occupied cells n0..n1 (one z-run of one column)
            for (uint32_t w = n0 >> 6; w <= (n1 >> 6); ++w) {
                const uint64_t word = g.bitmask[w];
                const uint32_t lo = w == (n0 >> 6) ? (n0 & 63u) : 0u, hi = w == (n1 >> 6) ? (n1 & 63u) : 63u;
                uint64_t bits = word & (~0ull << lo) & (~0ull >> (63u - hi));
                if (!bits) continue;
                const uint32_t rk = g.rank[w];
                while (bits) {
                    const int bpos = __builtin_ctzll(bits);
                    bits &= bits - 1ull;
                    visit((int)(rk + (uint32_t)__popcll(word & ((1ull << bpos) - 1ull))));
                }
            }
        };

        for (int r = 0; r <= S; ++r) {
            int lo[3], hi[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = c[a] - r < 0 ? 0 : c[a] - r;
                hi[a] = c[a] + r > S - 1 ? S - 1 : c[a] + r;
            }
            for (int x = lo[0]; x <= hi[0]; ++x) {
                const uint32_t xb = (uint32_t)x << (2 * L);
                const uint32_t w0 = (xb | ((uint32_t)lo[1] << L)) >> 6, w1 = (xb | ((uint32_t)hi[1] << L) | (uint32_t)(S - 1)) >> 6;
                if (g.rank[w1] + (uint32_t)__popcll(g.bitmask[w1]) == g.rank[w0]) continue;   // nothing in this slab's columns
                const bool xface = x == c[0] - r || x == c[0] + r;
                for (int y = lo[1]; y <= hi[1]; ++y) {
                    const uint32_t base = xb | ((uint32_t)y << L);
                    if (xface || y == c[1] - r || y == c[1] + r) segment(base + (uint32_t)lo[2], base + (uint32_t)hi[2]);
                    else {
                        if (c[2] - r >= 0) segment(base + (uint32_t)(c[2] - r), base + (uint32_t)(c[2] - r));
                        if (c[2] + r <= S - 1) segment(base + (uint32_t)(c[2] + r), base + (uint32_t)(c[2] + r));
                    }
                }
            }
            // every face not seen yet lies beyond an open side of K_r
            float bound = __builtin_huge_valf();
            bool open = false;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (lo[a] > 0) {
                    open = true;
                    bound = fminf(bound, p[a] - (g0[a] + (float)lo[a] * cs));
                }
                if (hi[a] < S - 1) {
                    open = true;
                    bound = fminf(bound, (g0[a] + (float)(hi[a] + 1) * cs) - p[a]);
                }
            }
            if (!open) break;
            bound = fmaxf(bound - m, 0.0f);   // (a NaN from inf - inf gives 0: the search goes on)
            if (fminf(best.d2, md2) < bound * bound) break;
        }
    }
    write_out((size_t)i, p, best, md2, dist2, face, closest);
    if (COUNT) {
        counters[2 * (size_t)i] = n_cells;
        counters[2 * (size_t)i + 1] = n_tests;
    }
}

// every face, no grid; a face answers iff the build registers it (mesh.hip face_cells: indices in [0, V), box not outside the cube,
// cell > 0) and it is live
__global__ void __launch_bounds__(256) k_closest_brute(const float *__restrict__ points, int N, const float *__restrict__ vertices,
                                                       const int32_t *__restrict__ faces, int V, int F, const float *__restrict__ scene_info,
                                                       int L, float max_dist, float *__restrict__ dist2, int32_t *__restrict__ face,
                                                       float *__restrict__ closest)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float p[3] = { points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2] };
    const float md2 = max_dist * max_dist;
    Best best = { __builtin_huge_valf(), INT_MAX, { p[0], p[1], p[2] } };
    if (finite3(p) && F > 0) {
        const float cell = scene_info[3], side = (float)(1 << L);
        for (int f = 0; f < F; ++f) {
            const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
            if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) continue;
            float A[3], ab[3], ac[3];
            bool out = !(cell > 0.0f);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float Aa = vertices[3 * (size_t)ia + a], Ba = vertices[3 * (size_t)ib + a], Ca = vertices[3 * (size_t)ic + a];
                const float gmin = scene_info[a], gmax = gmin + side * cell;
                out |= fmaxf(fmaxf(Aa, Ba), Ca) < gmin || fminf(fminf(Aa, Ba), Ca) > gmax;
                A[a] = Aa;
                ab[a] = Ba - Aa;
                ac[a] = Ca - Aa;
            }
            if (!out) best.offer(p, A, ab, ac, f);
        }
    }
    write_out((size_t)i, p, best, md2, dist2, face, closest);
}

int require_query_args(const char *what, const float *points, int N, int log2dim, float max_dist, const float *dist2, const int32_t *face)
{
    SCANERF_REQUIRE(N > 0 && N <= (1 << 30), "%s: N=%d", what, N);
    SCANERF_REQUIRE(log2dim >= 4 && log2dim <= 7, "%s: log2dim=%d outside 4..7", what, log2dim);
    SCANERF_REQUIRE(max_dist >= 0.0f, "%s: max_dist=%g (must be >= 0; +inf for no cut)", what, (double)max_dist);
    SCANERF_REQUIRE(points && dist2 && face, "%s: null pointer", what);
    return 0;
}

int closest_grid(const char *what, const float *points, int N, const float *vertices, const int32_t *faces, const float *tris,
                 const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces,
                 const float *cell_box, const float *scene_info, int log2dim, float max_dist, float *dist2, int32_t *face,
                 float *closest, int32_t *counters, bool count, scanerf_stream_t stream)
{
    if (N == 0) return 0;
    if (int r = require_query_args(what, points, N, log2dim, max_dist, dist2, face)) return r;
    SCANERF_REQUIRE(bitmask && rank && start_num && cell_faces && cell_box && scene_info && (!count || counters), "%s: null pointer", what);
    SCANERF_REQUIRE(tris || (vertices && faces), "%s: null pointer (neither triangles nor an indexed mesh)", what);
    const Grid g = { bitmask, rank, start_num, scene_info, log2dim };
    const dim3 grid(ceil_div(N, 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define SCANERF_CLOSEST(PRE, COUNT) \
    hipLaunchKernelGGL((k_closest_grid<PRE, COUNT>), grid, block, 0, st, points, N, g, cell_box, vertices, faces, cell_faces, tris, max_dist, \
                       dist2, face, closest, counters)
    if (count && tris) SCANERF_CLOSEST(true, true);
    else if (count) SCANERF_CLOSEST(false, true);
    else if (tris) SCANERF_CLOSEST(true, false);
    else SCANERF_CLOSEST(false, false);
#undef SCANERF_CLOSEST
    return check_launch(what);
}

}  // namespace

SCANERF_API int scanerf_mesh_closest_point(const float *points, int N, const float *vertices, const int32_t *faces, const float *tris,
                                           const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                                           const int32_t *cell_faces, const float *cell_box, const float *scene_info, int log2dim,
                                           float max_dist, float *dist2, int32_t *face, float *closest, scanerf_stream_t stream)
{
    return closest_grid("mesh_closest_point", points, N, vertices, faces, tris, bitmask, rank, start_num, cell_faces, cell_box, scene_info,
                        log2dim, max_dist, dist2, face, closest, nullptr, false, stream);
}

SCANERF_API int scanerf_mesh_closest_point_counted(const float *points, int N, const float *vertices, const int32_t *faces,
                                                   const float *tris, const uint64_t *bitmask, const uint32_t *rank,
                                                   const int32_t *start_num, const int32_t *cell_faces, const float *cell_box,
                                                   const float *scene_info, int log2dim, float max_dist, float *dist2, int32_t *face,
                                                   float *closest, int32_t *counters, scanerf_stream_t stream)
{
    return closest_grid("mesh_closest_point_counted", points, N, vertices, faces, tris, bitmask, rank, start_num, cell_faces, cell_box,
                        scene_info, log2dim, max_dist, dist2, face, closest, counters, true, stream);
}

SCANERF_API int scanerf_mesh_closest_point_brute(const float *points, int N, const float *vertices, const int32_t *faces, int V, int F,
                                                 const float *scene_info, int log2dim, float max_dist, float *dist2, int32_t *face,
                                                 float *closest, scanerf_stream_t stream)
{
    if (N == 0) return 0;
    if (int r = require_query_args("mesh_closest_point_brute", points, N, log2dim, max_dist, dist2, face)) return r;
    SCANERF_REQUIRE(V >= 0 && F >= 0, "mesh_closest_point_brute: V=%d F=%d", V, F);
    SCANERF_REQUIRE(F == 0 || (vertices && faces && scene_info), "mesh_closest_point_brute: null pointer");
    hipLaunchKernelGGL(k_closest_brute, dim3(ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, points, N, vertices, faces, V, F,
                       scene_info, log2dim, max_dist, dist2, face, closest);
    return check_launch("mesh_closest_point_brute");
}
