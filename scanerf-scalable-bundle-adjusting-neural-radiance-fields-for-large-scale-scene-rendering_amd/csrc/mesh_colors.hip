// mesh_colors.hip -- vertex colours for any mesh from posed images: every point is projected into every camera, the
// cameras that see it (the rule of mesh_visibility.hip, shared through mesh_visibility_device.h) are sampled bilinearly there and
// blended with the cosine between the normal and the direction to the eye.  The reference has no counterpart; the definition is the
// comment in include/scanerf_mesh_tools_hip.h.
//
// The structure is k_point_views': a WAVEFRONT owns 64 points, one per lane, and takes the cameras in passes of kCamsPerPass.
//   1. the frustum test of the 64 points against ONE camera (wave-uniform reads of K and C2W); the lanes in view are compacted by
//      ballot + popcount into the wave's queue in the LDS, and whenever 64 entries wait every lane walks one segment; a free segment
//      ORs the pair's bit into the owner's word in the LDS.  The walks run on full wavefronts.
//   2. NEW: when the pass's bits are complete every lane reads its own words, and the pass's cameras are taken again IN ASCENDING
//      ORDER (wave-uniform reads; a camera nobody of the wave is seen by is skipped by one ballot).  A lane whose bit is set forms
//      px, py again from the same operands, the weight, the 12 taps, and adds into its four registers.
// The order of a point's sums is the camera loop's, never the order of the walks.  acc / count are loaded once before the first
// pass and stored once after the last, by the lane that owns the row: no atomics on floats, no global atomics, nothing else written.
#include "mesh_visibility_device.h"

#include "scanerf_mesh_tools_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kWordsPerPass = 2;                     // mask words a lane keeps in the LDS
constexpr int kCamsPerPass = 32 * kWordsPerPass;     // 64: an entry's camera fits 6 bits
constexpr int kQueue = 2 * kWave;                    // fewer than 64 entries wait when up to 64 arrive
constexpr int kMaxGroups = 2048;

__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) < __builtin_huge_valf(); }

// One seen pair: the weight and the bilinear sample of the definition, added to the lane's sums.  Returns whether it contributed.
__device__ __forceinline__ bool blend_pair(const float p[3], const float n[3], float nl, bool weighted, float min_cos,
                                           const float *__restrict__ K, const float *__restrict__ T, const float *__restrict__ img, int H,
                                           int W, float sum[4])
{
    const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const float w[3] = { p[0] - T[3], p[1] - T[7], p[2] - T[11] };
    const float xc = (w[0] * T[0] + w[1] * T[4]) + w[2] * T[8];
    const float yc = (w[0] * T[1] + w[1] * T[5]) + w[2] * T[9];
    const float zc = (w[0] * T[2] + w[1] * T[6]) + w[2] * T[10];
    const float len = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    const float px = fx * (xc / zc) + cx, py = fy * (yc / zc) + cy;      // in_view's, bit for bit: 0 <= px < W, 0 <= py < H here
    float wt = 1.0f;
    if (weighted) {
        const float q = (n[0] * w[0] + n[1] * w[1]) + n[2] * w[2];
        wt = (-q) / (len * nl);
        if (!(wt > min_cos)) return false;   // (a NaN never faces)
    }
    const float u = px - 0.5f, v = py - 0.5f;
    const float x0f = floorf(u), y0f = floorf(v);
    const float ax = u - x0f, ay = v - y0f;
    const int xi = (int)x0f, yi = (int)y0f;   // -1 .. W-1, -1 .. H-1
    const int x0 = min(max(xi, 0), W - 1), x1 = min(max(xi + 1, 0), W - 1);
    const int y0 = min(max(yi, 0), H - 1), y1 = min(max(yi + 1, 0), H - 1);
    const float *r0 = img + (size_t)y0 * W * 3, *r1 = img + (size_t)y1 * W * 3;
    float val[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = r0[3 * x0 + k], b = r0[3 * x1 + k], c = r1[3 * x0 + k], d = r1[3 * x1 + k];
        ok = ok && is_finite(a) && is_finite(b) && is_finite(c) && is_finite(d);
        const float top = (1.0f - ax) * a + ax * b;
        const float bot = (1.0f - ax) * c + ax * d;
        val[k] = (1.0f - ay) * top + ay * bot;
    }
    if (!ok) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) sum[k] = sum[k] + wt * val[k];
    sum[3] = sum[3] + wt;
    return true;
}

template <bool PRE, bool COUNT>
__global__ void __launch_bounds__(kThreads) k_project_colors(const float *__restrict__ points, const float *__restrict__ normals, int N,
                                                             const float *__restrict__ images, const float *__restrict__ Ks,
                                                             const float *__restrict__ C2Ws, int C, int H, int W, float bias, float near,
                                                             float far, float min_cos, Grid g, const float *__restrict__ vertices,
                                                             const int32_t *__restrict__ faces, const int32_t *__restrict__ cell_faces,
                                                             const float *__restrict__ tris, float *__restrict__ acc,
                                                             int32_t *__restrict__ count, unsigned long long *__restrict__ counters)
{
    __shared__ uint32_t queue[kWaves][kQueue];
    __shared__ uint32_t seen[kWaves][kWordsPerPass][kWave];
    const Words<false> words(g, nullptr);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    uint32_t *q = queue[wave];
    const unsigned long long below = (1ull << lane) - 1ull;
    const int units = (N + kWave - 1) / kWave;
    const float Hf = (float)H, Wf = (float)W;
    const bool weighted = normals != nullptr;   // wave-uniform
    const size_t image = (size_t)H * W * 3;
    unsigned long long n_pairs = 0, n_cells = 0, n_tests = 0, n_used = 0;

    for (int unit = blockIdx.x * kWaves + wave; unit < units; unit += gridDim.x * kWaves) {   // wave-uniform
        const int i = unit * kWave + lane;
        const bool live = i < N;
        float p[3] = { 0.0f, 0.0f, 0.0f }, n[3] = { 0.0f, 0.0f, 0.0f };
        float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int seen_by = 0;
        if (live) {
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = points[3 * (size_t)i + a];
            if (weighted) {
#pragma unroll
                for (int a = 0; a < 3; ++a) n[a] = normals[3 * (size_t)i + a];
            }
            row = reinterpret_cast<const float4 *>(acc)[i];
            seen_by = count[i];
        }
        float sum[4] = { row.x, row.y, row.z, row.w };
        const float nl = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        const bool finite = live && is_finite(p[0]) && is_finite(p[1]) && is_finite(p[2]);

        // one queue entry: the segment of (point of lane e >> 6, camera cbase + (e & 63)), walked by THIS lane
        auto walk = [&](bool take, uint32_t e, int cbase) {
            const int src = (int)(e >> 6) & (kWave - 1);
            const float s[3] = { __shfl(p[0], src), __shfl(p[1], src), __shfl(p[2], src) };   // every lane of the wave is here
            if (!take) return;
            const int cc = (int)(e & 63u);
            const float *T = C2Ws + 12 * (size_t)(cbase + cc);
            const float E[3] = { T[3], T[7], T[11] };
            const float w[3] = { s[0] - E[0], s[1] - E[1], s[2] - E[2] };
            const float len = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
            const float sc = bias / len;
            float P[3], d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                P[a] = s[a] - sc * w[a];
                d[a] = E[a] - P[a];
            }
            if (COUNT) ++n_pairs;
            if (!segment_hidden<PRE, COUNT>(P, d, g, words, vertices, faces, cell_faces, tris, n_cells, n_tests))
                atomicOr(&seen[wave][cc >> 5][src], 1u << (cc & 31));
        };

        for (int cbase = 0; cbase < C; cbase += kCamsPerPass) {
#pragma unroll
            for (int k = 0; k < kWordsPerPass; ++k) seen[wave][k][lane] = 0u;
            wave_sync();
            const int ncam = min(kCamsPerPass, C - cbase);
            int nq = 0;   // wave-uniform: the entries waiting
            for (int cc = 0; cc < ncam; ++cc) {
                const size_t cam = (size_t)(cbase + cc);
                const bool iv = in_view(p, finite, Ks + 9 * cam, C2Ws + 12 * cam, Hf, Wf, bias, near, far);
                const unsigned long long b = __ballot(iv);
                if (iv) q[nq + __popcll(b & below)] = ((uint32_t)lane << 6) | (uint32_t)cc;
                nq += __popcll(b);
                if (nq >= kWave) {
                    nq -= kWave;
                    wave_sync();
                    const uint32_t e = q[nq + lane];
                    wave_sync();   // the entries are read before the next camera's overwrite them
                    walk(true, e, cbase);
                }
            }
            wave_sync();
            if (nq > 0) {
                const bool take = lane < nq;
                walk(take, take ? q[lane] : 0u, cbase);
            }
            wave_sync();
            uint32_t word[kWordsPerPass];
#pragma unroll
            for (int k = 0; k < kWordsPerPass; ++k) word[k] = seen[wave][k][lane];
            wave_sync();   // the words are read before the next pass clears them
            // the blend, in ascending camera order
            for (int cc = 0; cc < ncam; ++cc) {
                const bool mine = ((cc < 32 ? word[0] : word[1]) >> (cc & 31)) & 1u;
                if (__ballot(mine) == 0ull) continue;   // wave-uniform
                if (mine) {
                    const size_t cam = (size_t)(cbase + cc);
                    if (blend_pair(p, n, nl, weighted, min_cos, Ks + 9 * cam, C2Ws + 12 * cam, images + cam * image, H, W, sum)) {
                        ++seen_by;
                        if (COUNT) ++n_used;
                    }
                }
            }
        }
        if (live) {
            reinterpret_cast<float4 *>(acc)[i] = make_float4(sum[0], sum[1], sum[2], sum[3]);
            count[i] = seen_by;
        }
    }
    if (COUNT) {
        atomicAdd(&counters[0], n_pairs);
        atomicAdd(&counters[1], n_cells);
        atomicAdd(&counters[2], n_tests);
        atomicAdd(&counters[3], n_used);
    }
}

__global__ void __launch_bounds__(kThreads) k_resolve_colors(const float *__restrict__ acc, int N, float f0, float f1, float f2,
                                                             float *__restrict__ colors, uint8_t *__restrict__ valid)
{
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < N; i += gridDim.x * kThreads) {
        const float4 row = reinterpret_cast<const float4 *>(acc)[i];
        const bool ok = row.w > 0.0f;
        colors[3 * (size_t)i] = ok ? row.x / row.w : f0;
        colors[3 * (size_t)i + 1] = ok ? row.y / row.w : f1;
        colors[3 * (size_t)i + 2] = ok ? row.z / row.w : f2;
        valid[i] = ok ? 1 : 0;
    }
}

int project_colors(const char *what, const float *points, const float *normals, int N, const float *images, const float *Ks,
                   const float *C2Ws, int C, int H, int W, float bias, float near, float far, float min_cos, const float *vertices,
                   const int32_t *faces, const float *tris, const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                   const int32_t *cell_faces, const float *scene_info, int log2dim, float *acc, int32_t *count, uint64_t *counters,
                   bool counted, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(N >= 0 && C >= 0, "%s: N=%d C=%d (negative size)", what, N, C);
    if (N == 0) return 0;
    SCANERF_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d (an image has at least one pixel)", what, H, W);
    SCANERF_REQUIRE(log2dim >= 4 && log2dim <= 7, "%s: log2dim=%d outside 4..7", what, log2dim);
    SCANERF_REQUIRE(bias > 0.0f && bias < __builtin_huge_valf(), "%s: bias=%g (must be > 0 and finite)", what, (double)bias);
    SCANERF_REQUIRE(near >= 0.0f, "%s: near=%g (must be >= 0)", what, (double)near);
    SCANERF_REQUIRE(far > 0.0f, "%s: far=%g (must be > 0; +inf for no limit)", what, (double)far);
    SCANERF_REQUIRE(min_cos >= 0.0f && min_cos < 1.0f, "%s: min_cos=%g (must be in [0, 1))", what, (double)min_cos);
    SCANERF_REQUIRE(points && acc && count && (!counted || counters), "%s: null pointer", what);
    SCANERF_REQUIRE(((uintptr_t)acc & 15u) == 0, "%s: acc is not 16-byte aligned", what);
    if (C == 0) return 0;
    SCANERF_REQUIRE(images && Ks && C2Ws && bitmask && rank && start_num && scene_info, "%s: null pointer", what);
    SCANERF_REQUIRE(tris || (vertices && faces && cell_faces), "%s: null pointer (neither triangles nor an indexed mesh)", what);
    const Grid g = { bitmask, rank, start_num, scene_info, log2dim };
    const int units = ceil_div(N, kWave);
    const dim3 grid(min(ceil_div(units, kWaves), kMaxGroups)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ctr = reinterpret_cast<unsigned long long *>(counters);
#define SCANERF_COLORS(PRE, COUNT) \
    hipLaunchKernelGGL((k_project_colors<PRE, COUNT>), grid, block, 0, st, points, normals, N, images, Ks, C2Ws, C, H, W, bias, near, far, \
                       min_cos, g, vertices, faces, cell_faces, tris, acc, count, ctr)
    if (counted && tris) SCANERF_COLORS(true, true);
    else if (counted) SCANERF_COLORS(false, true);
    else if (tris) SCANERF_COLORS(true, false);
    else SCANERF_COLORS(false, false);
#undef SCANERF_COLORS
    return check_launch(what);
}

}  // namespace

SCANERF_API int scanerf_mesh_project_colors(const float *points, const float *normals, int N, const float *images, const float *Ks,
                                            const float *C2Ws, int C, int H, int W, float bias, float near, float far, float min_cos,
                                            const float *vertices, const int32_t *faces, const float *tris, const uint64_t *bitmask,
                                            const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces,
                                            const float *scene_info, int log2dim, float *acc, int32_t *count, scanerf_stream_t stream)
{
    return project_colors("mesh_project_colors", points, normals, N, images, Ks, C2Ws, C, H, W, bias, near, far, min_cos, vertices, faces,
                          tris, bitmask, rank, start_num, cell_faces, scene_info, log2dim, acc, count, nullptr, false, stream);
}

SCANERF_API int scanerf_mesh_project_colors_counted(const float *points, const float *normals, int N, const float *images, const float *Ks,
                                                    const float *C2Ws, int C, int H, int W, float bias, float near, float far,
                                                    float min_cos, const float *vertices, const int32_t *faces, const float *tris,
                                                    const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                                                    const int32_t *cell_faces, const float *scene_info, int log2dim, float *acc,
                                                    int32_t *count, uint64_t *counters, scanerf_stream_t stream)
{
    return project_colors("mesh_project_colors_counted", points, normals, N, images, Ks, C2Ws, C, H, W, bias, near, far, min_cos, vertices,
                          faces, tris, bitmask, rank, start_num, cell_faces, scene_info, log2dim, acc, count, counters, true, stream);
}

SCANERF_API int scanerf_mesh_resolve_colors(const float *acc, int N, const float *fill, float *colors, uint8_t *valid,
                                            scanerf_stream_t stream)
{
    const char *what = "mesh_resolve_colors";
    SCANERF_REQUIRE(N >= 0, "%s: N=%d (negative size)", what, N);
    if (N == 0) return 0;
    SCANERF_REQUIRE(acc && fill && colors && valid, "%s: null pointer", what);
    SCANERF_REQUIRE(((uintptr_t)acc & 15u) == 0, "%s: acc is not 16-byte aligned", what);
    const dim3 grid(min(ceil_div(N, kThreads), kMaxGroups)), block(kThreads);
    hipLaunchKernelGGL(k_resolve_colors, grid, block, 0, (hipStream_t)stream, acc, N, fill[0], fill[1], fill[2], colors, valid);
    return check_launch(what);
}
