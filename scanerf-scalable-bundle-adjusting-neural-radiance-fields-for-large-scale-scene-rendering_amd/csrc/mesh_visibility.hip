// mesh_visibility.hip -- which cameras see which points of a mesh: for every (point, camera) pair a frustum test and,
// for the pairs in view, a segment-limited any-hit walk of the tracer's grid.  The reference has no counterpart; the definition is
// the comment in include/scanerf_mesh_tools_hip.h.  The structure is the tracer's (mesh.hip), read as it is; the walk is RayWalk and
// ray_triangle of mesh_device.h with first_hit_walk's operands, ended early (below).
//
// A WAVEFRONT owns 64 points, one per lane, and walks the cameras in passes of kCamsPerPass.  Two phases alternate inside a pass:
//   1. the frustum test of the wave's 64 points against ONE camera (its K and C2W are wave-uniform reads).  The lanes in view are
//      compacted by ballot + popcount into the wave's queue in the LDS: one entry = (lane of the point, camera within the pass);
//   2. as soon as the queue holds 64 entries, every lane takes one, fetches that point from its owner lane (a shuffle), forms the
//      segment again from the same operands, walks it, and ORs the pair's bit into the owner's mask word in the LDS when the segment
//      is free.  What is left at the end of the pass is walked by the first lanes.
// So the rare, long walks run on full wavefronts whatever share of the pairs is in view, and the cheap test stays uniform.  At the
// end of a pass every lane stores its own mask words (plain stores) and adds their popcounts to its count of views.  No workgroup
// barrier: the four wavefronts of a workgroup share nothing; a wavefront's LDS traffic is ordered by wave_sync().  No float
// atomics and no global atomics; the LDS ORs are integer: the outputs do not depend on the order of the walks.
//
// The early ends against first_hit_walk (which carries its nearest candidate until it is not beyond the current cell's exit t1 and
// returns h): the pair is hidden iff 0 < h < 1.  This walk visits the same cells in the same order and tests the same faces with the
// same operands, stops at the first t in (0, 1) (then h <= t < 1) and after the first cell with t1 >= 1.  If first_hit_walk ends
// earlier, at best <= t1 with best >= 1, that cell's t1 is >= 1 as well; if it goes on beyond a cell with t1 >= 1 it can only meet
// faces whose hit lies in a cell already passed.
#include "mesh_visibility_device.h"   // wave_sync, in_view, segment_hidden: shared with mesh_colors.hip

#include "scanerf_mesh_tools_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kWordsPerPass = 2;                     // mask words a lane keeps in the LDS
constexpr int kCamsPerPass = 32 * kWordsPerPass;     // 64: an entry's camera fits 6 bits
constexpr int kQueue = 2 * kWave;                    // fewer than 64 entries wait when up to 64 arrive
constexpr int kMaxGroups = 2048;

template <bool PRE, bool COUNT>
__global__ void __launch_bounds__(kThreads) k_point_views(const float *__restrict__ points, int N, const float *__restrict__ Ks,
                                                          const float *__restrict__ C2Ws, int C, float Hf, float Wf, float bias,
                                                          float near, float far, Grid g, const float *__restrict__ vertices,
                                                          const int32_t *__restrict__ faces, const int32_t *__restrict__ cell_faces,
                                                          const float *__restrict__ tris, int32_t *__restrict__ views,
                                                          uint32_t *__restrict__ mask, int nwords, unsigned long long *__restrict__ counters)
{
    __shared__ uint32_t queue[kWaves][kQueue];
    __shared__ uint32_t seen[kWaves][kWordsPerPass][kWave];
    const Words<false> words(g, nullptr);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    uint32_t *q = queue[wave];
    const unsigned long long below = (1ull << lane) - 1ull;
    const int units = (N + kWave - 1) / kWave;
    unsigned long long n_pairs = 0, n_cells = 0, n_tests = 0;

    for (int unit = blockIdx.x * kWaves + wave; unit < units; unit += gridDim.x * kWaves) {   // wave-uniform
        const int i = unit * kWave + lane;
        const bool live = i < N;
        float p[3] = { 0.0f, 0.0f, 0.0f };
        if (live) {
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = points[3 * (size_t)i + a];
        }
        const bool finite = live && fabsf(p[0]) < __builtin_huge_valf() && fabsf(p[1]) < __builtin_huge_valf() &&
                            fabsf(p[2]) < __builtin_huge_valf();

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

        int total = 0;
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
#pragma unroll
            for (int k = 0; k < kWordsPerPass; ++k) {
                const uint32_t word = seen[wave][k][lane];
                total += __popc(word);
                const int col = cbase / 32 + k;
                if (mask && live && col < nwords) mask[(size_t)i * nwords + col] = word;
            }
            wave_sync();   // the words are read before the next pass clears them
        }
        if (live) views[i] = total;
    }
    if (COUNT) {
        atomicAdd(&counters[0], n_pairs);
        atomicAdd(&counters[1], n_cells);
        atomicAdd(&counters[2], n_tests);
    }
}

int point_views(const char *what, const float *points, int N, const float *Ks, const float *C2Ws, int C, int H, int W, float bias,
                float near, float far, const float *vertices, const int32_t *faces, const float *tris, const uint64_t *bitmask,
                const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces, const float *scene_info, int log2dim,
                int32_t *views, uint32_t *mask, uint64_t *counters, bool count, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(N >= 0 && C >= 0, "%s: N=%d C=%d (negative size)", what, N, C);
    if (N == 0) return 0;
    SCANERF_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d (an image has at least one pixel)", what, H, W);
    SCANERF_REQUIRE(log2dim >= 4 && log2dim <= 7, "%s: log2dim=%d outside 4..7", what, log2dim);
    SCANERF_REQUIRE(bias > 0.0f && bias < __builtin_huge_valf(), "%s: bias=%g (must be > 0 and finite)", what, (double)bias);
    SCANERF_REQUIRE(near >= 0.0f, "%s: near=%g (must be >= 0)", what, (double)near);
    SCANERF_REQUIRE(far > 0.0f, "%s: far=%g (must be > 0; +inf for no limit)", what, (double)far);
    SCANERF_REQUIRE(points && views && (!count || counters), "%s: null pointer", what);
    if (C > 0) {
        SCANERF_REQUIRE(Ks && C2Ws && bitmask && rank && start_num && scene_info, "%s: null pointer", what);
        SCANERF_REQUIRE(tris || (vertices && faces && cell_faces), "%s: null pointer (neither triangles nor an indexed mesh)", what);
    }
    const Grid g = { bitmask, rank, start_num, scene_info, log2dim };
    const int nwords = (C + 31) / 32;
    const int units = ceil_div(N, kWave);
    const dim3 grid(min(ceil_div(units, kWaves), kMaxGroups)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ctr = reinterpret_cast<unsigned long long *>(counters);
#define SCANERF_VIEWS(PRE, COUNT) \
    hipLaunchKernelGGL((k_point_views<PRE, COUNT>), grid, block, 0, st, points, N, Ks, C2Ws, C, (float)H, (float)W, bias, near, far, g, \
                       vertices, faces, cell_faces, tris, views, mask, nwords, ctr)
    if (count && tris) SCANERF_VIEWS(true, true);
    else if (count) SCANERF_VIEWS(false, true);
    else if (tris) SCANERF_VIEWS(true, false);
    else SCANERF_VIEWS(false, false);
#undef SCANERF_VIEWS
    return check_launch(what);
}

}  // namespace

SCANERF_API int scanerf_mesh_point_views_cameras_per_pass(void) { return kCamsPerPass; }

SCANERF_API int scanerf_mesh_point_views(const float *points, int N, const float *Ks, const float *C2Ws, int C, int H, int W, float bias,
                                         float near, float far, const float *vertices, const int32_t *faces, const float *tris,
                                         const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                                         const int32_t *cell_faces, const float *scene_info, int log2dim, int32_t *views, uint32_t *mask,
                                         scanerf_stream_t stream)
{
    return point_views("mesh_point_views", points, N, Ks, C2Ws, C, H, W, bias, near, far, vertices, faces, tris, bitmask, rank, start_num,
                       cell_faces, scene_info, log2dim, views, mask, nullptr, false, stream);
}

SCANERF_API int scanerf_mesh_point_views_counted(const float *points, int N, const float *Ks, const float *C2Ws, int C, int H, int W,
                                                 float bias, float near, float far, const float *vertices, const int32_t *faces,
                                                 const float *tris, const uint64_t *bitmask, const uint32_t *rank,
                                                 const int32_t *start_num, const int32_t *cell_faces, const float *scene_info,
                                                 int log2dim, int32_t *views, uint32_t *mask, uint64_t *counters,
                                                 scanerf_stream_t stream)
{
    return point_views("mesh_point_views_counted", points, N, Ks, C2Ws, C, H, W, bias, near, far, vertices, faces, tris, bitmask, rank,
                       start_num, cell_faces, scene_info, log2dim, views, mask, counters, true, stream);
}
