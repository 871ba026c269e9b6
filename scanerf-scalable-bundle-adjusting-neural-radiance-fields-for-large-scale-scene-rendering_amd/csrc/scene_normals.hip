// scene_normals.hip -- density, gradient and normal of a tiled scene's BLENDED density at arbitrary world points.
//
// The reference has no counterpart; the definition is the comment of include/scanerf_hip.h (scanerf_scene_sigma_normals_points).
// The field is the scene mesh's, v = sum_b w_b sigma_b / W (csrc/isosurface.hip, iso_fill_tiles); its gradient carries, by the quotient
// rule, the gradients of the blend weights:
//     g = (sum_b w_b grad sigma_b + sum_b sigma_b grad w_b - v sum_b grad w_b) / W        (the last sum over every LISTED tile).
// Built as isosurface.hip is (contraction on for the shared per-sample code: density_grad / finish_sample give
// scanerf_sigma_normals_points' bits); the geometry and the blend stand under `fp contract(off)`, product by product.
//
// One wave per workgroup; a lane owns one point of a 64-point group, a workgroup walks a contiguous range of groups (the mesh's
// vertices come in brick order: neighbouring groups lie in the same tiles).  Per group the wave reduces the points' extent, tests
// the tile boxes against it 64 at a time (no table read) and visits the candidates in ascending index: position, membership, weight
// and weight gradient per lane; only where some lane contributes are the tile's operands staged (nrm_stage, kept across groups) and
// the 64-point density pass run.  A lane's sums are ordered by tile index alone: its bits depend on nothing but its own position.
#include "normals_device.h"
#include "render_infer_device.h"

namespace scanerf {
namespace {

constexpr int kSnThreads = 64;
constexpr int kSnMaxBlocks = kNumCU * 8;   // two waves per SIMD resident (register-bound, as normals.hip)

struct SceneNormalArgs {
    const float *points;          // [N,3] world
    const void *tables;           // [nb,16,T,2] f16
    const float *blobs;           // [nb, SCANERF_PARAMSIZE]
    const int32_t *res;           // [nb,16,3]
    Tiles t;
    float *sigma, *grad, *normal; // [N], [N,3] or null, [N,3]
    int T, N;
};

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// a wave-uniform value, said so (it then lives in a scalar register)
__device__ __forceinline__ float sn_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// sign of the weight's distance along one axis: d (0.5 - |pt - 0.5|) / d pt
__device__ __forceinline__ float sn_side(float pt) { return pt < 0.5f ? 1.0f : (pt > 0.5f ? -1.0f : 0.0f); }

__global__ void __launch_bounds__(kSnThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) k_scene_sigma_normals(SceneNormalArgs a)
{
#pragma clang fp contract(off)   // every product and every sum of the definition separately rounded
    __shared__ __attribute__((aligned(16))) float lds[NL_TOTAL];
    const int lane = threadIdx.x;
    const int ngroups = (a.N + 63) >> 6;
    const int per = (ngroups + (int)gridDim.x - 1) / (int)gridDim.x;
    const int g_begin = (int)blockIdx.x * per, g_end = g_begin + per < ngroups ? g_begin + per : ngroups;
    const int nb = a.t.nb;
    int staged = -1;   // the tile whose operands LDS holds (wave-uniform)
    float c = 0.0f;

    for (int grp = g_begin; grp < g_end; ++grp) {
        const int i = grp * 64 + lane;
        const bool live = i < a.N;
        float wp[3] = { 0.0f, 0.0f, 0.0f };
        if (live) {
#pragma unroll
            for (int k = 0; k < 3; ++k) wp[k] = a.points[3 * (size_t)i + k];
        }
        // the group's extent (dead lanes and NaN coordinates do not take part).  Tile coordinate and membership are monotone in the
        // position, so a tile lists a point of the group only if it passes the test at the extent's ends.
        float wlo[3], whi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            wlo[k] = sn_uniform(wave_min(live ? wp[k] : __builtin_inff()));
            whi[k] = sn_uniform(wave_max(live ? wp[k] : -__builtin_inff()));
        }
        // (the weight has no y term: B and C hold x and z; their y sums are +0.0)
        float W = 0.0f, num = 0.0f, A[3] = { 0.0f, 0.0f, 0.0f }, B[2] = { 0.0f, 0.0f }, C[2] = { 0.0f, 0.0f };
        bool contributed = false;
        for (int base = 0; base < nb; base += 64) {
            const int bt = base + lane;
            bool reach = bt < nb;
            if (reach) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float ck = a.t.corners[3 * bt + k], sk = a.t.sizes[3 * bt + k];
                    reach = reach && tile_coord(wlo[k], ck, sk) <= 1.0f && tile_coord(whi[k], ck, sk) >= 0.0f;
                }
            }
            unsigned long long cand = __ballot(reach);
            while (cand != 0ull) {   // wave-uniform, ascending tile index
                const int b = base + __ffsll((long long)cand) - 1;
                cand &= cand - 1ull;
                const float *cb = a.t.corners + 3 * b, *sb = a.t.sizes + 3 * b;
                float pt[3];
                tile_point(wp, cb, sb, pt);
                const bool listed = live && pt[0] >= 0.0f && pt[0] <= 1.0f && pt[1] >= 0.0f && pt[1] <= 1.0f && pt[2] >= 0.0f && pt[2] <= 1.0f;
                const float w = tile_weight(pt, sb);
                const int64_t cell = tile_cell(a.t, b, pt);   // (for every lane: render_infer_device.h)
                // the weight's gradient in world units, by the branch xz_weight takes
                const float dx = (0.5f - fabsf(pt[0] - 0.5f)) * sb[0], dz = (0.5f - fabsf(pt[2] - 0.5f)) * sb[2];
                const float sx = sn_side(pt[0]), sz = sn_side(pt[2]);
                float gw[2] = { 0.0f, 0.0f };   // (x, z)
                if (dx != 0 && dz != 0) {
                    gw[0] = sx * dz;
                    gw[1] = sz * dx;
                } else if (dx != 0) {
                    gw[0] = sx;
                } else if (dz != 0) {
                    gw[1] = sz;
                }
                if (listed) {   // weight and weight gradient count whether or not the cell is occupied
                    W = W + w;
                    C[0] = C[0] + gw[0];
                    C[1] = C[1] + gw[1];
                }
                const bool run = listed && a.t.occ[cell] != 0;
                if (__ballot(run) == 0ull) continue;   // wave-uniform: listed, nobody contributes -- the weight arithmetic only
                if (b != staged) {
                    __syncthreads();   // (one wave: the reads of the tile staged before are done)
                    const float *blob = a.blobs + (size_t)b * SCANERF_PARAMSIZE;
                    nrm_stage<false>(lds, blob, nullptr, a.res + (size_t)b * 48, lane);
                    c = nrm_c(blob);
                    staged = b;
                    __syncthreads();
                }
                float x[3] = { 0.0f, 0.0f, 0.0f }, asc[3];   // (lanes that do not run: any finite x)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    asc[k] = 2.0f / sb[k];   // the contracted coordinate is 2 pt - 1
                    if (run) {
                        const float m = 2.0f * pt[k];
                        x[k] = m - 1.0f;
                    }
                }
                float s, gsum[3], sg, gs[3], unused[3];
                density_grad<SCANERF_F16, false, false>(lds, (const char *)a.tables + (size_t)b * 16 * a.T * 4, a.T, asc, c, lane, x, s, gsum);
                finish_sample(s, gsum, sg, gs, unused);
                if (run) {
                    const float ws = w * sg;
                    num = num + ws;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float wa = w * gs[k];
                        A[k] = A[k] + wa;
                    }
                    const float bx = sg * gw[0], bz = sg * gw[1];
                    B[0] = B[0] + bx;
                    B[1] = B[1] + bz;
                    contributed = true;
                }
            }
        }
        if (!live) continue;
        float v = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f }, n[3] = { 0.0f, 0.0f, 0.0f };   // no tile contributes: +0.0 everywhere
        if (contributed) {
            const float inv = inv_weight(W);
            v = num * inv;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float ab = A[k] + (k == 1 ? 0.0f : B[k >> 1]), vc = v * (k == 1 ? 0.0f : C[k >> 1]);
                g[k] = (ab - vc) * inv;
            }
            const float q0 = g[0] * g[0], q1 = g[1] * g[1], q2 = g[2] * g[2];
            const float q = (q0 + q1) + q2;
            const float r = -1.0f / (sqrtf(q) + 1e-8f);
#pragma unroll
            for (int k = 0; k < 3; ++k) n[k] = g[k] * r;
        }
        a.sigma[i] = v;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (a.grad) a.grad[3 * (size_t)i + k] = g[k];
            a.normal[3 * (size_t)i + k] = n[k];
        }
    }
}

}  // namespace
}  // namespace scanerf

using namespace scanerf;

SCANERF_API int scanerf_scene_sigma_normals_points(const float *points, const void *tables_f16, const float *blobs,
                                                   const int32_t *resolution, const uint8_t *occ, const int64_t *grid_starts,
                                                   const int32_t *log2dim, const float *corners, const float *sizes, int T, int nb,
                                                   float *sigma, float *grad, float *normal, int N, scanerf_stream_t stream)
{
    const char *op = "scene_sigma_normals_points";
    SCANERF_REQUIRE(N >= 0, "%s: N=%d", op, N);
    SCANERF_REQUIRE(nb >= 1, "%s: nb=%d (at least one tile)", op, nb);
    SCANERF_REQUIRE(T >= 2 && (T & (T - 1)) == 0, "%s: T=%d must be a power of two", op, T);
    SCANERF_REQUIRE(points && tables_f16 && blobs && resolution && occ && grid_starts && log2dim && corners && sizes && sigma && normal,
                    "%s: null pointer", op);
    SCANERF_REQUIRE(((uintptr_t)tables_f16 & 15) == 0, "%s: tables must be 16-byte aligned", op);
    if (N == 0) return 0;
    SceneNormalArgs a;
    a.points = points; a.tables = tables_f16; a.blobs = blobs; a.res = resolution;
    a.t = make_tiles(corners, sizes, occ, grid_starts, log2dim, nb);
    a.sigma = sigma; a.grad = grad; a.normal = normal; a.T = T; a.N = N;
    int blocks = ceil_div(N, 64);
    if (blocks > kSnMaxBlocks) blocks = kSnMaxBlocks;
    hipLaunchKernelGGL(k_scene_sigma_normals, dim3(blocks), dim3(kSnThreads), 0, (hipStream_t)stream, a);
    return check_launch(op);
}
