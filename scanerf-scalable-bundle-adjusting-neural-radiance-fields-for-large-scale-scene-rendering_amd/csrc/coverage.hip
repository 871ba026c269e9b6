// coverage.hip -- tile allocation's one hot step, fused: for every camera c and every candidate tile box k the number of pixels of
// the reduced frame whose ray enters the box BEFORE it meets the mesh (the reference's preprocess/build_tiles.py:129-156 does this
// camera by camera with torch rays, a [B,K,2] bounds tensor, a depth pass and a reduction).  Nothing but the K x C table of pixel
// counts is written: no rays, no depths, no bounds.
//
// Rays (the reference's get_rays_torch_v2 on K / scale, tools/utils.py:72-85 -- NOT compute_ray_forward: no +0.5 pixel centre).
// With Ks [C,9] row-major (fx = K[0], cx = K[2], fy = K[4], cy = K[5]) and C2Ws [C,12] row-major 3 x 4 (R | t), in float32,
// operation by operation:
//   h = H / scale, w = W / scale                    (integer division)
//   fx' = fx / scale, fy' = fy / scale, cx' = cx / scale, cy' = cy / scale
//   pixel p of camera c: j = p / w, i = p % w;      x = (i - cx') / fx',  y = (j - cy') / fy'
//   d_r = x * R[r][0] + y * R[r][1] + R[r][2]       (left to right, not normalised),   o = C2W[:,3]
// Depth = the first-hit walk of mesh_device.h (the carried candidate, as scanerf_mesh_first_hit), 0 (nothing) -> 1e5.
// near_k = clip_box(o, d, center_k, size_k / 2).x, the interval [0, 1e5] (what k_ray_aabb of rays.hip computes); a miss never counts.
// counts[k][c] = |{ p : near_k < depth }|.
//
// One ray per lane; a workgroup takes 256-pixel chunks of ONE camera (blockIdx.y).  Per box the covered lanes of a wavefront are
// counted by ballot + popcount; lane (k mod 64) keeps the running count of box k in a register, so a pass of kBoxesPerPass boxes
// costs kBoxesPerPass / 64 registers.  At the end of a pass the four wavefronts' rows meet in the LDS and one integer atomic per
// non-zero (box, workgroup) goes to counts.  K <= kBoxesPerPass: the registers run over all of a workgroup's chunks and are flushed
// once.  Larger K: the boxes are walked in passes per chunk (the depth is traced once per chunk either way).  Integer adds only:
// the counts are exact and two launches give equal bits.
#include "mesh_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBoxesPerPass = 256;   // boxes per pass: the LDS holds kThreads / 64 rows of this many counts (4 KB)
constexpr int kSlots = kBoxesPerPass / kWave;

template <bool PRE>
__global__ void __launch_bounds__(kThreads) k_view_coverage(const float *__restrict__ Ks, const float *__restrict__ C2Ws, int C, int h,
                                                            int w, float scale, const float *__restrict__ box_centers,
                                                            const float *__restrict__ box_sizes, int K, Grid g,
                                                            const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                            const int32_t *__restrict__ cell_faces, const float *__restrict__ tris,
                                                            int32_t *__restrict__ counts)
{
    __shared__ int32_t rows[kThreads / kWave][kBoxesPerPass];
    const Words<false> words(g, nullptr);
    const int cam = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const float *Kc = Ks + 9 * (size_t)cam, *Tc = C2Ws + 12 * (size_t)cam;
    const float fx = Kc[0] / scale, fy = Kc[4] / scale, cx = Kc[2] / scale, cy = Kc[5] / scale;
    const float o[3] = { Tc[3], Tc[7], Tc[11] };
    const int P = h * w, nchunks = (P + kThreads - 1) / kThreads;
    const bool one_pass = K <= kBoxesPerPass;
    int32_t acc[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) acc[s] = 0;

    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {   // workgroup-uniform
        const int p = chunk * kThreads + threadIdx.x;
        const bool live = p < P;
        float d[3] = { 0.0f, 0.0f, 0.0f };
        float depth = 0.0f;
        if (live) {
            const int j = p / w, i = p % w;
            const float x = ((float)i - cx) / fx, y = ((float)j - cy) / fy;
#pragma unroll
            for (int r = 0; r < 3; ++r) d[r] = x * Tc[4 * r] + y * Tc[4 * r + 1] + Tc[4 * r + 2];
            depth = first_hit_walk<false, PRE>(o, d, g, words, vertices, faces, cell_faces, tris);
            if (depth == 0.0f) depth = 100000.0f;
        }
        const bool last = chunk + (int)gridDim.x >= nchunks;
        for (int base = 0; base < K; base += kBoxesPerPass) {
            const int n = min(kBoxesPerPass, K - base);
#pragma unroll
            for (int s = 0; s < kSlots; ++s) {
                const int m = min(kWave, n - s * kWave);
                for (int l = 0; l < m; ++l) {
                    const int k = base + s * kWave + l;   // wave-uniform: the box is read once per wavefront
                    const float c3[3] = { box_centers[3 * k], box_centers[3 * k + 1], box_centers[3 * k + 2] };
                    const float h3[3] = { box_sizes[3 * k] / 2.0f, box_sizes[3 * k + 1] / 2.0f, box_sizes[3 * k + 2] / 2.0f };
                    const F2 span = clip_box(o, d, c3, h3);
                    const bool covered = live && span.x != -1.0f && span.x < depth;
                    const int pop = __popcll(__ballot(covered));
                    acc[s] += lane == l ? pop : 0;
                }
            }
            if (!one_pass || last) {
#pragma unroll
                for (int s = 0; s < kSlots; ++s) {
                    rows[wave][s * kWave + lane] = acc[s];
                    acc[s] = 0;
                }
                __syncthreads();
                if ((int)threadIdx.x < n) {
                    int32_t sum = 0;
#pragma unroll
                    for (int v = 0; v < kThreads / kWave; ++v) sum += rows[v][threadIdx.x];
                    if (sum) atomicAdd(&counts[(size_t)(base + (int)threadIdx.x) * C + cam], sum);
                }
                __syncthreads();
            }
        }
    }
}

}  // namespace

SCANERF_API int scanerf_view_coverage_boxes_per_pass(void) { return kBoxesPerPass; }

SCANERF_API int scanerf_view_coverage(const float *Ks, const float *C2Ws, int C, int H, int W, int scale, const float *box_centers,
                                      const float *box_sizes, int K, const float *vertices, const int32_t *faces, const float *tris,
                                      const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                                      const int32_t *cell_faces, const float *scene_info, int log2dim, int32_t *counts,
                                      scanerf_stream_t stream)
{
    if (C == 0 || K == 0) return 0;
    SCANERF_REQUIRE(C > 0 && C <= 65535 && K > 0 && (long long)K * C < ((long long)1 << 31), "view_coverage: C=%d K=%d", C, K);
    SCANERF_REQUIRE(scale >= 1, "view_coverage: scale=%d (must be at least 1)", scale);
    SCANERF_REQUIRE(H > 0 && W > 0 && H / scale > 0 && W / scale > 0, "view_coverage: H=%d W=%d leave no pixel at scale=%d", H, W, scale);
    const int h = H / scale, w = W / scale;
    SCANERF_REQUIRE((long long)h * w <= (1 << 29), "view_coverage: %d x %d pixels per camera", h, w);
    SCANERF_REQUIRE(log2dim >= 4 && log2dim <= 7, "view_coverage: log2dim=%d outside 4..7", log2dim);
    SCANERF_REQUIRE(Ks && C2Ws && box_centers && box_sizes && bitmask && rank && start_num && scene_info && counts,
                    "view_coverage: null pointer");
    SCANERF_REQUIRE(tris || (vertices && faces && cell_faces), "view_coverage: null pointer (neither triangles nor an indexed mesh)");
    const Grid g = { bitmask, rank, start_num, scene_info, log2dim };
    const int nchunks = ceil_div((int64_t)h * w, kThreads);
    // a few resident workgroups per CU over all cameras; a workgroup strides over its camera's chunks
    const dim3 grid(min(nchunks, max(1, kNumCU * 8 / C)), C), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (tris) hipLaunchKernelGGL(k_view_coverage<true>, grid, block, 0, st, Ks, C2Ws, C, h, w, (float)scale, box_centers, box_sizes, K, g,
                                 vertices, faces, cell_faces, tris, counts);
    else hipLaunchKernelGGL(k_view_coverage<false>, grid, block, 0, st, Ks, C2Ws, C, h, w, (float)scale, box_centers, box_sizes, K, g,
                            vertices, faces, cell_faces, tris, counts);
    return check_launch("view_coverage");
}
