// render_normals_tiles.hip -- normal maps of the multi-tile novel-view render: pts_normals blends the tiles' density
// normals per sample exactly as pts_inference blends their colours (rendering_kernel.cu:467-581), accumulate_normal composites them
// per ray by accumulate_color's rule (:624-702).  The reference has no multi-tile normal; the definition is scanerf_hip.h's.
// Built with -ffp-contract=off, as render_time.hip and render_infer.hip: the slot list, position, weight, cell and table
// coordinate are render_infer_device.h's, the one definition that both units evaluate.
//
// The per-sample mathematics is normals.hip's (normals_device.h: one gather pass with the three position tangents, the 64 x 32
// first-layer product on v_mfma_f32_32x32x2_f32, the density path in closed form).  New here: the tile varies per lane and per
// slot.  One wave per workgroup; a lane owns a sample of a 64-sample group.  A tile's operands (first-layer weights, a, b0, the
// resolutions: 9 KB) are staged in LDS and the lanes that list that tile in an occupied cell run, tile by tile (the wave-uniform
// leader loop of k_pts_inference).  Three things keep the restagings down:
//   * a wave walks a CONTIGUOUS range of groups: in layout 2 that is along 32 neighbouring rays, two depths per group, so the
//     tile staged for one group is almost always the next group's;
//   * the staged tile is kept across groups and taken FIRST among the tiles a group lists (two tiles that alternate cost one
//     restaging per group, not two);
//   * slots in unoccupied cells and groups without any slot never reach the loop.
// A sample's slots are therefore processed in an order that depends on its wave's other samples; each slot's contribution is
// parked (LDS, lane-private) and summed afterwards in SLOT order, so a sample's bits do not depend on layout, ray order or launch.
#include "normals_device.h"
#include "render_infer_device.h"

using namespace scanerf;

namespace {

constexpr int kTnThreads = 64;
constexpr int kTnMaxBlocks = kNumCU * 8;   // two waves per SIMD resident (register-bound, as normals.hip)

constexpr int TL_CON = NL_TOTAL;           // [slot 4][xyz 3][lane 64]: w pa n of the slot
constexpr int TL_W = TL_CON + 12 * 64;     // [slot 4][lane 64]: blend weight
constexpr int TL_TOTAL = TL_W + 4 * 64;

struct TileNormalArgs {
    const float *rays_o, *rays_d, *z_vals, *dists;
    const int16_t *block_idxs;    // [B,S,4] in the layout
    const void *tables;           // [nb,16,T,2] f16
    const float *blobs;           // [nb, SCANERF_PARAMSIZE]
    const int32_t *res;           // [nb,16,3]
    Tiles t;
    float *out;                   // [B,S,3] in the layout
    unsigned int *counts;         // COUNT: [0] += groups that reached the tile loop, [1] += restagings, [2] += passes of the tile loop,
                                  // [3] += lanes that held a sample in those passes (of 64 each)
    int T, B, S, sm;
};

template <bool COUNT>
__global__ void __launch_bounds__(kTnThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) k_pts_normals(TileNormalArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[TL_TOTAL];
    const int lane = threadIdx.x;
    const uint32_t total = (uint32_t)a.B * (uint32_t)a.S;
    const uint32_t ngroups = (total + 63u) >> 6;
    const uint32_t per = (ngroups + gridDim.x - 1) / gridDim.x;
    const uint32_t g_begin = blockIdx.x * per, g_end = g_begin + per < ngroups ? g_begin + per : ngroups;
    const int nb = a.t.nb;
    int staged = -1;   // the tile whose operands LDS holds (wave-uniform)
    float c = 0.0f;
    unsigned int n_groups = 0, n_stage = 0, n_iter = 0, n_lanes = 0;

    for (uint32_t grp = g_begin; grp < g_end; ++grp) {
        const uint32_t e = grp * 64u + (uint32_t)lane;
        const bool in_range = e < total;
        const uint32_t ec = in_range ? e : total - 1u;
        int i, s;
        pt_decompose(ec, (uint32_t)a.B, (uint32_t)a.S, a.sm, i, s);
        // the slot list: ends at the first -1 (:499); a tile index outside [0, nb) ends it too (nothing is read for it)
        int slot[kMaxPtsBlocks] = { -1, -1, -1, -1 };
        if (in_range) slot_list_bounded(*reinterpret_cast<const uint2 *>(a.block_idxs + (size_t)ec * kMaxPtsBlocks), nb, slot);
        float *o3 = a.out + 3 * (size_t)ec;
        if (!__any(slot[0] != -1)) {   // wave-uniform: nothing listed in the whole group (unsampled rays, z == -1)
            if (in_range) o3[0] = o3[1] = o3[2] = 0.0f;
            continue;
        }
        float wp[3] = { 0.0f, 0.0f, 0.0f }, delta = 0.0f;   // world position; what multiplies sigma in pa
        if (slot[0] != -1) {
            float o[3], d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                o[k] = a.rays_o[3 * (size_t)i + k];
                d[k] = a.rays_d[3 * (size_t)i + k];
            }
            world_point(o, a.z_vals[ec], d, wp);
            delta = a.dists[ec] * sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);   // :557
        }
        // blend weights of every listed tile (they count whether or not the cell is occupied) and the slots that run
        float weight = 0.0f;
        unsigned pend = 0;
#pragma unroll
        for (int k = 0; k < kMaxPtsBlocks; ++k) {
            const int bk = slot[k];
            float w = 0.0f;
            if (bk != -1) {
                float pt[3];
                tile_point(wp, a.t.corners + 3 * bk, a.t.sizes + 3 * bk, pt);
                w = tile_weight(pt, a.t.sizes + 3 * bk);
                weight += w;
                if (a.t.occ[tile_cell(a.t, bk, pt)] != 0) pend |= 1u << k;
            }
            lds[TL_W + k * 64 + lane] = w;
        }
        const unsigned ran = pend;
        if (COUNT && __any(pend != 0)) ++n_groups;

        while (true) {
            const unsigned long long waiting = __ballot(pend != 0);
            if (!waiting) break;
            bool has_staged = false;
#pragma unroll
            for (int k = 0; k < kMaxPtsBlocks; ++k) has_staged |= ((pend >> k) & 1u) && slot[k] == staged;
            int b = staged;
            if (!__any(has_staged)) {
                int first = -1;
#pragma unroll
                for (int k = kMaxPtsBlocks - 1; k >= 0; --k) first = ((pend >> k) & 1u) ? slot[k] : first;
                b = __shfl(first, __ffsll((long long)waiting) - 1, 64);   // wave-uniform tile
            }
            if (b != staged) {
                __syncthreads();   // (one wave: the reads of the tile staged before are done)
                const float *blob = a.blobs + (size_t)b * SCANERF_PARAMSIZE;
                nrm_stage<false>(lds, blob, nullptr, a.res + (size_t)b * 48, lane);
                c = nrm_c(blob);
                staged = b;
                if (COUNT) ++n_stage;
                __syncthreads();
            }
            int kb = -1;
#pragma unroll
            for (int k = 0; k < kMaxPtsBlocks; ++k) kb = (((pend >> k) & 1u) && slot[k] == b) ? k : kb;
            const bool mine = kb >= 0;
            if (mine) pend &= ~(1u << kb);
            if (COUNT) {
                ++n_iter;
                n_lanes += (unsigned int)__popcll(__ballot(mine));
            }
            float asc[3], p01[3] = { 0.0f, 0.0f, 0.0f };   // (lanes without this tile: cell 0 of every level, one line per level)
            // (component by component, each beside its 2 / size: with tile_point / fg_p01 over the three at once the counted
            // kernel spills two registers more)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float sz = a.t.sizes[3 * b + q];
                asc[q] = 2.0f / sz;   // the contracted coordinate is 2 pts - 1
                if (mine) p01[q] = fg_coord(tile_coord(wp[q], a.t.corners[3 * b + q], sz));   // :548
            }
            float sg, gsum[3], sigma, g[3], n[3];
            density_grad<SCANERF_F16, true>(lds, (const char *)a.tables + (size_t)b * 16 * a.T * 4, a.T, asc, c, lane, p01, sg, gsum);
            finish_sample(sg, gsum, sigma, g, n);
            if (mine) {
                const float f = lds[TL_W + kb * 64 + lane] * (1.0f - expf(-sigma * delta));
#pragma unroll
                for (int q = 0; q < 3; ++q) lds[TL_CON + (3 * kb + q) * 64 + lane] = f * n[q];
            }
        }
        float acc[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int k = 0; k < kMaxPtsBlocks; ++k) {
            if ((ran >> k) & 1u) {
#pragma unroll
                for (int q = 0; q < 3; ++q) acc[q] += lds[TL_CON + (3 * k + q) * 64 + lane];
            }
        }
        if (weight > 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] /= weight;
        }
        if (in_range) {
            o3[0] = acc[0];
            o3[1] = acc[1];
            o3[2] = acc[2];
        }
    }
    if (COUNT && lane == 0) {
        atomicAdd(a.counts, n_groups);
        atomicAdd(a.counts + 1, n_stage);
        atomicAdd(a.counts + 2, n_iter);
        atomicAdd(a.counts + 3, n_lanes);
    }
}

// accumulate_color's rule for the normal, one thread per ray in every layout, the sums in the reference's serial order (the ray's
// running sum starts from what `normal` holds).  The transparency is read, never written: accumulate_color updates it afterwards.
__global__ void __launch_bounds__(256) k_accumulate_normal(const float *__restrict__ pts_normal, const float *__restrict__ pts_alpha,
                                                           const float *__restrict__ transp, const float *__restrict__ z_vals,
                                                           float *__restrict__ normal, int B, int S, int lay, int skip)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B; i += gridDim.x * blockDim.x) {
        float T = transp[i];
        if (T < 0.00001f) continue;
        if (skip && z_vals[pt_index(i, 0, B, S, lay)] == -1.0f) continue;   // SCANERF_SKIP_UNSAMPLED: pts_alpha may be uninitialised
        float n[3] = { normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2] };
        for (int s = 0; s < S; ++s) {
            const size_t e = pt_index(i, s, B, S, lay);
#pragma unroll
            for (int q = 0; q < 3; ++q) n[q] += T * pts_normal[3 * e + q];
            T = T * (1.0f - pts_alpha[e]);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) normal[3 * (size_t)i + q] = n[q];
    }
}

int run_pts_normals(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists, const int16_t *block_idxs,
                    const void *tables_f16, const float *blobs, const int32_t *resolution, const uint8_t *occ,
                    const int64_t *grid_starts, const int32_t *log2dim, const float *corners, const float *sizes, float *pts_normal,
                    unsigned int *counts, int B, int S, int T, int nb, int sample_major, scanerf_stream_t stream)
{
    const char *name = "pts_normals";
    RT_REQ(B >= 0 && S >= 1, name);
    SCANERF_REQUIRE(nb >= 1 && nb <= 32767, "%s: nb=%d (the slot lists are int16)", name, nb);
    RT_REQ_LAYOUT(sample_major, B, name);
    SCANERF_REQUIRE(T >= 2 && (T & (T - 1)) == 0, "%s: T=%d must be a power of two", name, T);
    SCANERF_REQUIRE((int64_t)B * S < ((int64_t)1 << 31), "%s: B * S = %lld samples (fewer than 2^31)", name, (long long)B * S);
    if (B == 0) return 0;
    RT_REQ(rays_o && rays_d && z_vals && dists && block_idxs && tables_f16 && blobs && resolution && occ && grid_starts && log2dim &&
               corners && sizes && pts_normal, name);
    SCANERF_REQUIRE(((uintptr_t)block_idxs & 7) == 0 && ((uintptr_t)tables_f16 & 7) == 0, "%s: block_idxs and tables must be 8-byte aligned", name);
    TileNormalArgs a;
    a.rays_o = rays_o; a.rays_d = rays_d; a.z_vals = z_vals; a.dists = dists; a.block_idxs = block_idxs;
    a.tables = tables_f16; a.blobs = blobs; a.res = resolution; a.t = make_tiles(corners, sizes, occ, grid_starts, log2dim, nb);
    a.out = pts_normal; a.counts = counts; a.T = T; a.B = B; a.S = S; a.sm = sample_major;
    int blocks = ceil_div((int64_t)B * S, 64);
    if (blocks > kTnMaxBlocks) blocks = kTnMaxBlocks;
    if (counts) hipLaunchKernelGGL((k_pts_normals<true>), dim3(blocks), dim3(kTnThreads), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_pts_normals<false>), dim3(blocks), dim3(kTnThreads), 0, (hipStream_t)stream, a);
    return check_launch(name);
}

}  // namespace

SCANERF_API int scanerf_pts_normals(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                                    const int16_t *block_idxs, const void *tables_f16, const float *blobs, const int32_t *resolution,
                                    const uint8_t *occ, const int64_t *grid_starts, const int32_t *log2dim, const float *corners,
                                    const float *sizes, float *pts_normal, int B, int S, int T, int nb, int sample_major,
                                    scanerf_stream_t stream)
{
    return run_pts_normals(rays_o, rays_d, z_vals, dists, block_idxs, tables_f16, blobs, resolution, occ, grid_starts, log2dim, corners,
                           sizes, pts_normal, nullptr, B, S, T, nb, sample_major, stream);
}

SCANERF_API int scanerf_pts_normals_counted(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                                            const int16_t *block_idxs, const void *tables_f16, const float *blobs,
                                            const int32_t *resolution, const uint8_t *occ, const int64_t *grid_starts,
                                            const int32_t *log2dim, const float *corners, const float *sizes, float *pts_normal,
                                            unsigned int *counts, int B, int S, int T, int nb, int sample_major, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(counts, "pts_normals_counted: null counts");
    return run_pts_normals(rays_o, rays_d, z_vals, dists, block_idxs, tables_f16, blobs, resolution, occ, grid_starts, log2dim, corners,
                           sizes, pts_normal, counts, B, S, T, nb, sample_major, stream);
}

SCANERF_API int scanerf_accumulate_normal(const float *pts_normal, const float *pts_alpha, const float *transparency,
                                          const float *z_vals, float *normal, int B, int S, int sample_major, scanerf_stream_t stream)
{
    RT_REQ(B >= 0 && S >= 1, "accumulate_normal");
    const int skip = (sample_major & SCANERF_SKIP_UNSAMPLED) != 0;
    sample_major &= ~SCANERF_SKIP_UNSAMPLED;
    RT_REQ_LAYOUT(sample_major, B, "accumulate_normal");
    if (B == 0) return 0;
    RT_REQ(pts_normal && pts_alpha && transparency && z_vals && normal, "accumulate_normal");
    hipLaunchKernelGGL(k_accumulate_normal, dim3(stream_grid(B, 256)), dim3(256), 0, (hipStream_t)stream, pts_normal, pts_alpha,
                       transparency, z_vals, normal, B, S, sample_major, skip);
    return check_launch("accumulate_normal");
}
