// render_infer_device.h -- the per-sample tile geometry of the render-time inference, said once: the slot list of a sample, its
// position in a tile, blend weight, cell and occupancy, the table coordinate of the foreground and of the contracted background,
// and the output stage.  Used by render_infer.hip (pts_inference / bg_pts_inference_v2, every kernel) and render_normals_tiles.hip
// (pts_normals).  Both units are built with -ffp-contract=off and match the oracle bit for bit: an expression written here is
// the one every kernel evaluates, so a fix cannot reach one kernel variant and miss another.
// Reference behaviour: hashgrid/src/rendering_kernel.cu:499-557 (foreground) and :1040-1096 (background).
#pragma once
#include "render_time_common.h"

namespace {

// ---- slot list: four int16 tile indices per sample (prepare_points'), packed in 8 bytes
__device__ __forceinline__ void slots_unpack(uint2 raw, int slot[kMaxPtsBlocks])
{
    slot[0] = (int16_t)(raw.x & 0xffffu); slot[1] = (int16_t)(raw.x >> 16);
    slot[2] = (int16_t)(raw.y & 0xffffu); slot[3] = (int16_t)(raw.y >> 16);
}
// A list ends at its first end mark: what follows reads as -1.  For pts_inference the mark is -1 (:499); for pts_normals any index
// outside [0, nb) (nothing is read for it).  Two rules on purpose: they are not unified.
// The -1 rule is stated in two more places, which a change of it must reach: chunk_tileset (render_infer.hip: as nested branches, the
// loop being unrolled over a wave's groups) and k_pts_inference's `ended` flag (it loads a slot only while the list runs).
template <typename End>
__device__ __forceinline__ void slots_until(uint2 raw, int slot[kMaxPtsBlocks], End end)
{
    slots_unpack(raw, slot);
    bool ended = false;
#pragma unroll
    for (int k = 0; k < kMaxPtsBlocks; ++k) {
        ended |= end(slot[k]);
        if (ended) slot[k] = -1;
    }
}
__device__ __forceinline__ void slot_list(uint2 raw, int slot[kMaxPtsBlocks]) { slots_until(raw, slot, [](int t) { return t == -1; }); }
__device__ __forceinline__ void slot_list_bounded(uint2 raw, int nb, int slot[kMaxPtsBlocks])
{
    slots_until(raw, slot, [nb](int t) { return t < 0 || t >= nb; });
}
__device__ __forceinline__ bool slots_list_tile(const int slot[kMaxPtsBlocks], int b)
{
    bool mine = false;
#pragma unroll
    for (int k = 0; k < kMaxPtsBlocks; ++k) mine |= slot[k] == b;
    return mine;
}

// ---- position.  wp = o + z d is the sample in the world; pt = (wp - corner) / size its position in a tile, [0,1] inside.
// Without contraction `o + z * d` is one rounded product and one rounded sum wherever it is written, so a kernel that keeps wp
// (pts_normals) and one that writes the sum out per use hold the same value: every kernel calls world_point with (o, z, d).
__device__ __forceinline__ void world_point(const float o[3], float z, const float d[3], float wp[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) wp[c] = o[c] + z * d[c];
}
// corner, size: the tile's three floats (rows of Tiles::corners / sizes, or a wave-uniform copy of them)
__device__ __forceinline__ float tile_coord(float wp, float corner, float size) { return (wp - corner) / size; }
__device__ __forceinline__ void tile_point(const float wp[3], const float *corner, const float *size, float pt[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) pt[c] = tile_coord(wp[c], corner[c], size[c]);
}

// ---- blend weight of a listed tile: the distances to the nearer x and z faces, in world units (:523-541; it counts whether or
// not the sample's cell is occupied)
__device__ __forceinline__ float tile_weight(const float pt[3], const float *size)
{
    float dis[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dis[c] = (0.5f - fabsf(pt[c] - 0.5f)) * size[c];
    return xz_weight(dis[0], dis[2]);
}

// ---- the sample's cell of tile b's occupancy grid (clamped: always a cell of b), as an index into Tiles::occ.  A kernel that
// reads the occupancy of some lanes only calls tile_cell for all of them: for a wave-uniform b its loads are scalar and
// loop-invariant, and stay so only outside the lanes' branch.
__device__ __forceinline__ int64_t tile_cell(const Tiles &t, int b, const float pt[3])
{
    int loc[3];
    const int l2d[3] = { t.log2dim[3 * b], t.log2dim[3 * b + 1], t.log2dim[3 * b + 2] };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int r = 1 << l2d[c];
        const int cc = (int)(pt[c] * (float)r);
        loc[c] = cc < 0 ? 0 : (cc > r - 1 ? r - 1 : cc);
    }
    return t.grid_starts[b] + cell_offset(loc, l2d[1], l2d[2]);
}

// the sum of the blend weights of every listed tile; w_b = tile b's (0 when the sample does not list b)
__device__ __forceinline__ float slots_weight(const Tiles &t, const int slot[kMaxPtsBlocks], int b, const float wp[3], float &w_b)
{
    float weight = 0.0f;
    w_b = 0.0f;
#pragma unroll
    for (int k = 0; k < kMaxPtsBlocks; ++k) {
        const int bk = slot[k];
        if (bk == -1) continue;
        float pt[3];
        tile_point(wp, t.corners + 3 * bk, t.sizes + 3 * bk, pt);
        const float w = tile_weight(pt, t.sizes + 3 * bk);
        weight += w;
        if (bk == b) w_b = w;
    }
    return weight;
}
__device__ __forceinline__ float inv_weight(float weight) { return weight > 0 ? 1.0f / weight : 1.0f; }

// ---- table coordinate in [0,1].  Foreground: the tile is the middle half of the 2x box (:548)
__device__ __forceinline__ float fg_coord(float pt) { return pt / 2.0f + 0.25f; }
__device__ __forceinline__ void fg_p01(const float pt[3], float p01[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) p01[c] = fg_coord(pt[c]);
}
// A foreground sample at the step of tile b (cb, sb = b's corner and size): its table coordinate, b's blend weight and the sum of
// all (:523-541), and whether it runs b's decoder -- it lists b (`mine`) in an occupied cell
__device__ __forceinline__ bool fg_sample(const Tiles &t, const int slot[kMaxPtsBlocks], int b, const float *cb, const float *sb,
                                          const float wp[3], bool mine, float p01[3], float &w_b, float &weight)
{
    weight = slots_weight(t, slot, b, wp, w_b);
    float pt[3];
    tile_point(wp, cb, sb, pt);
    fg_p01(pt, p01);
    const int64_t cell = tile_cell(t, b, pt);
    return mine && t.occ[cell] != 0;
}
// Background: L-infinity contraction of the 2x-box coordinates (:1056-1096), then [-2,2] -> [0,1]
__device__ __forceinline__ void bg_p01(const float wp[3], const float *corner, const float *size, float p01[3])
{
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = 2.0f * (wp[c] - corner[c]) / size[c] - 1.0f;
    const float linf = fmaxf(fabsf(q[0]), fmaxf(fabsf(q[1]), fabsf(q[2])));
    const float ratio = (2.0f - 1.0f / linf) / linf;
#pragma unroll
    for (int c = 0; c < 3; ++c) p01[c] = (q[c] * ratio + 2.0f) / 4.0f;
}

// ---- output stage of the chunk-major kernels.  Out = the decoder's SampleOut (sigma, dif, spec, tint); pa = the opacity
// 1 - exp(-sigma delta); dif, spec, alpha = the op's three output arrays ([.,3], [.,3], [.]).
// Tile b's share of a blended sample, w_b pa colour / sum_k w_k, as v = { dif[3], spec[3], alpha }: add_fg adds it; the t16 kernel's
// "first listed tile writes, later tiles add" stage takes it from here
template <typename Out>
__device__ __forceinline__ void fg_values(float w_b, float pa, float inv, const Out &so, float v[7])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = (w_b * pa * so.dif[c]) * inv;
        v[3 + c] = (w_b * pa * (so.tint[c] * so.spec[c])) * inv;
    }
    v[6] = (w_b * pa) * inv;
}
__device__ __forceinline__ void zero_sample(float *dif, float *spec, float *alpha, size_t e)
{
    alpha[e] = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dif[3 * e + c] = 0.0f;
        spec[3 * e + c] = 0.0f;
    }
}
template <typename Out>
__device__ __forceinline__ void store_bg(float *dif, float *spec, float *alpha, size_t e, float pa, const Out &so)
{
    alpha[e] = pa;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dif[3 * e + c] = pa * so.dif[c];
        spec[3 * e + c] = pa * (so.tint[c] * so.spec[c]);
    }
}
// into arrays that hold zeros or the shares of the tiles before b (one workgroup owns a sample and its tile steps are sequential)
template <typename Out>
__device__ __forceinline__ void add_fg(float *dif, float *spec, float *alpha, size_t e, float w_b, float pa, float inv, const Out &so)
{
    float v[7];
    fg_values(w_b, pa, inv, so, v);
    alpha[e] += v[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dif[3 * e + c] += v[c];
        spec[3 * e + c] += v[3 + c];
    }
}

}  // namespace
