// render_time_common.h -- what the two render-time units share (render_time.hip: the per-ray ops; render_infer.hip: the
// inference hot loop): the tile set, the layouts of the per-sample arrays and the entry points' argument checks.
#pragma once
#include "common.h"

namespace {   // (unnamed, in both units: the kernels' mangled names carry it)

constexpr int kMaxPtsBlocks = 4;          // MAX_PTS_BLOCKS, rendering_kernel.cu:25
constexpr float kInf = 10000000.0f;       // INF_INTERSECTION, :26

struct Tiles {
    const float *corners, *sizes;         // [nb,3]
    const uint8_t *occ;                   // concatenated bool grids
    const int64_t *grid_starts;           // [nb]
    const int32_t *log2dim;               // [nb,3]
    int nb;
};

__device__ __forceinline__ uint32_t cell_offset(const int c[3], int ly, int lz)
{
    return ((uint32_t)c[0] << (ly + lz)) | ((uint32_t)c[1] << lz) | (uint32_t)c[2];
}

// Layout of the per-sample arrays of the render-time ops (scanerf_hip.h `sample_major`): element (ray i, sample s) of B x S
//   0  [B][S]          the reference's
//   1  [S][B]          sample-major
//   2  [B/32][S][32]   ray blocks: 32 neighbouring rays side by side, their samples in order (B a multiple of 32)
// In 1 and 2 a wave's 32 samples are one depth index of 32 neighbouring rays (neighbouring pixels share their cells down to
// the fine levels: the gathers of a wave fall on a few lines); in 2 consecutive groups of a wave also walk ALONG those rays, and
// the chip is spread over all depths at any time (in 1 every CU works on the same depth slab and the same few lines of the
// coarse levels -- measured 1.5-2x slower than 0).
__device__ __forceinline__ size_t pt_index(int i, int s, int B, int S, int lay)
{
    return lay == 0 ? (size_t)i * S + s : lay == 1 ? (size_t)s * B + i : ((size_t)(i >> 5) * S + s) * 32 + (i & 31);
}
__device__ __forceinline__ void pt_decompose(uint32_t e, uint32_t B, uint32_t S, int lay, int &i, int &s)
{
    if (lay == 0) { i = (int)(e / S); s = (int)(e - (uint32_t)i * S); }
    else if (lay == 1) { s = (int)(e / B); i = (int)(e - (uint32_t)s * B); }
    else { const uint32_t g = e >> 5, rb = g / S; s = (int)(g - rb * S); i = (int)(rb * 32 + (e & 31u)); }
}
__device__ __forceinline__ size_t pt_sample_stride(int B, int lay) { return lay == 0 ? 1 : lay == 1 ? (size_t)B : 32; }

// xz-distance blend weight (rendering_kernel.cu:523-537, :1335-1351)
__device__ __forceinline__ float xz_weight(float dx, float dz)
{
    if (dx != 0 && dz != 0) return dx * dz;
    if (dx != 0) return dx;
    if (dz != 0) return dz;
    return 0.0f;
}

inline Tiles make_tiles(const float *corners, const float *sizes, const uint8_t *occ, const int64_t *gst, const int32_t *l2d, int nb)
{
    Tiles t;
    t.corners = corners; t.sizes = sizes; t.occ = occ; t.grid_starts = gst; t.log2dim = l2d; t.nb = nb;
    return t;
}

}  // namespace

// ---- argument checks of the C entry points (`name` = the op's name in the error text)
#define RT_REQ(cond, name) SCANERF_REQUIRE(cond, "%s: bad argument (null pointer or negative size)", name)
// the layout argument of every entry that takes one (pt_index above; any SCANERF_* flag bits already taken out)
#define RT_REQ_LAYOUT(sample_major, B, name)                                                                   \
    SCANERF_REQUIRE((sample_major) >= 0 && (sample_major) <= 2 && ((sample_major) != 2 || (B) % 32 == 0),      \
                    "%s: sample_major=%d (0, 1, or 2 with B a multiple of 32; B=%d)", name, sample_major, B)
