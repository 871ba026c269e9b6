// render_infer.hip -- pts_inference / bg_pts_inference_v2, the hot loop of the multi-tile novel-view render (gfx950), in its
// three arithmetic forms.  The per-ray ops around it are render_time.hip; what both units use is render_time_common.h.
// The per-sample tile geometry -- slot list, position in a tile, blend weight, cell and occupancy, table coordinate, output
// stage -- has ONE definition, render_infer_device.h (shared with pts_normals, render_normals_tiles.hip); the kernels here are
// what differs between them: how samples are grouped, where the decoder's operands come from, what is in flight when.
//
// Reference behaviour: hashgrid/src/rendering_kernel.cu:467-621 and :1012-1171.  Built with -ffp-contract=off, as render_time.hip.
//
// The reference runs the whole 13 994-MAC decoder serially in one thread per sample, weights from global memory.  Here a wave
// takes 32 consecutive samples and runs the decoder on the matrix cores.  Default: chunk-major with the split-f16 decoder image
// of each tile a chunk touches staged in LDS (k_pts_inference_t16, k_pts_inference_chunks: the rate of the training forward --
// table gathers bound it).  Kept for comparison (SCANERF_INFER_F32 in sample_major): a single pass on the fp32 matrix pipe that
// reads the packed image of whichever tile the samples reference through L2 and loops over the distinct tiles of a wave
// (k_pts_inference: 1.5e9 samples/s).
#include <hip/hip_fp16.h>

#include <stdlib.h>

#include <type_traits>

#include "render_device.h"
#define H3_OPAQUE_ADDR 1  // (render_h3.h: one base register for the decoder image reads; measured clean on this kernel, tools/render_soak.py)
#include "render_h3.h"
#include "render_t16.h"
#include "render_infer_device.h"

using namespace scanerf;

namespace {

struct InferArgs {
    const float *rays_o, *rays_d, *z_vals, *dists;
    const int16_t *block_idxs;    // fg: [B,S,4]; bg: [B,4] (+ step)
    const void *tables;           // [nb,16,T,2] f16
    const float *images;          // [nb, PK_TOTAL] packed decoders (weight_feature == 1)
    const int32_t *res;           // [nb,16,3]
    Tiles t;
    float *out_dif, *out_spec, *out_alpha;
    int T, B, S, step;
    int sm;   // layout of the per-sample arrays (pt_index)
    const uint8_t *running;   // scanerf_pts_inference_tracing: the slot lists are derived in the kernel from the running mask,
    const float *inter;       // the samples' depths and the rays' [nb] (near, far) intervals (= prepare_points, :391-449)
    int skip_unsampled;       // (tracing only) rays whose first depth is -1 hold no sample: their outputs are left unwritten
};


// ---- rendering_kernel.cu:467-621 (BG == false) and :1012-1171 (BG == true) -------------------------
template <bool BG>
__global__ void __launch_bounds__(256, 2) k_pts_inference(InferArgs a)
{
    const int lane = threadIdx.x & 63, sl = lane & 31, h = lane >> 5;
    const int64_t total = (int64_t)a.B * a.S;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 32; base < total; base += nwaves * 32) {
        const int64_t e = base + sl;
        const bool in_range = e < total;
        const int64_t ec = in_range ? e : total - 1;
        const int i = (int)(ec / a.S), s = (int)(ec % a.S);
        float o[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = a.rays_o[3 * i + k];
            d[k] = a.rays_d[3 * i + k];
        }
        const float dnorm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const float z = a.z_vals[ec];
        float wp[3];
        world_point(o, z, d, wp);
        float delta;  // what multiplies sigma in alpha = 1 - exp(-sigma*delta)
        if (BG) delta = (s == a.S - 1) ? 10000000.0f : a.z_vals[ec + 1] - z;   // :1045-1047: raw depth step
        else delta = a.dists[ec] * dnorm;                                       // :557
        float dif[3] = { 0, 0, 0 }, spc[3] = { 0, 0, 0 }, alpha = 0.0f, weight = 0.0f;

        const int nslots = BG ? 1 : kMaxPtsBlocks;
        bool ended = !in_range;  // fg: the slot list stops at the first -1 (:499)
        for (int k = 0; k < nslots; ++k) {
            int b_lane = -1;
            if (!ended) b_lane = BG ? a.block_idxs[i * kMaxPtsBlocks + a.step] : a.block_idxs[ec * kMaxPtsBlocks + k];
            if (b_lane == -1) ended = true;
            unsigned long long pending = __ballot(b_lane != -1);
            while (pending) {
                const int leader = __ffsll((long long)pending) - 1;
                const int b = __shfl(b_lane, leader, 64);  // wave-uniform tile
                const bool mine = b_lane == b;
                pending &= ~__ballot(mine);
                // tile-space position, blend weight, occupancy
                float p01[3], w = 0.0f;
                bool run = mine;
                const float *cb = a.t.corners + 3 * b, *sb = a.t.sizes + 3 * b;
                if (BG) {
                    bg_p01(wp, cb, sb, p01);
                } else {
                    float pt[3];
                    tile_point(wp, cb, sb, pt);
                    fg_p01(pt, p01);
                    w = tile_weight(pt, sb);
                    const int64_t cell = tile_cell(a.t, b, pt);
                    if (mine) {
                        weight += w;
                        run = a.t.occ[cell] != 0;
                    }
                }
                if (!__any(run)) continue;  // wave-uniform
                v16f x;
                encode8_01<SCANERF_F16>((const char *)a.tables + (size_t)b * 16 * a.T * 4, a.res + (size_t)b * 48, a.T, h, p01,
                                        run, x);
                SampleOut so = decode_tile_dir(a.images + (size_t)b * WS_FLOATS, lane, x, d, dnorm, 0.0f);
                if (run) {
                    const float pa = 1.0f - expf(-1.0f * so.sigma * delta);
                    if (BG) {
                        alpha = pa;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            dif[c] = pa * so.dif[c];
                            spc[c] = pa * (so.tint[c] * so.spec[c]);
                        }
                    } else {
                        alpha += w * pa;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            dif[c] += w * pa * so.dif[c];
                            spc[c] += w * pa * (so.tint[c] * so.spec[c]);
                        }
                    }
                }
            }
        }
        if (!BG && weight > 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { dif[c] /= weight; spc[c] /= weight; }
            alpha /= weight;
        }
        // every sample is written: fg zeros when no tile applies (:569-571); bg rays without a tile at this blend step -- which
        // the reference leaves as its caller cleared them (:1032-1036, rendering.py:493-495) -- get their zeros here
        const bool wr = in_range && h == 0;
        if (wr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a.out_dif[3 * e + c] = dif[c];
                a.out_spec[3 * e + c] = spc[c];
            }
            a.out_alpha[e] = alpha;
        }
    }
}


// ---- pieces of the group loops of k_pts_inference_chunks (pipelined, and plain in the experiments build) ----------------------
// acc += w * (float)(low / high half of an f16 pair): one instruction instead of a conversion and an fma, the same value.  The
// result stays in acc's register, which ordinary instructions have written before (render_h3.h, h3_residual_lo: inline asm is
// invisible to the hazard recogniser, so it must not be handed a register that a matrix instruction in flight may own).
__device__ __forceinline__ float fma_mix_lo(uint32_t h2, float w, float acc)
{
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(h2), "v"(w));
    return acc;
}
__device__ __forceinline__ float fma_mix_hi(uint32_t h2, float w, float acc)
{
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(h2), "v"(w));
    return acc;
}

// what one 32-sample group reads from the per-sample arrays (loaded one group ahead of its use)
struct GroupIn {
    float z, aux;     // depth; fg: dists, bg: the next sample's depth
    uint32_t s0, s1;  // fg: the four 16-bit slots; bg: s0 = the ray's background tile at this blend step (sign-extended)
    uint32_t e;       // element index (clamped into range)
    int i;            // ray
    bool in_range, last;
};
// a group found to have samples in the staged tile: what its decoder and output stage needs
struct GroupPrep {
    uint32_t e;
    bool run;
};

// a foreground sample's four slots, packed
__device__ __forceinline__ uint2 load_slots(const InferArgs &a, uint32_t e)
{
    return *reinterpret_cast<const uint2 *>(a.block_idxs + (size_t)e * kMaxPtsBlocks);
}

template <bool BG>
__device__ __forceinline__ void group_load(const InferArgs &a, int64_t total, int64_t base, int sl, GroupIn &in)
{
    const int64_t e = base + sl;
    in.in_range = e < total;
    const uint32_t ec = (uint32_t)(in.in_range ? e : total - 1);
    int s;
    pt_decompose(ec, (uint32_t)a.B, (uint32_t)a.S, a.sm, in.i, s);
    in.e = ec;
    in.z = a.z_vals[ec];
    if (BG) {
        in.last = s == a.S - 1;
        in.aux = a.z_vals[in.last ? ec : ec + (uint32_t)pt_sample_stride(a.B, a.sm)];
        in.s0 = (uint32_t)(int)a.block_idxs[in.i * kMaxPtsBlocks + a.step];
        in.s1 = 0;
    } else {
        in.last = false;
        in.aux = a.dists[ec];
        const uint2 raw = load_slots(a, ec);
        in.s0 = raw.x;
        in.s1 = raw.y;
    }
}

// What a loaded group needs for the step of tile b (rendering_kernel.cu:499-557 / :1040-1060): the table coordinate p01 and
// st = { direction[3], depth step, blend weight of b, 1 / sum of the blend weights }.  Returns whether any sample of the group
// runs the decoder of tile b (wave-uniform).
template <bool BG>
__device__ __forceinline__ bool group_prep(const InferArgs &a, int b, const float cb[3], const float sb[3], const GroupIn &in,
                                           GroupPrep &P, float p01[3], float st[6])
{
    int slot[kMaxPtsBlocks] = { -1, -1, -1, -1 };
    bool mine = false;
    if (BG) {
        mine = in.in_range && (int)in.s0 == b;
    } else if (in.in_range) {
        slot_list(make_uint2(in.s0, in.s1), slot);
        mine = slots_list_tile(slot, b);
    }
    P.run = false;
    if (!__any(mine)) return false;
    float o[3], d[3], wp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = a.rays_o[3 * in.i + k];
        d[k] = a.rays_d[3 * in.i + k];
    }
    world_point(o, in.z, d, wp);
    float delta, w_b = 0.0f, weight = 0.0f;
    bool run = mine;
    if (BG) {
        delta = in.last ? 10000000.0f : in.aux - in.z;  // :1045-1047: raw depth step
        bg_p01(wp, cb, sb, p01);
    } else {
        delta = in.aux * sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);  // :557
        run = fg_sample(a.t, slot, b, cb, sb, wp, mine, p01, w_b, weight);
    }
    P.e = in.e;
    P.run = run;
    st[0] = d[0]; st[1] = d[1]; st[2] = d[2];
    st[3] = delta; st[4] = w_b; st[5] = inv_weight(weight);
    return __any(run);
}

// the output stage of a decoded sample of the 32-sample-tile kernel: bg writes, fg adds tile b's share
template <bool BG>
__device__ __forceinline__ void group_store(const InferArgs &a, uint32_t e, const SampleOut &so, float delta, float w_b, float inv)
{
    const float pa = 1.0f - expf(-1.0f * so.sigma * delta);
    if (BG) store_bg(a.out_dif, a.out_spec, a.out_alpha, e, pa, so);
    else add_fg(a.out_dif, a.out_spec, a.out_alpha, e, w_b, pa, inv, so);
}

// Step 1 of both chunk-major kernels: the tiles that the samples of this wave's NG groups of W list, OR-ed into tileset[0..1]
// (bit t = tile t); all slot loads of the wave in flight together.  W = 32: the wave's upper half sits out.
// slots(e, unsampled) -> a foreground sample's packed slot list (load_slots, or tracing_slots).
// A background sample without a tile at this blend step gets its zeros here (the caller need not clear them).  ZERO: so does a
// foreground sample that lists no tile (:569-571), unless `slots` calls it unsampled -- the 16-sample-tile kernel, where every
// other sample is WRITTEN by the step of its first listed tile and added to by the later ones, so that the caller's arrays need
// no clearing pass (7.4 GB per launch at 1920x1080x128); the 32-sample-tile kernel adds into arrays the host cleared.
template <bool BG, int W, int NG, bool ZERO, typename Slots>
__device__ __forceinline__ void chunk_tileset(const InferArgs &a, int64_t wbase, int64_t total, int lane, uint32_t *tileset, Slots slots)
{
    uint32_t mlo = 0, mhi = 0;
    auto mark = [&](int t) {
        if (t >= 0) {
            if (t < 32) mlo |= 1u << t;
            else mhi |= 1u << (t - 32);
        }
    };
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int64_t e = wbase + g * W + (lane & (W - 1));
        if (e >= total || lane >= W) continue;
        const uint32_t e32 = (uint32_t)e;
        if (BG) {
            int ri, rs;
            pt_decompose(e32, (uint32_t)a.B, (uint32_t)a.S, a.sm, ri, rs);
            const int tb = a.block_idxs[ri * kMaxPtsBlocks + a.step];
            mark(tb);
            if (tb < 0) zero_sample(a.out_dif, a.out_spec, a.out_alpha, e);
        } else {
            bool unsampled = false;
            int slot[kMaxPtsBlocks];
            slots_unpack(slots(e32, unsampled), slot);
            // (slot_list's rule -- the list ends at the first -1 -- as nested branches: this loop is unrolled NG times, and
            // rewriting the list's tail first costs ~12 instructions per group)
            mark(slot[0]);
            if (slot[0] != -1) { mark(slot[1]); if (slot[1] != -1) { mark(slot[2]); if (slot[2] != -1) mark(slot[3]); } }
            if (ZERO && slot[0] == -1 && !unsampled) zero_sample(a.out_dif, a.out_spec, a.out_alpha, e);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mlo |= __shfl_xor(mlo, off, 64);
        mhi |= __shfl_xor(mhi, off, 64);
    }
    if (lane == 0) {
        if (mlo) atomicOr(&tileset[0], mlo);
        if (mhi) atomicOr(&tileset[1], mhi);
    }
}

// First half of encode8_01<F16, 8, STRAIGHT>: the 64 corner loads of a group go out (raw f16 pairs; uniform level base + a
// 32-bit lane offset) and the interpolation offsets are parked in LDS; nothing here waits for memory.  Level by level (fenced),
// so that only one level's addresses are live beside the 64 destinations.
__device__ __forceinline__ void gather_issue(const char *table, const float *rs, int T, int h, const float p01[3],
                                             uint32_t raw[64], float (*tp)[64], int lane)
{
    const uint32_t mask = (uint32_t)T - 1u, hoff = (uint32_t)(2 * h) * (uint32_t)T;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int lu = 4 * (j >> 1) + (j & 1);  // level lu + 2h
        int bc[3];
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float v = p01[k] * rs[3 * lu + k];  // rs = (float)(res - 1) of this half's levels (staged in LDS with the tile's image)
                bc[k] = (int)v;
                tp[3 * j + k][lane] = v - (float)bc[k];
            }
        }
        uint32_t idx[8];
        corner_indices(idx, bc[0], bc[1], bc[2], mask);
        const char *base = table + (size_t)lu * T * 4;
#pragma unroll
        for (int c = 0; c < 8; ++c) raw[8 * j + c] = *reinterpret_cast<const uint32_t *>(base + (size_t)((hoff + idx[c]) * 4u));
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Second half: trilinear interpolation of the loaded corners (same sums, in the same order, as encode8_01)
__device__ __forceinline__ void gather_finish(const uint32_t raw[64], float (*tp)[64], int lane, v16f &x)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float w[8];
        trilinear_weights(w, tp[3 * j][lane], tp[3 * j + 1][lane], tp[3 * j + 2][lane]);
        float ax = 0.0f, ay = 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            ax = fma_mix_lo(raw[8 * j + c], w[c], ax);
            ay = fma_mix_hi(raw[8 * j + c], w[c], ay);
        }
        x[2 * j] = ax;  // (lanes without a live sample decode whatever their valid-address loads returned; nothing of theirs is written)
        x[2 * j + 1] = ay;
    }
}

// ---- pts_inference / bg_pts_inference_v2, chunk-major with the tile's decoder in LDS (default) ---------------------------
// The kernel above reads every MFMA operand of whichever tile a sample references from global memory and multiplies on
// the f32 matrix pipe (1.5e9 samples/s).  Here a workgroup takes a chunk of 64 consecutive 32-sample groups (16 rays at
// 128 samples), finds the set of tiles its samples list (one 8-byte slot load per lane and group), and for each tile of the
// set in ascending order stages that tile's split-f16 decoder image (render_h3.h, the arithmetic of the training kernels;
// 70 KB, from L2) in LDS and runs the groups that list it.  Neighbouring rays see the same one or two tiles, so a chunk
// stages one or two images for 2048 samples; the cost does not grow with the number of tiles of the scene (a first version
// made one launch per tile: every pass re-read all slot lists, ~1 ms per tile the view does not even see).  Samples in
// the overlap of several tiles are blended across the chunk's tile steps: each adds w_b * pa * colour / sum_k w_k into the
// (zero-filled) outputs; a sample belongs to one workgroup and the steps are sequential, so the read-modify-write is
// race-free and its order (ascending tile index) is fixed.
// 8 waves share one staged image (two per SIMD; with 4, the 104 KB image left one wave per SIMD and the decoder's dependent
// MFMA chains exposed: 3.3e9 samples/s whatever the gathers did)
constexpr int kChunkThreads = 512, kChunkWaves = kChunkThreads / 64, kChunkWaveGroups = 16;
constexpr int RT_GATHER_BATCH = 8;      // encode8_01 of the group loop without the pipeline: gathers in flight per batch,
constexpr bool RT_STRAIGHT = true;      // its straight-line form
// PIPE: the software-pipelined group loop (two waves per SIMD by its 142 KB of LDS); without it (SCANERF_RENDER_PIPE=0 in the
// experiments build) the plain loop, the same bits
template <bool BG, bool PIPE>
__global__ void __launch_bounds__(kChunkThreads, 1) k_pts_inference_chunks(InferArgs a)
{
    // One block of LDS, the decoder image first: its reads then are `lane base + 16-bit immediate` (with the image behind the
    // other arrays every read past 64 KB took an address register of its own, ~25 live across the group loop).
    // PIPE: tpark = interpolation offsets of the group whose gathers are in flight; ppark = direction, depth step and blend
    // weights of the two groups in the pipeline; rscale = (float)(res - 1) of the staged tile's 16 levels
    constexpr int kImg = (H3_BYTES + 15) & ~15, kTp = PIPE ? kChunkWaves * 24 * 64 * 4 : 0, kPp = PIPE ? kChunkWaves * 2 * 6 * 64 * 4 : 0;
    __shared__ __attribute__((aligned(16))) char smem[kImg + kTp + kPp + 48 * 4 + 8];
    char *const lds = smem;
    float (*const tpark)[24][64] = reinterpret_cast<float (*)[24][64]>(smem + kImg);
    float (*const ppark)[2][6][64] = reinterpret_cast<float (*)[2][6][64]>(smem + kImg + kTp);
    float *const rscale = reinterpret_cast<float *>(smem + kImg + kTp + kPp);
    uint32_t *const tileset = reinterpret_cast<uint32_t *>(smem + kImg + kTp + kPp + 48 * 4);
    const int lane = threadIdx.x & 63, sl = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    const int64_t total = (int64_t)a.B * a.S;
    constexpr int kWaveGroups = kChunkWaveGroups, kChunkGroups = kChunkWaves * kWaveGroups;
    const int64_t ngroups = (total + 31) / 32, nchunks = (ngroups + kChunkGroups - 1) / kChunkGroups;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (threadIdx.x < 2) tileset[threadIdx.x] = 0;
        __syncthreads();  // (also: the previous chunk's last tile step is complete)
        const int64_t wbase = (chunk * kChunkGroups + (int64_t)wave * kWaveGroups) * 32;
        // 1. the tiles this chunk's samples list
        chunk_tileset<BG, 32, kWaveGroups, false>(a, wbase, total, lane, tileset, [&](uint32_t e, bool &) { return load_slots(a, e); });
        __syncthreads();
        uint64_t todo = (uint64_t)tileset[0] | ((uint64_t)tileset[1] << 32);
      while (todo) {  // 2. one step per listed tile, ascending
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        __syncthreads();  // every wave is done with the previous image
        {
            const float4 *src = reinterpret_cast<const float4 *>(a.images + (size_t)b * WS_FLOATS + PK_TOTAL);
            float4 *dst = reinterpret_cast<float4 *>(lds);
            for (int i = threadIdx.x; i < H3_BYTES / 16; i += kChunkThreads) dst[i] = src[i];
            if (PIPE && threadIdx.x < 48) rscale[threadIdx.x] = (float)(a.res[(size_t)b * 48 + threadIdx.x] - 1);
        }
        __syncthreads();
        float cb[3], sb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cb[c] = a.t.corners[3 * b + c];
            sb[c] = a.t.sizes[3 * b + c];
        }
        // the wave's groups of this chunk (a ragged last one included)
        const int64_t rem = total - wbase;
        const int ng = rem <= 0 ? 0 : (int)(rem >= (int64_t)kWaveGroups * 32 ? kWaveGroups : (rem + 31) / 32);
        const char *table = (const char *)a.tables + (size_t)b * 16 * a.T * 4;
      if constexpr (PIPE) {
        // Software pipeline over the wave's groups that run this tile's decoder: while group g is decoded, the 64 corner
        // loads of the next running group and the per-sample inputs of the group after it are in flight (the kernel is bound
        // by the round trips of these loads, not by their number -- DESIGN.md 4.8).
        int rso = 6 * h;  // (opaque, or every rscale address becomes its own lane-dependent register instead of base + immediate)
        asm volatile("" : "+v"(rso));
        const float *rsh = rscale + rso;
        GroupIn in;
        GroupPrep cur, nxt;
        uint32_t raw[64];
        float p01[3];
        int g_in = 0, slot_cur = 0;
        if (ng > 0) group_load<BG>(a, total, wbase, sl, in);
        auto advance = [&](GroupPrep &P, int sl_) -> bool {  // the next group with samples to decode; keeps one group of inputs ahead
            while (g_in < ng) {
                // (direction, depth step, blend weight and 1/sum of weights wait in LDS for the output stage -- registers the
                // compiler would otherwise spill to scratch, whose reloads wait behind the gathers in flight)
                float st[6];
                const bool r = group_prep<BG>(a, b, cb, sb, in, P, p01, st);
                if (r) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) ppark[wave][sl_][k][lane] = st[k];
                }
                ++g_in;
                if (g_in < ng) group_load<BG>(a, total, wbase + (int64_t)g_in * 32, sl, in);
                if (r) return true;
            }
            return false;
        };
        bool have = advance(cur, 0);
        if (have) gather_issue(table, rsh, a.T, h, p01, raw, tpark[wave], lane);
        while (have) {
            v16f x;
            gather_finish(raw, tpark[wave], lane, x);
            __builtin_amdgcn_sched_barrier(0);  // the next group's loads go out after this group's corners are consumed ...
            const bool more = advance(nxt, slot_cur ^ 1);
            if (more) gather_issue(table, rsh, a.T, h, p01, raw, tpark[wave], lane);
            __builtin_amdgcn_sched_barrier(0);  // ... and before its decoder starts
            float (*pk)[64] = ppark[wave][slot_cur];
            v16f dinit[2];
            {
                const float d[3] = { pk[0][lane], pk[1][lane], pk[2][lane] };
                const float dnorm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                float sh[16];
                ray_sh(d, dnorm, sh, 0.0f);
                h3_dinit(lds, lane, sh, dinit);
            }
            const SampleOut so = decode_tile_h3(lds, lane, x, dinit);
            if (cur.run && h == 0) group_store<BG>(a, cur.e, so, pk[3][lane], pk[4][lane], pk[5][lane]);
            cur = nxt;
            slot_cur ^= 1;
            have = more;
        }
      } else {
        // the same steps one group at a time: nothing in flight across the decoder
        GroupIn in;
        GroupPrep cur;
        float p01[3], st[6];
#pragma unroll 1
        for (int g = 0; g < ng; ++g) {
            group_load<BG>(a, total, wbase + (int64_t)g * 32, sl, in);
            if (!group_prep<BG>(a, b, cb, sb, in, cur, p01, st)) continue;  // wave-uniform: nothing of this group is occupied (the outputs stay as they are)
            v16f x;
            encode8_01<SCANERF_F16, RT_GATHER_BATCH, RT_STRAIGHT>(table, a.res + (size_t)b * 48, a.T, h, p01, cur.run, x);
            const float d[3] = { st[0], st[1], st[2] };
            const SampleOut so = decode_tile_h3<true>(lds, lane, x, nullptr, d, 0.0f);
            if (cur.run && h == 0) group_store<BG>(a, cur.e, so, st[3], st[4], st[5]);
        }
      }
      }
    }
}

// ---- the same chunk-major kernel on 16-SAMPLE tiles at four waves per SIMD (default) ------------------------------------------
// k_pts_inference_chunks above runs two waves per SIMD: ~250 registers (64 gather destinations of the software pipeline beside the
// 32-sample decoder) and 142 KB of LDS per workgroup, and its decoder's dependent MFMA -> activation -> split chains have one
// other wave to hide behind (de-phasing the two waves changes nothing: profiles/r05_render_pmc.txt).  Here the decoder is
// decode_tile_s16 (render_t16.h: v_mfma_f32_16x16x32_f16 on the t16s image, the arithmetic of the training backward's recompute,
// ~95 registers) and a lane gathers 4 levels instead of 8 (32 destinations, dead before the decoder starts): <= 128 registers,
// no software pipeline, 77 KB of LDS -> two workgroups = 16 waves per CU, and the gathers of one wave wait behind the matrix and
// vector work of three others.  A wave takes 64 consecutive samples at a time: lane l prepares sample l (position, blend weights,
// occupancy), then each of the four 16-sample tiles with a live sample is decoded with lane (c, q) = sample 16 t + c, quarter q
// (inputs by ds_bpermute from the preparing lane).
constexpr int T16_WAVE_GROUPS = 8;   // 8 x 64 = the 512 samples per wave and chunk of the kernel above
constexpr int kT16Threads = 512, kT16Waves = kT16Threads / 64, kT16WaveGroups = T16_WAVE_GROUPS;
constexpr int kT16ChunkGroups32 = kT16Waves * kT16WaveGroups * 2;   // a chunk in 32-sample groups

// lane (c, q): levels l0 + {0, 1, 4, 5}, l0 = 8 (q & 1) + 2 (q >> 1)  =  decoder inputs 2 l0 + {0..3} (xa) and + 8 (xb)
__device__ __forceinline__ void encode4_t16(const char *table, const float *rs, int T, int q, const float p01[3], v4f &xa, v4f &xb)
{
    const uint32_t mask = (uint32_t)T - 1u, l0 = (uint32_t)(8 * (q & 1) + 2 * (q >> 1)), hoff = l0 * (uint32_t)T;
    uint32_t raw[32];
    float tf[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int lu = (k & 1) + 4 * (k >> 1);  // level l0 + lu
        int bc[3];
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float v = p01[j] * rs[3 * lu + j];  // rs = (float)(res - 1) from level l0 on (staged in LDS with the tile's image)
                bc[j] = (int)v;
                tf[k][j] = __builtin_amdgcn_fractf(v);    // = v - (float)(int)v for the v >= 0 of a live sample, one instruction
            }
        }
        uint32_t idx[8];
        corner_indices(idx, bc[0], bc[1], bc[2], mask);
        const char *base = table + (size_t)lu * T * 4;
#pragma unroll
        for (int c = 0; c < 8; ++c) raw[8 * k + c] = *reinterpret_cast<const uint32_t *>(base + (size_t)((hoff + idx[c]) * 4u));
    }
    float x[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float w[8];
        trilinear_weights(w, tf[k][0], tf[k][1], tf[k][2]);
        float ax = 0.0f, ay = 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            ax = fma_mix_lo(raw[8 * k + c], w[c], ax);
            ay = fma_mix_hi(raw[8 * k + c], w[c], ay);
        }
        x[2 * k] = ax;  // (lanes without a live sample decode whatever their valid-address loads returned; nothing of theirs is written)
        x[2 * k + 1] = ay;
    }
    xa = v4f{ x[0], x[1], x[2], x[3] };
    xb = v4f{ x[4], x[5], x[6], x[7] };
}

// the slot list of one sample -- what prepare_points (rendering_kernel.cu:391-449) would have stored for it: the first
// kMaxPtsBlocks tiles (ascending) whose (near, far) interval along the ray holds its depth; none for a stopped ray or an unset depth
__device__ __forceinline__ uint2 tracing_slots(const InferArgs &a, int i, float z)
{
    int sl[kMaxPtsBlocks] = { -1, -1, -1, -1 };
    if (a.running[i] && z != -1.0f) {
        const float2 *ci = reinterpret_cast<const float2 *>(a.inter) + (size_t)i * a.t.nb;
        int n = 0;
        for (int b = 0; b < a.t.nb; ++b) {
            const float2 bd = ci[b];
            const bool hit = z >= bd.x && z <= bd.y;
#pragma unroll
            for (int k = 0; k < kMaxPtsBlocks; ++k) sl[k] = hit && n == k ? b : sl[k];
            n += hit;
        }
    }
    return make_uint2(((uint32_t)sl[0] & 0xffffu) | ((uint32_t)sl[1] << 16), ((uint32_t)sl[2] & 0xffffu) | ((uint32_t)sl[3] << 16));
}

// SHT: the split SH operands of the chunk's rays wait in LDS (render_t16.h s16_sh_row), one row per ray of the chunk's contiguous
// ray range -- 32 rays for 4096 samples at S = 128 in the layouts 0 and 2 -- written once per chunk, read per tile; the host picks
// SHT when that range fits (t16_sh_rows_fit), otherwise every tile evaluates the harmonics of its 16 samples' directions.
constexpr int kShRows = (S16_BIAS - T16_FWD_BYTES) / 64 - 1;   // rows in the unused 12 KB of the image's footprint, less the row of zeros
__host__ __device__ inline void t16_chunk_rays(int64_t e0, int64_t e1, int B, int S, int sm, int &r0, int &r1)
{
    if (sm == 0) { r0 = (int)(e0 / S); r1 = (int)(e1 / S); }
    else if (sm == 2) { r0 = (int)((e0 >> 5) / S) * 32; r1 = (int)((e1 >> 5) / S) * 32 + 31; }
    else { r0 = 0; r1 = B - 1; }
    if (r1 > B - 1) r1 = B - 1;
}
inline bool t16_sh_rows_fit(int B, int S, int sm)
{
    constexpr int64_t kChunkSamples = kT16Waves * kT16WaveGroups * 64;
    if (sm == 1) return B <= kShRows;
    // the widest range any chunk can see: ceil(chunk / (samples per ray or ray block)) + 1 units
    const int64_t per = sm == 0 ? S : (int64_t)S * 32, units = (kChunkSamples + per - 1) / per + 1;
    return units * (sm == 0 ? 1 : 32) <= kShRows;
}
// TR (fg): no block_idxs array -- every use derives the sample's slot list (tracing_slots)
// FOLD: the images hold the activation constant in the three Gaussian layers (SCANERF_INFER_FOLDED; decode_tile_s16<.., FOLD>)
template <bool BG, bool SHT, bool TR = false, bool FOLD = false>
__global__ void __launch_bounds__(kT16Threads, 4) k_pts_inference_t16(InferArgs a)
{
    // the t16s image at its own offsets (decode_tile_s16 reads the forward sub-images and the f32 tail; the transposed narrow
    // sub-images between them are the backward's and are not staged: their 12 KB hold the chunk's SH rows)
    __shared__ __attribute__((aligned(16))) char smem[S16_BYTES + 48 * 4 + 8];
    char *const lds = smem;
    float *const rscale = reinterpret_cast<float *>(smem + S16_BYTES);
    uint32_t *const tileset = reinterpret_cast<uint32_t *>(smem + S16_BYTES + 48 * 4);
    char *const shrows = smem + T16_FWD_BYTES;
    const int lane = threadIdx.x & 63, c16 = lane & 15, q = lane >> 4, wave = threadIdx.x >> 6;
    const int64_t total = (int64_t)a.B * a.S;
    constexpr int kChunkSamples = kT16Waves * kT16WaveGroups * 64;

    const int64_t nchunks = (total + kChunkSamples - 1) / kChunkSamples;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (threadIdx.x < 2) tileset[threadIdx.x] = 0;
        __syncthreads();  // (also: the previous chunk's last tile step is complete)
        const int64_t wbase = chunk * kChunkSamples + (int64_t)wave * (kT16WaveGroups * 64);
        int r0 = 0;
        if constexpr (SHT) {   // the chunk's rays' SH operands (visible after the barriers below, before any tile step)
            int r1;
            const int64_t e0 = chunk * kChunkSamples, e1 = e0 + kChunkSamples - 1 < total ? e0 + kChunkSamples - 1 : total - 1;
            t16_chunk_rays(e0, e1, a.B, a.S, a.sm, r0, r1);
            const int nr = r1 - r0 + 1 < kShRows ? r1 - r0 + 1 : kShRows;
            for (int r = threadIdx.x; r <= nr; r += kT16Threads) {
                if (r < nr) {
                    const float d[3] = { a.rays_d[3 * (size_t)(r0 + r)], a.rays_d[3 * (size_t)(r0 + r) + 1], a.rays_d[3 * (size_t)(r0 + r) + 2] };
                    s16_sh_row(shrows + 64 * r, d, 0.0f);
                }
            }
            if (threadIdx.x < 16) reinterpret_cast<float *>(shrows + 64 * kShRows)[threadIdx.x] = 0.0f;   // the row of the lanes with q >= 2
        }
        // 1. the tiles this chunk's samples list; samples without a tile get their zeros here
        chunk_tileset<BG, 64, kT16WaveGroups, true>(a, wbase, total, lane, tileset, [&](uint32_t e, bool &unsampled) {
            if constexpr (TR) {
                int ri, rs;
                pt_decompose(e, (uint32_t)a.B, (uint32_t)a.S, a.sm, ri, rs);
                // (sample_points fills a ray's depths from index 0: a first depth of -1 = a ray without samples in this pass,
                // which the accumulation under the same flag does not read)
                unsampled = a.skip_unsampled && a.z_vals[pt_index(ri, 0, a.B, a.S, a.sm)] == -1.0f;
                return tracing_slots(a, ri, a.z_vals[e]);
            } else {
                return load_slots(a, e);
            }
        });
        __syncthreads();
        uint64_t todo = (uint64_t)tileset[0] | ((uint64_t)tileset[1] << 32);
        while (todo) {  // 2. one step per listed tile, ascending
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            __syncthreads();  // every wave is done with the previous image
            {
                const float4 *src = reinterpret_cast<const float4 *>(a.images + (size_t)b * WS_FLOATS + WS_S16);
                float4 *dst = reinterpret_cast<float4 *>(lds);
                for (int i = threadIdx.x; i < T16_FWD_BYTES / 16; i += kT16Threads) dst[i] = src[i];
                for (int i = S16_BIAS / 16 + threadIdx.x; i < S16_BYTES / 16; i += kT16Threads) dst[i] = src[i];
                if (threadIdx.x < 48) rscale[threadIdx.x] = (float)(a.res[(size_t)b * 48 + threadIdx.x] - 1);
            }
            __syncthreads();
            float cb[3], sb[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                cb[c] = a.t.corners[3 * b + c];
                sb[c] = a.t.sizes[3 * b + c];
            }
            const char *table = (const char *)a.tables + (size_t)b * 16 * a.T * 4;
            int rso = 3 * (8 * (q & 1) + 2 * (q >> 1));
            asm volatile("" : "+v"(rso));  // (opaque: one lane-dependent base register + immediates)
            const float *rsq = rscale + rso;
#pragma unroll 1
            for (int g = 0; g < kT16WaveGroups; ++g) {
                const int64_t base = wbase + g * 64;
                if (base >= total) break;
                const int64_t e = base + lane;
                const bool in_range = e < total;
                const uint32_t ec = (uint32_t)(in_range ? e : total - 1);
                // (32-bit index arithmetic: the host keeps B*S below 2^31 for this kernel)
                int i, s;
                pt_decompose(ec, (uint32_t)a.B, (uint32_t)a.S, a.sm, i, s);
                // does this sample list tile b?
                int slot[kMaxPtsBlocks] = { -1, -1, -1, -1 };
                bool mine = false, first = false;   // first: b is the sample's first listed tile (fg): this step writes, later ones add
                if (BG) {
                    mine = in_range && a.block_idxs[i * kMaxPtsBlocks + a.step] == b;
                } else if (in_range) {
                    slot_list(TR ? tracing_slots(a, i, a.z_vals[ec]) : load_slots(a, ec), slot);
                    first = slot[0] == b;
                    mine = slots_list_tile(slot, b);
                }
                if (!__any(mine)) continue;  // wave-uniform
                float o[3], d[3], wp[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    o[k] = a.rays_o[3 * i + k];
                    d[k] = a.rays_d[3 * i + k];
                }
                const float z = a.z_vals[ec];
                world_point(o, z, d, wp);
                float delta;
                if (BG) delta = (s == a.S - 1) ? 10000000.0f : a.z_vals[ec + (uint32_t)pt_sample_stride(a.B, a.sm)] - z;   // :1045-1047: raw depth step
                else delta = a.dists[ec] * sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);                               // :557
                float p01[3], w_b = 0.0f, weight = 0.0f;
                bool run = mine;
                if (BG) bg_p01(wp, cb, sb, p01);
                else run = fg_sample(a.t, slot, b, cb, sb, wp, mine, p01, w_b, weight);
                if (!BG && first && !run) zero_sample(a.out_dif, a.out_spec, a.out_alpha, ec);   // listed but not occupied here: the sample's value starts at zero
                const uint64_t rm = __ballot(run);
                if (!rm) continue;  // wave-uniform: nothing of this group is occupied
                const float inv = inv_weight(weight);
                int shrow = i - r0;   // this sample's ray's row (bytes); the host launches SHT only where every chunk's range fits
                shrow = 64 * (shrow < kShRows ? shrow : kShRows);
#pragma unroll 1
                for (int t = 0; t < 4; ++t) {
                    if (((rm >> (16 * t)) & 0xffffu) == 0) continue;  // wave-uniform
                    const int src = 16 * t + c16;
                    const float pt[3] = { __shfl(p01[0], src, 64), __shfl(p01[1], src, 64), __shfl(p01[2], src, 64) };
                    const bool act = (rm >> src) & 1u;
                    v4f xa, xb;
                    encode4_t16(table, rsq, a.T, q, pt, xa, xb);
                    const uint32_t es = (uint32_t)__shfl((int)ec, src, 64);
                    const float dl = __shfl(delta, src, 64);
                    // no live sample of the tile with a non-zero opacity -> the directional layers are skipped (decode_tile_s16)
                    // (the opacity is evaluated ONCE, here, from the sigma the decoder hands the gate, and kept for the outputs below:
                    // the same expression gave the same bits twice, at ~20 vector instructions per tile for the second one)
                    float pa_keep = 0.0f;
                    auto gate = [&](float sigma) {
                        // (folded form: the exponential on v_exp_f32, ~1 ulp of e -- 1.2e-7 absolute on the opacity instead of 6e-8 --
                        // in place of the library's expf, ~15 vector instructions per tile)
                        pa_keep = FOLD ? 1.0f - __builtin_amdgcn_exp2f(-1.4426950408889634f * (sigma * dl)) : 1.0f - expf(-1.0f * sigma * dl);
                        return __any(act && q == 0 && pa_keep != 0.0f) != 0;
                    };
                    SampleOut so;
                    if constexpr (SHT) {
                        const int row = __shfl(shrow, src, 64);
                        so = decode_tile_s16<true, decltype(gate), FOLD>(lds, lane, xa, xb, nullptr, 0.0f, shrows + (q < 2 ? row + 16 * q : 64 * kShRows), gate);
                    } else {
                        const float dd[3] = { __shfl(d[0], src, 64), __shfl(d[1], src, 64), __shfl(d[2], src, 64) };
                        so = decode_tile_s16<false, decltype(gate), FOLD>(lds, lane, xa, xb, dd, 0.0f, nullptr, gate);
                    }
                    if (BG) {
                        if (act && q == 0) store_bg(a.out_dif, a.out_spec, a.out_alpha, es, pa_keep, so);
                    } else {
                        const float wb = __shfl(w_b, src, 64), iv = __shfl(inv, src, 64);
                        const bool fst = __shfl((int)first, src, 64) != 0;
                        if (act && q == 0) {
                            float v[7];
                            fg_values(wb, pa_keep, iv, so, v);
                            // the first listed tile's step writes, later ones add (0 + x == x exactly: writing x where the
                            // cleared array held 0 gives the bits the += gave)
                            a.out_alpha[es] = (fst ? 0.0f : a.out_alpha[es]) + v[6];
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                a.out_dif[3 * (size_t)es + c] = (fst ? 0.0f : a.out_dif[3 * (size_t)es + c]) + v[c];
                                a.out_spec[3 * (size_t)es + c] = (fst ? 0.0f : a.out_spec[3 * (size_t)es + c]) + v[3 + c];
                            }
                        }
                    }
                }
            }
        }
    }
}

// Decoder arithmetic of the inference entry points: flag bits OR-ed into their `sample_major` argument (scanerf_hip.h):
// none = the 16-sample-tile kernel at four waves per SIMD (k_pts_inference_t16, default); SCANERF_INFER_H3 = the 32-sample-tile
// kernel at two (k_pts_inference_chunks, round 4's; comparison); SCANERF_INFER_F32 = the f32-MFMA single-pass kernel (exact f32;
// comparison / debugging).
// (+ 4: SCANERF_INFER_FOLDED, the images carry the activation constant: the 16-sample-tile kernel only)
inline int infer_arith_of(int &sample_major)
{
    const int ar = ((sample_major & SCANERF_INFER_F32) ? 2 : ((sample_major & SCANERF_INFER_H3) ? 1 : 0)) | ((sample_major & SCANERF_INFER_FOLDED) ? 4 : 0);
    sample_major &= ~(SCANERF_INFER_F32 | SCANERF_INFER_H3 | SCANERF_INFER_FOLDED);
    return ar;
}
inline bool render_single_pass(int64_t total, int nb, int arith)
{
    // the chunk-major kernel indexes samples in 32 bits and keeps a chunk's tile set in 64 bits
    return (arith & 3) == 2 || total >= ((int64_t)1 << 31) || nb > 64;
}
inline bool render_t16_tiles(int arith) { return (arith & 3) == 0; }

// a run-time bool as a template argument: f(std::true_type / std::false_type)
template <typename F>
inline void with_bool(bool v, F &&f)
{
    if (v) f(std::true_type{});
    else f(std::false_type{});
}
// TR is the caller's constant: the background has no tracing form, <true, *, true, *> is never instantiated
template <bool BG, bool TR>
inline void launch_t16(const InferArgs &a, dim3 grid, bool rows, bool fold, hipStream_t stream)
{
    with_bool(rows, [&](auto sht) {
        with_bool(fold, [&](auto fo) {
            hipLaunchKernelGGL((k_pts_inference_t16<BG, decltype(sht)::value, TR, decltype(fo)::value>), grid, dim3(kT16Threads), 0, stream, a);
        });
    });
}

template <bool BG>
inline void launch_chunks(const InferArgs &a, int64_t tiles32, int arith, hipStream_t stream)
{
    // One workgroup per chunk (up to 2^20).  A foreground chunk's cost is anything between nothing (rays that miss) and 4096 decoded
    // samples; with 8 workgroups per CU walking ~30 chunks each at a fixed stride the busiest workgroup had ~1.6x the mean share
    // of live chunks and the launch waited for it.  The dispatcher hands a finished workgroup's slot to the next chunk instead
    // (same box, ms per frame: 8 per CU 71.2, 64 per CU 69.2, one per chunk 67.5; the background launch gains its tail too).
    const int cap_cu = tune_int("SCANERF_RENDER_GRID_CAP", 0);   // workgroups per CU (comparison; experiments build)
    const int64_t cap = cap_cu > 0 ? (int64_t)kNumCU * cap_cu : (int64_t)1 << 20;
    auto nblocks = [&](int64_t per_chunk) {
        const int64_t nchunks = (tiles32 + per_chunk - 1) / per_chunk;
        return (int)(nchunks < cap ? nchunks : cap);
    };
    if (render_t16_tiles(arith)) {
        // SCANERF_RENDER_SH_ROWS=0 (experiments build): every tile evaluates its samples' harmonics (comparison; the same bits)
        const bool rows = t16_sh_rows_fit(a.B, a.S, a.sm) && tune_int("SCANERF_RENDER_SH_ROWS", 1) != 0;
        const dim3 grid(nblocks(kT16ChunkGroups32));
        const bool fold = (arith & 4) != 0;
        if constexpr (!BG) {
            if (a.running) {   // scanerf_pts_inference_tracing
                launch_t16<false, true>(a, grid, rows, fold, stream);
                return;
            }
        }
        launch_t16<BG, false>(a, grid, rows, fold, stream);
        return;
    }
    const dim3 grid(nblocks(kChunkWaves * kChunkWaveGroups));
#ifdef SCANERF_EXPERIMENTS
    // SCANERF_RENDER_PIPE=0 (experiments build): the group loop without the software pipeline (comparison; the two give the same bits)
    if (tune_int("SCANERF_RENDER_PIPE", 1) == 0) {
        hipLaunchKernelGGL((k_pts_inference_chunks<BG, false>), grid, dim3(kChunkThreads), 0, stream, a);
        return;
    }
#endif
    hipLaunchKernelGGL((k_pts_inference_chunks<BG, true>), grid, dim3(kChunkThreads), 0, stream, a);
}

// The one path of the three inference entries, from their filled arguments (a.sm and a.skip_unsampled are set here, from
// `sample_major` and its flag bits) to the launch.  `name` = the op's name in the error texts.
// images: [nb][scanerf_render_workspace_floats()] decoders packed by scanerf_pack_decoder with weight_feature == 1
constexpr int kTracingMaxTiles = 8;
template <bool BG>
int run_inference(InferArgs a, const char *name, int sample_major, hipStream_t stream)
{
    const int nb = a.t.nb;
    const int64_t total = (int64_t)a.B * a.S;
    a.skip_unsampled = 0;
    if constexpr (!BG) {
        a.skip_unsampled = a.running && (sample_major & SCANERF_SKIP_UNSAMPLED);   // (the tracing entry point only)
        sample_major &= ~SCANERF_SKIP_UNSAMPLED;
    }
    const int arith = infer_arith_of(sample_major);
    RT_REQ_LAYOUT(sample_major, a.B, name);
    a.sm = sample_major;
    SCANERF_REQUIRE(a.T >= 2 && (a.T & (a.T - 1)) == 0, "%s: T=%d must be a power of two", name, a.T);
    if (a.B == 0) return 0;
    RT_REQ(a.rays_o && a.rays_d && a.z_vals && a.tables && a.images && a.res && a.t.corners && a.t.sizes && a.out_dif && a.out_spec &&
               a.out_alpha && (BG ? a.block_idxs != nullptr
                                  : a.dists && (a.block_idxs || (a.running && a.inter)) && a.t.occ && a.t.grid_starts && a.t.log2dim),
           name);
    const bool single = render_single_pass(total, nb, arith), t16 = render_t16_tiles(arith);
    SCANERF_REQUIRE(!(arith & 4) || (t16 && !single),
                    "%s: SCANERF_INFER_FOLDED images are for the 16-sample-tile kernel only (nb <= 64, no SCANERF_INFER_H3 / _F32)", name);
    SCANERF_REQUIRE(!sample_major || !single, "%s: sample-major arrays need the chunk kernel", name);
    SCANERF_REQUIRE(!a.running || (t16 && !single && nb <= kTracingMaxTiles),
                    "pts_inference_tracing: needs the 16-sample-tile kernel and nb <= %d tiles (nb=%d); use prepare_points + pts_inference", kTracingMaxTiles, nb);
    const int64_t tiles32 = (total + 31) / 32;
    if (single) {
        const int blocks = (int)((tiles32 + 3) / 4 < kNumCU * 4 ? (tiles32 + 3) / 4 : kNumCU * 4);
        hipLaunchKernelGGL((k_pts_inference<BG>), dim3(blocks), dim3(256), 0, stream, a);
        return check_launch(name);
    }
    // every sample is written (zeros where no tile applies, :569-571).  The foreground's 32-sample-tile kernels add into cleared
    // arrays; the 16-sample-tile kernel writes each sample at its first listed tile's step and needs no clearing pass (the
    // background kernels write every sample themselves)
    if (!BG && (!t16 || tune_int("SCANERF_RENDER_CLEAR", 0) == 1)) {   // (=1: clear anyway: timing comparison, experiments build)
        const size_t n = (size_t)total;
        const hipError_t ce[3] = { hipMemsetAsync(a.out_dif, 0, n * 12, stream), hipMemsetAsync(a.out_spec, 0, n * 12, stream),
                                   hipMemsetAsync(a.out_alpha, 0, n * 4, stream) };
        for (hipError_t e : ce) SCANERF_REQUIRE(e == hipSuccess, "%s: clearing the outputs failed: %s", name, hipGetErrorString(e));
    }
    launch_chunks<BG>(a, tiles32, arith, stream);
    return check_launch(name);
}

// the two foreground entries: slot lists from block_idxs (prepare_points'), or derived in the kernel from running / inter
int fg_inference(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists, const int16_t *block_idxs,
                 const uint8_t *running, const float *inter, const void *tables_f16, const float *images, const int32_t *res,
                 const uint8_t *occ, const int64_t *grid_starts, const int32_t *log2dim, const float *corners, const float *sizes,
                 float *out_dif, float *out_spec, float *out_alpha, int B, int S, int T, int nb, int sample_major, scanerf_stream_t stream)
{
    RT_REQ(B >= 0 && S >= 1 && nb >= 1, "pts_inference");
    InferArgs a;
    a.rays_o = rays_o; a.rays_d = rays_d; a.z_vals = z_vals; a.dists = dists; a.block_idxs = block_idxs;
    a.tables = tables_f16; a.images = images; a.res = res; a.t = make_tiles(corners, sizes, occ, grid_starts, log2dim, nb);
    a.out_dif = out_dif; a.out_spec = out_spec; a.out_alpha = out_alpha; a.T = T; a.B = B; a.S = S; a.step = 0;
    a.running = running; a.inter = inter;
    return run_inference<false>(a, "pts_inference", sample_major, (hipStream_t)stream);
}

}  // namespace

// ---------------------------------------------------------------------------- C ABI
SCANERF_API int scanerf_pts_inference(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                                      const int16_t *block_idxs, const void *tables_f16, const float *images,
                                      const int32_t *res, const uint8_t *occ, const int64_t *grid_starts,
                                      const int32_t *log2dim, const float *corners, const float *sizes, float *out_dif,
                                      float *out_spec, float *out_alpha, int B, int S, int T, int nb, int sample_major,
                                      scanerf_stream_t stream)
{
    SCANERF_REQUIRE(block_idxs, "pts_inference: null block_idxs");
    return fg_inference(rays_o, rays_d, z_vals, dists, block_idxs, nullptr, nullptr, tables_f16, images, res, occ, grid_starts, log2dim,
                        corners, sizes, out_dif, out_spec, out_alpha, B, S, T, nb, sample_major, stream);
}

// prepare_points + pts_inference in one launch: the slot lists (8 bytes per sample written, then read once per tile step) never
// exist; every use re-derives them from the ray's intervals (nb comparisons per sample, nb <= 8).  Same values as the two ops.
SCANERF_API int scanerf_pts_inference_tracing(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                                              const uint8_t *running_mask, const float *intersections, const void *tables_f16,
                                              const float *images, const int32_t *res, const uint8_t *occ, const int64_t *grid_starts,
                                              const int32_t *log2dim, const float *corners, const float *sizes, float *out_dif,
                                              float *out_spec, float *out_alpha, int B, int S, int T, int nb, int sample_major,
                                              scanerf_stream_t stream)
{
    SCANERF_REQUIRE(running_mask && intersections, "pts_inference_tracing: null running_mask / intersections");
    return fg_inference(rays_o, rays_d, z_vals, dists, nullptr, running_mask, intersections, tables_f16, images, res, occ, grid_starts,
                        log2dim, corners, sizes, out_dif, out_spec, out_alpha, B, S, T, nb, sample_major, stream);
}

SCANERF_API int scanerf_bg_pts_inference_v2(const float *rays_o, const float *rays_d, const float *z_vals,
                                            const int16_t *bg_idxs, int step, const float *corners, const float *sizes,
                                            const int32_t *res, const void *tables_f16, const float *images, float *out_dif,
                                            float *out_spec, float *out_alpha, int B, int S, int T, int nb, int sample_major,
                                            scanerf_stream_t stream)
{
    RT_REQ(B >= 0 && S >= 1 && nb >= 1 && step >= 0 && step < kMaxPtsBlocks, "bg_pts_inference_v2");
    InferArgs a;
    a.rays_o = rays_o; a.rays_d = rays_d; a.z_vals = z_vals; a.dists = nullptr; a.block_idxs = bg_idxs;
    a.tables = tables_f16; a.images = images; a.res = res; a.t = make_tiles(corners, sizes, nullptr, nullptr, nullptr, nb);
    a.out_dif = out_dif; a.out_spec = out_spec; a.out_alpha = out_alpha; a.T = T; a.B = B; a.S = S; a.step = step;
    a.running = nullptr; a.inter = nullptr;
    return run_inference<true>(a, "bg_pts_inference_v2", sample_major, (hipStream_t)stream);
}
