// isosurface.hip -- level-set mesh extraction: surface nets over a tile's density, brick by brick.
//
// The reference has no mesh extraction; the definition is the comment of include/scanerf_hip.h.  A lattice of n = (nx, ny, nz)
// cells over the tile box, the field v = sigma at the live lattice points (0 elsewhere), one vertex per cell whose corners
// straddle the level, one quad per interior lattice edge that does.
//
// The lattice is never stored.  A one-wave workgroup takes a brick of 8^3 cells = 9^3 points at a time (grid-stride):
//   * liveness of the brick's points from the sampler's occupancy grid, integers only; a brick with no live point is left after
//     that, before any table read;
//   * the density of the live points through density_grad<VALUE> of normals_device.h, 64 points a pass (a pass with no live lane
//     is skipped), the values -- or, for the dense op, the caller's array -- into LDS (729 floats);
//   * classification there: per cell the 8 inside bits of its corners.
// Count pass: per brick the 512-bit mask of active cells (8 words, word = local x, bit = 8 local y + local z), the number of
// vertices and the number of quads.  One workgroup scans both counts (exclusive, in place).  Emit pass: a brick with a vertex
// is evaluated AGAIN (staging the values would cost 4 bytes x points of scratch, which is what this unit exists to avoid; bricks
// without a surface -- most of a pruned tile's live bricks -- are not), its vertices go to base + rank in the mask, its quads to
// the brick's quad base + a ballot rank, and the ids of the cells a quad joins, in whichever brick they lie, come from that
// brick's base and the popcount of its mask below the cell.  No atomics anywhere: order and bits are the same launch to launch.
// Scratch: 72 bytes per brick + 72 (0.14 bytes per cell of the lattice rounded up to whole bricks).
//
// A point on a brick border is evaluated by every brick that holds it (9^3 / 8^3: 42 % more evaluations than points); its bits are
// the same in each, because a lane's density depends on nothing but its own position.
//
// Three value sources fill a brick (IsoSrc): the caller's array, one tile's density, and -- the scene mesh, DESIGN.md 4.15 -- the
// densities of a whole tile set blended with the renderer's weights (render_infer_device.h) on a lattice over a world box.  The
// scene fill walks the tiles whose box reaches the brick in ascending index; per tile it forms position, membership, weight and
// occupancy bit of the brick's points (no table read), adds the weight into a second LDS array, and only where some point
// contributes stages that tile's operands (nrm_stage, kept across bricks) and runs the 64-point density passes, adding w sigma into
// val.  A point's sums are ordered by tile index alone: its bits depend neither on the brick that evaluates it nor on the launch.
// The source is a template parameter of the two brick kernels, k_iso_count<SRC, DT> and k_iso_emit<SRC, DT>, and reaches no further
// than iso_fill<SRC, DT>: everything behind the fill -- classification, count, scan, emit -- is written once, as is the host side
// (one args struct, one check chain and one launch dispatch behind the six launching exports).
#include "normals_device.h"
#include "render_infer_device.h"

namespace scanerf {
namespace {

constexpr int kIsoB = 8;                          // cells of a brick per axis
constexpr int kIsoP = kIsoB + 1;                  // points
constexpr int kIsoPts = kIsoP * kIsoP * kIsoP;    // 729
constexpr int kIsoVal = kIsoPts + 7;              // floats of a brick's value array in LDS
constexpr int kIsoPasses = (kIsoPts + 63) / 64;   // 12
constexpr int kIsoMaxBlocks = kNumCU * 12;        // three one-wave workgroups per SIMD (140 VGPRs, 12.6 KB of LDS each), grid-stride beyond
constexpr int kIsoScanThreads = 1024;
constexpr size_t kIsoHead = 64;                   // scratch: totals (int64 V, int64 F), padded

enum IsoSrc { ISO_LOAD = 0, ISO_TILE = 1, ISO_TILES = 2 };   // the caller's array; one tile's density; a tile set's blended density

struct IsoArgs {
    const float *values;          // ISO_LOAD: [nx+1, ny+1, nz+1]
    const void *features;         // ISO_TILE: [16,T,2] f32 / f16; ISO_TILES: [nb,16,T,2] f16
    const int32_t *resolutions;   // [16,3]; [nb,16,3]
    const float *blob;            // the flat decoder blob; [nb, SCANERF_PARAMSIZE]
    const float *wf;              // ISO_TILE: weight_feature [32]
    const uint8_t *occ;           // ISO_TILE: the sampler's occupancy grid, G cells per axis
    Tiles t;                      // ISO_TILES (the definition: include/scanerf_hip.h)
    int T, G[3];
    int n[3], nb[3], nbricks;
    float level, h[3];
    float origin[3], step[3];     // world position of lattice coordinate L: origin + L step (ISO_TILES: the world box's corner, size / n)
    unsigned long long *mask;     // [nbricks][8]
    int *vbase, *qbase;           // [nbricks + 1] each: counts, after the scan exclusive sums
    float *vertices, *lattice;
    int *faces, *cells;
    int V, F;
};

// the occupancy cells whose closed extent holds lattice point i along one axis: c with c n <= i G <= (c + 1) n, 0 <= c < G
__device__ __forceinline__ void iso_axis_cells(int i, int n, int G, int &c0, int &c1)
{
    const long long iG = (long long)i * G;
    const int c = (int)(iG / n);
    const bool exact = iG == (long long)c * n;
    c1 = c < G ? c : G - 1;
    c0 = exact && c > 0 ? c - 1 : c;
}

__device__ __forceinline__ bool iso_point_live(const IsoArgs &a, int i, int j, int k)
{
    int x0, x1, y0, y1, z0, z1;
    iso_axis_cells(i, a.n[0], a.G[0], x0, x1);
    iso_axis_cells(j, a.n[1], a.G[1], y0, y1);
    iso_axis_cells(k, a.n[2], a.G[2], z0, z1);
    bool live = false;
    for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y)
            for (int z = z0; z <= z1; ++z) live = live || a.occ[((size_t)x * a.G[1] + y) * a.G[2] + z] != 0;
    return live;
}

// contracted position of a lattice point: the multiply and the subtract separately rounded
__device__ __forceinline__ float iso_position(int i, float h)
{
#pragma clang fp contract(off)
    const float m = (float)i * h;
    return m - 1.0f;
}

// world position of the lattice coordinate L (a vertex, or a lattice point's index): the multiply and the sum separately rounded
__device__ __forceinline__ float iso_world(float origin, float L, float step)
{
#pragma clang fp contract(off)
    const float m = L * step;
    return origin + m;
}

__device__ __forceinline__ float iso_contracted(float pt)
{
#pragma clang fp contract(off)
    const float m = 2.0f * pt;
    return m - 1.0f;
}

__device__ __forceinline__ float iso_add_product(float acc, float w, float s)
{
#pragma clang fp contract(off)
    const float m = w * s;
    return acc + m;
}

__device__ __forceinline__ void iso_brick_origin(const IsoArgs &a, int brick, int b0[3])
{
    const int bz = brick % a.nb[2], r = brick / a.nb[2];
    b0[0] = (r / a.nb[1]) * kIsoB;
    b0[1] = (r % a.nb[1]) * kIsoB;
    b0[2] = bz * kIsoB;
}

// point p of the brick -> its lattice index; false: past the brick's 729 points or outside the lattice
__device__ __forceinline__ bool iso_point(const IsoArgs &a, const int b0[3], int p, int &i, int &j, int &k)
{
    const int lx = p / (kIsoP * kIsoP), r = p - lx * (kIsoP * kIsoP), ly = r / kIsoP, lz = r - ly * kIsoP;
    i = b0[0] + lx;
    j = b0[1] + ly;
    k = b0[2] + lz;
    return p < kIsoPts && i <= a.n[0] && j <= a.n[1] && k <= a.n[2];
}

// ISO_TILES: the brick's 9^3 blended values -> val, the weight sums in wsum (both LDS); false: no point of the brick contributes for
// any tile (no table and no decoder was read).  staged / c: the tile whose operands lds holds and its constant, kept across bricks.
__device__ __forceinline__ bool iso_fill_tiles(const IsoArgs &a, float *lds, float *val, float *wsum, int lane, const int b0[3],
                                               int &staged, float &c)
{
#pragma clang fp contract(off)   // (the sums below take products of render_infer_device.h's functions: separately rounded)
    for (int p = lane; p < kIsoVal; p += 64) {
        val[p] = 0.0f;
        wsum[p] = 0.0f;
    }
    // The brick's world extent.  Position, tile coordinate and membership are monotone in the lattice index (step, size > 0 and every
    // operation rounds monotonically), so a tile lists a point of the brick only if it passes this test at the brick's end points.
    float wlo[3], whi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int last = b0[k] + kIsoB < a.n[k] ? b0[k] + kIsoB : a.n[k];
        wlo[k] = iso_world(a.origin[k], (float)b0[k], a.step[k]);
        whi[k] = iso_world(a.origin[k], (float)last, a.step[k]);
    }
    bool any = false;
    for (int base = 0; base < a.t.nb; base += 64) {
        const int bt = base + lane;
        bool reach = bt < a.t.nb;
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
#pragma unroll 1
            for (int pass = 0; pass < kIsoPasses; ++pass) {
                const int p = pass * 64 + lane;
                int i, j, k;
                const bool in = iso_point(a, b0, p, i, j, k);
                const float wp[3] = { iso_world(a.origin[0], (float)i, a.step[0]), iso_world(a.origin[1], (float)j, a.step[1]),
                                      iso_world(a.origin[2], (float)k, a.step[2]) };
                float pt[3];
                tile_point(wp, cb, sb, pt);
                const bool listed = in && pt[0] >= 0.0f && pt[0] <= 1.0f && pt[1] >= 0.0f && pt[1] <= 1.0f && pt[2] >= 0.0f && pt[2] <= 1.0f;
                const float w = tile_weight(pt, sb);
                const int64_t cell = tile_cell(a.t, b, pt);   // (for every lane: render_infer_device.h)
                if (listed) wsum[p] = wsum[p] + w;            // the weight counts whether or not the cell is occupied
                const bool run = listed && a.t.occ[cell] != 0;
                if (__ballot(run) == 0ull) continue;          // wave-uniform
                if (b != staged) {
                    __syncthreads();   // (one wave: the reads of the tile staged before are done)
                    const float *blob = a.blob + (size_t)b * SCANERF_PARAMSIZE;
                    nrm_stage<false>(lds, blob, nullptr, a.resolutions + (size_t)b * 48, lane);
                    c = nrm_c(blob);
                    staged = b;
                    __syncthreads();
                }
                float x[3] = { 0.0f, 0.0f, 0.0f };   // (lanes that do not run: the one-tile fill's dead lanes)
                if (run) {
                    x[0] = iso_contracted(pt[0]);
                    x[1] = iso_contracted(pt[1]);
                    x[2] = iso_contracted(pt[2]);
                }
                const float unused[3] = { 0.0f, 0.0f, 0.0f };
                float s, gsum[3];
                density_grad<SCANERF_F16, false, true>(lds, (const char *)a.features + (size_t)b * 16 * a.T * 4, a.T, unused, c, lane, x, s, gsum);
                if (run) val[p] = iso_add_product(val[p], w, nrm_softplus(s));
                any = true;
            }
        }
    }
    if (any) {
        for (int p = lane; p < kIsoPts; p += 64) val[p] = val[p] * inv_weight(wsum[p]);
    }
    return any;
}

// A brick kernel's LDS: the decoder operands of the staged tile, the brick's values and, for the tile set alone, its weight sums
// (2.9, 12.6 and 15.5 KB for the three sources; a source pays for no array it does not use)
template <IsoSrc SRC>
struct IsoLds {
    float operands[SRC == ISO_LOAD ? 0 : NL_TOTAL] __attribute__((aligned(16)));
    float val[kIsoVal];
    float wsum[SRC == ISO_TILES ? kIsoVal : 0];
};

// which tile's operands the LDS holds (-1: none yet) and that tile's constant: kept by a kernel across its bricks
struct IsoStaged {
    int tile;
    float c;
};

// ISO_TILE stages its one tile here, once; ISO_TILES stages in the fill, tile after tile
template <IsoSrc SRC>
__device__ __forceinline__ IsoStaged iso_begin(const IsoArgs &a, IsoLds<SRC> &s, int lane)
{
    IsoStaged st = { -1, 0.0f };
    if constexpr (SRC == ISO_TILE) {
        nrm_stage(s.operands, a.blob, a.wf, a.resolutions, lane);
        st.c = nrm_c(a.blob);
    }
    __syncthreads();
    return st;
}

// the brick's 9^3 values -> s.val; false: no live point (ISO_TILES: no contributing one) -- nothing else was read
template <IsoSrc SRC, int DT>
__device__ __forceinline__ bool iso_fill(const IsoArgs &a, IsoLds<SRC> &s, IsoStaged &st, int lane, const int b0[3])
{
    if constexpr (SRC == ISO_TILES) {
        return iso_fill_tiles(a, s.operands, s.val, s.wsum, lane, b0, st.tile, st.c);
    } else {
        bool any = SRC == ISO_LOAD;
#pragma unroll 1
        for (int pass = 0; pass < kIsoPasses; ++pass) {
            const int p = pass * 64 + lane;
            int i, j, k;
            const bool in = iso_point(a, b0, p, i, j, k);
            float v = 0.0f;
            if constexpr (SRC == ISO_LOAD) {
                if (in) v = a.values[((size_t)i * (a.n[1] + 1) + j) * (a.n[2] + 1) + k];
            } else {
                const bool live = in && iso_point_live(a, i, j, k);
                if (__ballot(live) != 0ull) {   // wave-uniform: every lane takes part in the product
                    float x[3] = { 0.0f, 0.0f, 0.0f };
                    if (live) {
                        x[0] = iso_position(i, a.h[0]);
                        x[1] = iso_position(j, a.h[1]);
                        x[2] = iso_position(k, a.h[2]);
                    }
                    const float unused[3] = { 0.0f, 0.0f, 0.0f };
                    float sg, gsum[3];
                    density_grad<DT, false, true>(s.operands, a.features, a.T, unused, st.c, lane, x, sg, gsum);
                    if (live) v = nrm_softplus(sg);
                    any = true;
                }
            }
            if (p < kIsoPts) s.val[p] = v;
        }
        return any;
    }
}

// cell (w, lane >> 3, lane & 7) of the brick: its corner values (corner = dx << 2 | dy << 1 | dz), inside bits, and whether the
// cell lies in the lattice
__device__ __forceinline__ bool iso_cell(const IsoArgs &a, const float *val, const int b0[3], int w, int lane, int cc[3], float cv[8],
                                         unsigned &ins)
{
    const int ly = lane >> 3, lz = lane & 7;
    cc[0] = b0[0] + w;
    cc[1] = b0[1] + ly;
    cc[2] = b0[2] + lz;
    ins = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        cv[q] = val[(w + (q >> 2)) * (kIsoP * kIsoP) + (ly + ((q >> 1) & 1)) * kIsoP + lz + (q & 1)];
        ins |= (cv[q] > a.level ? 1u : 0u) << q;
    }
    return cc[0] < a.n[0] && cc[1] < a.n[1] && cc[2] < a.n[2];
}

// lattice edge from the cell's corner 0 along axis A: does it give a quad?  (ends differ; interior along the two other axes)
template <int A>
__device__ __forceinline__ bool iso_quad(const IsoArgs &a, bool valid, const int cc[3], unsigned ins)
{
    constexpr int O1 = (A + 1) % 3, O2 = (A + 2) % 3;
    const unsigned far = ins >> (4 >> A);
    return valid && ((ins ^ far) & 1u) && cc[O1] >= 1 && cc[O2] >= 1;
}

// count pass: per brick the active-cell mask and the vertex / quad counts
template <IsoSrc SRC, int DT>
__global__ void __launch_bounds__(64) k_iso_count(IsoArgs a)
{
    __shared__ IsoLds<SRC> s;
    const int lane = threadIdx.x;
    IsoStaged st = iso_begin(a, s, lane);
    for (int brick = blockIdx.x; brick < a.nbricks; brick += gridDim.x) {
        int b0[3];
        iso_brick_origin(a, brick, b0);
        __syncthreads();   // (the previous brick's reads of val are done)
        const bool any = iso_fill<SRC, DT>(a, s, st, lane, b0);
        __syncthreads();
        unsigned long long word = 0ull;
        int vc = 0, qc = 0;
        if (any) {
            for (int w = 0; w < kIsoB; ++w) {
                int cc[3];
                float cv[8];
                unsigned ins;
                const bool valid = iso_cell(a, s.val, b0, w, lane, cc, cv, ins);
                const unsigned long long m = __ballot(valid && ins != 0u && ins != 0xffu);
                if (lane == w) word = m;
                vc += __popcll(m);
                qc += __popcll(__ballot(iso_quad<0>(a, valid, cc, ins))) + __popcll(__ballot(iso_quad<1>(a, valid, cc, ins))) +
                      __popcll(__ballot(iso_quad<2>(a, valid, cc, ins)));
            }
        }
        if (lane < kIsoB) a.mask[(size_t)brick * kIsoB + lane] = word;
        if (lane == 0) {
            a.vbase[brick] = vc;
            a.qbase[brick] = qc;
        }
    }
}

// exclusive sums of both counts in place, entry [nbricks] = the sum; totals = (V, F = 2 Q) as int64
__global__ void __launch_bounds__(kIsoScanThreads) k_iso_scan(int *vb, int *qb, int nbricks, long long *totals)
{
    __shared__ int sh[2][kIsoScanThreads];
    const int t = threadIdx.x;
    long long carry0 = 0, carry1 = 0;
    for (int base = 0; base < nbricks; base += kIsoScanThreads) {
        const int i = base + t;
        const int x0 = i < nbricks ? vb[i] : 0, x1 = i < nbricks ? qb[i] : 0;
        sh[0][t] = x0;
        sh[1][t] = x1;
        __syncthreads();
        for (int off = 1; off < kIsoScanThreads; off <<= 1) {
            const int y0 = t >= off ? sh[0][t - off] : 0, y1 = t >= off ? sh[1][t - off] : 0;
            __syncthreads();
            sh[0][t] += y0;
            sh[1][t] += y1;
            __syncthreads();
        }
        if (i < nbricks) {
            vb[i] = (int)(carry0 + sh[0][t] - x0);
            qb[i] = (int)(carry1 + sh[1][t] - x1);
        }
        carry0 += sh[0][kIsoScanThreads - 1];
        carry1 += sh[1][kIsoScanThreads - 1];
        __syncthreads();
    }
    if (t == 0) {
        vb[nbricks] = (int)carry0;
        qb[nbricks] = (int)carry1;
        totals[0] = carry0;
        totals[1] = 2 * carry1;
    }
}

// vertex id of an active cell anywhere in the lattice: its brick's base + the active cells before it in the brick's mask
__device__ __forceinline__ int iso_vertex_id(const IsoArgs &a, int cx, int cy, int cz)
{
    const int brick = ((cx >> 3) * a.nb[1] + (cy >> 3)) * a.nb[2] + (cz >> 3);
    const unsigned long long *mk = a.mask + (size_t)brick * kIsoB;
    const int w = cx & 7, bit = (cy & 7) * 8 + (cz & 7);
    int rank = __popcll(mk[w] & ((1ull << bit) - 1ull));
    for (int i = 0; i < w; ++i) rank += __popcll(mk[i]);
    return a.vbase[brick] + rank;
}

// the vertex of an active cell in lattice coordinates: the mean of its edges' crossing points, summed in the definition's order
__device__ __forceinline__ void iso_cell_vertex(const int cc[3], const float cv[8], float level, float L[3])
{
#pragma clang fp contract(off)
    float sum[3] = { 0.0f, 0.0f, 0.0f };
    int cnt = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int o1 = (ax + 1) % 3, o2 = (ax + 2) % 3;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int q[3];
            q[ax] = 0;
            q[o1] = e & 1;
            q[o2] = e >> 1;
            const int ca = q[0] << 2 | q[1] << 1 | q[2], cb = ca | (4 >> ax);
            const float va = cv[ca], vb = cv[cb];
            if ((va > level) != (vb > level)) {
                float pt[3];
                pt[0] = (float)(cc[0] + q[0]);
                pt[1] = (float)(cc[1] + q[1]);
                pt[2] = (float)(cc[2] + q[2]);
                const float t = (level - va) / (vb - va);
                pt[ax] = pt[ax] + t;
                sum[0] = sum[0] + pt[0];
                sum[1] = sum[1] + pt[1];
                sum[2] = sum[2] + pt[2];
                ++cnt;
            }
        }
    }
    const float fc = (float)cnt;
    L[0] = sum[0] / fc;
    L[1] = sum[1] / fc;
    L[2] = sum[2] / fc;
}

template <int A>
__device__ __forceinline__ void iso_emit_quad(const IsoArgs &a, const int cc[3], unsigned ins, int slot)
{
    constexpr int O1 = (A + 1) % 3, O2 = (A + 2) % 3;
    const int d1[4] = { -1, 0, 0, -1 }, d2[4] = { -1, -1, 0, 0 };
    int id[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int nc[3] = { cc[0], cc[1], cc[2] };
        nc[O1] += d1[q];
        nc[O2] += d2[q];
        id[q] = iso_vertex_id(a, nc[0], nc[1], nc[2]);
    }
    if (!(ins & 1u)) {   // the edge's first end is outside: reversed
        const int t0 = id[0], t1 = id[1];
        id[0] = id[3];
        id[1] = id[2];
        id[2] = t1;
        id[3] = t0;
    }
    int *f = a.faces + 6 * (size_t)slot;
    f[0] = id[0];
    f[1] = id[1];
    f[2] = id[2];
    f[3] = id[0];
    f[4] = id[2];
    f[5] = id[3];
}

// emit pass: per brick with a vertex, its vertices from the brick's vertex base on and its quads from its quad base on
template <IsoSrc SRC, int DT>
__global__ void __launch_bounds__(64) k_iso_emit(IsoArgs a)
{
    __shared__ IsoLds<SRC> s;
    const int lane = threadIdx.x;
    IsoStaged st = iso_begin(a, s, lane);
    const unsigned long long below = (1ull << lane) - 1ull;   // the lanes before this one
    for (int brick = blockIdx.x; brick < a.nbricks; brick += gridDim.x) {
        const int v0 = a.vbase[brick], v1 = a.vbase[brick + 1], q0 = a.qbase[brick], q1 = a.qbase[brick + 1];
        // no vertex: no quad either (a crossing edge makes its cell active).  Outputs smaller than the scratch says: not written.
        if (v1 == v0 || v0 < 0 || q0 < 0 || v1 > a.V || q1 > a.F / 2) continue;
        int b0[3];
        iso_brick_origin(a, brick, b0);
        __syncthreads();
        iso_fill<SRC, DT>(a, s, st, lane, b0);
        __syncthreads();
        int vrun = v0, qrun = q0;
        for (int w = 0; w < kIsoB; ++w) {
            int cc[3];
            float cv[8];
            unsigned ins;
            const bool valid = iso_cell(a, s.val, b0, w, lane, cc, cv, ins);
            const bool active = valid && ins != 0u && ins != 0xffu;
            const unsigned long long m = __ballot(active);
            if (active) {
                const int vid = vrun + __popcll(m & below);
                float L[3];
                iso_cell_vertex(cc, cv, a.level, L);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    a.vertices[3 * (size_t)vid + k] = iso_world(a.origin[k], L[k], a.step[k]);
                    a.cells[3 * (size_t)vid + k] = cc[k];
                    if (a.lattice) a.lattice[3 * (size_t)vid + k] = L[k];
                }
            }
            vrun += __popcll(m);
            const bool qa = iso_quad<0>(a, valid, cc, ins), qb = iso_quad<1>(a, valid, cc, ins), qc = iso_quad<2>(a, valid, cc, ins);
            const unsigned long long ma = __ballot(qa), mb = __ballot(qb), mc = __ballot(qc);
            if (qa) iso_emit_quad<0>(a, cc, ins, qrun + __popcll(ma & below));
            qrun += __popcll(ma);
            if (qb) iso_emit_quad<1>(a, cc, ins, qrun + __popcll(mb & below));
            qrun += __popcll(mb);
            if (qc) iso_emit_quad<2>(a, cc, ins, qrun + __popcll(mc & below));
            qrun += __popcll(mc);
        }
    }
}

// ---- host side: the checks of the seven exports, in the order they fire, and one launcher per pass
int64_t iso_bricks(int nx, int ny, int nz)
{
    return (int64_t)ceil_div(nx, kIsoB) * ceil_div(ny, kIsoB) * ceil_div(nz, kIsoB);
}

size_t iso_scratch_bytes(int nx, int ny, int nz)
{
    const int64_t nb = iso_bricks(nx, ny, nz);
    return kIsoHead + (size_t)nb * kIsoB * sizeof(unsigned long long) + 2 * (size_t)(nb + 1) * sizeof(int);
}

int iso_check_lattice(const char *op, int nx, int ny, int nz, float level)
{
    SCANERF_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: n=(%d,%d,%d): every n_k must be >= 1", op, nx, ny, nz);
    // (the first product of two ints below 2^31 fits int64; the second factor is applied only while the product is small)
    const int64_t cxy = (int64_t)nx * ny, pxy = ((int64_t)nx + 1) * ((int64_t)ny + 1);
    SCANERF_REQUIRE(cxy < (1ll << 31) && cxy * nz < (1ll << 31), "%s: n=(%d,%d,%d): 2^31 cells or more", op, nx, ny, nz);
    SCANERF_REQUIRE(pxy < (1ll << 31) && pxy * ((int64_t)nz + 1) < (1ll << 31), "%s: n=(%d,%d,%d): 2^31 lattice points or more", op, nx,
                    ny, nz);
    SCANERF_REQUIRE(level > 0.0f, "%s: level=%g must be > 0 (the field is 0 outside the occupied cells)", op, (double)level);
    return 0;
}

// the one-tile source's arguments
int iso_check_model(const char *op, IsoArgs &a, const void *features, int feat_dtype, const int32_t *resolutions, const float *mlp_blob,
                    const float *weight_feature, int T, const uint8_t *occupied_grid, const int32_t *log2dim, long long occ_cells)
{
    SCANERF_REQUIRE(T >= 2 && (T & (T - 1)) == 0, "%s: T=%d must be a power of two", op, T);
    SCANERF_REQUIRE(feat_dtype == SCANERF_F32 || feat_dtype == SCANERF_F16, "%s: feat_dtype=%d (f32 and f16 tables)", op, feat_dtype);
    SCANERF_REQUIRE(log2dim, "%s: null pointer (log2dim)", op);
    long long cells = 1;
    for (int k = 0; k < 3; ++k) {
        SCANERF_REQUIRE(log2dim[k] >= 0 && log2dim[k] <= 10, "%s: log2dim[%d]=%d (0..10)", op, k, log2dim[k]);
        a.G[k] = 1 << log2dim[k];
        cells *= a.G[k];
    }
    SCANERF_REQUIRE(occ_cells == cells, "%s: occupied_grid holds %lld cells, log2dim=(%d,%d,%d) says %lld", op, occ_cells, log2dim[0],
                    log2dim[1], log2dim[2], cells);
    SCANERF_REQUIRE(features && resolutions && mlp_blob && weight_feature && occupied_grid, "%s: null pointer", op);
    SCANERF_REQUIRE(((uintptr_t)features & 15) == 0, "%s: features must be 16-byte aligned", op);
    a.features = features; a.resolutions = resolutions; a.blob = mlp_blob; a.wf = weight_feature; a.occ = occupied_grid; a.T = T;
    return 0;
}

// the scene source's arguments (everything but lattice, scratch and outputs); origin / step: the world box
int iso_check_tiles(const char *op, IsoArgs &a, const void *tables_f16, const float *blobs, const int32_t *resolution, const uint8_t *occ,
                    const int64_t *grid_starts, const int32_t *log2dim, const float *corners, const float *sizes, int T, int nb,
                    const float *box_corner, const float *box_size, int nx, int ny, int nz)
{
    SCANERF_REQUIRE(nb >= 1, "%s: nb=%d (at least one tile)", op, nb);
    SCANERF_REQUIRE(T >= 2 && (T & (T - 1)) == 0, "%s: T=%d must be a power of two", op, T);
    SCANERF_REQUIRE(tables_f16 && blobs && resolution && occ && grid_starts && log2dim && corners && sizes, "%s: null pointer", op);
    SCANERF_REQUIRE(box_corner && box_size, "%s: null pointer (box_corner / box_size)", op);
    SCANERF_REQUIRE(((uintptr_t)tables_f16 & 15) == 0, "%s: tables must be 16-byte aligned", op);
    const int n[3] = { nx, ny, nz };
    for (int k = 0; k < 3; ++k) {
        SCANERF_REQUIRE(box_size[k] > 0.0f && box_size[k] <= 3.0e38f, "%s: box_size[%d]=%g must be positive and finite", op, k,
                        (double)box_size[k]);
        a.origin[k] = box_corner[k];
        a.step[k] = box_size[k] / (float)n[k];
    }
    a.features = tables_f16; a.blob = blobs; a.resolutions = resolution; a.T = T;
    a.t = make_tiles(corners, sizes, occ, grid_starts, log2dim, nb);
    return 0;
}

// the emit pass's own arguments.  The world step is `extent` itself for the dense op (its spacing) and extent / n for a box
struct IsoOut {
    const float *origin, *extent;
    float *vertices;
    int32_t *faces, *cells;
    float *lattice;
    int V, F;
};

int iso_check_outputs(const char *op, IsoSrc src, IsoArgs &a, const IsoOut &o)
{
    SCANERF_REQUIRE(o.V >= 0 && o.F >= 0 && (o.F & 1) == 0, "%s: V=%d F=%d (F counts triangles, two per quad)", op, o.V, o.F);
    SCANERF_REQUIRE(o.origin && o.extent, "%s: null pointer (origin / spacing)", op);
    SCANERF_REQUIRE(o.V == 0 || (o.vertices && o.cells), "%s: null pointer (vertices / cells)", op);
    SCANERF_REQUIRE(o.F == 0 || o.faces, "%s: null pointer (faces)", op);
    for (int k = 0; k < 3; ++k) {
        a.origin[k] = o.origin[k];
        a.step[k] = src == ISO_LOAD ? o.extent[k] : o.extent[k] / (float)a.n[k];
    }
    a.vertices = o.vertices; a.faces = o.faces; a.cells = o.cells; a.lattice = o.lattice; a.V = o.V; a.F = o.F;
    return 0;
}

template <IsoSrc SRC, int DT>
void iso_launch(bool emit, const IsoArgs &a, hipStream_t st)
{
    const dim3 grid(a.nbricks < kIsoMaxBlocks ? a.nbricks : kIsoMaxBlocks);
    if (emit) hipLaunchKernelGGL((k_iso_emit<SRC, DT>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_iso_count<SRC, DT>), grid, dim3(64), 0, st, a);
}

// Everything behind the source's own checks, for all six launching exports: lattice, scratch carving and the brick grid, the emit
// pass's outputs (out != nullptr), then the pass's kernel for (source, table dtype) -- behind the count kernel the scan.
int iso_run(const char *op, IsoSrc src, int feat_dtype, IsoArgs &a, int nx, int ny, int nz, float level, void *scratch,
            size_t scratch_bytes, const IsoOut *out, scanerf_stream_t stream)
{
    if (int e = iso_check_lattice(op, nx, ny, nz, level)) return e;
    SCANERF_REQUIRE(scratch, "%s: null pointer (scratch)", op);
    SCANERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", op);
    const size_t need = iso_scratch_bytes(nx, ny, nz);
    SCANERF_REQUIRE(scratch_bytes >= need, "%s: scratch holds %zu B, %zu needed (scanerf_isosurface_scratch_bytes)", op, scratch_bytes, need);
    SCANERF_REQUIRE(src != ISO_LOAD || a.values, "%s: null pointer (values)", op);
    a.n[0] = nx; a.n[1] = ny; a.n[2] = nz;
    for (int k = 0; k < 3; ++k) {
        a.nb[k] = ceil_div(a.n[k], kIsoB);
        a.h[k] = 2.0f / (float)a.n[k];
    }
    a.nbricks = (int)iso_bricks(nx, ny, nz);
    a.level = level;
    char *p = (char *)scratch + kIsoHead;
    a.mask = (unsigned long long *)p;
    p += (size_t)a.nbricks * kIsoB * sizeof(unsigned long long);
    a.vbase = (int *)p;
    a.qbase = a.vbase + a.nbricks + 1;
    if (out) {
        if (int e = iso_check_outputs(op, src, a, *out)) return e;
        if (out->V == 0) return 0;
    }
    const hipStream_t st = (hipStream_t)stream;
    const bool emit = out != nullptr;
    if (src == ISO_LOAD) iso_launch<ISO_LOAD, SCANERF_F32>(emit, a, st);
    else if (src == ISO_TILES) iso_launch<ISO_TILES, SCANERF_F16>(emit, a, st);
    else if (feat_dtype == SCANERF_F32) iso_launch<ISO_TILE, SCANERF_F32>(emit, a, st);
    else iso_launch<ISO_TILE, SCANERF_F16>(emit, a, st);
    if (int e = check_launch(op)) return e;
    if (emit) return 0;
    hipLaunchKernelGGL(k_iso_scan, dim3(1), dim3(kIsoScanThreads), 0, st, a.vbase, a.qbase, a.nbricks, (long long *)scratch);
    return check_launch(op);
}

}  // namespace
}  // namespace scanerf

using namespace scanerf;

SCANERF_API size_t scanerf_isosurface_scratch_bytes(int nx, int ny, int nz)
{
    if (iso_check_lattice("isosurface_scratch_bytes", nx, ny, nz, 1.0f)) return 0;
    return iso_scratch_bytes(nx, ny, nz);
}

SCANERF_API int scanerf_isosurface_count_dense(const float *values, int nx, int ny, int nz, float level, void *scratch, size_t scratch_bytes,
                                               scanerf_stream_t stream)
{
    IsoArgs a = {};
    a.values = values;
    return iso_run("isosurface_count_dense", ISO_LOAD, SCANERF_F32, a, nx, ny, nz, level, scratch, scratch_bytes, nullptr, stream);
}

SCANERF_API int scanerf_isosurface_emit_dense(const float *values, int nx, int ny, int nz, float level, const float *origin,
                                              const float *spacing, const void *scratch, size_t scratch_bytes, float *vertices,
                                              int32_t *faces, int32_t *cells, float *lattice, int V, int F, scanerf_stream_t stream)
{
    IsoArgs a = {};
    a.values = values;
    const IsoOut out = { origin, spacing, vertices, faces, cells, lattice, V, F };
    return iso_run("isosurface_emit_dense", ISO_LOAD, SCANERF_F32, a, nx, ny, nz, level, const_cast<void *>(scratch), scratch_bytes, &out,
                   stream);
}

SCANERF_API int scanerf_isosurface_count(const void *features, int feat_dtype, const int32_t *resolutions, const float *mlp_blob,
                                         const float *weight_feature, int T, const uint8_t *occupied_grid, const int32_t *log2dim,
                                         long long occ_cells, int nx, int ny, int nz, float level, void *scratch, size_t scratch_bytes,
                                         scanerf_stream_t stream)
{
    const char *op = "isosurface_count";
    IsoArgs a = {};
    if (int e = iso_check_lattice(op, nx, ny, nz, level)) return e;
    if (int e = iso_check_model(op, a, features, feat_dtype, resolutions, mlp_blob, weight_feature, T, occupied_grid, log2dim, occ_cells))
        return e;
    return iso_run(op, ISO_TILE, feat_dtype, a, nx, ny, nz, level, scratch, scratch_bytes, nullptr, stream);
}

SCANERF_API int scanerf_isosurface_emit(const void *features, int feat_dtype, const int32_t *resolutions, const float *mlp_blob,
                                        const float *weight_feature, int T, const uint8_t *occupied_grid, const int32_t *log2dim,
                                        long long occ_cells, int nx, int ny, int nz, float level, const float *occ_corner,
                                        const float *occ_size, const void *scratch, size_t scratch_bytes, float *vertices, int32_t *faces,
                                        int32_t *cells, float *lattice, int V, int F, scanerf_stream_t stream)
{
    const char *op = "isosurface_emit";
    IsoArgs a = {};
    if (int e = iso_check_lattice(op, nx, ny, nz, level)) return e;
    if (int e = iso_check_model(op, a, features, feat_dtype, resolutions, mlp_blob, weight_feature, T, occupied_grid, log2dim, occ_cells))
        return e;
    const IsoOut out = { occ_corner, occ_size, vertices, faces, cells, lattice, V, F };
    return iso_run(op, ISO_TILE, feat_dtype, a, nx, ny, nz, level, const_cast<void *>(scratch), scratch_bytes, &out, stream);
}

SCANERF_API int scanerf_isosurface_count_tiles(const void *tables_f16, const float *blobs, const int32_t *resolution, const uint8_t *occ,
                                               const int64_t *grid_starts, const int32_t *log2dim, const float *corners,
                                               const float *sizes, int T, int nb, const float *box_corner, const float *box_size, int nx,
                                               int ny, int nz, float level, void *scratch, size_t scratch_bytes, scanerf_stream_t stream)
{
    const char *op = "isosurface_count_tiles";
    IsoArgs a = {};
    if (int e = iso_check_lattice(op, nx, ny, nz, level)) return e;
    if (int e = iso_check_tiles(op, a, tables_f16, blobs, resolution, occ, grid_starts, log2dim, corners, sizes, T, nb, box_corner, box_size,
                                nx, ny, nz))
        return e;
    return iso_run(op, ISO_TILES, SCANERF_F16, a, nx, ny, nz, level, scratch, scratch_bytes, nullptr, stream);
}

SCANERF_API int scanerf_isosurface_emit_tiles(const void *tables_f16, const float *blobs, const int32_t *resolution, const uint8_t *occ,
                                              const int64_t *grid_starts, const int32_t *log2dim, const float *corners,
                                              const float *sizes, int T, int nb, const float *box_corner, const float *box_size, int nx,
                                              int ny, int nz, float level, const void *scratch, size_t scratch_bytes, float *vertices,
                                              int32_t *faces, int32_t *cells, float *lattice, int V, int F, scanerf_stream_t stream)
{
    const char *op = "isosurface_emit_tiles";
    IsoArgs a = {};
    if (int e = iso_check_lattice(op, nx, ny, nz, level)) return e;
    if (int e = iso_check_tiles(op, a, tables_f16, blobs, resolution, occ, grid_starts, log2dim, corners, sizes, T, nb, box_corner, box_size,
                                nx, ny, nz))
        return e;
    const IsoOut out = { box_corner, box_size, vertices, faces, cells, lattice, V, F };
    return iso_run(op, ISO_TILES, SCANERF_F16, a, nx, ny, nz, level, const_cast<void *>(scratch), scratch_bytes, &out, stream);
}
