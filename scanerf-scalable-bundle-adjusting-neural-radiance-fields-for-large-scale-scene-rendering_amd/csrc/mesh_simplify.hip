// mesh_simplify.hip -- mesh simplification by vertex clustering on a world-aligned grid (gfx950).  The reference has
// no counterpart; the definition is the comment of include/scanerf_mesh_tools_hip.h.  Compiled without FMA contraction: every float
// operation of the key and of the output is one IEEE float32 operation; everything that is summed is an integer.
//
// Cluster pass (scanerf_mesh_simplify_cluster), all before the one host read of (V', F', n_bad):
//   k_insert        one thread per vertex: the packed 63-bit key of its cell goes into a lock-free open-addressing table
//                   (keys [T] u64, T a power of two >= 2 V; linear probing from a multiplicative hash), and the parallel word
//                   first [T] i32 takes an atomic min of the vertex index.  slot[v] is kept; bad vertices are counted.
//   k_labels        label[v] = first[slot[v]] (a launch of its own: every min has landed); roots (label == v) counted per workgroup
//   k_scan          (ordered_device.h) -> V' in the header
//   k_root_rows     root_row[v] = the number of root v among the roots in ascending order, -1 for every other vertex
//   k_vertex_rows   row[v] = root_row[label[v]]
//   k_count_faces   per-workgroup counts of the faces whose three corners have three different rows; k_scan -> F'
// INVARIANTS of k_insert, on which the labels' independence of thread order, launch geometry and timing rests:
//   (1) a slot's key word changes once, from EMPTY to a key, by a compare-and-swap whose expected value is EMPTY, and never again;
//       no key equals EMPTY (a key has 63 bits);
//   (2) a probe for key K walks the slots hash(K), hash(K) + 1, ... (mod T) and leaves a slot only after it has SEEN there a key
//       other than K -- by (1) that slot holds that key for good, so every later probe for K leaves it too;
//   (3) it ends at the first slot where it sees K (loaded, or handed back by its own failed swap) or where its swap from EMPTY
//       succeeds.  Hence all probes for K end at ONE slot: the first of K's sequence that did not already hold another key when the
//       first probe for K passed it -- were K in two slots, the probe that claimed the later one would have left the earlier one
//       having seen another key there, which (1) forbids;
//   (4) no loop waits on another thread: every turn ends the probe or moves it one slot on, and with at most V <= T / 2 keys there
//       is always an EMPTY slot ahead.  A stale load can only show EMPTY where a key already is; the swap then hands back the truth.
//   WHICH slot a key lands in depends on who came first; only first[slot], the minimum over the members' indices, leaves the table,
//   and a minimum does not depend on the order of its operands.  All accesses to keys in k_insert are agent-scope atomics.
//
// Emit pass (scanerf_mesh_simplify_emit): reads (V', F', n_bad) back from the header and refuses other declared sizes; zeroes sums
//   [V',9] i64 and counts [V'] i32; k_accumulate adds every vertex's q and fixed-point attributes to its row with no-return integer
//   atomics (order-independent: the same bits from launch to launch); k_finalise, one thread per root, forms the cluster's vertex
//   (a one-member cluster copies its member's bits); k_emit_faces compacts the kept faces in order (ordered_device.h), no atomics.
//
// Faces whose indices lie outside [0, V) are never dereferenced (the Python layer refuses them; here they count for nothing).
#include <limits.h>
#include <math.h>

#include "common.h"
#include "ordered_device.h"
#include "scanerf_mesh_tools_hip.h"

using namespace scanerf;

namespace {

constexpr int kBlock = kOrderedBlock;
constexpr int kWaves = kOrderedWaves;
constexpr size_t kHeader = 64;                       // int64 V', F', n_bad (+ spare)
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kMaxV = 1 << 29;                       // the table then has at most 2^30 slots
constexpr float kCellLimit = 1048576.0f;             // |k| < 2^20 per axis: 21 bits each in the key

struct Layout {
    size_t keys, first, lab, root_row, vblocks, fblocks, total;
    size_t T;
    int nvb, nfb;
};

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

inline size_t table_slots(int V)
{
    size_t T = 64;
    while (T < 2 * (size_t)V) T <<= 1;
    return T;
}

inline Layout layout(int V, int F)
{
    Layout l;
    l.nvb = ceil_div(V, kBlock);
    l.nfb = ceil_div(F, kBlock);
    l.T = table_slots(V);
    l.keys = kHeader;
    l.first = l.keys + l.T * 8;
    l.lab = l.first + l.T * 4;
    l.root_row = l.lab + align16((size_t)V * 4);
    l.vblocks = l.root_row + align16((size_t)V * 4);
    l.fblocks = l.vblocks + align16((size_t)(l.nvb + 1) * 4);
    l.total = l.fblocks + align16((size_t)(l.nfb + 1) * 4);
    return l;
}

inline bool sizes_ok(int V, int F) { return V >= 1 && F >= 0 && V <= kMaxV && F <= (INT_MAX - kBlock) / 3; }

struct Grid {
    float o[3], h;
};

struct Key {
    bool bad;
    int k[3], q[3];
};

// The key of the definition: u = (x - o) / h, k = floorf(u), f = u - k, q = (int)(f * 65536), one rounding each.
__device__ __forceinline__ Key key_of(const float *__restrict__ vertices, int v, const Grid &g)
{
    Key key;
    key.bad = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = vertices[3 * (size_t)v + a];
        const float u = (x - g.o[a]) / g.h;
        const float kf = floorf(u);
        const float f = u - kf;
        const bool ok = isfinite(x) && fabsf(kf) < kCellLimit;      // (a NaN kf fails the comparison)
        key.bad |= !ok;
        key.k[a] = ok ? (int)kf : 0;
        key.q[a] = ok ? (int)(f * 65536.0f) : 0;
    }
    return key;
}

__device__ __forceinline__ unsigned long long pack(const Key &key)
{
    return ((unsigned long long)(key.k[0] + (1 << 20)) << 42) | ((unsigned long long)(key.k[1] + (1 << 20)) << 21) |
           (unsigned long long)(key.k[2] + (1 << 20));
}

__device__ __forceinline__ bool finite3(const float *__restrict__ a, int v)
{
    return isfinite(a[3 * (size_t)v]) && isfinite(a[3 * (size_t)v + 1]) && isfinite(a[3 * (size_t)v + 2]);
}

// t = rintf(clamp(a, -32767, 32767) * 65536) as an integer (|t| < 2^31)
__device__ __forceinline__ long long fixed_of(float a) { return (long long)rintf(fminf(fmaxf(a, -32767.0f), 32767.0f) * 65536.0f); }

// M = floor((2 S + n) / (2 n)), n >= 1
__device__ __forceinline__ long long rounded_mean(long long S, long long n)
{
    const long long num = 2 * S + n, den = 2 * n;
    long long m = num / den;
    if (num % den < 0) --m;
    return m;
}

// ---- the cluster pass ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_insert(const float *__restrict__ vertices, const float *__restrict__ normals,
                                                   const float *__restrict__ colors, int V, Grid g, unsigned long long *keys,
                                                   int *first, unsigned mask, int shift, int *__restrict__ slot_of,
                                                   unsigned long long *n_bad)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    if (v < V) {
        const Key key = key_of(vertices, v, g);
        bad = key.bad || (normals && !finite3(normals, v)) || (colors && !finite3(colors, v));
        int slot = -1;
        if (!bad) {
            const unsigned long long K = pack(key);
            unsigned s = (unsigned)((K * 0x9E3779B97F4A7C15ull) >> shift) & mask;
            for (unsigned turn = 0; turn <= mask; ++turn) {          // (invariant 4: it ends long before the table is walked)
                unsigned long long seen = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (seen == kEmpty) {
                    seen = atomicCAS(keys + s, kEmpty, K);
                    if (seen == kEmpty) seen = K;
                }
                if (seen == K) {
                    slot = (int)s;
                    break;
                }
                s = (s + 1) & mask;
            }
            if (slot >= 0) atomicMin(first + slot, v);
        }
        slot_of[v] = slot;
    }
    const unsigned long long ballot = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(n_bad, (unsigned long long)__popcll(ballot));
}

// lab: slot[v] in, label[v] out (-1 for a bad vertex); blocks[b] = the roots of workgroup b
__global__ void __launch_bounds__(kBlock) k_labels(int V, const int *__restrict__ first, int *__restrict__ lab, int *__restrict__ blocks)
{
    __shared__ int part[kWaves];
    const int v = blockIdx.x * kBlock + threadIdx.x;
    int label = -1;
    if (v < V) {
        const int s = lab[v];
        if (s >= 0) label = first[s];
        lab[v] = label;
    }
    count_flagged(v < V && label == v, blocks, part);
}

__global__ void __launch_bounds__(kBlock) k_root_rows(int V, const int *__restrict__ lab, const int *__restrict__ blocks,
                                                      int *__restrict__ root_row)
{
    __shared__ int part[kWaves];
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const bool root = v < V && lab[v] == v;
    const int dst = destination(root, blocks, part);
    if (v < V) root_row[v] = root ? dst : -1;
}

// lab: label[v] in, row[v] out
__global__ void __launch_bounds__(kBlock) k_vertex_rows(int V, const int *__restrict__ root_row, int *__restrict__ lab)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const int l = lab[v];
    lab[v] = (unsigned)l < (unsigned)V ? root_row[l] : -1;
}

// the rows of a face's corners; false for a face that is dropped
__device__ __forceinline__ bool face_rows(int f, int F, int V, const int *__restrict__ faces, const int *__restrict__ row, int (&r)[3])
{
    if (f >= F) return false;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return false;
    r[0] = row[a];
    r[1] = row[b];
    r[2] = row[c];
    return r[0] >= 0 && r[1] >= 0 && r[2] >= 0 && r[0] != r[1] && r[0] != r[2] && r[1] != r[2];
}

__global__ void __launch_bounds__(kBlock) k_count_faces(int V, int F, const int *__restrict__ faces, const int *__restrict__ row,
                                                        int *__restrict__ blocks)
{
    __shared__ int part[kWaves];
    int r[3];
    count_flagged(face_rows(blockIdx.x * kBlock + threadIdx.x, F, V, faces, row, r), blocks, part);
}

// ---- the emit pass ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_accumulate(const float *__restrict__ vertices, const float *__restrict__ normals,
                                                       const float *__restrict__ colors, int V, int Vout, Grid g,
                                                       const int *__restrict__ row, unsigned long long *sums, int *counts)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const int r = row[v];
    if ((unsigned)r >= (unsigned)Vout) return;
    const Key key = key_of(vertices, v, g);
    unsigned long long *s = sums + 9 * (size_t)r;
    atomicAdd(counts + r, 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicAdd(s + a, (unsigned long long)key.q[a]);
        if (normals) atomicAdd(s + 3 + a, (unsigned long long)fixed_of(normals[3 * (size_t)v + a]));      // (two's complement: a signed sum)
        if (colors) atomicAdd(s + 6 + a, (unsigned long long)fixed_of(colors[3 * (size_t)v + a]));
    }
}

__global__ void __launch_bounds__(kBlock) k_finalise(const float *__restrict__ vertices, const float *__restrict__ normals,
                                                     const float *__restrict__ colors, int V, int Vout, Grid g,
                                                     const int *__restrict__ root_row, const long long *__restrict__ sums,
                                                     const int *__restrict__ counts, float *__restrict__ out_vertices,
                                                     float *__restrict__ out_normals, float *__restrict__ out_colors)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const int r = root_row[v];
    if ((unsigned)r >= (unsigned)Vout) return;
    const long long n = counts[r];
    const size_t src = 3 * (size_t)v, dst = 3 * (size_t)r;
    if (n <= 1) {          // one member: its bits
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            out_vertices[dst + a] = vertices[src + a];
            if (normals) out_normals[dst + a] = normals[src + a];
            if (colors) out_colors[dst + a] = colors[src + a];
        }
        return;
    }
    const Key key = key_of(vertices, v, g);
    const long long *s = sums + 9 * (size_t)r;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float m = (float)rounded_mean(s[a], n) * 0x1p-16f;
        out_vertices[dst + a] = g.o[a] + ((float)key.k[a] + m) * g.h;
    }
    if (normals) {
        float m[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = (float)rounded_mean(s[3 + a], n) * 0x1p-16f;
        const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) + 1e-8f;
#pragma unroll
        for (int a = 0; a < 3; ++a) out_normals[dst + a] = m[a] / len;
    }
    if (colors) {
#pragma unroll
        for (int a = 0; a < 3; ++a) out_colors[dst + a] = (float)rounded_mean(s[6 + a], n) * 0x1p-16f;
    }
}

__global__ void __launch_bounds__(kBlock) k_emit_faces(int V, int F, int Fout, const int *__restrict__ faces, const int *__restrict__ row,
                                                       const int *__restrict__ blocks, int *__restrict__ out_faces)
{
    __shared__ int part[kWaves];
    int r[3];
    const bool on = face_rows(blockIdx.x * kBlock + threadIdx.x, F, V, faces, row, r);
    const int dst = destination(on, blocks, part);
    if (!on || dst >= Fout) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[3 * (size_t)dst + k] = r[k];
}

inline int common_ok(const char *op, const float *vertices, const int32_t *faces, int V, int F, const float *origin, float cell,
                     const void *scratch, size_t scratch_bytes)
{
    SCANERF_REQUIRE(sizes_ok(V, F), "%s: V=%d F=%d is not supported (1 <= V <= 2^29, 0 <= F < 2^31 / 3)", op, V, F);
    SCANERF_REQUIRE(vertices && origin && (faces || F == 0), "%s: null pointer", op);
    SCANERF_REQUIRE(cell > 0.0f && isfinite(cell), "%s: cell=%g must be positive and finite", op, (double)cell);
    SCANERF_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "%s: origin=(%g, %g, %g) must be finite", op,
                    (double)origin[0], (double)origin[1], (double)origin[2]);
    SCANERF_REQUIRE(scratch, "%s: scratch is null", op);
    SCANERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", op);
    SCANERF_REQUIRE(scratch_bytes >= layout(V, F).total, "%s: scratch holds %zu bytes, V=%d F=%d needs %zu", op, scratch_bytes, V, F,
                    layout(V, F).total);
    return 0;
}

inline Grid grid_of(const float *origin, float cell)
{
    Grid g;
    g.o[0] = origin[0];
    g.o[1] = origin[1];
    g.o[2] = origin[2];
    g.h = cell;
    return g;
}

}  // namespace

SCANERF_API int scanerf_mesh_simplify_scratch_bytes(int V, int F, size_t *bytes)
{
    SCANERF_REQUIRE(bytes, "mesh_simplify_scratch_bytes: bytes is null");
    *bytes = 0;
    SCANERF_REQUIRE(sizes_ok(V, F), "mesh_simplify_scratch_bytes: V=%d F=%d is not supported (1 <= V <= 2^29, 0 <= F < 2^31 / 3)", V, F);
    *bytes = layout(V, F).total;
    return 0;
}

SCANERF_API int scanerf_mesh_simplify_cluster(const float *vertices, const int32_t *faces, const float *normals, const float *colors,
                                              int V, int F, const float *origin, float cell, void *scratch, size_t scratch_bytes,
                                              scanerf_stream_t stream)
{
    if (int e = common_ok("mesh_simplify_cluster", vertices, faces, V, F, origin, cell, scratch, scratch_bytes)) return e;
    const Layout l = layout(V, F);
    const Grid g = grid_of(origin, cell);
    char *base = (char *)scratch;
    unsigned long long *keys = (unsigned long long *)(base + l.keys);
    int *first = (int *)(base + l.first), *lab = (int *)(base + l.lab), *root_row = (int *)(base + l.root_row);
    int *vblocks = (int *)(base + l.vblocks), *fblocks = (int *)(base + l.fblocks);
    long long *header = (long long *)base;
    hipStream_t st = (hipStream_t)stream;
    int log2T = 0;
    while (((size_t)1 << log2T) < l.T) ++log2T;
    // header = 0; keys = EMPTY (all ones); first = 0x7f7f7f7f, above every vertex index
    hipError_t err = hipMemsetAsync(base, 0, kHeader, st);
    if (err == hipSuccess) err = hipMemsetAsync(keys, 0xff, l.T * 8, st);
    if (err == hipSuccess) err = hipMemsetAsync(first, 0x7f, l.T * 4, st);
    SCANERF_REQUIRE(err == hipSuccess, "mesh_simplify_cluster: clearing the table: %s", hipGetErrorString(err));
    hipLaunchKernelGGL(k_insert, dim3(l.nvb), dim3(kBlock), 0, st, vertices, normals, colors, V, g, keys, first, (unsigned)(l.T - 1),
                       64 - log2T, lab, (unsigned long long *)(header + 2));
    hipLaunchKernelGGL(k_labels, dim3(l.nvb), dim3(kBlock), 0, st, V, (const int *)first, lab, vblocks);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, st, vblocks, l.nvb, header);
    hipLaunchKernelGGL(k_root_rows, dim3(l.nvb), dim3(kBlock), 0, st, V, (const int *)lab, (const int *)vblocks, root_row);
    hipLaunchKernelGGL(k_vertex_rows, dim3(l.nvb), dim3(kBlock), 0, st, V, (const int *)root_row, lab);
    if (F) hipLaunchKernelGGL(k_count_faces, dim3(l.nfb), dim3(kBlock), 0, st, V, F, faces, (const int *)lab, fblocks);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, st, fblocks, l.nfb, header + 1);
    return check_launch("mesh_simplify_cluster");
}

SCANERF_API int scanerf_mesh_simplify_emit(const float *vertices, const int32_t *faces, const float *normals, const float *colors, int V,
                                           int F, const float *origin, float cell, const void *scratch, size_t scratch_bytes,
                                           int64_t *sums, int32_t *counts, float *out_vertices, int32_t *out_faces, float *out_normals,
                                           float *out_colors, int Vout, int Fout, scanerf_stream_t stream)
{
    if (int e = common_ok("mesh_simplify_emit", vertices, faces, V, F, origin, cell, scratch, scratch_bytes)) return e;
    SCANERF_REQUIRE(Vout >= 1 && Vout <= V && Fout >= 0 && Fout <= F, "mesh_simplify_emit: Vout=%d Fout=%d with V=%d F=%d", Vout, Fout, V, F);
    SCANERF_REQUIRE(sums && counts && out_vertices && (out_faces || Fout == 0), "mesh_simplify_emit: null pointer");
    SCANERF_REQUIRE((normals != nullptr) == (out_normals != nullptr) && (colors != nullptr) == (out_colors != nullptr),
                    "mesh_simplify_emit: normals / colors and their outputs go together");
    hipStream_t st = (hipStream_t)stream;
    long long totals[3] = {-1, -1, -1};      // (V', F', n_bad) as the cluster pass left them: the one 24-byte read of this call
    hipError_t err = hipMemcpyAsync(totals, scratch, sizeof(totals), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    SCANERF_REQUIRE(err == hipSuccess, "mesh_simplify_emit: reading (V', F', n_bad) from the scratch: %s", hipGetErrorString(err));
    SCANERF_REQUIRE(totals[2] == 0, "mesh_simplify_emit: %lld bad vertices (not finite, or more than 2^20 cells from the origin)", totals[2]);
    SCANERF_REQUIRE(totals[0] == Vout && totals[1] == Fout,
                    "mesh_simplify_emit: the outputs are declared with Vout=%d Fout=%d rows, the cluster pass found V'=%lld F'=%lld", Vout,
                    Fout, totals[0], totals[1]);
    const Layout l = layout(V, F);
    const Grid g = grid_of(origin, cell);
    const char *base = (const char *)scratch;
    const int *row = (const int *)(base + l.lab), *root_row = (const int *)(base + l.root_row);
    const int *fblocks = (const int *)(base + l.fblocks);
    err = hipMemsetAsync(sums, 0, (size_t)Vout * 9 * 8, st);
    if (err == hipSuccess) err = hipMemsetAsync(counts, 0, (size_t)Vout * 4, st);
    SCANERF_REQUIRE(err == hipSuccess, "mesh_simplify_emit: zeroing the sums: %s", hipGetErrorString(err));
    hipLaunchKernelGGL(k_accumulate, dim3(l.nvb), dim3(kBlock), 0, st, vertices, normals, colors, V, Vout, g, row,
                       (unsigned long long *)sums, counts);
    hipLaunchKernelGGL(k_finalise, dim3(l.nvb), dim3(kBlock), 0, st, vertices, normals, colors, V, Vout, g, root_row,
                       (const long long *)sums, (const int *)counts, out_vertices, out_normals, out_colors);
    if (Fout)
        hipLaunchKernelGGL(k_emit_faces, dim3(l.nfb), dim3(kBlock), 0, st, V, F, Fout, faces, row, fblocks, out_faces);
    return check_launch("mesh_simplify_emit");
}
