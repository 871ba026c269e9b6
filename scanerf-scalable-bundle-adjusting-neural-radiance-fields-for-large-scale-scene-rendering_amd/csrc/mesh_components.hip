// mesh_components.hip -- connected components of a triangle mesh and the order-preserving filter by component (gfx950;
// DESIGN.md 4.17).  The reference has no counterpart; the definition is the comment of include/scanerf_hip.h.  Integers only.
//
// Labels: a lock-free union-find over parent [V] (the caller's labels array), three launches.
//   k_identity   parent[v] = v
//   k_hook       one thread per face, two unions (corner 0 with corner 1, corner 0 with corner 2)
//   k_flatten    a launch of its own: parent[v] = the root of v = the smallest index of v's component
// INVARIANTS of k_hook, on which the labels' independence of face order, launch geometry and timing rests:
//   (1) parent[x] <= x, always;
//   (2) a parent only ever decreases (the hook's compare-and-swap writes a smaller index; path shortening is an atomic min);
//   (3) a ROOT (parent[x] == x) changes only through a compare-and-swap whose expected value is x itself: the hook puts the LARGER
//       of two roots under the smaller; path shortening touches only a vertex that was SEEN not to be a root, which never becomes
//       one again (1, 2), and writes only an ancestor of it;
//   (4) no loop waits on a load: every turn of a union's loop either ends it (a successful swap; both sides under one parent),
//       or moves one side strictly down the index order (1), or is a FAILED swap, which continues from the value the swap
//       returned -- smaller than the one it expected -- and does not load that word again.
//   Every value parent[x] ever held is a vertex of x's component that is <= x, so an old value -- a line another XCD's L2 or this
//   CU's L1 still holds -- leads to the same root by a longer way: it can cost a retry (the swap on a vertex that is no longer a root
//   fails and hands back the truth), never a wrong label and never a spin.  All accesses to parent in k_hook are agent-scope atomics
//   (relaxed loads, compare-and-swap, min), so nothing is register-cached either.  A tree's root is the smallest index that was ever
//   united into it (the smaller root always wins), hence after the last union the root of a component is its smallest vertex.
//
// Table: roots are counted and compacted in ascending order without atomics (ballot + popcount per wave, per-workgroup counts, one
//   single-workgroup scan: csrc/compact.hip's way), row_of[root] = its row.  k_sums adds n_vertices, n_faces and the cell extremes
//   into the rows with integer atomics (order-independent: the same bits from launch to launch).  A scene mesh is mostly ONE
//   component, so the sums are aggregated before they reach memory: per wave-load the lanes that share a row are counted by ballot
//   and reduced by shuffles (several rows in a wave: a loop over the distinct ones); the wave keeps a running partial for the row it
//   carries the most items for across its whole grid-stride loop (a lighter row met on the way goes to memory at once, a heavier
//   one takes its place); at the end the workgroup's waves merge their partials per row through LDS and one lane sends each
//   distinct row once.  No atomic returns a value.
//
// Filter: keep [C] u8 per row (the caller's rule) -> per-workgroup counts of kept vertices / faces, their scans, (V', F') in the
//   scratch header; the emit pass checks the caller's V' / F' against that header (one 16-byte read), writes new_index [V], gathers
//   the per-vertex arrays row for row and remaps the kept faces.  Order-preserving, no atomics.
//
// Faces whose indices lie outside [0, V) are never dereferenced (the Python layer refuses them; here they join nothing, count for
// nothing and are not kept).
#include <limits.h>

#include "common.h"
#include "ordered_device.h"

using namespace scanerf;

namespace {

constexpr int kBlock = 256;                 // threads, and items per workgroup of the order-preserving passes
constexpr int kWaves = kBlock / kWave;
constexpr size_t kHeader = 64;              // int64 C, V', F' (+ spare), 16-byte aligned like every section behind it

struct Layout {
    size_t row_of, new_index, vblocks, fblocks, total;
    int nvb, nfb;
};

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

inline Layout layout(int V, int F)
{
    Layout l;
    l.nvb = ceil_div(V, kBlock);
    l.nfb = ceil_div(F, kBlock);
    l.row_of = kHeader;
    l.new_index = l.row_of + align16((size_t)V * 4);
    l.vblocks = l.new_index + align16((size_t)V * 4);
    l.fblocks = l.vblocks + align16((size_t)(l.nvb + 1) * 4);
    l.total = l.fblocks + align16((size_t)(l.nfb + 1) * 4);
    return l;
}

inline bool sizes_ok(int V, int F) { return V >= 1 && F >= 0 && V <= INT_MAX - kBlock && F <= (INT_MAX - kBlock) / 3; }

__device__ __forceinline__ int ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- labels -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_identity(int *__restrict__ parent, int V)
{
    for (int v = blockIdx.x * kBlock + threadIdx.x; v < V; v += gridDim.x * kBlock) parent[v] = v;
}

// Join the trees of a and b.  u walks up a's tree and v up b's, always the one whose parent is LARGER (it lies deeper in the
// index order), and the walk ends as soon as both have the same parent: two vertices of one flattened tree never read its root,
// which matters because a scene mesh is mostly one component and every thread reading that root's word serialises on one L2
// channel (measured: 6.4 ms for 3.2 M faces with a find-both-roots union).  A vertex seen not to be a root is
// pointed at its grandparent by an atomic min before the walk leaves it (invariants 2, 3); a root is hooked under the other
// side's parent -- a smaller index of the other tree, itself a root or not -- by compare-and-swap (invariant 3).
__device__ __forceinline__ void unite(int *parent, int u, int v)
{
    int pu = ld(parent + u), pv = ld(parent + v);
    while (pu != pv) {
        if (pu < pv) {          // keep u the side with the larger parent
            int t = u;
            u = v;
            v = t;
            t = pu;
            pu = pv;
            pv = t;
        }
        if (pu == u) {          // u was seen as a root, and pv < u
            const int seen = atomicCAS(parent + u, u, pv);
            if (seen == u) return;
            pu = seen;          // seen < u: u had been hooked meanwhile; go on from the value the swap returned (invariant 4)
        } else {
            const int g = ld(parent + pu);
            if (g != pu) atomicMin(parent + u, g);
            u = pu;
            pu = g;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_hook(const int *__restrict__ faces, int V, int F, int *parent)
{
    for (int f = blockIdx.x * kBlock + threadIdx.x; f < F; f += gridDim.x * kBlock) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) continue;
        if (a != b) unite(parent, a, b);
        if (a != c && b != c) unite(parent, a, c);
    }
}

// No union runs in this launch: roots stay roots.  Other threads' stores (roots of the same component) may or may not be seen: both
// an old parent and the root lead to the root.
__global__ void __launch_bounds__(kBlock) k_flatten(int *parent, int V)
{
    for (int v = blockIdx.x * kBlock + threadIdx.x; v < V; v += gridDim.x * kBlock) {
        const int p = ld(parent + v);
        int r = p;
        for (int q = ld(parent + r); q != r; q = ld(parent + r)) r = q;
        if (r != p) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- order-preserving counts, scans and destinations ------------------------------------------------------------------------------
enum { kRoots = 0, kKeptVertices = 1, kKeptFaces = 2 };

template <int WHAT>
__device__ __forceinline__ bool flag_of(int i, int n, int V, int C, const int *__restrict__ faces, const int *__restrict__ labels,
                                        const int *__restrict__ row_of, const uint8_t *__restrict__ keep)
{
    if (i >= n) return false;
    int v = i;
    if (WHAT == kKeptFaces) {
        v = faces[3 * (size_t)i];
        const int b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
        if ((unsigned)v >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return false;
    }
    const int l = labels[v];
    if (WHAT == kRoots) return l == v;
    if ((unsigned)l >= (unsigned)V) return false;
    const int r = row_of[l];
    return (unsigned)r < (unsigned)C && keep[r] != 0;
}

// blocks[b] = the flagged items among the kBlock items of workgroup b
template <int WHAT>
__global__ void __launch_bounds__(kBlock) k_count(int n, int V, int C, const int *__restrict__ faces, const int *__restrict__ labels,
                                                  const int *__restrict__ row_of, const uint8_t *__restrict__ keep,
                                                  int *__restrict__ blocks)
{
    __shared__ int part[kWaves];
    const bool on = flag_of<WHAT>(blockIdx.x * kBlock + threadIdx.x, n, V, C, faces, labels, row_of, keep);
    const unsigned long long ballot = __ballot(on);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kWaves; ++w) s += part[w];
        blocks[blockIdx.x] = s;
    }
}

// (the scan of the per-workgroup counts and an item's destination: ordered_device.h)
// row_of[v] = the row of root v among the roots in ascending order; -1 for every other vertex
__global__ void __launch_bounds__(kBlock) k_root_rows(int V, const int *__restrict__ labels, const int *__restrict__ blocks,
                                                      int *__restrict__ row_of)
{
    __shared__ int part[kWaves];
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const bool root = v < V && labels[v] == v;
    const int dst = destination(root, blocks, part);
    if (v < V) row_of[v] = root ? dst : -1;
}

// ---- the table ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_table_init(int V, int C, const int *__restrict__ labels, const int *__restrict__ row_of,
                                                       int *__restrict__ label, int *__restrict__ n_vertices, int *__restrict__ n_faces,
                                                       int *__restrict__ cell_min, int *__restrict__ cell_max)
{
    for (int v = blockIdx.x * kBlock + threadIdx.x; v < V; v += gridDim.x * kBlock) {
        if (labels[v] != v) continue;
        const int r = row_of[v];
        if ((unsigned)r >= (unsigned)C) continue;
        label[r] = v;
        n_vertices[r] = 0;
        n_faces[r] = 0;
        if (cell_min) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                cell_min[3 * (size_t)r + k] = INT_MAX;
                cell_max[3 * (size_t)r + k] = INT_MIN;
            }
        }
    }
}

struct Partial {      // wave-uniform: the sums a wave holds for one row
    int row, nv, nf, mn[3], mx[3];
};

__device__ __forceinline__ void clear(Partial &p)
{
    p.row = -1;
    p.nv = p.nf = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p.mn[k] = INT_MAX;
        p.mx[k] = INT_MIN;
    }
}

__device__ __forceinline__ void merge(Partial &into, const Partial &p)
{
    into.nv += p.nv;
    into.nf += p.nf;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        into.mn[k] = min(into.mn[k], p.mn[k]);
        into.mx[k] = max(into.mx[k], p.mx[k]);
    }
}

// one lane: a partial goes to memory (no value comes back)
__device__ __forceinline__ void send(const Partial &p, int *n_vertices, int *n_faces, int *cell_min, int *cell_max)
{
    if (p.row < 0) return;
    if (p.nv) atomicAdd(n_vertices + p.row, p.nv);
    if (p.nf) atomicAdd(n_faces + p.row, p.nf);
    if (cell_min && p.nv) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(cell_min + 3 * (size_t)p.row + k, p.mn[k]);
            atomicMax(cell_max + 3 * (size_t)p.row + k, p.mx[k]);
        }
    }
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// The lanes' rows (-1: none) and, for vertices, their cells -> the wave's running partial or memory.
template <bool VERTICES>
__device__ __forceinline__ void wave_accumulate(Partial &run, int row, const int (&cell)[3], bool with_cells, int *n_vertices,
                                                int *n_faces, int *cell_min, int *cell_max)
{
    unsigned long long todo = __ballot(row >= 0);
    while (todo) {
        const int R = __shfl(row, __builtin_ctzll(todo), 64);
        const bool mine = row == R;
        const unsigned long long same = __ballot(mine);
        todo &= ~same;
        Partial p;
        clear(p);
        p.row = R;
        (VERTICES ? p.nv : p.nf) = __popcll(same);
        if (VERTICES && with_cells) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p.mn[k] = wave_min(mine ? cell[k] : INT_MAX);
                p.mx[k] = wave_max(mine ? cell[k] : INT_MIN);
            }
        }
        // the wave HOLDS the heavier of the two and sends the lighter: the dominant component's partial, once held, is displaced
        // only by a heavier one, so floaters between its vertices go to their own rows and its row sees one add per workgroup
        if (run.row == R) {
            merge(run, p);
        } else if (p.nv + p.nf > run.nv + run.nf) {
            if ((threadIdx.x & 63) == 0) send(run, n_vertices, n_faces, cell_min, cell_max);
            run = p;
        } else if ((threadIdx.x & 63) == 0) {
            send(p, n_vertices, n_faces, cell_min, cell_max);
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_sums(int V, int F, int C, const int *__restrict__ faces, const int *__restrict__ cells,
                                                 const int *__restrict__ labels, const int *__restrict__ row_of, int *n_vertices,
                                                 int *n_faces, int *cell_min, int *cell_max)
{
    __shared__ Partial held[kWaves];
    Partial run;
    clear(run);
    const bool with_cells = cells != nullptr && cell_min != nullptr;
    const int stride = gridDim.x * kBlock;
    // (the bounds are rounded up to whole waves: every lane of a wave makes the same number of trips)
    for (int base = blockIdx.x * kBlock + (threadIdx.x & ~63); base < V; base += stride) {
        const int v = base + (threadIdx.x & 63);
        int row = -1, cell[3] = {0, 0, 0};
        if (v < V) {
            const int l = labels[v];
            if ((unsigned)l < (unsigned)V) row = row_of[l];
            if ((unsigned)row >= (unsigned)C) row = -1;
            if (with_cells && row >= 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) cell[k] = cells[3 * (size_t)v + k];
            }
        }
        wave_accumulate<true>(run, row, cell, with_cells, n_vertices, n_faces, cell_min, cell_max);
    }
    for (int base = blockIdx.x * kBlock + (threadIdx.x & ~63); base < F; base += stride) {
        const int f = base + (threadIdx.x & 63);
        int row = -1;
        const int none[3] = {0, 0, 0};
        if (f < F) {
            const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
            if ((unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V) {
                const int l = labels[a];
                if ((unsigned)l < (unsigned)V) row = row_of[l];
                if ((unsigned)row >= (unsigned)C) row = -1;
            }
        }
        wave_accumulate<false>(run, row, none, false, n_vertices, n_faces, cell_min, cell_max);
    }
    // the workgroup's waves merge what they still hold, per row, through LDS; each distinct row goes to memory once
    if ((threadIdx.x & 63) == 0) held[threadIdx.x >> 6] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < kWaves; ++w) {
            Partial p = held[w];
            if (p.row < 0) continue;
            for (int u = w + 1; u < kWaves; ++u) {
                if (held[u].row == p.row) {
                    merge(p, held[u]);
                    held[u].row = -1;
                }
            }
            send(p, n_vertices, n_faces, cell_min, cell_max);
        }
    }
}

// ---- the filter ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_filter_vertices(int V, int C, int Vout, const int *__restrict__ labels,
                                                            const int *__restrict__ row_of, const uint8_t *__restrict__ keep,
                                                            const int *__restrict__ blocks, int *__restrict__ new_index,
                                                            const float *__restrict__ vertices, const int *__restrict__ cells,
                                                            const float *__restrict__ lattice, const float *__restrict__ normals,
                                                            float *__restrict__ out_vertices, int *__restrict__ out_cells,
                                                            float *__restrict__ out_lattice, float *__restrict__ out_normals)
{
    __shared__ int part[kWaves];
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const bool on = flag_of<kKeptVertices>(v, V, V, C, nullptr, labels, row_of, keep);
    const int dst = destination(on, blocks, part);
    if (v < V) new_index[v] = on && dst < Vout ? dst : -1;
    if (!on || dst >= Vout) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (vertices) out_vertices[3 * (size_t)dst + k] = vertices[3 * (size_t)v + k];
        if (cells) out_cells[3 * (size_t)dst + k] = cells[3 * (size_t)v + k];
        if (lattice) out_lattice[3 * (size_t)dst + k] = lattice[3 * (size_t)v + k];
        if (normals) out_normals[3 * (size_t)dst + k] = normals[3 * (size_t)v + k];
    }
}

__global__ void __launch_bounds__(kBlock) k_filter_faces(int V, int F, int C, int Fout, const int *__restrict__ faces,
                                                         const int *__restrict__ labels, const int *__restrict__ row_of,
                                                         const uint8_t *__restrict__ keep, const int *__restrict__ blocks,
                                                         const int *__restrict__ new_index, int *__restrict__ out_faces)
{
    __shared__ int part[kWaves];
    const int f = blockIdx.x * kBlock + threadIdx.x;
    const bool on = flag_of<kKeptFaces>(f, F, V, C, faces, labels, row_of, keep);
    const int dst = destination(on, blocks, part);
    if (!on || dst >= Fout) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[3 * (size_t)dst + k] = new_index[faces[3 * (size_t)f + k]];
}

inline int scratch_ok(const char *op, int V, int F, const void *scratch, size_t scratch_bytes)
{
    SCANERF_REQUIRE(sizes_ok(V, F), "%s: V=%d F=%d is not supported (V >= 1, F >= 0, both below 2^31 / 3)", op, V, F);
    SCANERF_REQUIRE(scratch, "%s: scratch is null", op);
    SCANERF_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", op);
    SCANERF_REQUIRE(scratch_bytes >= layout(V, F).total, "%s: scratch holds %zu bytes, V=%d F=%d needs %zu", op, scratch_bytes, V, F,
                    layout(V, F).total);
    return 0;
}

}  // namespace

SCANERF_API size_t scanerf_mesh_components_scratch_bytes(int V, int F)
{
    if (!sizes_ok(V, F)) {
        set_error("mesh_components_scratch_bytes: V=%d F=%d is not supported (V >= 1, F >= 0, both below 2^31 / 3)", V, F);
        return 0;
    }
    return layout(V, F).total;
}

SCANERF_API int scanerf_mesh_components_label(const int32_t *faces, int V, int F, int32_t *labels, void *scratch, size_t scratch_bytes,
                                              scanerf_stream_t stream)
{
    if (int e = scratch_ok("mesh_components_label", V, F, scratch, scratch_bytes)) return e;
    SCANERF_REQUIRE(labels && (faces || F == 0), "mesh_components_label: null pointer");
    const Layout l = layout(V, F);
    char *base = (char *)scratch;
    int *row_of = (int *)(base + l.row_of), *vblocks = (int *)(base + l.vblocks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_identity, dim3(stream_grid(V, kBlock)), dim3(kBlock), 0, st, labels, V);
    if (F) hipLaunchKernelGGL(k_hook, dim3(stream_grid(F, kBlock)), dim3(kBlock), 0, st, faces, V, F, labels);
    hipLaunchKernelGGL(k_flatten, dim3(stream_grid(V, kBlock)), dim3(kBlock), 0, st, labels, V);
    hipLaunchKernelGGL(k_count<kRoots>, dim3(l.nvb), dim3(kBlock), 0, st, V, V, 0, (const int *)nullptr, (const int *)labels,
                       (const int *)nullptr, (const uint8_t *)nullptr, vblocks);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, st, vblocks, l.nvb, (long long *)base);
    hipLaunchKernelGGL(k_root_rows, dim3(l.nvb), dim3(kBlock), 0, st, V, (const int *)labels, (const int *)vblocks, row_of);
    return check_launch("mesh_components_label");
}

SCANERF_API int scanerf_mesh_components_table(const int32_t *faces, const int32_t *cells, const int32_t *labels, int V, int F,
                                              const void *scratch, size_t scratch_bytes, int C, int32_t *label, int32_t *n_vertices,
                                              int32_t *n_faces, int32_t *cell_min, int32_t *cell_max, scanerf_stream_t stream)
{
    if (int e = scratch_ok("mesh_components_table", V, F, scratch, scratch_bytes)) return e;
    SCANERF_REQUIRE(C >= 1 && C <= V, "mesh_components_table: C=%d with V=%d", C, V);
    SCANERF_REQUIRE(labels && label && n_vertices && n_faces && (faces || F == 0), "mesh_components_table: null pointer");
    SCANERF_REQUIRE(cells ? (cell_min && cell_max) : (!cell_min && !cell_max),
                    "mesh_components_table: cells, cell_min and cell_max go together (all three or none)");
    const Layout l = layout(V, F);
    const int *row_of = (const int *)((const char *)scratch + l.row_of);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_table_init, dim3(stream_grid(V, kBlock)), dim3(kBlock), 0, st, V, C, labels, row_of, label, n_vertices, n_faces,
                       cell_min, cell_max);
    hipLaunchKernelGGL(k_sums, dim3(stream_grid(V > F ? V : F, kBlock, kNumCU * 4)), dim3(kBlock), 0, st, V, F, C, faces, cells, labels,
                       row_of, n_vertices, n_faces, cell_min, cell_max);
    return check_launch("mesh_components_table");
}

SCANERF_API int scanerf_mesh_filter_count(const int32_t *faces, const int32_t *labels, const uint8_t *keep, int V, int F, int C,
                                          void *scratch, size_t scratch_bytes, scanerf_stream_t stream)
{
    if (int e = scratch_ok("mesh_filter_count", V, F, scratch, scratch_bytes)) return e;
    SCANERF_REQUIRE(C >= 1 && C <= V, "mesh_filter_count: C=%d with V=%d", C, V);
    SCANERF_REQUIRE(labels && keep && (faces || F == 0), "mesh_filter_count: null pointer");
    const Layout l = layout(V, F);
    char *base = (char *)scratch;
    const int *row_of = (const int *)(base + l.row_of);
    int *vblocks = (int *)(base + l.vblocks), *fblocks = (int *)(base + l.fblocks);
    long long *header = (long long *)base;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_count<kKeptVertices>, dim3(l.nvb), dim3(kBlock), 0, st, V, V, C, (const int *)nullptr, labels, row_of, keep,
                       vblocks);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, st, vblocks, l.nvb, header + 1);
    if (F) hipLaunchKernelGGL(k_count<kKeptFaces>, dim3(l.nfb), dim3(kBlock), 0, st, F, V, C, faces, labels, row_of, keep, fblocks);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, st, fblocks, l.nfb, header + 2);
    return check_launch("mesh_filter_count");
}

SCANERF_API int scanerf_mesh_filter_emit(const int32_t *faces, const int32_t *labels, const uint8_t *keep, int V, int F, int C,
                                         void *scratch, size_t scratch_bytes, const float *vertices, const int32_t *cells,
                                         const float *lattice, const float *normals, float *out_vertices, int32_t *out_faces,
                                         int32_t *out_cells, float *out_lattice, float *out_normals, int Vout, int Fout,
                                         scanerf_stream_t stream)
{
    if (int e = scratch_ok("mesh_filter_emit", V, F, scratch, scratch_bytes)) return e;
    SCANERF_REQUIRE(C >= 1 && C <= V, "mesh_filter_emit: C=%d with V=%d", C, V);
    SCANERF_REQUIRE(labels && keep && (faces || F == 0), "mesh_filter_emit: null pointer");
    SCANERF_REQUIRE(Vout >= 0 && Fout >= 0, "mesh_filter_emit: Vout=%d Fout=%d", Vout, Fout);
    SCANERF_REQUIRE((!vertices || out_vertices) && (!cells || out_cells) && (!lattice || out_lattice) && (!normals || out_normals) &&
                        (out_faces || Fout == 0),
                    "mesh_filter_emit: an input array without its output");
    hipStream_t st = (hipStream_t)stream;
    long long totals[2] = {-1, -1};      // (V', F') as mesh_filter_count left them: the one 16-byte read of this call
    hipError_t err = hipMemcpyAsync(totals, (const char *)scratch + 8, sizeof(totals), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    SCANERF_REQUIRE(err == hipSuccess, "mesh_filter_emit: reading (V', F') from the scratch: %s", hipGetErrorString(err));
    SCANERF_REQUIRE(totals[0] == Vout && totals[1] == Fout,
                    "mesh_filter_emit: the outputs are declared with Vout=%d Fout=%d rows, the count pass found V'=%lld F'=%lld", Vout,
                    Fout, totals[0], totals[1]);
    const Layout l = layout(V, F);
    char *base = (char *)scratch;
    const int *row_of = (const int *)(base + l.row_of);
    int *new_index = (int *)(base + l.new_index);
    const int *vblocks = (const int *)(base + l.vblocks), *fblocks = (const int *)(base + l.fblocks);
    hipLaunchKernelGGL(k_filter_vertices, dim3(l.nvb), dim3(kBlock), 0, st, V, C, Vout, labels, row_of, keep, vblocks, new_index, vertices,
                       cells, lattice, normals, out_vertices, out_cells, out_lattice, out_normals);
    if (F && Fout)
        hipLaunchKernelGGL(k_filter_faces, dim3(l.nfb), dim3(kBlock), 0, st, V, F, C, Fout, faces, labels, row_of, keep, fblocks,
                           (const int *)new_index, out_faces);
    return check_launch("mesh_filter_emit");
}
