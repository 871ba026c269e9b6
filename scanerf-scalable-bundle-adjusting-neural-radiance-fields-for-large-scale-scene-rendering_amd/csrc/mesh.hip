// mesh.hip -- ray / triangle-mesh tracer over a uniform grid: the counterpart of the reference's third compiled module
// (fastMesh: fastMesh/include/tile_structure.h:13-106 break_into_tiles, fastMesh/src/fastMesh_kernel.cu:125-329 firstEnter / firstHit).
//
// Structure (built on the device, fastmesh.py drives it): 2^L cells per axis over the cube [min_corner, min_corner + side * cell],
// cell = largest extent of the vertex bounds / side.  A face is registered in every cell its axis-aligned box overlaps
// (int((min - min_corner) / cell) .. int((max - min_corner) / cell), clamped).  Per cell index n = (x << 2L) | (y << L) | z:
//   bitmask    one bit per cell in 64-bit words;
//   rank       per word the number of set bits in all earlier words: the occupied-cell ordinal is rank[w] + popcount(word below the
//              bit) -- the reference recounts every earlier word on every lookup (fastMesh_kernel.cu:9-14);
//   start_num  per occupied cell (start, count) into cell_faces; cell_faces: face indices, ascending inside a cell;
//   cell_box   per occupied cell min / max over the vertices of its faces (the reference recomputes it per ray, :157-184);
//   tris       optional, per cell_faces entry (A, B - A, C - A): the face loop without its two indirections.
// The build is free of atomics: k_face_cells counts, the caller scans, k_emit_keys writes (cell << 32) | face at each face's
// offset, the caller sorts; k_cell_boxes reduces per cell in a fixed order.
//
// Traces: one ray per lane; the ray is clipped to the grid cube (clip_box) and the Walker of dda_device.h starts at the entry point
// (the reference clamps the start cell of an outside origin and walks with the tMax of the real origin, dda.h:34-75 "[FIXME] camera
// must be inside the scene").  first_hit carries its nearest candidate ACROSS cells and stops once the candidate is not beyond the
// current cell's exit; the reference returns on the first cell with any hit, even a hit beyond that cell (:284-290) -- DESIGN.md.
// The device side of the traces (Grid, Words, ray_triangle, RayWalk, first_hit_walk) lives in mesh_device.h, shared with coverage.hip.
// Built without FMA contraction (dda_device.h).  No atomics, no allocation, no host synchronisation; two launches give equal bits.
#include "mesh_device.h"

namespace {

struct FaceCells {
    int lo[3], hi[3];
    bool ok;
};

// the registration rule, float32, operation by operation (tests/fastmesh_reference.py does the same in numpy)
__device__ __forceinline__ FaceCells face_cells(const float *__restrict__ vertices, const int32_t *__restrict__ faces, int V, int f,
                                                int L, const float *__restrict__ scene_info)
{
    FaceCells r;
    r.ok = false;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return r;
    const int side = 1 << L;
    const float cell = scene_info[3];
    bool out = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float A = vertices[3 * i0 + c], B = vertices[3 * i1 + c], C = vertices[3 * i2 + c];
        const float mn = fminf(fminf(A, B), C), mx = fmaxf(fmaxf(A, B), C);
        const float gmin = scene_info[c], gmax = gmin + (float)side * cell;
        out |= mx < gmin || mn > gmax;
        const int l = (int)((mn - gmin) / cell), h = (int)((mx - gmin) / cell);
        r.lo[c] = l < 0 ? 0 : (l > side - 1 ? side - 1 : l);
        r.hi[c] = h < 0 ? 0 : (h > side - 1 ? side - 1 : h);
    }
    r.ok = !out && cell > 0.0f;
    return r;
}

__global__ void __launch_bounds__(256) k_face_cells(const float *__restrict__ vertices, const int32_t *__restrict__ faces, int V, int F,
                                                    int L, const float *__restrict__ scene_info, int32_t *__restrict__ counts)
{
    for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < F; f += gridDim.x * blockDim.x) {
        const FaceCells r = face_cells(vertices, faces, V, f, L, scene_info);
        counts[f] = r.ok ? (r.hi[0] - r.lo[0] + 1) * (r.hi[1] - r.lo[1] + 1) * (r.hi[2] - r.lo[2] + 1) : 0;
    }
}

// one wavefront per face: its cells in (x, y, z) order from offsets[f]
__global__ void __launch_bounds__(256) k_emit_keys(const float *__restrict__ vertices, const int32_t *__restrict__ faces, int V, int F,
                                                   int L, const float *__restrict__ scene_info, const int64_t *__restrict__ offsets,
                                                   int64_t *__restrict__ keys, int64_t n_keys)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int f = wave; f < F; f += nwaves) {
        const FaceCells r = face_cells(vertices, faces, V, f, L, scene_info);
        if (!r.ok) continue;   // wave-uniform
        const int ny = r.hi[1] - r.lo[1] + 1, nz = r.hi[2] - r.lo[2] + 1;
        const int n = (r.hi[0] - r.lo[0] + 1) * ny * nz;
        const int64_t at = offsets[f];
        for (int i = lane; i < n; i += 64) {
            const int z = r.lo[2] + i % nz, y = r.lo[1] + (i / nz) % ny, x = r.lo[0] + i / (nz * ny);
            const int64_t cellidx = ((int64_t)x << (2 * L)) | ((int64_t)y << L) | (int64_t)z;
            if (at + i >= 0 && at + i < n_keys) keys[at + i] = (cellidx << 32) | (int64_t)f;
        }
    }
}

// one wavefront per occupied cell: min / max over its faces' vertices (exact, any order gives the same bits)
__global__ void __launch_bounds__(256) k_cell_boxes(const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                    const int32_t *__restrict__ start_num, const int32_t *__restrict__ cell_faces,
                                                    int n_cells, float *__restrict__ cell_box)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int c = wave; c < n_cells; c += nwaves) {
        const int start = start_num[2 * c], num = start_num[2 * c + 1];
        float mn[3] = { kInf, kInf, kInf }, mx[3] = { -kInf, -kInf, -kInf };
        for (int i = lane; i < num; i += 64) {
            const int f = cell_faces[start + i];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int v = faces[3 * f + k];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float x = vertices[3 * v + a];
                    mn[a] = fminf(mn[a], x);
                    mx[a] = fmaxf(mx[a], x);
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            for (int s = 32; s >= 1; s >>= 1) {
                mn[a] = fminf(mn[a], __shfl_xor(mn[a], s, 64));
                mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], s, 64));
            }
        }
        if (lane < 3) cell_box[6 * c + lane] = lane == 0 ? mn[0] : (lane == 1 ? mn[1] : mn[2]);
        else if (lane < 6) cell_box[6 * c + lane] = lane == 3 ? mx[0] : (lane == 4 ? mx[1] : mx[2]);
    }
}

__global__ void __launch_bounds__(256) k_gather_tris(const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                     const int32_t *__restrict__ cell_faces, int64_t n, float *__restrict__ tris)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = cell_faces[i];
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float A = vertices[3 * a + k];
            tris[9 * i + k] = A;
            tris[9 * i + 3 + k] = vertices[3 * b + k] - A;
            tris[9 * i + 6 + k] = vertices[3 * c + k] - A;
        }
    }
}

template <bool LDS, bool PRE>
__global__ void __launch_bounds__(256) k_first_hit(const float *__restrict__ rays_o, const float *__restrict__ rays_d, int B, Grid g,
                                                   const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                   const int32_t *__restrict__ cell_faces, const float *__restrict__ tris,
                                                   float *__restrict__ out)
{
    extern __shared__ uint64_t lds[];
    const Words<LDS> words(g, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B; i += gridDim.x * blockDim.x) {
        const float o[3] = { rays_o[3 * i], rays_o[3 * i + 1], rays_o[3 * i + 2] };
        const float d[3] = { rays_d[3 * i], rays_d[3 * i + 1], rays_d[3 * i + 2] };
        out[i] = first_hit_walk<LDS, PRE>(o, d, g, words, vertices, faces, cell_faces, tris);
    }
}

template <bool LDS>
__global__ void __launch_bounds__(256) k_first_enter(const float *__restrict__ rays_o, const float *__restrict__ rays_d, int B, Grid g,
                                                     const float *__restrict__ cell_box, float *__restrict__ out)
{
    extern __shared__ uint64_t lds[];
    const Words<LDS> words(g, lds);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B; i += gridDim.x * blockDim.x) {
        const float o[3] = { rays_o[3 * i], rays_o[3 * i + 1], rays_o[3 * i + 2] };
        const float d[3] = { rays_d[3 * i], rays_d[3 * i + 1], rays_d[3 * i + 2] };
        float res = 0.0f;
        RayWalk rw;
        if (rw.start(o, d, g)) {
            while (!rw.done()) {
                rw.w.pick();
                const int c = words.lookup(rw.cell(g.L));
                if (c >= 0) {
                    const float *b = cell_box + 6 * (size_t)c;
                    float ctr[3], half[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        ctr[a] = (b[3 + a] + b[a]) / 2.0f;
                        half[a] = (b[3 + a] - b[a]) / 2.0f;
                    }
                    const F2 s = clip_box(o, d, ctr, half);   // the WORLD-space ray against the cell's box, interval [0, 1e5]
                    if (s.x >= 0.0f) {
                        res = s.x;
                        break;
                    }
                }
                rw.w.advance();
            }
        }
        out[i] = res;
    }
}

int require_build_args(const char *what, const float *vertices, const int32_t *faces, int V, int F, int log2dim, const float *scene_info)
{
    SCANERF_REQUIRE(F > 0 && V > 0, "%s: V=%d F=%d (an empty mesh cannot be traced)", what, V, F);
    SCANERF_REQUIRE(log2dim >= 4 && log2dim <= 7, "%s: log2dim=%d outside 4..7", what, log2dim);
    SCANERF_REQUIRE(vertices && faces && scene_info, "%s: null pointer", what);
    return 0;
}

int require_trace_args(const char *what, int B, const void *a, const void *b, const void *c, const void *d, const void *e, const void *f,
                       const void *g, int log2dim, int lds)
{
    SCANERF_REQUIRE(B > 0 && B <= (1 << 29), "%s: B=%d", what, B);
    SCANERF_REQUIRE(log2dim >= 4 && log2dim <= 7, "%s: log2dim=%d outside 4..7", what, log2dim);
    SCANERF_REQUIRE(a && b && c && d && e && f && g, "%s: null pointer", what);
    SCANERF_REQUIRE(!lds || log2dim <= 6, "%s: the LDS-staged lookup holds at most log2dim=6 (48 KB), got %d", what, log2dim);
    return 0;
}

inline size_t lds_bytes(int log2dim) { return ((size_t)1 << (3 * log2dim - 6)) * 12; }
// LDS-staged: a few resident workgroups per CU, each staging once and striding over the rays
inline int trace_grid(int B, int lds) { return lds ? stream_grid(B, 256, kNumCU * 3) : ceil_div(B, 256); }

}  // namespace

SCANERF_API int scanerf_mesh_count_cells(const float *vertices, const int32_t *faces, int V, int F, int log2dim,
                                         const float *scene_info, int32_t *counts, scanerf_stream_t stream)
{
    if (int r = require_build_args("mesh_count_cells", vertices, faces, V, F, log2dim, scene_info)) return r;
    SCANERF_REQUIRE(counts, "mesh_count_cells: null pointer");
    hipLaunchKernelGGL(k_face_cells, dim3(stream_grid(F, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces, V, F, log2dim,
                       scene_info, counts);
    return check_launch("mesh_count_cells");
}

SCANERF_API int scanerf_mesh_emit_keys(const float *vertices, const int32_t *faces, int V, int F, int log2dim, const float *scene_info,
                                       const int64_t *offsets, int64_t *keys, long long n_keys, scanerf_stream_t stream)
{
    if (int r = require_build_args("mesh_emit_keys", vertices, faces, V, F, log2dim, scene_info)) return r;
    SCANERF_REQUIRE(n_keys > 0 && n_keys < ((long long)1 << 31), "mesh_emit_keys: n_keys=%lld", n_keys);
    SCANERF_REQUIRE(offsets && keys, "mesh_emit_keys: null pointer");
    hipLaunchKernelGGL(k_emit_keys, dim3(stream_grid((int64_t)F * 64, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces, V, F,
                       log2dim, scene_info, offsets, keys, (int64_t)n_keys);
    return check_launch("mesh_emit_keys");
}

SCANERF_API int scanerf_mesh_cell_boxes(const float *vertices, const int32_t *faces, const int32_t *start_num,
                                        const int32_t *cell_faces, int n_cells, float *cell_box, scanerf_stream_t stream)
{
    if (n_cells == 0) return 0;
    SCANERF_REQUIRE(n_cells > 0, "mesh_cell_boxes: n_cells=%d", n_cells);
    SCANERF_REQUIRE(vertices && faces && start_num && cell_faces && cell_box, "mesh_cell_boxes: null pointer");
    hipLaunchKernelGGL(k_cell_boxes, dim3(stream_grid((int64_t)n_cells * 64, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces,
                       start_num, cell_faces, n_cells, cell_box);
    return check_launch("mesh_cell_boxes");
}

SCANERF_API int scanerf_mesh_gather_triangles(const float *vertices, const int32_t *faces, const int32_t *cell_faces,
                                              long long n_entries, float *tris, scanerf_stream_t stream)
{
    if (n_entries == 0) return 0;
    SCANERF_REQUIRE(n_entries > 0 && n_entries < ((long long)1 << 31), "mesh_gather_triangles: n_entries=%lld", n_entries);
    SCANERF_REQUIRE(vertices && faces && cell_faces && tris, "mesh_gather_triangles: null pointer");
    hipLaunchKernelGGL(k_gather_tris, dim3(stream_grid(n_entries, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces, cell_faces,
                       (int64_t)n_entries, tris);
    return check_launch("mesh_gather_triangles");
}

SCANERF_API int scanerf_mesh_first_hit(const float *rays_o, const float *rays_d, int B, const float *vertices, const int32_t *faces,
                                       const float *tris, const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                                       const int32_t *cell_faces, const float *scene_info, int log2dim, int lds, float *out,
                                       scanerf_stream_t stream)
{
    if (B == 0) return 0;
    if (int r = require_trace_args("mesh_first_hit", B, rays_o, rays_d, bitmask, rank, start_num, scene_info, out, log2dim, lds)) return r;
    SCANERF_REQUIRE(tris || (vertices && faces && cell_faces), "mesh_first_hit: null pointer (neither triangles nor an indexed mesh)");
    const Grid g = { bitmask, rank, start_num, scene_info, log2dim };
    const dim3 grid(trace_grid(B, lds)), block(256);
    const size_t sh = lds ? lds_bytes(log2dim) : 0;
    hipStream_t st = (hipStream_t)stream;
    if (lds && tris) hipLaunchKernelGGL((k_first_hit<true, true>), grid, block, sh, st, rays_o, rays_d, B, g, vertices, faces, cell_faces, tris, out);
    else if (lds) hipLaunchKernelGGL((k_first_hit<true, false>), grid, block, sh, st, rays_o, rays_d, B, g, vertices, faces, cell_faces, tris, out);
    else if (tris) hipLaunchKernelGGL((k_first_hit<false, true>), grid, block, sh, st, rays_o, rays_d, B, g, vertices, faces, cell_faces, tris, out);
    else hipLaunchKernelGGL((k_first_hit<false, false>), grid, block, sh, st, rays_o, rays_d, B, g, vertices, faces, cell_faces, tris, out);
    return check_launch("mesh_first_hit");
}

SCANERF_API int scanerf_mesh_first_enter(const float *rays_o, const float *rays_d, int B, const uint64_t *bitmask, const uint32_t *rank,
                                         const int32_t *start_num, const float *cell_box, const float *scene_info, int log2dim, int lds,
                                         float *out, scanerf_stream_t stream)
{
    if (B == 0) return 0;
    if (int r = require_trace_args("mesh_first_enter", B, rays_o, rays_d, bitmask, rank, start_num, scene_info, out, log2dim, lds)) return r;
    SCANERF_REQUIRE(cell_box, "mesh_first_enter: null pointer");
    const Grid g = { bitmask, rank, start_num, scene_info, log2dim };
    const dim3 grid(trace_grid(B, lds)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (lds) hipLaunchKernelGGL(k_first_enter<true>, grid, block, lds_bytes(log2dim), st, rays_o, rays_d, B, g, cell_box, out);
    else hipLaunchKernelGGL(k_first_enter<false>, grid, block, 0, st, rays_o, rays_d, B, g, cell_box, out);
    return check_launch("mesh_first_enter");
}
