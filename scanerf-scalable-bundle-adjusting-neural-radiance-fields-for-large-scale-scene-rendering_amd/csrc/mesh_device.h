// mesh_device.h -- the device side of the ray / triangle-mesh tracer shared by its kernels: the traces of mesh.hip, the fused
// view-coverage kernel of coverage.hip and the hit-record kernels of mesh_render.hip.  The structure's arrays are described in mesh.hip.  Include only from files built with
// -ffp-contract=off (dda_device.h).  Everything here sits in an unnamed namespace, as it did inside mesh.hip: Grid is a kernel
// parameter, so its namespace is part of the kernels' names in csrc/isa_manifest.json.
#pragma once
#include "dda_device.h"

using namespace scanerf;

namespace {

constexpr float kInf = 3.0e38f;

struct Grid {
    const uint64_t *bitmask;   // [2^(3L) / 64]
    const uint32_t *rank;      // [2^(3L) / 64]
    const int32_t *start_num;  // [C,2]
    const float *scene_info;   // [4]
    int L;
};

// The bitmask and rank words of a workgroup's lookups: global memory (L2-resident: 32 KB + 16 KB at L = 6), or staged into the LDS.
template <bool LDS>
struct Words {
    const uint64_t *bm;
    const uint32_t *rk;
    __device__ __forceinline__ Words(const Grid &g, uint64_t *lds)
    {
        if (LDS) {
            const int nw = 1 << (3 * g.L - 6);
            uint32_t *lrk = reinterpret_cast<uint32_t *>(lds + nw);
            for (int i = threadIdx.x; i < nw; i += blockDim.x) {
                lds[i] = g.bitmask[i];
                lrk[i] = g.rank[i];
            }
            __syncthreads();
            bm = lds;
            rk = lrk;
        } else {
            bm = g.bitmask;
            rk = g.rank;
        }
    }
    // ordinal of the occupied cell n, or -1
    __device__ __forceinline__ int lookup(uint32_t n) const
    {
        const uint64_t w = bm[n >> 6];
        const uint64_t bit = 1ull << (n & 63u);
        if (!(w & bit)) return -1;
        return (int)(rk[n >> 6] + (uint32_t)__popcll(w & (bit - 1ull)));
    }
};

// Moeller-Trumbore, two-sided, edges inclusive; A, e1 = B - A, e2 = C - A.  Returns t, or -1 for no intersection.
__device__ __forceinline__ float ray_triangle(const float o[3], const float d[3], const float A[3], const float e1[3], const float e2[3])
{
    const float p[3] = { d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0] };
    const float det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (!(fabsf(det) > 1e-12f)) return -1.0f;
    const float inv = 1.0f / det;
    const float tv[3] = { o[0] - A[0], o[1] - A[1], o[2] - A[2] };
    const float u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) * inv;
    const float q[3] = { tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0] };
    const float v = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) * inv;
    const float t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv;
    return (u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t > 0.0f) ? t : -1.0f;
}

struct RayWalk {
    Walker w;
    int left;   // steps still allowed: a walk crosses at most 3 * side cells; the cap ends a walk over non-finite input
    __device__ __forceinline__ bool start(const float o[3], const float d[3], const Grid &g)
    {
        const int side = 1 << g.L;
        const float cell = g.scene_info[3];
        const float half = (float)side * cell / 2.0f;
        const float corner[3] = { g.scene_info[0], g.scene_info[1], g.scene_info[2] };
        const float ctr[3] = { corner[0] + half, corner[1] + half, corner[2] + half };
        const float h3[3] = { half, half, half };
        const F2 span = clip_box(o, d, ctr, h3);
        if (span.x == -1.0f) return false;
        const float og[3] = { o[0] - corner[0], o[1] - corner[1], o[2] - corner[2] };
        const int s3[3] = { side, side, side };
        const float cs[3] = { cell, cell, cell };
        w.start(og, d, span, s3, cs);
        left = 3 * side + 3;
        return true;
    }
    __device__ __forceinline__ bool done() { return left-- <= 0 || w.done(); }
    __device__ __forceinline__ uint32_t cell(int L) const
    {
        return ((uint32_t)w.cell[0] << (2 * L)) | ((uint32_t)w.cell[1] << L) | (uint32_t)w.cell[2];
    }
};

// The first-hit walk of one ray: nearest intersection t > 0 over the cells the ray crosses, the candidate carried ACROSS cells until
// it is not beyond the current cell's exit; 0 = nothing.  PRE: pre-gathered triangles (tris), else vertices / faces / cell_faces.
template <bool LDS, bool PRE>
__device__ __forceinline__ float first_hit_walk(const float o[3], const float d[3], const Grid &g, const Words<LDS> &words,
                                                const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                const int32_t *__restrict__ cell_faces, const float *__restrict__ tris)
{
    float best = kInf;
    RayWalk rw;
    if (rw.start(o, d, g)) {
        while (!rw.done()) {
            rw.w.pick();
            const int c = words.lookup(rw.cell(g.L));
            if (c >= 0) {
                const int start = g.start_num[2 * c], num = g.start_num[2 * c + 1];
                for (int k = 0; k < num; ++k) {
                    float A[3], e1[3], e2[3];
                    if (PRE) {
                        const float *t = tris + 9 * (size_t)(start + k);
#pragma unroll
                        for (int a = 0; a < 3; ++a) { A[a] = t[a]; e1[a] = t[3 + a]; e2[a] = t[6 + a]; }
                    } else {
                        const int f = cell_faces[start + k];
                        const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            A[a] = vertices[3 * ia + a];
                            e1[a] = vertices[3 * ib + a] - A[a];
                            e2[a] = vertices[3 * ic + a] - A[a];
                        }
                    }
                    const float t = ray_triangle(o, d, A, e1, e2);
                    if (t > 0.0f && t < best) best = t;
                }
            }
            if (best <= rw.w.t1) break;   // nothing in a later cell can be nearer
            rw.w.advance();
        }
    }
    return best < kInf ? best : 0.0f;
}

// ---- the hit record (mesh_render.hip; include/scanerf_mesh_tools_hip.h): which face, and where on it ----------------------------

struct TriHit {
    float t, u, v;   // t = -1: no intersection (u, v then mean nothing)
};

// ray_triangle with its barycentrics kept: the same operations in the same order, so t has ray_triangle's bits.
__device__ __forceinline__ TriHit ray_triangle_uv(const float o[3], const float d[3], const float A[3], const float e1[3], const float e2[3])
{
    TriHit r = { -1.0f, 0.0f, 0.0f };
    const float p[3] = { d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0] };
    const float det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (!(fabsf(det) > 1e-12f)) return r;
    const float inv = 1.0f / det;
    const float tv[3] = { o[0] - A[0], o[1] - A[1], o[2] - A[2] };
    const float u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) * inv;
    const float q[3] = { tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0] };
    const float v = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) * inv;
    const float t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv;
    if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t > 0.0f) {
        r.t = t;
        r.u = u;
        r.v = v;
    }
    return r;
}

// The nearest hit as (t, face, u, v).  Candidates are compared as (t, face index): a later face or a later cell replaces the
// candidate only with a smaller t, or an equal t and a lower index, so the answer does not depend on the order of the tests.
struct HitRecord {
    float t;
    int face;
    float u, v;
    __device__ __forceinline__ void clear()
    {
        t = kInf;
        face = 0x7fffffff;
        u = v = 0.0f;
    }
    __device__ __forceinline__ void offer(const float o[3], const float d[3], const float A[3], const float e1[3], const float e2[3], int f)
    {
        const TriHit h = ray_triangle_uv(o, d, A, e1, e2);
        if (h.t > 0.0f && (h.t < t || (h.t == t && f < face))) {   // (a NaN is never taken)
            t = h.t;
            face = f;
            u = h.u;
            v = h.v;
        }
    }
    // the miss: t = 0, face = -1, u = v = 0
    __device__ __forceinline__ void finish()
    {
        if (!(t < kInf)) {
            t = 0.0f;
            face = -1;
            u = v = 0.0f;
        }
    }
};

// first_hit_walk with the record kept: the same cells, the same tests, the same stop rule (the candidate's t against the cell's
// exit), so t has first_hit_walk's bits.  cell_faces names the faces in both triangle forms.  A face that ties the candidate
// exactly at the exit of the cell the walk stops in, and is registered only beyond it, is never tested: face is the lowest index
// among the faces the walk tested.
template <bool LDS, bool PRE>
__device__ __forceinline__ HitRecord hit_record_walk(const float o[3], const float d[3], const Grid &g, const Words<LDS> &words,
                                                     const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                     const int32_t *__restrict__ cell_faces, const float *__restrict__ tris)
{
    HitRecord best;
    best.clear();
    RayWalk rw;
    if (rw.start(o, d, g)) {
        while (!rw.done()) {
            rw.w.pick();
            const int c = words.lookup(rw.cell(g.L));
            if (c >= 0) {
                const int start = g.start_num[2 * c], num = g.start_num[2 * c + 1];
                for (int k = 0; k < num; ++k) {
                    const int f = cell_faces[start + k];
                    float A[3], e1[3], e2[3];
                    if (PRE) {
                        const float *t = tris + 9 * (size_t)(start + k);
#pragma unroll
                        for (int a = 0; a < 3; ++a) { A[a] = t[a]; e1[a] = t[3 + a]; e2[a] = t[6 + a]; }
                    } else {
                        const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            A[a] = vertices[3 * ia + a];
                            e1[a] = vertices[3 * ib + a] - A[a];
                            e2[a] = vertices[3 * ic + a] - A[a];
                        }
                    }
                    best.offer(o, d, A, e1, e2, f);
                }
            }
            if (best.t <= rw.w.t1) break;   // nothing in a later cell can be nearer
            rw.w.advance();
        }
    }
    best.finish();
    return best;
}

}  // namespace
