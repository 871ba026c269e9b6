// mesh_visibility_device.h -- the (point, camera) pair of the point-visibility op (include/scanerf_mesh_tools_hip.h): the in-view
// test and the segment-limited any-hit walk, shared by mesh_visibility.hip and mesh_colors.hip so that both decide "seen" with the
// same operands, the same walk and the same early ends.  Include only from files built with -ffp-contract=off.
#pragma once
#include "mesh_device.h"

namespace {

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the in-view test of the definition
__device__ __forceinline__ bool in_view(const float p[3], bool finite, const float *__restrict__ K, const float *__restrict__ T, float Hf,
                                        float Wf, float bias, float near, float far)
{
    const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const float w[3] = { p[0] - T[3], p[1] - T[7], p[2] - T[11] };
    const float xc = (w[0] * T[0] + w[1] * T[4]) + w[2] * T[8];
    const float yc = (w[0] * T[1] + w[1] * T[5]) + w[2] * T[9];
    const float zc = (w[0] * T[2] + w[1] * T[6]) + w[2] * T[10];
    const float len = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    const float px = fx * (xc / zc) + cx, py = fy * (yc / zc) + cy;
    return finite && zc > near && len <= far && len > bias && px >= 0.0f && px < Wf && py >= 0.0f && py < Hf;
}

// true iff some registered face meets the segment o + t d at 0 < t < 1
template <bool PRE, bool COUNT>
__device__ __forceinline__ bool segment_hidden(const float o[3], const float d[3], const Grid &g, const Words<false> &words,
                                               const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                               const int32_t *__restrict__ cell_faces, const float *__restrict__ tris,
                                               unsigned long long &n_cells, unsigned long long &n_tests)
{
    RayWalk rw;
    if (!rw.start(o, d, g)) return false;
    while (!rw.done()) {
        rw.w.pick();
        const int c = words.lookup(rw.cell(g.L));
        if (c >= 0) {
            if (COUNT) ++n_cells;
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
                if (COUNT) ++n_tests;
                const float t = ray_triangle(o, d, A, e1, e2);
                if (t > 0.0f && t < 1.0f) return true;
            }
        }
        if (rw.w.t1 >= 1.0f) break;   // the eye lies in this cell or before it
        rw.w.advance();
    }
    return false;
}

}  // namespace
