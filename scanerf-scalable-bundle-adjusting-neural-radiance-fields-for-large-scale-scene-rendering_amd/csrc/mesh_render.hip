// mesh_render.hip -- the hit record of the mesh tracer and the rendering of a mesh with its vertex attributes through a set of
// cameras: what "look at the coloured mesh from the capture's cameras and compare it with the field's renders"
// needs.  The reference has no counterpart; the definition is the comment in include/scanerf_mesh_tools_hip.h.  The structure is the
// tracer's (mesh.hip), read as it is; the walk and the ray / triangle test are mesh_device.h's (hit_record_walk, ray_triangle_uv).
//
// k_trace: one ray per lane, as k_first_hit.  k_trace_brute: the witness, every registered face in index order through the same
// HitRecord::offer.  k_render_views: one wavefront per 8 x 8 pixel block of one camera (lane = 8 * row + column; the lanes beyond the
// right and bottom borders idle): the rays of a block stay together in the grid, which is what DESIGN.md 4.10 measured for frames
// and could not apply to a caller's ray list.  The ray is k_compute_ray_fwd's (rays.hip), formed in registers and stored nowhere.
// The attributes are gathered once per pixel, after the walk, from the winning face's three vertices.
// Built without FMA contraction.  No LDS, no atomics, no allocation, no host synchronisation; every output element is written exactly
// once by a plain store; the mapping of pixels to lanes decides no bit.
#include "mesh_device.h"

#include "scanerf_mesh_tools_hip.h"

namespace {

// Does the ray meet the grid cube at all?  RayWalk::start's clip, for the route without a walk.
__device__ __forceinline__ bool meets_cube(const float o[3], const float d[3], const float *__restrict__ scene_info, int L)
{
    const int side = 1 << L;
    const float cell = scene_info[3];
    const float half = (float)side * cell / 2.0f;
    const float ctr[3] = { scene_info[0] + half, scene_info[1] + half, scene_info[2] + half };
    const float h3[3] = { half, half, half };
    return clip_box(o, d, ctr, h3).x != -1.0f;
}

template <bool PRE>
__global__ void __launch_bounds__(256) k_trace(const float *__restrict__ rays_o, const float *__restrict__ rays_d, int B, Grid g,
                                               const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                               const int32_t *__restrict__ cell_faces, const float *__restrict__ tris,
                                               float *__restrict__ out_t, int32_t *__restrict__ out_face, float *__restrict__ out_bary)
{
    const Words<false> words(g, nullptr);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const float o[3] = { rays_o[3 * (size_t)i], rays_o[3 * (size_t)i + 1], rays_o[3 * (size_t)i + 2] };
    const float d[3] = { rays_d[3 * (size_t)i], rays_d[3 * (size_t)i + 1], rays_d[3 * (size_t)i + 2] };
    const HitRecord h = hit_record_walk<false, PRE>(o, d, g, words, vertices, faces, cell_faces, tris);
    out_t[i] = h.t;
    out_face[i] = h.face;
    out_bary[2 * (size_t)i] = h.u;
    out_bary[2 * (size_t)i + 1] = h.v;
}

// every face, no grid; a face answers iff the build registers it (mesh.hip face_cells: indices in [0, V), box not outside the cube,
// cell > 0), and a ray answers iff it meets the cube
__global__ void __launch_bounds__(256) k_trace_brute(const float *__restrict__ rays_o, const float *__restrict__ rays_d, int B,
                                                     const float *__restrict__ vertices, const int32_t *__restrict__ faces, int V, int F,
                                                     const float *__restrict__ scene_info, int L, float *__restrict__ out_t,
                                                     int32_t *__restrict__ out_face, float *__restrict__ out_bary)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const float o[3] = { rays_o[3 * (size_t)i], rays_o[3 * (size_t)i + 1], rays_o[3 * (size_t)i + 2] };
    const float d[3] = { rays_d[3 * (size_t)i], rays_d[3 * (size_t)i + 1], rays_d[3 * (size_t)i + 2] };
    HitRecord best;
    best.clear();
    if (F > 0 && meets_cube(o, d, scene_info, L)) {
        const float cell = scene_info[3], side = (float)(1 << L);
        for (int f = 0; f < F; ++f) {
            const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
            if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) continue;
            float A[3], e1[3], e2[3];
            bool out = !(cell > 0.0f);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float Aa = vertices[3 * (size_t)ia + a], Ba = vertices[3 * (size_t)ib + a], Ca = vertices[3 * (size_t)ic + a];
                const float gmin = scene_info[a], gmax = gmin + side * cell;
                out |= fmaxf(fmaxf(Aa, Ba), Ca) < gmin || fminf(fminf(Aa, Ba), Ca) > gmax;
                A[a] = Aa;
                e1[a] = Ba - Aa;
                e2[a] = Ca - Aa;
            }
            if (!out) best.offer(o, d, A, e1, e2, f);
        }
    }
    best.finish();
    out_t[i] = best.t;
    out_face[i] = best.face;
    out_bary[2 * (size_t)i] = best.u;
    out_bary[2 * (size_t)i + 1] = best.v;
}

// n / (|n| + 1e-8), the rule of the fused mesh's normals (tsdf.hip)
__device__ __forceinline__ void store_unit(float *__restrict__ out, const float n[3])
{
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) + 1e-8f;
    out[0] = n[0] / len;
    out[1] = n[1] / len;
    out[2] = n[2] / len;
}

template <bool PRE>
__global__ void __launch_bounds__(256) k_render_views(const float *__restrict__ Ks, const float *__restrict__ C2Ws, int H, int W,
                                                      int tiles_x, int tiles_y, int n_tiles, Grid g, const float *__restrict__ vertices,
                                                      const int32_t *__restrict__ faces, const int32_t *__restrict__ cell_faces,
                                                      const float *__restrict__ tris, const float *__restrict__ vertex_normals,
                                                      const float *__restrict__ vertex_colors, float *__restrict__ out_depth,
                                                      int32_t *__restrict__ out_face, float *__restrict__ out_normal,
                                                      float *__restrict__ out_color)
{
    const Words<false> words(g, nullptr);
    const int lane = threadIdx.x & 63;
    const int waves = blockDim.x >> 6;
    // (tile is wave-uniform; the stride keeps any image count inside one launch)
    for (long long tile = (long long)blockIdx.x * waves + (threadIdx.x >> 6); tile < n_tiles; tile += (long long)gridDim.x * waves) {
        const int per_cam = tiles_x * tiles_y;
        const int cam = (int)(tile / per_cam), rest = (int)(tile - (long long)cam * per_cam);
        const int by = rest / tiles_x, bx = rest - by * tiles_x;
        const int px = 8 * bx + (lane & 7), py = 8 * by + (lane >> 3);
        if (px >= W || py >= H) continue;
        const float *K = Ks + 9 * (size_t)cam, *M = C2Ws + 12 * (size_t)cam;
        const float x = (1.0f * px + 0.5f - K[2]) / K[0];
        const float y = (1.0f * py + 0.5f - K[5]) / K[4];
        const float d[3] = { M[0] * x + M[1] * y + M[2], M[4] * x + M[5] * y + M[6], M[8] * x + M[9] * y + M[10] };
        const float o[3] = { M[3], M[7], M[11] };
        const HitRecord h = hit_record_walk<false, PRE>(o, d, g, words, vertices, faces, cell_faces, tris);
        const size_t at = ((size_t)cam * H + py) * W + px;
        out_depth[at] = h.t;
        out_face[at] = h.face;
        if (!out_normal && !out_color) continue;
        if (h.face < 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (out_normal) out_normal[3 * at + a] = 0.0f;
                if (out_color) out_color[3 * at + a] = 0.0f;
            }
            continue;
        }
        const size_t ia = (size_t)faces[3 * (size_t)h.face], ib = (size_t)faces[3 * (size_t)h.face + 1], ic = (size_t)faces[3 * (size_t)h.face + 2];
        const float w0 = (1.0f - h.u) - h.v;
        if (out_normal) {
            float n[3];
            if (vertex_normals) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    n[a] = (w0 * vertex_normals[3 * ia + a] + h.u * vertex_normals[3 * ib + a]) + h.v * vertex_normals[3 * ic + a];
            } else {
                float e1[3], e2[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float A = vertices[3 * ia + a];
                    e1[a] = vertices[3 * ib + a] - A;
                    e2[a] = vertices[3 * ic + a] - A;
                }
                n[0] = e1[1] * e2[2] - e1[2] * e2[1];
                n[1] = e1[2] * e2[0] - e1[0] * e2[2];
                n[2] = e1[0] * e2[1] - e1[1] * e2[0];
            }
            store_unit(out_normal + 3 * at, n);
        }
        if (out_color) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
                out_color[3 * at + a] = (w0 * vertex_colors[3 * ia + a] + h.u * vertex_colors[3 * ib + a]) + h.v * vertex_colors[3 * ic + a];
        }
    }
}

int require_trace(const char *what, int B, int log2dim, const void *rays_o, const void *rays_d, const void *scene_info, const void *t,
                  const void *face, const void *bary)
{
    SCANERF_REQUIRE(B > 0 && B <= (1 << 29), "%s: B=%d", what, B);
    SCANERF_REQUIRE(log2dim >= 4 && log2dim <= 7, "%s: log2dim=%d outside 4..7", what, log2dim);
    SCANERF_REQUIRE(rays_o && rays_d && scene_info && t && face && bary, "%s: null pointer", what);
    return 0;
}

}  // namespace

SCANERF_API int scanerf_mesh_trace(const float *rays_o, const float *rays_d, int B, const float *vertices, const int32_t *faces,
                                   const float *tris, const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                                   const int32_t *cell_faces, const float *scene_info, int log2dim, float *t, int32_t *face, float *bary,
                                   scanerf_stream_t stream)
{
    if (B == 0) return 0;
    if (int r = require_trace("mesh_trace", B, log2dim, rays_o, rays_d, scene_info, t, face, bary)) return r;
    SCANERF_REQUIRE(bitmask && rank && start_num && cell_faces, "mesh_trace: null pointer");
    SCANERF_REQUIRE(tris || (vertices && faces), "mesh_trace: null pointer (neither triangles nor an indexed mesh)");
    const Grid g = { bitmask, rank, start_num, scene_info, log2dim };
    const dim3 grid(ceil_div(B, 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (tris) hipLaunchKernelGGL(k_trace<true>, grid, block, 0, st, rays_o, rays_d, B, g, vertices, faces, cell_faces, tris, t, face, bary);
    else hipLaunchKernelGGL(k_trace<false>, grid, block, 0, st, rays_o, rays_d, B, g, vertices, faces, cell_faces, tris, t, face, bary);
    return check_launch("mesh_trace");
}

SCANERF_API int scanerf_mesh_trace_brute(const float *rays_o, const float *rays_d, int B, const float *vertices, const int32_t *faces,
                                         int V, int F, const float *scene_info, int log2dim, float *t, int32_t *face, float *bary,
                                         scanerf_stream_t stream)
{
    if (B == 0) return 0;
    if (int r = require_trace("mesh_trace_brute", B, log2dim, rays_o, rays_d, scene_info, t, face, bary)) return r;
    SCANERF_REQUIRE(V >= 0 && F >= 0, "mesh_trace_brute: V=%d F=%d", V, F);
    SCANERF_REQUIRE(F == 0 || (vertices && faces), "mesh_trace_brute: null pointer");
    hipLaunchKernelGGL(k_trace_brute, dim3(ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, B, vertices, faces, V,
                       F, scene_info, log2dim, t, face, bary);
    return check_launch("mesh_trace_brute");
}

SCANERF_API int scanerf_mesh_render_views(const float *Ks, const float *C2Ws, int C, int H, int W, const float *vertices,
                                          const int32_t *faces, const float *tris, const uint64_t *bitmask, const uint32_t *rank,
                                          const int32_t *start_num, const int32_t *cell_faces, const float *scene_info, int log2dim,
                                          const float *vertex_normals, const float *vertex_colors, float *depth, int32_t *face,
                                          float *normal, float *color, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(C >= 0, "mesh_render_views: C=%d", C);
    SCANERF_REQUIRE(H >= 1 && W >= 1, "mesh_render_views: H=%d W=%d", H, W);
    SCANERF_REQUIRE((long long)C * H * W < ((long long)1 << 31), "mesh_render_views: C * H * W = %lld does not fit 31 bits",
                    (long long)C * H * W);
    SCANERF_REQUIRE(log2dim >= 4 && log2dim <= 7, "mesh_render_views: log2dim=%d outside 4..7", log2dim);
    SCANERF_REQUIRE(Ks && C2Ws && vertices && faces && bitmask && rank && start_num && cell_faces && scene_info && depth && face,
                    "mesh_render_views: null pointer");
    SCANERF_REQUIRE(!color || vertex_colors, "mesh_render_views: a color output needs vertex_colors");
    if (C == 0) return 0;
    const int tiles_x = ceil_div(W, 8), tiles_y = ceil_div(H, 8);
    const long long n_tiles = (long long)C * tiles_x * tiles_y;   // < 2^31: every block holds a pixel
    const Grid g = { bitmask, rank, start_num, scene_info, log2dim };
    const dim3 grid(stream_grid(n_tiles, 4, 1 << 22)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (tris)
        hipLaunchKernelGGL(k_render_views<true>, grid, block, 0, st, Ks, C2Ws, H, W, tiles_x, tiles_y, (int)n_tiles, g, vertices, faces,
                           cell_faces, tris, vertex_normals, vertex_colors, depth, face, normal, color);
    else
        hipLaunchKernelGGL(k_render_views<false>, grid, block, 0, st, Ks, C2Ws, H, W, tiles_x, tiles_y, (int)n_tiles, g, vertices, faces,
                           cell_faces, tris, vertex_normals, vertex_colors, depth, face, normal, color);
    return check_launch("mesh_render_views");
}
