// tsdf.hip -- depth-map fusion into a truncated signed distance volume: every lattice point against every camera's
// depth map, the sums (S, Wt) per point; then the value lattice the surface-nets op cuts at 0.5 and the observed-corner count of a
// mesh vertex's cell.  The reference has no counterpart; the definition is the comment in include/scanerf_mesh_tools_hip.h.
//
// A WORKGROUP of 256 threads owns a block of kBX x kBY x 64 lattice points: a wavefront's 64 lanes run along z, the fastest axis of
// [nx+1, ny+1, nz+1], so its accumulator load and store are 512 contiguous bytes and its 64 depth gathers of one camera fall on
// neighbouring pixels; the four wavefronts are the block's (x, y) columns.  Each thread owns ONE point for all cameras: (S, Wt) live
// in two registers from one load to at most one store, no atomics.
//
// COLOUR: k_tsdf_integrate<COUNT, true> also owns the point's (R, G, B, Wc) of cacc [P,4], one 16-byte load, four
// registers, at most one 16-byte store.  An observed pair with sdf <= trunc whose pixel of colors [C,H,W,3] is finite in all three
// channels adds the pixel to them: the three gathers happen only for such a pair (a free-space pair, sdf > trunc, shows a surface
// further away).  <COUNT, false> is the kernel of 4.20, instruction for instruction.  k_tsdf_vertex_colors reads the sums back at a
// mesh vertex: the eight corners of its cell weighted trilinearly, sums and weight interpolated separately, then one division.
//
// NORMALS: k_tsdf_vertex_normals reads the value lattice back at a mesh vertex: per corner of its cell and per axis the
// difference of the observed neighbours' values (central, or one-sided where a neighbour is missing), weighted trilinearly; -G
// normalised is the normal.  One thread per vertex, the 32 points of the stencil loaded once each; see the kernel.
//
// The camera loop runs inside the kernel, in passes of kCamsPerPass.  Per pass the workgroup copies the cameras' 21 floats into the
// LDS (coalesced), then thread t decides whether camera t can be skipped for the whole block, then every thread walks the cameras in
// ascending order; the 21 floats are wave-uniform LDS reads (one address per instruction: a broadcast).
//
// THE SKIP.  Ball: centre c = the midpoint of the block's corner points (formed exactly as the points are, so by the monotonicity of
// float32 + and * every point of the block lies in the corner box), radius r = the half diagonal times (1 + 2^-16).  With w = c - E:
//   behind:   zc(c) + r |R2|            <  near - m |R2|             every point has zc <= near
//   left:     g(c)  + r |fx R0 + cx R2|       < -m M,   g = fx xc + cx zc          every point with zc > 0 has u < 0
//   right:    g'(c) - r |fx R0 + (cx-W) R2|   >  m M,   g' = fx xc + (cx - W) zc   every point with zc > 0 has u >= W
//   top / bottom likewise with fy, cy, H and column 1,
// M = |fx| |R0| + (|cx| + W) |R2| (resp. fy, R1, cy, H), m = 2^-16 (|w| + r): THE MARGIN.  What it has to cover: the kernel's xc, zc
// carry at most 4 ulp of |w| |R_k| each, the quotient, the product and the sum of u three more roundings, u < (float)W one ulp of W,
// so a point the float32 test puts in view has g >= -8 u |w| M (resp. g' <= 8 u |w| M, zc > near - 4 u |w| |R2|) with u = 2^-24; the
// skip's own arithmetic (about a dozen roundings of the same magnitudes) adds as much again.  2^-16 = 256 u is ten times both.  The
// halfspace forms hold for any matrix R and any sign of fx, fy; a non-finite camera or block makes every comparison false: no skip.
// A skipped pair would have been "not in view" for every point: the skip never changes a bit (tests/test_gpu_tsdf.py compares with a
// route that has no skip, bit for bit).
#include "common.h"

#include "scanerf_mesh_tools_hip.h"

using namespace scanerf;

namespace {

constexpr int kThreads = 256;
constexpr int kBX = 2, kBY = 2, kBZ = kWave;      // the block of points: kBX * kBY wavefronts
constexpr int kCamsPerPass = 64;
constexpr int kCamFloats = 21;                     // K[9] then C2W[12]
constexpr float kSkipMargin = 1.52587890625e-05f;  // 2^-16
static_assert(kBX * kBY * kBZ == kThreads, "one point per thread");
static_assert(kCamsPerPass <= kThreads, "thread t decides camera t");

struct Lattice {
    float origin[3], spacing[3];
    int n[3];
};

__device__ __forceinline__ float len3(float a, float b, float c) { return sqrtf((a * a + b * b) + c * c); }

// can camera `cam` (21 floats) be skipped for the ball (c, r)?  See THE SKIP above; every test is false on a NaN.
__device__ __forceinline__ bool skip_camera(const float *cam, const float c[3], float r, float Hf, float Wf, float near)
{
    const float *K = cam, *T = cam + 9;
    const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const float w[3] = { c[0] - T[3], c[1] - T[7], c[2] - T[11] };
    const float R0[3] = { T[0], T[4], T[8] }, R1[3] = { T[1], T[5], T[9] }, R2[3] = { T[2], T[6], T[10] };
    const float l0 = len3(R0[0], R0[1], R0[2]), l1 = len3(R1[0], R1[1], R1[2]), l2 = len3(R2[0], R2[1], R2[2]);
    const float xc = (w[0] * R0[0] + w[1] * R0[1]) + w[2] * R0[2];
    const float yc = (w[0] * R1[0] + w[1] * R1[1]) + w[2] * R1[2];
    const float zc = (w[0] * R2[0] + w[1] * R2[1]) + w[2] * R2[2];
    const float m = kSkipMargin * (len3(w[0], w[1], w[2]) + r);
    if (zc + r * l2 < near - m * l2) return true;
    const float Mx = fabsf(fx) * l0 + (fabsf(cx) + Wf) * l2, My = fabsf(fy) * l1 + (fabsf(cy) + Hf) * l2;
    const float cw = cx - Wf, ch = cy - Hf;
    const float nl = len3(fx * R0[0] + cx * R2[0], fx * R0[1] + cx * R2[1], fx * R0[2] + cx * R2[2]);
    const float nr = len3(fx * R0[0] + cw * R2[0], fx * R0[1] + cw * R2[1], fx * R0[2] + cw * R2[2]);
    const float nt = len3(fy * R1[0] + cy * R2[0], fy * R1[1] + cy * R2[1], fy * R1[2] + cy * R2[2]);
    const float nb = len3(fy * R1[0] + ch * R2[0], fy * R1[1] + ch * R2[1], fy * R1[2] + ch * R2[2]);
    if ((fx * xc + cx * zc) + r * nl < -(m * Mx)) return true;
    if ((fx * xc + cw * zc) - r * nr > m * Mx) return true;
    if ((fy * yc + cy * zc) + r * nt < -(m * My)) return true;
    if ((fy * yc + ch * zc) - r * nb > m * My) return true;
    return false;
}

template <bool COUNT, bool COLOR>
__global__ void __launch_bounds__(kThreads) k_tsdf_integrate(const float *__restrict__ depths, const float *__restrict__ Ks,
                                                             const float *__restrict__ C2Ws, int C, int H, int W, Lattice L, int tiles_y,
                                                             int tiles_z, float trunc, float near, float far, float2 *__restrict__ acc,
                                                             unsigned long long *__restrict__ counters,
                                                             const float *__restrict__ colors, float4 *__restrict__ cacc)
{
    constexpr int kTally = COLOR ? 4 : 3;
    __shared__ float cams[kCamsPerPass * kCamFloats];
    __shared__ int skip[kCamsPerPass];
    __shared__ unsigned long long tally[kTally];

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    // the block's tile (block-uniform) and this thread's point
    const int tz = (int)(blockIdx.x % (unsigned)tiles_z), ty = (int)((blockIdx.x / (unsigned)tiles_z) % (unsigned)tiles_y);
    const int tx = (int)(blockIdx.x / ((unsigned)tiles_z * (unsigned)tiles_y));
    const int lo[3] = { tx * kBX, ty * kBY, tz * kBZ };
    const int idx[3] = { lo[0] + wave / kBY, lo[1] + wave % kBY, lo[2] + lane };
    const bool live = idx[0] <= L.n[0] && idx[1] <= L.n[1] && idx[2] <= L.n[2];
    const size_t p = ((size_t)idx[0] * (size_t)(L.n[1] + 1) + (size_t)idx[1]) * (size_t)(L.n[2] + 1) + (size_t)idx[2];
    float P[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) P[a] = L.origin[a] + (float)idx[a] * L.spacing[a];

    // the ball around the block's live points
    float ctr[3], half[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int ext = a == 0 ? kBX : a == 1 ? kBY : kBZ;
        const int hi = min(lo[a] + ext - 1, L.n[a]);
        const float pl = L.origin[a] + (float)lo[a] * L.spacing[a], ph = L.origin[a] + (float)hi * L.spacing[a];
        ctr[a] = 0.5f * pl + 0.5f * ph;
        half[a] = fmaxf(ph - ctr[a], ctr[a] - pl);
    }
    const float radius = len3(half[0], half[1], half[2]) * (1.0f + kSkipMargin);
    const float Hf = (float)H, Wf = (float)W;
    const float ninf = -__builtin_huge_valf(), pinf = __builtin_huge_valf();

    float2 sw = make_float2(0.0f, 0.0f);
    if (live) sw = acc[p];
    bool touched = false;
    float4 cw = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool coloured = false;
    if (COLOR) {
        if (live) cw = cacc[p];
    }
    unsigned long long n_pairs = 0, n_updates = 0, n_skipped = 0, n_coloured = 0;
    if (COUNT) {
        if (threadIdx.x < kTally) tally[threadIdx.x] = 0ull;
    }

    for (int cbase = 0; cbase < C; cbase += kCamsPerPass) {
        const int ncam = min(kCamsPerPass, C - cbase);
        __syncthreads();   // the previous pass's cameras have been read by every wavefront
        for (int t = threadIdx.x; t < ncam * 9; t += kThreads) cams[(t / 9) * kCamFloats + t % 9] = Ks[(size_t)cbase * 9 + t];
        for (int t = threadIdx.x; t < ncam * 12; t += kThreads) cams[(t / 12) * kCamFloats + 9 + t % 12] = C2Ws[(size_t)cbase * 12 + t];
        __syncthreads();
        if ((int)threadIdx.x < ncam) skip[threadIdx.x] = skip_camera(cams + threadIdx.x * kCamFloats, ctr, radius, Hf, Wf, near) ? 1 : 0;
        __syncthreads();
        for (int cc = 0; cc < ncam; ++cc) {
            if (__builtin_amdgcn_readfirstlane(skip[cc])) {   // block-uniform
                if (COUNT) ++n_skipped;
                continue;
            }
            const float *K = cams + cc * kCamFloats, *T = K + 9;
            const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
            const float w[3] = { P[0] - T[3], P[1] - T[7], P[2] - T[11] };
            const float xc = (w[0] * T[0] + w[1] * T[4]) + w[2] * T[8];
            const float yc = (w[0] * T[1] + w[1] * T[5]) + w[2] * T[9];
            const float zc = (w[0] * T[2] + w[1] * T[6]) + w[2] * T[10];
            const float u = fx * (xc / zc) + cx, v = fy * (yc / zc) + cy;
            const bool inview = live && zc > near && u >= 0.0f && u < Wf && v >= 0.0f && v < Hf;
            if (COUNT) n_pairs += live ? 1ull : 0ull;
            if (inview) {
                const int px = (int)u, py = (int)v;   // 0 <= px < W, 0 <= py < H by the test above
                const size_t pixel = ((size_t)(cbase + cc) * (size_t)H + (size_t)py) * (size_t)W + (size_t)px;
                const float D = depths[pixel];
                const bool valid = D > ninf && D < pinf && D > near && D <= far;
                const float sdf = D - zc;
                if (valid && sdf >= -trunc) {
                    sw.x = sw.x + fminf(1.0f, sdf / trunc);
                    sw.y = sw.y + 1.0f;
                    touched = true;
                    if (COUNT) ++n_updates;
                    if (COLOR) {
                        if (sdf <= trunc) {   // in the band: the pixel shows THIS surface (pixel < C H W: in bounds of colors)
                            const float *rgb = colors + 3 * pixel;
                            const float r = rgb[0], g = rgb[1], b = rgb[2];
                            if (r > ninf && r < pinf && g > ninf && g < pinf && b > ninf && b < pinf) {
                                cw.x = cw.x + r;
                                cw.y = cw.y + g;
                                cw.z = cw.z + b;
                                cw.w = cw.w + 1.0f;
                                coloured = true;
                                if (COUNT) ++n_coloured;
                            }
                        }
                    }
                }
            }
        }
    }
    if (touched) acc[p] = sw;
    if (COLOR) {
        if (coloured) cacc[p] = cw;
    }
    if (COUNT) {
        __syncthreads();
        atomicAdd(&tally[0], n_pairs);
        atomicAdd(&tally[2], n_updates);
        if (COLOR) atomicAdd(&tally[3], n_coloured);
        if (threadIdx.x == 0) atomicAdd(&tally[1], n_skipped);
        __syncthreads();
        if (threadIdx.x < kTally) atomicAdd(&counters[threadIdx.x], tally[threadIdx.x]);
    }
}

__global__ void __launch_bounds__(kThreads) k_tsdf_values(const float2 *__restrict__ acc, int P, float min_weight,
                                                          float *__restrict__ values, uint8_t *__restrict__ observed)
{
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < P; p += (int64_t)gridDim.x * kThreads) {
        const float2 sw = acc[p];
        const bool obs = sw.y >= min_weight;
        values[p] = obs ? 0.5f - 0.5f * (sw.x / sw.y) : 0.0f;
        observed[p] = obs ? 1 : 0;
    }
}

__global__ void __launch_bounds__(kThreads) k_tsdf_cell_support(const uint8_t *__restrict__ observed, int nx, int ny, int nz,
                                                                const int32_t *__restrict__ cells, int V, int32_t *__restrict__ support)
{
    for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kThreads) {
        const int a = cells[3 * v], b = cells[3 * v + 1], c = cells[3 * v + 2];
        int s = 0;
        if (a >= 0 && a < nx && b >= 0 && b < ny && c >= 0 && c < nz) {
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const size_t q = ((size_t)(a + (d >> 2)) * (size_t)(ny + 1) + (size_t)(b + ((d >> 1) & 1))) * (size_t)(nz + 1) +
                                 (size_t)(c + (d & 1));
                s += observed[q] != 0 ? 1 : 0;
            }
        }
        support[v] = s;
    }
}

// one thread per vertex: the (R, G, B, Wc) of the eight corners of its cell, weighted trilinearly; see the header for the order
__global__ void __launch_bounds__(kThreads) k_tsdf_vertex_colors(const float4 *__restrict__ cacc, int nx, int ny, int nz,
                                                                 const int32_t *__restrict__ cells, const float *__restrict__ lattice, int V,
                                                                 float *__restrict__ rgb, float *__restrict__ weight)
{
    for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kThreads) {
        const int a = cells[3 * v], b = cells[3 * v + 1], c = cells[3 * v + 2];
        float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a >= 0 && a < nx && b >= 0 && b < ny && c >= 0 && c < nz) {
            const int cell[3] = { a, b, c };
            float w[3][2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float t = fminf(fmaxf(lattice[3 * v + k] - (float)cell[k], 0.0f), 1.0f);
                w[k][0] = 1.0f - t;
                w[k][1] = t;
            }
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const size_t q = ((size_t)(a + (d >> 2)) * (size_t)(ny + 1) + (size_t)(b + ((d >> 1) & 1))) * (size_t)(nz + 1) +
                                 (size_t)(c + (d & 1));
                const float wd = (w[0][d >> 2] * w[1][(d >> 1) & 1]) * w[2][d & 1];
                const float4 s = cacc[q];
                if (d == 0) {
                    sum = make_float4(wd * s.x, wd * s.y, wd * s.z, wd * s.w);
                } else {
                    sum.x = sum.x + wd * s.x;
                    sum.y = sum.y + wd * s.y;
                    sum.z = sum.z + wd * s.z;
                    sum.w = sum.w + wd * s.w;
                }
            }
        }
        const bool any = sum.w > 0.0f;
        rgb[3 * v] = any ? sum.x / sum.w : 0.0f;
        rgb[3 * v + 1] = any ? sum.y / sum.w : 0.0f;
        rgb[3 * v + 2] = any ? sum.z / sum.w : 0.0f;
        weight[v] = sum.w;
    }
}

// one thread per vertex: the volume's own gradient at the vertex; see the header for the definition.  The stencil of a
// cell is 32 distinct lattice points: its 8 corners and, per axis, the 8 points one step beyond them.  Each is loaded once.  Along an
// axis the 8 corners form 4 lines (m, p0, p1, pp): p0 and p1 are corners, m and pp the points beyond.  A vertex is evaluated only when
// all 8 corners are observed, so p0 always has its + neighbour (p1) and p1 its - neighbour (p0): the definition's "neither" branch
// cannot arise here, and both one-sided forms are (val[p1] - val[p0]) / h.  What is left to decide per line is whether m and pp exist
// (inside the lattice and observed).  The loads beyond the cell use a clamped row (the corner's own) where the point is outside, so
// every load is in bounds and none sits behind a branch; numerator and denominator are selected, then divided once: the operations of
// the definition, one division per corner and axis.
__global__ void __launch_bounds__(kThreads) k_tsdf_vertex_normals(const float *__restrict__ values, const uint8_t *__restrict__ observed,
                                                                  int nx, int ny, int nz, float hx, float hy, float hz,
                                                                  const int32_t *__restrict__ cells, const float *__restrict__ lattice, int V,
                                                                  float *__restrict__ normal, float *__restrict__ grad)
{
    for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kThreads) {
        const int cell[3] = { cells[3 * v], cells[3 * v + 1], cells[3 * v + 2] };
        const int n[3] = { nx, ny, nz };
        const size_t stride[3] = { (size_t)(ny + 1) * (size_t)(nz + 1), (size_t)(nz + 1), 1 };
        float G[3] = { 0.0f, 0.0f, 0.0f }, N[3] = { 0.0f, 0.0f, 0.0f };
        bool ok = cell[0] >= 0 && cell[0] < nx && cell[1] >= 0 && cell[1] < ny && cell[2] >= 0 && cell[2] < nz;
        size_t q[8];
        if (ok) {
            const size_t q0 = (size_t)cell[0] * stride[0] + (size_t)cell[1] * stride[1] + (size_t)cell[2];
            int seen = 0;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                q[d] = q0 + (size_t)(d >> 2) * stride[0] + (size_t)((d >> 1) & 1) * stride[1] + (size_t)(d & 1);
                seen += observed[q[d]] != 0 ? 1 : 0;
            }
            ok = seen == 8;
        }
        if (ok) {
            const float h[3] = { hx, hy, hz };
            float val[8], w[3][2], wd[8];
#pragma unroll
            for (int d = 0; d < 8; ++d) val[d] = values[q[d]];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float t = fminf(fmaxf(lattice[3 * v + k] - (float)cell[k], 0.0f), 1.0f);
                w[k][0] = 1.0f - t;
                w[k][1] = t;
            }
#pragma unroll
            for (int d = 0; d < 8; ++d) wd[d] = (w[0][d >> 2] * w[1][(d >> 1) & 1]) * w[2][d & 1];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int bit = 4 >> k;                                      // the corner bit of axis k: (d >> 2, (d >> 1) & 1, d & 1)
                const bool lo = cell[k] >= 1, hi = cell[k] + 2 <= n[k];      // do m = p0 - e_k and pp = p1 + e_k lie inside the lattice?
                const float h2 = h[k] + h[k];
                float g[8];
#pragma unroll
                for (int d0 = 0; d0 < 8; ++d0) {
                    if (d0 & bit) continue;
                    const int d1 = d0 | bit;
                    const size_t qm = lo ? q[d0] - stride[k] : q[d0], qp = hi ? q[d1] + stride[k] : q[d1];
                    const bool has_m = lo && observed[qm] != 0, has_p = hi && observed[qp] != 0;
                    const float vm = values[qm], vp = values[qp];
                    g[d0] = (val[d1] - (has_m ? vm : val[d0])) / (has_m ? h2 : h[k]);
                    g[d1] = ((has_p ? vp : val[d1]) - val[d0]) / (has_p ? h2 : h[k]);
                }
                float s = wd[0] * g[0];
#pragma unroll
                for (int d = 1; d < 8; ++d) s = s + wd[d] * g[d];
                G[k] = s;
            }
            const float len = sqrtf((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
            const float den = len + 1e-8f;
#pragma unroll
            for (int k = 0; k < 3; ++k) N[k] = (-G[k]) / den;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            normal[3 * v + k] = N[k];
            grad[3 * v + k] = G[k];
        }
    }
}

bool lattice_ok(int nx, int ny, int nz)      // fewer than 2^31 lattice points (every n_k >= 1)
{
    const int64_t xy = ((int64_t)nx + 1) * ((int64_t)ny + 1);
    return xy < (1ll << 31) && xy * ((int64_t)nz + 1) < (1ll << 31);
}

int integrate(const char *what, const float *depths, const float *Ks, const float *C2Ws, int C, int H, int W, const float *origin,
              const float *spacing, int nx, int ny, int nz, float trunc, float near, float far, float *acc, uint64_t *counters,
              bool count, scanerf_stream_t stream, const float *colors = nullptr, float *cacc = nullptr, bool color = false)
{
    const float inf = __builtin_huge_valf();
    SCANERF_REQUIRE(C >= 0, "%s: C=%d (negative size)", what, C);
    SCANERF_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d (an image has at least one pixel)", what, H, W);
    SCANERF_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: n=(%d, %d, %d) (every n_k must be >= 1)", what, nx, ny, nz);
    SCANERF_REQUIRE(lattice_ok(nx, ny, nz), "%s: n=(%d, %d, %d) has 2^31 or more lattice points", what, nx, ny, nz);
    SCANERF_REQUIRE(trunc > 0.0f && trunc < inf, "%s: trunc=%g (must be > 0 and finite)", what, (double)trunc);
    SCANERF_REQUIRE(near >= 0.0f, "%s: near=%g (must be >= 0)", what, (double)near);
    SCANERF_REQUIRE(far > near, "%s: far=%g (must be > near=%g; +inf for no limit)", what, (double)far, (double)near);
    SCANERF_REQUIRE(depths && Ks && C2Ws && origin && spacing && acc && (!count || counters), "%s: null pointer", what);
    SCANERF_REQUIRE(!color || (colors && cacc), "%s: null pointer", what);
    SCANERF_REQUIRE(!color || ((uintptr_t)cacc & 15) == 0, "%s: cacc must be 16-byte aligned (it is loaded and stored as float4)", what);
    Lattice L;
    for (int a = 0; a < 3; ++a) {
        SCANERF_REQUIRE(spacing[a] > 0.0f && spacing[a] < inf, "%s: spacing[%d]=%g (must be > 0 and finite)", what, a, (double)spacing[a]);
        SCANERF_REQUIRE(origin[a] > -inf && origin[a] < inf, "%s: origin[%d]=%g (must be finite)", what, a, (double)origin[a]);
        L.origin[a] = origin[a];
        L.spacing[a] = spacing[a];
    }
    L.n[0] = nx, L.n[1] = ny, L.n[2] = nz;
    if (C == 0) return 0;
    const int tiles_x = ceil_div(nx + 1, kBX), tiles_y = ceil_div(ny + 1, kBY), tiles_z = ceil_div(nz + 1, kBZ);
    const int64_t tiles = (int64_t)tiles_x * tiles_y * tiles_z;      // < 2^31: every tile holds a lattice point of its own
    const dim3 grid((unsigned)tiles), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ctr = reinterpret_cast<unsigned long long *>(counters);
    float2 *a2 = reinterpret_cast<float2 *>(acc);
    float4 *c4 = reinterpret_cast<float4 *>(cacc);
#define SCANERF_TSDF_LAUNCH(COUNT, COLOR)                                                                                                  \
    hipLaunchKernelGGL((k_tsdf_integrate<COUNT, COLOR>), grid, block, 0, st, depths, Ks, C2Ws, C, H, W, L, tiles_y, tiles_z, trunc, near, \
                       far, a2, ctr, colors, c4)
    if (color) {
        if (count) SCANERF_TSDF_LAUNCH(true, true);
        else SCANERF_TSDF_LAUNCH(false, true);
    } else {
        if (count) SCANERF_TSDF_LAUNCH(true, false);
        else SCANERF_TSDF_LAUNCH(false, false);
    }
#undef SCANERF_TSDF_LAUNCH
    return check_launch(what);
}

}  // namespace

SCANERF_API int scanerf_tsdf_cameras_per_pass(void) { return kCamsPerPass; }

SCANERF_API int scanerf_tsdf_integrate(const float *depths, const float *Ks, const float *C2Ws, int C, int H, int W, const float *origin,
                                       const float *spacing, int nx, int ny, int nz, float trunc, float near, float far, float *acc,
                                       scanerf_stream_t stream)
{
    return integrate("tsdf_integrate", depths, Ks, C2Ws, C, H, W, origin, spacing, nx, ny, nz, trunc, near, far, acc, nullptr, false, stream);
}

SCANERF_API int scanerf_tsdf_integrate_counted(const float *depths, const float *Ks, const float *C2Ws, int C, int H, int W,
                                               const float *origin, const float *spacing, int nx, int ny, int nz, float trunc, float near,
                                               float far, float *acc, uint64_t *counters, scanerf_stream_t stream)
{
    return integrate("tsdf_integrate_counted", depths, Ks, C2Ws, C, H, W, origin, spacing, nx, ny, nz, trunc, near, far, acc, counters, true,
                     stream);
}

SCANERF_API int scanerf_tsdf_integrate_color(const float *depths, const float *colors, const float *Ks, const float *C2Ws, int C, int H, int W,
                                             const float *origin, const float *spacing, int nx, int ny, int nz, float trunc, float near,
                                             float far, float *acc, float *cacc, scanerf_stream_t stream)
{
    return integrate("tsdf_integrate_color", depths, Ks, C2Ws, C, H, W, origin, spacing, nx, ny, nz, trunc, near, far, acc, nullptr, false,
                     stream, colors, cacc, true);
}

SCANERF_API int scanerf_tsdf_integrate_color_counted(const float *depths, const float *colors, const float *Ks, const float *C2Ws, int C, int H,
                                                     int W, const float *origin, const float *spacing, int nx, int ny, int nz, float trunc,
                                                     float near, float far, float *acc, float *cacc, uint64_t *counters,
                                                     scanerf_stream_t stream)
{
    return integrate("tsdf_integrate_color_counted", depths, Ks, C2Ws, C, H, W, origin, spacing, nx, ny, nz, trunc, near, far, acc, counters,
                     true, stream, colors, cacc, true);
}

SCANERF_API int scanerf_tsdf_values(const float *acc, int P, float min_weight, float *values, uint8_t *observed, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(P >= 0, "tsdf_values: P=%d (negative size)", P);
    SCANERF_REQUIRE(min_weight >= 1.0f, "tsdf_values: min_weight=%g (must be >= 1)", (double)min_weight);
    if (P == 0) return 0;
    SCANERF_REQUIRE(acc && values && observed, "tsdf_values: null pointer");
    hipLaunchKernelGGL(k_tsdf_values, dim3(stream_grid(P, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2 *>(acc), P, min_weight, values, observed);
    return check_launch("tsdf_values");
}

SCANERF_API int scanerf_tsdf_cell_support(const uint8_t *observed, int nx, int ny, int nz, const int32_t *cells, int V, int32_t *support,
                                          scanerf_stream_t stream)
{
    SCANERF_REQUIRE(V >= 0, "tsdf_cell_support: V=%d (negative size)", V);
    SCANERF_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "tsdf_cell_support: n=(%d, %d, %d) (every n_k must be >= 1)", nx, ny, nz);
    SCANERF_REQUIRE(lattice_ok(nx, ny, nz), "tsdf_cell_support: n=(%d, %d, %d) has 2^31 or more lattice points", nx, ny, nz);
    if (V == 0) return 0;
    SCANERF_REQUIRE(observed && cells && support, "tsdf_cell_support: null pointer");
    hipLaunchKernelGGL(k_tsdf_cell_support, dim3(stream_grid(V, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, observed, nx, ny, nz,
                       cells, V, support);
    return check_launch("tsdf_cell_support");
}

SCANERF_API int scanerf_tsdf_vertex_colors(const float *cacc, int nx, int ny, int nz, const int32_t *cells, const float *lattice, int V,
                                           float *rgb, float *weight, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(V >= 0, "tsdf_vertex_colors: V=%d (negative size)", V);
    SCANERF_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "tsdf_vertex_colors: n=(%d, %d, %d) (every n_k must be >= 1)", nx, ny, nz);
    SCANERF_REQUIRE(lattice_ok(nx, ny, nz), "tsdf_vertex_colors: n=(%d, %d, %d) has 2^31 or more lattice points", nx, ny, nz);
    if (V == 0) return 0;
    SCANERF_REQUIRE(cacc && cells && lattice && rgb && weight, "tsdf_vertex_colors: null pointer");
    SCANERF_REQUIRE(((uintptr_t)cacc & 15) == 0, "tsdf_vertex_colors: cacc must be 16-byte aligned (it is loaded as float4)");
    hipLaunchKernelGGL(k_tsdf_vertex_colors, dim3(stream_grid(V, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(cacc), nx, ny, nz, cells, lattice, V, rgb, weight);
    return check_launch("tsdf_vertex_colors");
}

SCANERF_API int scanerf_tsdf_vertex_normals(const float *values, const uint8_t *observed, int nx, int ny, int nz, const float *spacing,
                                            const int32_t *cells, const float *lattice, int V, float *normal, float *grad,
                                            scanerf_stream_t stream)
{
    const float inf = __builtin_huge_valf();
    SCANERF_REQUIRE(V >= 0, "tsdf_vertex_normals: V=%d (negative size)", V);
    SCANERF_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "tsdf_vertex_normals: n=(%d, %d, %d) (every n_k must be >= 1)", nx, ny, nz);
    SCANERF_REQUIRE(lattice_ok(nx, ny, nz), "tsdf_vertex_normals: n=(%d, %d, %d) has 2^31 or more lattice points", nx, ny, nz);
    SCANERF_REQUIRE(values && observed && spacing && cells && lattice && normal && grad, "tsdf_vertex_normals: null pointer");
    for (int a = 0; a < 3; ++a)
        SCANERF_REQUIRE(spacing[a] > 0.0f && spacing[a] < inf, "tsdf_vertex_normals: spacing[%d]=%g (must be > 0 and finite)", a,
                        (double)spacing[a]);
    if (V == 0) return 0;
    hipLaunchKernelGGL(k_tsdf_vertex_normals, dim3(stream_grid(V, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, values, observed, nx,
                       ny, nz, spacing[0], spacing[1], spacing[2], cells, lattice, V, normal, grad);
    return check_launch("tsdf_vertex_normals");
}
