// mono.hip -- the monocular depth-consistency and depth-smoothness prior losses (mono_loss.py DepthConsistencyLoss /
// DepthSmoothLoss, criterions.py:99-105,170-183) and their gradient w.r.t. the per-ray rendered depth p.
//
// A ray b is valid (m_b = 1) iff ray_valid[b] and its locs (view, px, py) lie inside [0,N) x [0,W) x [0,H).
//   depth : per view v, over its valid rays, the least-squares scale / shift (h0, h1) of p onto the monocular depth t (MiDaS'
//           compute_scale_and_shift) from the moments a00 = sum p^2, a01 = sum p, a11 = sum 1, b0 = sum p t, b1 = sum t, all in f64
//           (in f32, det = a00 a11 - a01^2 cancels to noise for views whose depths vary by a few per cent); h = 0 when det = 0.
//           L_depth = sum_all m (h0 p + h1 - t)^2 / sum_all m.  h minimises the same quadratic, so dL/dh = 0 and
//           dL/dp_b = 2 m_b h0 (h0 p_b + h1 - t_b) / sum_all m.
//   smooth: rays 4k..4k+3 are a 2x2 patch (r = 2 dy + dx) of one view; P_r = K^-1 (x_r, y_r, 1) p_r; valid iff all four rays are
//           valid, share one view and n_r . mean(n) > 0.9 for the raw monocular normals; c = 0.25 sum over the edges P2-P0, P3-P1,
//           P1-P0, P3-P2 of |normalize(mean n) . normalize(edge)|; L_smooth = mean of c over the valid patches (0 when none).
// Launches (no allocation, no host synchronisation, no float atomics -- every sum in a fixed order, bit-reproducible):
//   k_view_moments  one 1024-thread workgroup per view scans all B locs (B ~ 16k int triples, L2-resident) once: the five moments
//                   and sum m t^2 in f64 through an LDS tree, the 2x2 solve, and sum m r^2 expanded over the moments.  Grouping by
//                   locs[:,0] takes any ray order; one workgroup per view is simpler than per-chunk partials (no second launch, no
//                   partial buffer) and its O(N B) reads of L2-resident data cost next to nothing.
//   k_patch         one thread per patch: validity, c (or -1 for an invalid patch) and dc/dp of its four rays.
//   k_totals        one workgroup: the views' and the patches' sums in index order -> loss[3] and the two gradient coefficients.
//   k_grad          one thread per ray: coef_depth m h0 r + coef_smooth dc/dp.
#include "common.h"

using namespace scanerf;

namespace {

constexpr int kThreads = 256;
constexpr int kViewThreads = 1024;   // one workgroup per view scans all B rays
constexpr int kViewDoubles = 4;   // h0, h1, sum m r^2, sum m
constexpr int kTotalFloats = 8;   // coef_depth, coef_smooth (f32), spare

struct Ray { int v; int px; int py; bool m; };

__device__ inline Ray ray_at(const int32_t *locs, const uint8_t *ray_valid, int N, int H, int W, int b)
{
    const int v = locs[3 * (size_t)b], px = locs[3 * (size_t)b + 1], py = locs[3 * (size_t)b + 2];
    const bool inside = v >= 0 && v < N && px >= 0 && px < W && py >= 0 && py < H;
    return { v, px, py, inside && (!ray_valid || ray_valid[b]) };
}

__device__ inline size_t pix(const Ray &r, int H, int W) { return ((size_t)r.v * H + r.py) * W + r.px; }

// in-place LDS tree over T doubles per row; the result lands in row[0]
template <int R, int T = kThreads>
__device__ inline void tree(double (*red)[T])
{
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int j = 0; j < R; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + s];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kViewThreads) k_view_moments(const float *__restrict__ depth, const uint8_t *__restrict__ ray_valid,
                                                               const int32_t *__restrict__ locs, const float *__restrict__ mono_depth,
                                                               int N, int H, int W, int B, double *__restrict__ views)
{
    __shared__ double red[6][kViewThreads];
    const int view = blockIdx.x;
    double a00 = 0.0, a01 = 0.0, a11 = 0.0, b0 = 0.0, b1 = 0.0, c = 0.0;
    // branch-free body (a masked ray reads the map's first texel, in bounds): the unrolled loads of several rays are in flight
    // together -- the scan is latency-bound, not bandwidth-bound
#pragma unroll 4
    for (int b = threadIdx.x; b < B; b += kViewThreads) {
        const Ray r = ray_at(locs, ray_valid, N, H, W, b);
        const bool on = r.m && r.v == view;
        const double p = depth[b], t = mono_depth[on ? pix(r, H, W) : 0];
        a00 += on ? p * p : 0.0; a01 += on ? p : 0.0; a11 += on ? 1.0 : 0.0;
        b0 += on ? p * t : 0.0; b1 += on ? t : 0.0; c += on ? t * t : 0.0;
    }
    red[0][threadIdx.x] = a00; red[1][threadIdx.x] = a01; red[2][threadIdx.x] = a11;
    red[3][threadIdx.x] = b0; red[4][threadIdx.x] = b1; red[5][threadIdx.x] = c;
    tree<6, kViewThreads>(red);
    if (threadIdx.x == 0) {
        a00 = red[0][0]; a01 = red[1][0]; a11 = red[2][0]; b0 = red[3][0]; b1 = red[4][0]; c = red[5][0];
        const double det = a00 * a11 - a01 * a01;
        const double h0 = det != 0.0 ? (a11 * b0 - a01 * b1) / det : 0.0;
        const double h1 = det != 0.0 ? (-a01 * b0 + a00 * b1) / det : 0.0;
        // sum m (h0 p + h1 - t)^2 expanded over the moments: in f64 the cancellation costs ~1e-16 of sum t^2, far below the f32
        // result; h = 0 (det = 0) gives sum t^2 exactly
        const double se = h0 * h0 * a00 + 2.0 * h0 * h1 * a01 + h1 * h1 * a11 - 2.0 * h0 * b0 - 2.0 * h1 * b1 + c;
        double *o = views + (size_t)kViewDoubles * view;
        o[0] = h0; o[1] = h1; o[2] = se > 0.0 ? se : 0.0; o[3] = a11;
    }
}

struct D3 { double x, y, z; };
__device__ inline D3 sub(D3 a, D3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline D3 scale(D3 a, double s) { return { a.x * s, a.y * s, a.z * s }; }

__global__ void __launch_bounds__(kThreads) k_patch(const float *__restrict__ depth, const uint8_t *__restrict__ ray_valid,
                                                    const int32_t *__restrict__ locs, const float *__restrict__ mono_normal,
                                                    const float *__restrict__ kinv, int N, int H, int W, int B,
                                                    float *__restrict__ patch_c, float *__restrict__ patch_grad)
{
    const int k = blockIdx.x * kThreads + threadIdx.x, P = B / 4;
    if (k >= P) return;
    Ray r[4];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[i] = ray_at(locs, ray_valid, N, H, W, 4 * k + i);
        ok = ok && r[i].m && r[i].v == r[0].v;
    }
    D3 n[4], nm = { 0, 0, 0 };
    if (ok) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float *q = mono_normal + 3 * pix(r[i], H, W);
            n[i] = { q[0], q[1], q[2] };
            nm = { nm.x + n[i].x, nm.y + n[i].y, nm.z + n[i].z };
        }
        nm = scale(nm, 0.25);
#pragma unroll
        for (int i = 0; i < 4; ++i) ok = ok && dot(n[i], nm) > 0.9;
    }
    if (!ok) {
        patch_c[k] = -1.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) patch_grad[4 * k + i] = 0.0f;
        return;
    }
    const double nl = sqrt(dot(nm, nm));
    const D3 nn = scale(nm, 1.0 / fmax(nl, 1e-12));
    const float *ki = kinv + 9 * (size_t)r[0].v;
    D3 u[4], Pt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double x = r[i].px, y = r[i].py, p = depth[4 * k + i];
        u[i] = { ki[0] * x + ki[1] * y + ki[2], ki[3] * x + ki[4] * y + ki[5], ki[6] * x + ki[7] * y + ki[8] };
        Pt[i] = scale(u[i], p);
    }
    // edges (a, b) = P_a - P_b: y (2,0), (3,1); x (1,0), (3,2)
    const int ea[4] = { 2, 3, 1, 3 }, eb[4] = { 0, 1, 0, 2 };
    double c = 0.0, g[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const D3 e = sub(Pt[ea[j]], Pt[eb[j]]);
        const double el = sqrt(dot(e, e));
        const double den = fmax(el, 1e-12);
        const double s = dot(nn, e) / den;
        c += fabs(s);
        const double sg = s > 0.0 ? 0.25 : (s < 0.0 ? -0.25 : 0.0);   // d|s|/ds (0 at 0) and the 1/4 of the mean
        // d s / d e: (nn - ghat (ghat . nn)) / |e| above the clamp; nn / 1e-12 below it (the clamp's gradient is 0)
        const D3 ge = el > 1e-12 ? scale(sub(nn, scale(e, s / den)), sg / den) : scale(nn, sg / den);
        g[ea[j]] += dot(ge, u[ea[j]]);
        g[eb[j]] -= dot(ge, u[eb[j]]);
    }
    patch_c[k] = (float)(0.25 * c);
#pragma unroll
    for (int i = 0; i < 4; ++i) patch_grad[4 * k + i] = (float)g[i];
}

__global__ void __launch_bounds__(kThreads) k_totals(const double *__restrict__ views, const float *__restrict__ patch_c, int N,
                                                     int P, int depth_on, int smooth_on, float w_depth, float w_smooth,
                                                     float *__restrict__ loss, float *__restrict__ totals)
{
    __shared__ double red[4][kThreads];
    double se = 0.0, cnt = 0.0, cs = 0.0, np = 0.0;
    if (depth_on)
        for (int v = threadIdx.x; v < N; v += kThreads) { se += views[kViewDoubles * v + 2]; cnt += views[kViewDoubles * v + 3]; }
    if (smooth_on)
        for (int k = threadIdx.x; k < P; k += kThreads) {
            const float c = patch_c[k];
            if (c >= 0.0f) { cs += c; np += 1.0; }
        }
    red[0][threadIdx.x] = se; red[1][threadIdx.x] = cnt; red[2][threadIdx.x] = cs; red[3][threadIdx.x] = np;
    tree<4>(red);
    if (threadIdx.x == 0) {
        se = red[0][0]; cnt = red[1][0]; cs = red[2][0]; np = red[3][0];
        const double ld = cnt > 0.0 ? se / cnt : 0.0, ls = np > 0.0 ? cs / np : 0.0;
        loss[0] = (float)((double)w_depth * ld + (double)w_smooth * ls);
        loss[1] = (float)ld;
        loss[2] = (float)ls;
        totals[0] = cnt > 0.0 ? (float)(2.0 * (double)w_depth / cnt) : 0.0f;
        totals[1] = np > 0.0 ? (float)((double)w_smooth / np) : 0.0f;
    }
}

__global__ void __launch_bounds__(kThreads) k_grad(const float *__restrict__ depth, const uint8_t *__restrict__ ray_valid,
                                                   const int32_t *__restrict__ locs, const float *__restrict__ mono_depth,
                                                   const double *__restrict__ views, const float *__restrict__ patch_grad,
                                                   const float *__restrict__ totals, int N, int H, int W, int B, int depth_on,
                                                   int smooth_on, float *__restrict__ grad_depth)
{
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    float g = 0.0f;
    if (depth_on) {
        const Ray r = ray_at(locs, ray_valid, N, H, W, b);
        if (r.m) {
            const double *h = views + (size_t)kViewDoubles * r.v;
            const double e = h[0] * (double)depth[b] + h[1] - (double)mono_depth[pix(r, H, W)];
            g = (float)((double)totals[0] * h[0] * e);
        }
    }
    if (smooth_on) g += totals[1] * patch_grad[b];
    grad_depth[b] = g;
}

}  // namespace

SCANERF_API size_t scanerf_mono_scratch_floats(int B, int N)
{
    if (B < 0 || N < 0) return 0;
    return (size_t)kTotalFloats + (size_t)2 * kViewDoubles * N + (size_t)(B / 4) + (size_t)B;
}

SCANERF_API int scanerf_mono_loss_grad(const float *depth, const uint8_t *ray_valid, const int32_t *locs, const float *mono_depth,
                                       const float *mono_normal, const float *kinv, int N, int H, int W, int B, float w_depth,
                                       float w_smooth, float *loss, float *grad_depth, float *scratch, size_t scratch_floats,
                                       scanerf_stream_t stream)
{
    SCANERF_REQUIRE(B >= 0 && N >= 1 && H >= 1 && W >= 1, "mono_loss_grad: B=%d N=%d H=%d W=%d", B, N, H, W);
    SCANERF_REQUIRE(loss && scratch && (B == 0 || (depth && locs && grad_depth)), "mono_loss_grad: null pointer");
    const int depth_on = mono_depth && w_depth != 0.0f, smooth_on = mono_normal && w_smooth != 0.0f;
    SCANERF_REQUIRE(!smooth_on || kinv, "mono_loss_grad: the smoothness term needs kinv [N,9]");
    SCANERF_REQUIRE(!smooth_on || B % 4 == 0, "mono_loss_grad: B=%d is not a whole number of 2x2 patches", B);
    SCANERF_REQUIRE(scratch_floats >= scanerf_mono_scratch_floats(B, N), "mono_loss_grad: scratch holds %zu floats, needs %zu",
                    scratch_floats, scanerf_mono_scratch_floats(B, N));
    hipStream_t st = (hipStream_t)stream;
    float *totals = scratch;
    double *views = (double *)(scratch + kTotalFloats);   // kTotalFloats is even: 8-byte aligned on an aligned scratch
    float *patch_c = scratch + kTotalFloats + (size_t)2 * kViewDoubles * N, *patch_grad = patch_c + B / 4;
    SCANERF_REQUIRE(((uintptr_t)views & 7) == 0, "mono_loss_grad: scratch is not 8-byte aligned");
    const int P = B / 4;
    if (depth_on && B > 0)
        hipLaunchKernelGGL(k_view_moments, dim3(N), dim3(kViewThreads), 0, st, depth, ray_valid, locs, mono_depth, N, H, W, B, views);
    if (smooth_on && P > 0)
        hipLaunchKernelGGL(k_patch, dim3(ceil_div(P, kThreads)), dim3(kThreads), 0, st, depth, ray_valid, locs, mono_normal, kinv,
                           N, H, W, B, patch_c, patch_grad);
    hipLaunchKernelGGL(k_totals, dim3(1), dim3(kThreads), 0, st, views, patch_c, N, P, depth_on && B > 0, smooth_on && P > 0,
                       w_depth, w_smooth, loss, totals);
    if (B > 0)
        hipLaunchKernelGGL(k_grad, dim3(ceil_div(B, kThreads)), dim3(kThreads), 0, st, depth, ray_valid, locs, mono_depth, views,
                           patch_grad, totals, N, H, W, B, depth_on, smooth_on, grad_depth);
    return check_launch("mono_loss_grad");
}
