// warp.hip -- the multi-view warp loss (warp_loss.py:147-660, cuda/view_selection_kernel.cu:19-349): neighbour-view selection,
// projection + colour fetch, and the loss with its gradients w.r.t. the per-ray prediction, the rays and the cameras' rts.
//
// Per ray: p = rays_o + depth * rays_d (q = [depth, diffuse(3), specular(3)] rows of 7 floats, the merged prediction).
//   select : cost of every camera (view_selection_kernel.cu:19-72), the K lowest kept in registers by a sorted insert (ties: lower
//            camera index first); slot valid iff cost <= 0.176 (warp_loss.py:407-408).  Cameras stream through LDS in chunks.
//   project: per (ray, slot) the projection of proj2neighbor_forward_kernel (grid, proj_depth, neighbour ray) and the bilinear fetch
//            of sample_neighbor_color (warp_loss.py:441-521: top-left corner = trunc(grid), occlusion at trunc(grid + 0.5)).
//   loss   : L = scale / (n K) * sum_{valid rays, slots} score * mean_c((clamp(dif + spec, 0, 1) - colour)^2) (compute_loss), n = the
//            number of valid rays; the colour's gradient goes through the bilinear weights to grid and on through the projection
//            Jacobian (proj2neighbor_backward_kernel) to p and rts -- in the same kernel, no dL/dgrid pass.  dL/drts is reduced in a
//            fixed order (per-(ray, slot) partials, summed per (camera, chunk) workgroup in index order, then the chunks in order): no float atomics,
//            bit-reproducible like every other training kernel of the library.
#include "common.h"

using namespace scanerf;

namespace {

constexpr int kThreads = 256, kBlocks = 256;
constexpr int kMaxK = 16;             // slots per ray (the reference: 10)
constexpr int kCamChunk = 256;        // cameras staged in LDS per pass of the selection kernel
constexpr int kCamFloats = 24;        // K (9), R (9), t (3), centre (3)
constexpr float kCostValid = 0.176f;  // warp_loss.py:408

struct V3 { float x, y, z; };

__device__ inline V3 ray_point(const float *o, const float *d, const float *q, int b)
{
    const float t = q[7 * (size_t)b];
    return { o[3 * (size_t)b] + t * d[3 * (size_t)b], o[3 * (size_t)b + 1] + t * d[3 * (size_t)b + 1],
             o[3 * (size_t)b + 2] + t * d[3 * (size_t)b + 2] };
}

// q = R p + t (Extrinsic::proj), pix = K q (Intrinsic::proj); rt row-major [3][4], k row-major [3][3]
__device__ inline V3 to_cam(const float *rt, V3 p)
{
    return { rt[0] * p.x + rt[1] * p.y + rt[2] * p.z + rt[3], rt[4] * p.x + rt[5] * p.y + rt[6] * p.z + rt[7],
             rt[8] * p.x + rt[9] * p.y + rt[10] * p.z + rt[11] };
}
__device__ inline V3 to_pix(const float *k, V3 c)
{
    return { k[0] * c.x + k[1] * c.y + k[2] * c.z, k[3] * c.x + k[4] * c.y + k[5] * c.z, k[6] * c.x + k[7] * c.y + k[8] * c.z };
}
// camera centre -R^T t (Extrinsic::inverse().getTrans())
__device__ inline V3 centre(const float *rt)
{
    return { -(rt[0] * rt[3] + rt[4] * rt[7] + rt[8] * rt[11]), -(rt[1] * rt[3] + rt[5] * rt[7] + rt[9] * rt[11]),
             -(rt[2] * rt[3] + rt[6] * rt[7] + rt[10] * rt[11]) };
}

// ---- selection: one thread per ray, cameras through LDS ---------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_select(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                     const float *__restrict__ q, const uint8_t *__restrict__ ray_valid,
                                                     const float *__restrict__ ks, const float *__restrict__ rts, int N, int H,
                                                     int W, int K, int B, int *__restrict__ views, float *__restrict__ costs,
                                                     uint8_t *__restrict__ valid)
{
    __shared__ float cam[kCamChunk * kCamFloats];
    const int b = blockIdx.x * kThreads + threadIdx.x;
    const bool live = b < B && (!ray_valid || ray_valid[b]);
    V3 p = { 0, 0, 0 }, o = { 0, 0, 0 }, dir = { 0, 0, 1 };
    if (live) {
        p = ray_point(rays_o, rays_d, q, b);
        o = { rays_o[3 * (size_t)b], rays_o[3 * (size_t)b + 1], rays_o[3 * (size_t)b + 2] };
        V3 d = { rays_d[3 * (size_t)b], rays_d[3 * (size_t)b + 1], rays_d[3 * (size_t)b + 2] };
        const float r = rsqrtf(d.x * d.x + d.y * d.y + d.z * d.z);   // cutil_math normalize()
        dir = { d.x * r, d.y * r, d.z * r };
    }
    float best[kMaxK];
    int bidx[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) { best[j] = INFINITY; bidx[j] = 0; }
    for (int c0 = 0; c0 < N; c0 += kCamChunk) {
        const int nc = N - c0 < kCamChunk ? N - c0 : kCamChunk;
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += kThreads) {
            const float *k = ks + 9 * (size_t)(c0 + i), *rt = rts + 12 * (size_t)(c0 + i);
            float *s = cam + i * kCamFloats;
#pragma unroll
            for (int j = 0; j < 9; ++j) s[j] = k[j];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s[9 + 3 * j] = rt[4 * j]; s[10 + 3 * j] = rt[4 * j + 1]; s[11 + 3 * j] = rt[4 * j + 2]; s[18 + j] = rt[4 * j + 3];
            }
            const V3 c = centre(rt);
            s[21] = c.x; s[22] = c.y; s[23] = c.z;
        }
        __syncthreads();
        if (!live) continue;
        for (int i = 0; i < nc; ++i) {
            const float *s = cam + i * kCamFloats;   // same address across the wave: LDS broadcast
            const V3 qc = { s[9] * p.x + s[10] * p.y + s[11] * p.z + s[18], s[12] * p.x + s[13] * p.y + s[14] * p.z + s[19],
                            s[15] * p.x + s[16] * p.y + s[17] * p.z + s[20] };
            const V3 uv = to_pix(s, qc);
            float cost = 1.0f;
            if (uv.z > 0.001f) {
                const float x = uv.x / uv.z, y = uv.y / uv.z;
                if (!(x <= 0.0f || x >= (float)(W - 1) || y <= 0.0f || y >= (float)(H - 1))) {
                    const V3 e = { p.x - s[21], p.y - s[22], p.z - s[23] };
                    const float e2 = e.x * e.x + e.y * e.y + e.z * e.z;
                    const float r = rsqrtf(e2);
                    const float angle = 1.0f - (dir.x * e.x * r + dir.y * e.y * r + dir.z * e.z * r);
                    const V3 f = { p.x - o.x, p.y - o.y, p.z - o.z };
                    const float dis = fmaxf(0.0f, 1.0f - sqrtf(f.x * f.x + f.y * f.y + f.z * f.z) / sqrtf(e2));
                    cost = 0.9f * angle + 0.1f * dis;
                }
            }
            // sorted insert: strict < places the new camera behind the earlier (lower-index) ones it ties with; from there on
            // every entry shifts down one slot (a carried entry that ties with the next one must not be dropped in its favour)
            float cc = cost;
            int ci = c0 + i;
            bool placed = false;
#pragma unroll
            for (int j = 0; j < kMaxK; ++j) {
                if (j < K && (placed || cc < best[j])) {
                    const float tc = best[j]; best[j] = cc; cc = tc;
                    const int ti = bidx[j]; bidx[j] = ci; ci = ti;
                    placed = true;
                }
            }
        }
    }
    if (b >= B) return;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
        if (j < K) {
            const size_t s = (size_t)b * K + j;
            views[s] = live ? bidx[j] : 0;
            costs[s] = live ? best[j] : 1.0f;
            valid[s] = live && best[j] <= kCostValid;
        }
    }
}

// ---- projection + bilinear fetch: one thread per (ray, slot) ---------------------------------------------------------------
struct Bilinear { int lx, ly; float ox, oy; };

// warp_loss.py:456-478: lt = grid.long() (truncation toward zero), offsets from it.  The clamp only guards the image bounds;
// a slot that passed the selection projects inside (-0.5, W - 1.5) x (-0.5, H - 1.5), where it changes nothing.
__device__ inline Bilinear corners(float gx, float gy, int H, int W)
{
    int lx = (int)gx, ly = (int)gy;
    lx = lx < 0 ? 0 : (lx > W - 2 ? W - 2 : lx);
    ly = ly < 0 ? 0 : (ly > H - 2 ? H - 2 : ly);
    return { lx, ly, gx - (float)lx, gy - (float)ly };
}

__global__ void __launch_bounds__(kThreads) k_project(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                      const float *__restrict__ q, const float *__restrict__ ks,
                                                      const float *__restrict__ rts, const int *__restrict__ views,
                                                      const uint8_t *__restrict__ valid_in, const float *__restrict__ images,
                                                      const uint8_t *__restrict__ occl, int N, int H, int W, int K, int B,
                                                      float *__restrict__ grid, float *__restrict__ proj_depth,
                                                      float *__restrict__ nei_o, float *__restrict__ nei_d,
                                                      float *__restrict__ color, uint8_t *__restrict__ valid_out)
{
    const size_t n = (size_t)B * K;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const int b = (int)(i / K), v = views[i];
        if (!valid_in[i] || v < 0 || v >= N) {
            grid[2 * i] = grid[2 * i + 1] = 0.0f;
            proj_depth[i] = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) nei_o[3 * i + c] = nei_d[3 * i + c] = color[3 * i + c] = 0.0f;
            valid_out[i] = 0;
            continue;
        }
        const float *rt = rts + 12 * (size_t)v, *k = ks + 9 * (size_t)v;
        const V3 p = ray_point(rays_o, rays_d, q, b);
        const V3 c = to_cam(rt, p);
        const V3 pix = to_pix(k, c);
        const float gx = pix.x / (pix.z + 1e-8f) - 0.5f, gy = pix.y / (pix.z + 1e-8f) - 0.5f;
        grid[2 * i] = gx;
        grid[2 * i + 1] = gy;
        proj_depth[i] = pix.z;
        const V3 org = centre(rt);
        const float dx = c.x / (c.z + 1e-8f), dy = c.y / (c.z + 1e-8f);
        nei_o[3 * i] = org.x; nei_o[3 * i + 1] = org.y; nei_o[3 * i + 2] = org.z;
        nei_d[3 * i] = rt[0] * dx + rt[4] * dy + rt[8];
        nei_d[3 * i + 1] = rt[1] * dx + rt[5] * dy + rt[9];
        nei_d[3 * i + 2] = rt[2] * dx + rt[6] * dy + rt[10];
        const Bilinear s = corners(gx, gy, H, W);
        int nx = (int)(gx + 0.5f), ny = (int)(gy + 0.5f);
        nx = nx < 0 ? 0 : (nx > W - 1 ? W - 1 : nx);
        ny = ny < 0 ? 0 : (ny > H - 1 ? H - 1 : ny);
        valid_out[i] = occl ? (occl[((size_t)v * H + ny) * W + nx] != 0) : 1;
        const float *img = images + ((size_t)v * H + s.ly) * W * 3;
        const float wlt = (1.0f - s.ox) * (1.0f - s.oy), wrt = s.ox * (1.0f - s.oy), wlb = (1.0f - s.ox) * s.oy, wrb = s.ox * s.oy;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float lt = img[3 * s.lx + ch], rt_ = img[3 * (s.lx + 1) + ch];
            const float lb = img[(size_t)3 * W + 3 * s.lx + ch], rb = img[(size_t)3 * W + 3 * (s.lx + 1) + ch];
            color[3 * i + ch] = wlt * lt + wrt * rt_ + wlb * lb + wrb * rb;
        }
    }
}

// ---- loss: per-block partials (sum of score * mean_c err^2, number of valid rays), fixed tree -------------------------------
__device__ inline float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

__global__ void __launch_bounds__(kThreads) k_loss_partials(const float *__restrict__ q, const uint8_t *__restrict__ ray_valid,
                                                            const uint8_t *__restrict__ valid, const float *__restrict__ color,
                                                            const float *__restrict__ score, int K, int B,
                                                            float *__restrict__ partials)
{
    float se = 0.0f, nv = 0.0f;
    for (int b = blockIdx.x * kThreads + threadIdx.x; b < B; b += kBlocks * kThreads) {
        if (ray_valid && !ray_valid[b]) continue;
        nv += 1.0f;
        const float *r = q + 7 * (size_t)b;
        const float pr[3] = { clamp01(r[1] + r[4]), clamp01(r[2] + r[5]), clamp01(r[3] + r[6]) };
        for (int k = 0; k < K; ++k) {
            const size_t i = (size_t)b * K + k;
            if (!valid[i]) continue;
            const float e0 = pr[0] - color[3 * i], e1 = pr[1] - color[3 * i + 1], e2 = pr[2] - color[3 * i + 2];
            se += (e0 * e0 + e1 * e1 + e2 * e2) / 3.0f * score[i];
        }
    }
    __shared__ float red[2][kThreads];
    red[0][threadIdx.x] = se; red[1][threadIdx.x] = nv;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x < 2) partials[blockIdx.x * 2 + threadIdx.x] = red[threadIdx.x][0];
}

// ---- gradients: one thread per ray over its slots; dL/drts per (ray, slot) into `contrib` ------------------------------------
__global__ void __launch_bounds__(kThreads) k_loss_grad(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                        const float *__restrict__ q, const uint8_t *__restrict__ ray_valid,
                                                        const float *__restrict__ ks, const float *__restrict__ rts,
                                                        const int *__restrict__ views, const uint8_t *__restrict__ valid,
                                                        const float *__restrict__ grid, const float *__restrict__ color,
                                                        const float *__restrict__ score, const float *__restrict__ images, int N,
                                                        int H, int W, int K, int B, float scale, const float *__restrict__ partials,
                                                        float *__restrict__ loss, float *__restrict__ grad_q, float *__restrict__ g_o,
                                                        float *__restrict__ g_d, float *__restrict__ contrib)
{
    __shared__ float tot[2];
    if (threadIdx.x < 2) {   // every block adds the partials in the same order
        float s = 0.0f;
        for (int i = 0; i < kBlocks; ++i) s += partials[2 * i + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    const float denom = tot[1] * (float)K;
    const float sc = denom > 0.0f ? scale / denom : 0.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) *loss = tot[0] * sc;
    for (int b = blockIdx.x * kThreads + threadIdx.x; b < B; b += gridDim.x * kThreads) {
        float *gq = grad_q + 7 * (size_t)b;
        if (ray_valid && !ray_valid[b]) {
#pragma unroll
            for (int j = 0; j < 7; ++j) gq[j] = 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) g_o[3 * (size_t)b + j] = g_d[3 * (size_t)b + j] = 0.0f;
            continue;
        }
        const float *r = q + 7 * (size_t)b;
        float sum[3], pr[3], gpred[3] = { 0, 0, 0 };
#pragma unroll
        for (int c = 0; c < 3; ++c) { sum[c] = r[1 + c] + r[4 + c]; pr[c] = clamp01(sum[c]); }
        const V3 p = ray_point(rays_o, rays_d, q, b);
        V3 gp = { 0, 0, 0 };
        for (int k = 0; k < K; ++k) {
            const size_t i = (size_t)b * K + k;
            const int v = views[i];
            if (!valid[i] || v < 0 || v >= N) continue;
            const float e = sc * score[i] * (2.0f / 3.0f);
            float gcol[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float diff = pr[c] - color[3 * i + c];
                gpred[c] += e * diff;
                gcol[c] = -e * diff;
            }
            // d colour / d grid through the bilinear weights (the corner colours are constants)
            const float gx = grid[2 * i], gy = grid[2 * i + 1];
            const Bilinear s = corners(gx, gy, H, W);
            const float *img = images + ((size_t)v * H + s.ly) * W * 3;
            float ggx = 0.0f, ggy = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float lt = img[3 * s.lx + c], rt_ = img[3 * (s.lx + 1) + c];
                const float lb = img[(size_t)3 * W + 3 * s.lx + c], rb = img[(size_t)3 * W + 3 * (s.lx + 1) + c];
                ggx += gcol[c] * ((1.0f - s.oy) * (rt_ - lt) + s.oy * (rb - lb));
                ggy += gcol[c] * ((1.0f - s.ox) * (lb - lt) + s.ox * (rb - rt_));
            }
            // grid = pix.xy / (pix.z + 1e-8) - 0.5, pix = K (R p + t): chain to the camera-space point, then to p and [R | t]
            const float *rt = rts + 12 * (size_t)v, *kk = ks + 9 * (size_t)v;
            const V3 pix = to_pix(kk, to_cam(rt, p));
            const float iz = 1.0f / (pix.z + 1e-8f);
            const float gu = ggx * iz, gv = ggy * iz, gw = -(ggx * pix.x + ggy * pix.y) * iz * iz;
            const float gc[3] = { kk[0] * gu + kk[3] * gv + kk[6] * gw, kk[1] * gu + kk[4] * gv + kk[7] * gw,
                                  kk[2] * gu + kk[5] * gv + kk[8] * gw };
            gp.x += rt[0] * gc[0] + rt[4] * gc[1] + rt[8] * gc[2];
            gp.y += rt[1] * gc[0] + rt[5] * gc[1] + rt[9] * gc[2];
            gp.z += rt[2] * gc[0] + rt[6] * gc[1] + rt[10] * gc[2];
            float *w = contrib + 12 * i;
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                w[4 * rr] = gc[rr] * p.x; w[4 * rr + 1] = gc[rr] * p.y; w[4 * rr + 2] = gc[rr] * p.z; w[4 * rr + 3] = gc[rr];
            }
        }
        // clamp(diffuse + specular, 0, 1): torch passes the gradient where 0 <= x <= 1
        const float d[3] = { rays_d[3 * (size_t)b], rays_d[3 * (size_t)b + 1], rays_d[3 * (size_t)b + 2] };
        gq[0] = gp.x * d[0] + gp.y * d[1] + gp.z * d[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g = (sum[c] >= 0.0f && sum[c] <= 1.0f) ? gpred[c] : 0.0f;
            gq[1 + c] = g;
            gq[4 + c] = g;
        }
        const float t = r[0];
        g_o[3 * (size_t)b] = gp.x; g_o[3 * (size_t)b + 1] = gp.y; g_o[3 * (size_t)b + 2] = gp.z;
        g_d[3 * (size_t)b] = t * gp.x; g_d[3 * (size_t)b + 1] = t * gp.y; g_d[3 * (size_t)b + 2] = t * gp.z;
    }
}

// dL/drts in a fixed order: workgroup (camera, chunk) sums the (ray, slot) partials of that camera in one contiguous chunk of the
// (ray, slot) index range -- each thread in index order, then a fixed tree -- and k_rts_sum adds the chunks in chunk order
constexpr int kChunkEntries = 4096, kMaxChunks = 64;

inline int rts_chunks(size_t n)
{
    const size_t c = (n + kChunkEntries - 1) / kChunkEntries;
    return c < 1 ? 1 : (c > (size_t)kMaxChunks ? kMaxChunks : (int)c);
}

__global__ void __launch_bounds__(kThreads) k_rts_partial(const int *__restrict__ views, const uint8_t *__restrict__ valid,
                                                          const uint8_t *__restrict__ ray_valid, const float *__restrict__ contrib,
                                                          int K, int B, float *__restrict__ part)
{
    const int cam = blockIdx.x, C = gridDim.y;
    const size_t n = (size_t)B * K, per = (n + C - 1) / C;
    const size_t lo = per * blockIdx.y, hi = lo + per < n ? lo + per : n;
    float acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.0f;
    for (size_t i = lo + threadIdx.x; i < hi; i += kThreads) {
        if (!valid[i] || views[i] != cam || (ray_valid && !ray_valid[i / K])) continue;
        const float *w = contrib + 12 * i;
#pragma unroll
        for (int j = 0; j < 12; ++j) acc[j] += w[j];
    }
    __shared__ float red[12][kThreads];
#pragma unroll
    for (int j = 0; j < 12; ++j) red[j][threadIdx.x] = acc[j];
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int j = 0; j < 12; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 12) part[((size_t)cam * C + blockIdx.y) * 12 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ void __launch_bounds__(kThreads) k_rts_sum(const float *__restrict__ part, int N, int C, float *__restrict__ grad_rts)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;   // (camera, entry)
    if (t >= 12 * N) return;
    const int cam = t / 12, j = t % 12;
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s += part[((size_t)cam * C + c) * 12 + j];
    grad_rts[t] = s;
}

}  // namespace

SCANERF_API int scanerf_warp_max_neighbors(void) { return kMaxK; }

SCANERF_API size_t scanerf_warp_scratch_floats(int B, int K, int N)
{
    if (B < 0 || K < 0 || N < 0) return 0;
    return (size_t)2 * kBlocks + (size_t)12 * B * K + (size_t)12 * N * rts_chunks((size_t)B * K);
}

SCANERF_API int scanerf_warp_select_views(const float *rays_o, const float *rays_d, const float *ray_q, const uint8_t *ray_valid,
                                          const float *ks, const float *rts, int N, int H, int W, int K, int B, int *nei_views,
                                          float *nei_cost, uint8_t *nei_valid, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(B >= 0 && N >= 1 && K >= 1 && K <= kMaxK && K <= N && H >= 2 && W >= 2,
                    "warp_select_views: B=%d N=%d K=%d H=%d W=%d (need 1 <= K <= min(N, %d), H, W >= 2)", B, N, K, H, W, kMaxK);
    if (B == 0) return 0;
    SCANERF_REQUIRE(rays_o && rays_d && ray_q && ks && rts && nei_views && nei_cost && nei_valid, "warp_select_views: null pointer");
    hipLaunchKernelGGL(k_select, dim3(ceil_div(B, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, rays_o, rays_d, ray_q,
                       ray_valid, ks, rts, N, H, W, K, B, nei_views, nei_cost, nei_valid);
    return check_launch("warp_select_views");
}

SCANERF_API int scanerf_warp_project(const float *rays_o, const float *rays_d, const float *ray_q, const float *ks, const float *rts,
                                     const int *nei_views, const uint8_t *nei_valid_in, const float *images, const uint8_t *occlusions,
                                     int N, int H, int W, int K, int B, float *grid, float *proj_depth, float *nei_origin,
                                     float *nei_direction, float *nei_color, uint8_t *nei_valid, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(B >= 0 && N >= 1 && K >= 1 && K <= kMaxK && H >= 2 && W >= 2, "warp_project: B=%d N=%d K=%d H=%d W=%d", B, N, K, H, W);
    if (B == 0) return 0;
    SCANERF_REQUIRE(rays_o && rays_d && ray_q && ks && rts && nei_views && nei_valid_in && images && grid && proj_depth && nei_origin &&
                    nei_direction && nei_color && nei_valid, "warp_project: null pointer");
    hipLaunchKernelGGL(k_project, dim3(stream_grid((int64_t)B * K, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, rays_o, rays_d,
                       ray_q, ks, rts, nei_views, nei_valid_in, images, occlusions, N, H, W, K, B, grid, proj_depth, nei_origin,
                       nei_direction, nei_color, nei_valid);
    return check_launch("warp_project");
}

SCANERF_API int scanerf_warp_loss_grad(const float *rays_o, const float *rays_d, const float *ray_q, const uint8_t *ray_valid,
                                       const float *ks, const float *rts, const int *nei_views, const uint8_t *nei_valid,
                                       const float *grid, const float *nei_color, const float *score, const float *images, int N,
                                       int H, int W, int K, int B, float scale, float *loss, float *grad_q, float *grad_o,
                                       float *grad_d, float *grad_rts, float *scratch, size_t scratch_floats,
                                       scanerf_stream_t stream)
{
    SCANERF_REQUIRE(B >= 0 && N >= 1 && K >= 1 && K <= kMaxK && H >= 2 && W >= 2, "warp_loss_grad: B=%d N=%d K=%d H=%d W=%d", B, N, K, H, W);
    SCANERF_REQUIRE(rays_o && rays_d && ray_q && ks && rts && nei_views && nei_valid && grid && nei_color && score && images && loss &&
                    grad_q && grad_o && grad_d && grad_rts && scratch, "warp_loss_grad: null pointer");
    SCANERF_REQUIRE(scratch_floats >= scanerf_warp_scratch_floats(B, K, N), "warp_loss_grad: scratch holds %zu floats, needs %zu",
                    scratch_floats, scanerf_warp_scratch_floats(B, K, N));
    hipStream_t st = (hipStream_t)stream;
    const int C = rts_chunks((size_t)B * K);
    float *partials = scratch, *contrib = scratch + 2 * kBlocks, *part = contrib + (size_t)12 * B * K;
    hipLaunchKernelGGL(k_loss_partials, dim3(kBlocks), dim3(kThreads), 0, st, ray_q, ray_valid, nei_valid, nei_color, score, K, B,
                       partials);
    hipLaunchKernelGGL(k_loss_grad, dim3(stream_grid(B > 0 ? B : 1, kThreads)), dim3(kThreads), 0, st, rays_o, rays_d, ray_q,
                       ray_valid, ks, rts, nei_views, nei_valid, grid, nei_color, score, images, N, H, W, K, B, scale, partials, loss,
                       grad_q, grad_o, grad_d, contrib);
    hipLaunchKernelGGL(k_rts_partial, dim3(N, C), dim3(kThreads), 0, st, nei_views, nei_valid, ray_valid, contrib, K, B, part);
    hipLaunchKernelGGL(k_rts_sum, dim3(ceil_div(12 * (int64_t)N, kThreads)), dim3(kThreads), 0, st, part, N, C, grad_rts);
    return check_launch("warp_loss_grad");
}
