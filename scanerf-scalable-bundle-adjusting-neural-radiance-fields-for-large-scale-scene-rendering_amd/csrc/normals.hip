// normals.hip -- surface normals: the density's position gradient, fused.
//
// Reference behaviour: hashgrid/__init__.py:374-392 (compute_normal: -d sigma / d position by autograd, normalised with
// + 1e-8), :576-588 (render_batch_rays(out_normal=True): composited with the ray weights), tile.py:695-712 (render_normals).
//
// The density path is linear behind the first layer: sigma = softplus(s), s = a . G(u0) + c, u0 = W0 (wf * feat) + b0,
// a = W1[:32,:]^T ws^T (64 values), c = ws . b1[:32] + bs.  So
//     d sigma / d p_k = sigmoid(s) * sum_j a_j G'(u0_j) (W0 (wf * d feat / d p_k))_j,      G'(u) = -100 u G(u),
// one 64 x 32 product applied to four columns per sample: the features and their three position tangents, all formed from the
// same eight corner values of each level in ONE gather pass (no reverse pass, no second gather).
//
// One wave per workgroup; a lane owns a sample through the gather.  The product runs on the f32-input matrix instruction
// (v_mfma_f32_32x32x2_f32, f32 products and sums): the two features of a level are exactly one K = 2 step, the weights are the A
// operand (LDS, weight_feature folded in), and a half-wave exchange (lanes < 32 hand over feature 1, lanes >= 32 feature 0) turns
// the per-lane values into the B operands of samples 0-31 and 32-63.  Tangents reach (res - 1) / 4 * 4 / bbox_size ~ 2e3 per unit
// of table value: f32 operands need no scale (a split-f16 operand would).  The accumulators (register g of half h = hidden
// unit 32 mb + nmap(g, h), column = sample) are consumed in place; the partner half adds the other 16 units.
//
// Compositing (hashgrid/__init__.py:344-360) in the cumprod's own order: the wave's (alpha, n) go through LDS and the lane that
// owns a ray walks its samples front to back.  A ray belongs to one wave: no atomics, same bits launch to launch.
#include "hashgrid_common.h"
#include "render_common.h"

typedef float v16f __attribute__((ext_vector_type(16)));

namespace scanerf {
namespace {

constexpr int kNrmThreads = 64;
constexpr int kNrmMaxBlocks = kNumCU * 8;   // two waves per SIMD resident (register-bound), grid-stride beyond

struct NormalArgs {
    // ray form
    const float *rays_o, *rays_d, *z_vals, *dists;
    const uint8_t *ray_valid;
    float *out, *sample_normals;
    // point form
    const float *points;
    float *sigma, *grad, *normal;
    const void *features;
    const int32_t *resolutions;
    const float *blob, *wf;
    int B, S, T, N, infinity;
    float min_bbox[3], bbox_size[3];
    float ascale[3];   // d(contracted position)/d(position) per axis
};

// LDS of the one-wave workgroup (floats)
constexpr int NL_A = 0;                    // [mb 2][level 16][lane 64]: A operands, W0[32 mb + (lane & 31)][2 level + (lane >> 5)] * wf
constexpr int NL_AVEC = NL_A + 2048;       // a[64]
constexpr int NL_B0 = NL_AVEC + 64;        // b0[64]
constexpr int NL_RES = NL_B0 + 64;         // int [16][4]
constexpr int NL_COMP = NL_RES + 64;       // float4 [64]: (alpha, n) of the wave's samples
constexpr int NL_TOTAL = NL_COMP + 256;

// softplus_fast / sigmoid_fast of render_device.h (copied: that header stays as it is): v_exp_f32 / v_log_f32 / v_rcp_f32, 1 ulp
// each; softplus to ~2e-7 relative (series below 2^-6 truncated at 1e-6 of its last term), sigmoid to ~2e-7.
__device__ __forceinline__ float nrm_softplus(float x)
{
    const float e = __builtin_amdgcn_exp2f(-fabsf(x) * 1.4426950408889634f);
    const float l = e < 0x1p-6f ? e * (1.0f - e * (0.5f - e * 0.33333334f)) : __builtin_amdgcn_logf(1.0f + e) * 0.6931471805599453f;
    return fmaxf(x, 0.0f) + l;
}
__device__ __forceinline__ float nrm_sigmoid(float x)
{
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}

__device__ __forceinline__ float nrm_c(const float *__restrict__ blob)
{
    float c = blob[BLOB_SIG];
    for (int i = 0; i < 32; ++i) c = fmaf(blob[BLOB_SIG + 1 + i], blob[BLOB_S1 + i], c);
    return c;
}

// decoder constants and resolutions -> LDS (once per workgroup)
__device__ __forceinline__ void nrm_stage(float *lds, const NormalArgs &a, int lane)
{
    const float *blob = a.blob;
    const int h = lane >> 5, sl = lane & 31;
#pragma unroll 4
    for (int i = 0; i < 32; ++i) {   // i = mb * 16 + level
        const int mb = i >> 4, k = 2 * (i & 15) + h;
        lds[NL_A + i * 64 + lane] = blob[BLOB_S0 + 64 + k * 64 + 32 * mb + sl] * a.wf[k];
    }
    float av = 0.0f;   // a_j = sum_i ws[i] W1[i][j]; the blob holds W1^T: [in j][out i]
    for (int i = 0; i < 32; ++i) av = fmaf(blob[BLOB_SIG + 1 + i], blob[BLOB_S1 + 64 + lane * 64 + i], av);
    lds[NL_AVEC + lane] = av;
    lds[NL_B0 + lane] = blob[BLOB_S0 + lane];
    reinterpret_cast<int *>(lds + NL_RES)[lane] = (lane & 3) < 3 ? a.resolutions[3 * (lane >> 2) + (lane & 3)] : 0;
}

// This lane's sample at contracted position x -> s (sigma before the softplus) and gsum_k = sum_j a_j G'(u0_j) (W0 (wf * dfeat/dp_k))_j
// (d sigma / d p_k without its factor sigmoid(s)).  Every lane of the wave takes part (dead lanes: any finite x; every table index
// is masked to the table).
template <int DT>
__device__ __forceinline__ void density_grad(const float *lds, const void *features, int T, const float ascale[3], float c, int lane,
                                             const float x[3], float &s_out, float gsum[3])
{
    const uint32_t mask = (uint32_t)T - 1u;
    const int h = lane >> 5;
    const int *lres = reinterpret_cast<const int *>(lds + NL_RES);
    // F[level][nb][col]: after the exchange the B operand of samples 32 nb + (lane & 31), column col (0 = feature, 1 + k = d/dp_k)
    float F[16][2][4];
#pragma unroll
    for (int l = 0; l < 16; ++l) {
        const int4 res = reinterpret_cast<const int4 *>(lres)[l];
        int b[3];
        float t[3], sc[3];
        locate_bg(x[0], res.x, b[0], t[0], sc[0]);
        locate_bg(x[1], res.y, b[1], t[1], sc[1]);
        locate_bg(x[2], res.z, b[2], t[2], sc[2]);
        uint32_t idx[8];
        corner_indices(idx, b[0], b[1], b[2], mask);
        const char *slice = (const char *)features + (size_t)l * T * TableElem<DT>::bytes;
        float2 f[8];
        gather_cell<DT>(slice, idx, b[0] & 1, f);
        const float tx = t[0], ty = t[1], tz = t[2];
        float col[2][4];
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = ft ? f[q].y : f[q].x;
            // along z first (corner = dx << 2 | dy << 1 | dz): e[dx][dy] = the z-interpolations, d[dx][dy] = the z-differences
            const float d00 = v[1] - v[0], d01 = v[3] - v[2], d10 = v[5] - v[4], d11 = v[7] - v[6];
            const float e00 = fmaf(tz, d00, v[0]), e01 = fmaf(tz, d01, v[2]), e10 = fmaf(tz, d10, v[4]), e11 = fmaf(tz, d11, v[6]);
            const float dz0 = fmaf(ty, d01 - d00, d00), dz1 = fmaf(ty, d11 - d10, d10);
            const float y0 = fmaf(ty, e01 - e00, e00), y1 = fmaf(ty, e11 - e10, e10);
            col[ft][0] = fmaf(tx, y1 - y0, y0);
            col[ft][1] = (sc[0] * ascale[0]) * (y1 - y0);
            col[ft][2] = (sc[1] * ascale[1]) * fmaf(tx, (e11 - e10) - (e01 - e00), e01 - e00);
            col[ft][3] = (sc[2] * ascale[2]) * fmaf(tx, dz1 - dz0, dz0);
        }
        // half-wave exchange: lanes < 32 keep feature 0 and receive feature 0 of lane + 32; lanes >= 32 keep feature 1 and receive
        // feature 1 of lane - 32
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float y = __shfl_xor(h ? col[0][q] : col[1][q], 32, 64);
            F[l][0][q] = h ? y : col[0][q];
            F[l][1][q] = h ? col[1][q] : y;
        }
        if ((l & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // bound the gathers in flight per lane (4 levels = 32 loads)
    }

    float sp[2], gp[2][3];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        sp[nb] = 0.0f;
        gp[nb][0] = gp[nb][1] = gp[nb][2] = 0.0f;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            v16f acc[4];
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                acc[0][g] = lds[NL_B0 + 32 * mb + nmap(g, h)];
                acc[1][g] = acc[2][g] = acc[3][g] = 0.0f;
            }
#pragma unroll
            for (int l = 0; l < 16; ++l) {
                const float aw = lds[NL_A + (mb * 16 + l) * 64 + lane];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, F[l][nb][q], acc[q], 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const float aj = lds[NL_AVEC + 32 * mb + nmap(g, h)];
                const float u = acc[0][g];
                const float G = __expf(u * u * -50.0f);
                const float gd = aj * (-100.0f * u * G);
                sp[nb] = fmaf(aj, G, sp[nb]);
                gp[nb][0] = fmaf(gd, acc[1][g], gp[nb][0]);
                gp[nb][1] = fmaf(gd, acc[2][g], gp[nb][1]);
                gp[nb][2] = fmaf(gd, acc[3][g], gp[nb][2]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the partner half holds the other 16 hidden units of each block; this lane's own sample is column lane & 31 of nb = h
    float mine[4] = { h ? sp[1] : sp[0], h ? gp[1][0] : gp[0][0], h ? gp[1][1] : gp[0][1], h ? gp[1][2] : gp[0][2] };
    float other[4] = { h ? sp[0] : sp[1], h ? gp[0][0] : gp[1][0], h ? gp[0][1] : gp[1][1], h ? gp[0][2] : gp[1][2] };
#pragma unroll
    for (int q = 0; q < 4; ++q) mine[q] += __shfl_xor(other[q], 32, 64);
    s_out = mine[0] + c;
    gsum[0] = mine[1];
    gsum[1] = mine[2];
    gsum[2] = mine[3];
}

// sample point and contract_fore (render_device.h contract_point_box, mode 0)
__device__ __forceinline__ void contract_fore_point(const float min_bbox[3], const float bbox_size[3], const float o[3],
                                                    const float d[3], float z, float p[3])
{
#pragma clang fp contract(off)  // torch evaluates these as separate ops (hashgrid/__init__.py:394-395,519)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float w = o[k] + z * d[k];
        p[k] = (w - min_bbox[k]) / bbox_size[k] * 4.0f - 2.0f;
    }
}

// s, gsum -> sigma, g = d sigma / d p, n = -g / (|g| + 1e-8)
__device__ __forceinline__ void finish_sample(float s, const float gsum[3], float &sigma, float g[3], float n[3])
{
    sigma = nrm_softplus(s);
    const float sg = nrm_sigmoid(s);
    g[0] = sg * gsum[0];
    g[1] = sg * gsum[1];
    g[2] = sg * gsum[2];
    const float inv = -1.0f / (sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) + 1e-8f);
    n[0] = g[0] * inv;
    n[1] = g[1] * inv;
    n[2] = g[2] * inv;
}

template <int DT>
__global__ void __launch_bounds__(kNrmThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) k_sigma_normals_points(NormalArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[NL_TOTAL];
    const int lane = threadIdx.x;
    nrm_stage(lds, a, lane);
    const float c = nrm_c(a.blob);
    __syncthreads();
    const int ngroups = (a.N + 63) >> 6;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int i = grp * 64 + lane;
        const bool live = i < a.N;
        float x[3] = { 0.0f, 0.0f, 0.0f };
        if (live) {
            x[0] = a.points[3 * (size_t)i];
            x[1] = a.points[3 * (size_t)i + 1];
            x[2] = a.points[3 * (size_t)i + 2];
        }
        float s, gsum[3], sigma, g[3], n[3];
        density_grad<DT>(lds, a.features, a.T, a.ascale, c, lane, x, s, gsum);
        finish_sample(s, gsum, sigma, g, n);
        if (live) {
            a.sigma[i] = sigma;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (a.grad) a.grad[3 * (size_t)i + k] = g[k];
                a.normal[3 * (size_t)i + k] = n[k];
            }
        }
    }
}

// S <= 64: a wave takes 64 / S whole rays at once (lane = ray-in-group * S + sample); S > 64: one ray, 64 samples at a time.
template <int DT>
__global__ void __launch_bounds__(kNrmThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) k_render_normals(NormalArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[NL_TOTAL];
    const int lane = threadIdx.x;
    nrm_stage(lds, a, lane);
    const float c = nrm_c(a.blob);
    __syncthreads();
    const int S = a.S;
    const int rpw = S <= 64 ? 64 / S : 1;
    const int nbatch = S <= 64 ? 1 : (S + 63) >> 6;
    const int ngroups = (a.B + rpw - 1) / rpw;
    const int r = S <= 64 ? lane / S : 0;         // this lane's ray within the group (may be >= rpw: dead lane)
    const int i0 = S <= 64 ? lane - r * S : lane; // and its sample within the batch
    float4 *comp = reinterpret_cast<float4 *>(lds + NL_COMP);

    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int ray = grp * rpw + r;
        const bool ray_live = r < rpw && ray < a.B && !(a.ray_valid && !a.ray_valid[ray]);
        float o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 };
        if (ray_live) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                o[k] = a.rays_o[3 * (size_t)ray + k];
                d[k] = a.rays_d[3 * (size_t)ray + k];
            }
        }
        const float dnorm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        // the owner lane of ray q of the group is lane q (q < rpw): running transmittance and sums
        float T_run = 1.0f, acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int batch = 0; batch < nbatch; ++batch) {
            const int i = batch * 64 + i0;
            const bool live = ray_live && i < S;
            float x[3] = { 0.0f, 0.0f, 0.0f };
            float delta = 0.0f;
            if (live) {
                contract_fore_point(a.min_bbox, a.bbox_size, o, d, a.z_vals[(size_t)ray * S + i], x);
                delta = a.dists[(size_t)ray * S + i] * dnorm;
                if (a.infinity && i == S - 1) delta = 1e10f;
            }
            float s, gsum[3], sigma, g[3], n[3];
            density_grad<DT>(lds, a.features, a.T, a.ascale, c, lane, x, s, gsum);
            finish_sample(s, gsum, sigma, g, n);
            if (!live) n[0] = n[1] = n[2] = 0.0f;
            const float alpha = live ? 1.0f - expf(-sigma * delta) : 0.0f;
            if (a.sample_normals && r < rpw && ray < a.B && i < S) {   // (invalid rays: zeros)
                float *sn = a.sample_normals + ((size_t)ray * S + i) * 3;
                sn[0] = n[0];
                sn[1] = n[1];
                sn[2] = n[2];
            }
            __syncthreads();   // (the owners' reads of the previous batch or group are done)
            comp[lane] = make_float4(alpha, n[0], n[1], n[2]);
            __syncthreads();
            if (lane < rpw) {
                const int cnt = S <= 64 ? S : min(64, S - batch * 64);
                const float4 *row = comp + lane * (S <= 64 ? S : 0);
                for (int j = 0; j < cnt; ++j) {
                    const float4 v = row[j];
                    const float w = v.x * T_run;
                    acc[0] = fmaf(w, v.y, acc[0]);
                    acc[1] = fmaf(w, v.z, acc[1]);
                    acc[2] = fmaf(w, v.w, acc[2]);
                    acc[3] += w;
                    T_run *= 1.0f - v.x + 1e-6f;
                }
            }
        }
        const int own_ray = grp * rpw + lane;   // the owner lane's ray (not the ray of the sample this lane computed)
        if (lane < rpw && own_ray < a.B) reinterpret_cast<float4 *>(a.out)[own_ray] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

int check_common(const char *op, const void *features, int feat_dtype, const int32_t *resolutions, const float *mlp_blob,
                 const float *weight_feature, int T)
{
    SCANERF_REQUIRE(T >= 2 && (T & (T - 1)) == 0, "%s: T=%d must be a power of two", op, T);
    SCANERF_REQUIRE(feat_dtype == SCANERF_F32 || feat_dtype == SCANERF_F16, "%s: feat_dtype=%d (f32 and f16 tables)", op, feat_dtype);
    SCANERF_REQUIRE(features && resolutions && mlp_blob && weight_feature, "%s: null pointer", op);
    SCANERF_REQUIRE(((uintptr_t)features & 15) == 0, "%s: features must be 16-byte aligned", op);
    return 0;
}

}  // namespace
}  // namespace scanerf

using namespace scanerf;

SCANERF_API int scanerf_sigma_normals_points(const float *points, const float *axis_scale, const void *features, int feat_dtype,
                                             const int32_t *resolutions, const float *mlp_blob, const float *weight_feature,
                                             float *sigma, float *grad, float *normal, int N, int T, scanerf_stream_t stream)
{
    SCANERF_REQUIRE(N >= 0, "sigma_normals_points: N=%d", N);
    SCANERF_REQUIRE(axis_scale, "sigma_normals_points: axis_scale is null");
    if (int e = check_common("sigma_normals_points", features, feat_dtype, resolutions, mlp_blob, weight_feature, T)) return e;
    if (N == 0) return 0;
    SCANERF_REQUIRE(points && sigma && normal, "sigma_normals_points: null pointer");
    NormalArgs a = {};
    a.points = points; a.sigma = sigma; a.grad = grad; a.normal = normal;
    a.features = features; a.resolutions = resolutions; a.blob = mlp_blob; a.wf = weight_feature;
    a.N = N; a.T = T;
    for (int k = 0; k < 3; ++k) a.ascale[k] = axis_scale[k];
    int blocks = ceil_div(N, 64);
    if (blocks > kNrmMaxBlocks) blocks = kNrmMaxBlocks;
    hipStream_t st = (hipStream_t)stream;
    if (feat_dtype == SCANERF_F32) hipLaunchKernelGGL((k_sigma_normals_points<SCANERF_F32>), dim3(blocks), dim3(kNrmThreads), 0, st, a);
    else hipLaunchKernelGGL((k_sigma_normals_points<SCANERF_F16>), dim3(blocks), dim3(kNrmThreads), 0, st, a);
    return check_launch("sigma_normals_points");
}

SCANERF_API int scanerf_render_normals(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                                       const void *features, int feat_dtype, const int32_t *resolutions, const float *mlp_blob,
                                       const float *weight_feature, const float *min_bbox, const float *bbox_size, int infinity,
                                       const uint8_t *ray_valid, float *out, float *sample_normals, int B, int S, int T,
                                       scanerf_stream_t stream)
{
    SCANERF_REQUIRE(B >= 0 && S >= 1, "render_normals: B=%d S=%d", B, S);
    SCANERF_REQUIRE(min_bbox && bbox_size, "render_normals: min_bbox / bbox_size is null");
    for (int k = 0; k < 3; ++k) SCANERF_REQUIRE(bbox_size[k] > 0.0f, "render_normals: bbox_size[%d]=%g", k, (double)bbox_size[k]);
    if (int e = check_common("render_normals", features, feat_dtype, resolutions, mlp_blob, weight_feature, T)) return e;
    if (B == 0) return 0;
    SCANERF_REQUIRE(rays_o && rays_d && z_vals && dists && out, "render_normals: null pointer");
    SCANERF_REQUIRE(((uintptr_t)out & 15) == 0, "render_normals: out must be 16-byte aligned");
    NormalArgs a = {};
    a.rays_o = rays_o; a.rays_d = rays_d; a.z_vals = z_vals; a.dists = dists; a.ray_valid = ray_valid;
    a.out = out; a.sample_normals = sample_normals;
    a.features = features; a.resolutions = resolutions; a.blob = mlp_blob; a.wf = weight_feature;
    a.B = B; a.S = S; a.T = T; a.infinity = infinity;
    for (int k = 0; k < 3; ++k) {
        a.min_bbox[k] = min_bbox[k];
        a.bbox_size[k] = bbox_size[k];
        a.ascale[k] = 4.0f / bbox_size[k];
    }
    const int rpw = S <= 64 ? 64 / S : 1;
    int blocks = ceil_div(B, rpw);
    if (blocks > kNrmMaxBlocks) blocks = kNrmMaxBlocks;
    hipStream_t st = (hipStream_t)stream;
    if (feat_dtype == SCANERF_F32) hipLaunchKernelGGL((k_render_normals<SCANERF_F32>), dim3(blocks), dim3(kNrmThreads), 0, st, a);
    else hipLaunchKernelGGL((k_render_normals<SCANERF_F16>), dim3(blocks), dim3(kNrmThreads), 0, st, a);
    return check_launch("render_normals");
}
