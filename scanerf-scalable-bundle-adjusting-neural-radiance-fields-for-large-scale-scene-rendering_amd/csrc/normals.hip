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
#include "normals_device.h"   // the per-sample device code, shared with render_normals_tiles.hip

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

template <int DT>
__global__ void __launch_bounds__(kNrmThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) k_sigma_normals_points(NormalArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[NL_TOTAL];
    const int lane = threadIdx.x;
    nrm_stage(lds, a.blob, a.wf, a.resolutions, lane);
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
    nrm_stage(lds, a.blob, a.wf, a.resolutions, lane);
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
