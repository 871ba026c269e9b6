// normals_device.h -- the per-sample device code of the surface-normal kernels (normals.hip: one tile, one table;
// render_normals_tiles.hip: the multi-tile renderer's slot lists): decoder constants of a tile in LDS, the one-pass gather with its
// three position tangents, the 64 x 32 first-layer product on the f32-input matrix instruction and the closed-form density path
// behind it.
#pragma once
#include "hashgrid_common.h"
#include "render_common.h"

typedef float v16f __attribute__((ext_vector_type(16)));

namespace scanerf {
namespace {

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

// decoder constants and resolutions of one tile -> LDS (blob: its flat decoder blob, wf: weight_feature [32], resolutions [16,3]);
// WF = false: weight_feature == 1 (the render-time decoder has no coarse-to-fine mask), wf is not read
template <bool WF = true>
__device__ __forceinline__ void nrm_stage(float *lds, const float *blob, const float *wf, const int32_t *resolutions, int lane)
{
    const int h = lane >> 5, sl = lane & 31;
#pragma unroll 4
    for (int i = 0; i < 32; ++i) {   // i = mb * 16 + level
        const int mb = i >> 4, k = 2 * (i & 15) + h;
        const float w0 = blob[BLOB_S0 + 64 + k * 64 + 32 * mb + sl];
        lds[NL_A + i * 64 + lane] = WF ? w0 * wf[k] : w0;
    }
    float av = 0.0f;   // a_j = sum_i ws[i] W1[i][j]; the blob holds W1^T: [in j][out i]
    for (int i = 0; i < 32; ++i) av = fmaf(blob[BLOB_SIG + 1 + i], blob[BLOB_S1 + 64 + lane * 64 + i], av);
    lds[NL_AVEC + lane] = av;
    lds[NL_B0 + lane] = blob[BLOB_S0 + lane];
    reinterpret_cast<int *>(lds + NL_RES)[lane] = (lane & 3) < 3 ? resolutions[3 * (lane >> 2) + (lane & 3)] : 0;
}

// cell of a unit-cube position, as pts_inference locates it (rendering_kernel.cu:548-551): the same float32 expression, so a
// sample's normal and colour read the same cells
__device__ __forceinline__ void locate_p01(float p01, int res, int &b, float &t, float &scale)
{
#pragma clang fp contract(off)
    float v = p01 * (float)(res - 1);
    b = (int)v;
    t = v - (float)b;
    scale = (float)(res - 1) / 4.0f;
}

// This lane's sample at contracted position x -> s (sigma before the softplus) and gsum_k = sum_j a_j G'(u0_j) (W0 (wf * dfeat/dp_k))_j
// (d sigma / d p_k without its factor sigmoid(s)).  Every lane of the wave takes part (dead lanes: any finite x; every table index
// is masked to the table).  P01: x is the render-time ops' unit-cube position p01 = pts / 2 + 0.25 (the cell is pts_inference's
// v = p01 (res - 1), the contracted coordinate behind ascale 2 pts - 1) instead of a contracted position in [-2,2].
// VALUE: only s is formed (csrc/isosurface.hip): the feature column alone goes through the product, in the same order -- s has the
// bits of the full form; gsum and ascale are not touched.
template <int DT, bool P01 = false, bool VALUE = false>
__device__ __forceinline__ void density_grad(const float *lds, const void *features, int T, const float ascale[3], float c, int lane,
                                             const float x[3], float &s_out, float gsum[3])
{
    constexpr int NQ = VALUE ? 1 : 4;
    const uint32_t mask = (uint32_t)T - 1u;
    const int h = lane >> 5;
    const int *lres = reinterpret_cast<const int *>(lds + NL_RES);
    // F[level][nb][col]: after the exchange the B operand of samples 32 nb + (lane & 31), column col (0 = feature, 1 + k = d/dp_k)
    float F[16][2][NQ];
#pragma unroll
    for (int l = 0; l < 16; ++l) {
        const int4 res = reinterpret_cast<const int4 *>(lres)[l];
        int b[3];
        float t[3], sc[3];
        if constexpr (P01) {
            locate_p01(x[0], res.x, b[0], t[0], sc[0]);
            locate_p01(x[1], res.y, b[1], t[1], sc[1]);
            locate_p01(x[2], res.z, b[2], t[2], sc[2]);
        } else {
            locate_bg(x[0], res.x, b[0], t[0], sc[0]);
            locate_bg(x[1], res.y, b[1], t[1], sc[1]);
            locate_bg(x[2], res.z, b[2], t[2], sc[2]);
        }
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
            if constexpr (!VALUE) {
                col[ft][1] = (sc[0] * ascale[0]) * (y1 - y0);
                col[ft][2] = (sc[1] * ascale[1]) * fmaf(tx, (e11 - e10) - (e01 - e00), e01 - e00);
                col[ft][3] = (sc[2] * ascale[2]) * fmaf(tx, dz1 - dz0, dz0);
            }
        }
        // half-wave exchange: lanes < 32 keep feature 0 and receive feature 0 of lane + 32; lanes >= 32 keep feature 1 and receive
        // feature 1 of lane - 32
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
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
            v16f acc[NQ];
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                acc[0][g] = lds[NL_B0 + 32 * mb + nmap(g, h)];
                if constexpr (!VALUE) acc[1][g] = acc[2][g] = acc[3][g] = 0.0f;
            }
#pragma unroll
            for (int l = 0; l < 16; ++l) {
                const float aw = lds[NL_A + (mb * 16 + l) * 64 + lane];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, F[l][nb][q], acc[q], 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const float aj = lds[NL_AVEC + 32 * mb + nmap(g, h)];
                const float u = acc[0][g];
                const float G = __expf(u * u * -50.0f);
                [[maybe_unused]] const float gd = aj * (-100.0f * u * G);
                sp[nb] = fmaf(aj, G, sp[nb]);
                if constexpr (!VALUE) {
                    gp[nb][0] = fmaf(gd, acc[1][g], gp[nb][0]);
                    gp[nb][1] = fmaf(gd, acc[2][g], gp[nb][1]);
                    gp[nb][2] = fmaf(gd, acc[3][g], gp[nb][2]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the partner half holds the other 16 hidden units of each block; this lane's own sample is column lane & 31 of nb = h
    float mine[4] = { h ? sp[1] : sp[0], h ? gp[1][0] : gp[0][0], h ? gp[1][1] : gp[0][1], h ? gp[1][2] : gp[0][2] };
    float other[4] = { h ? sp[0] : sp[1], h ? gp[0][0] : gp[1][0], h ? gp[0][1] : gp[1][1], h ? gp[0][2] : gp[1][2] };
#pragma unroll
    for (int q = 0; q < NQ; ++q) mine[q] += __shfl_xor(other[q], 32, 64);
    s_out = mine[0] + c;
    if constexpr (!VALUE) {
        gsum[0] = mine[1];
        gsum[1] = mine[2];
        gsum[2] = mine[3];
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

}  // namespace
}  // namespace scanerf
