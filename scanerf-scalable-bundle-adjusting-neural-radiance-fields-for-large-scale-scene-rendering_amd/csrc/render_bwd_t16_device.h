// render_bwd_t16_device.h -- what the two 16-sample-tile backward kernels share: the fused per-ray backward k_render_bwd_t16
// (render_bwd_t16.hip) and the stand-alone decoder backward k_decoder_bwd_s16 (decoder.hip), which is its split-gradient
// ("t16s") structure with the compositing adjoint replaced by the incoming per-sample gradients.  Each piece is here once; the
// workgroup barriers stay in the kernels, between calls into this header (nothing here synchronises the workgroup).
//
// Everything here leaves both kernels' validated listings (isa_manifest.json) as they were; what did not is STILL WRITTEN TWICE,
// alike, in the two kernels -- a change to one copy belongs in the other:
//   * the owned accumulators gW_* / gB_*, their rescale and their flush: as a struct (with and without the scale K / sc / isc as
//     members, flush as a member or as text, its lambdas as functions) the audit found every k_render_bwd_t16 and k_decoder_bwd_s16
//     listing changed (the values are carried round the tile loop in another order; +1 to +90 instructions);
//   * the scale decision (tile maxima -> frexpf -> K, sc, isc): as a function that returns the factor, same finding;
//   * the narrow block's forming and staging, the u0 recompute, the narrow block's wgrad dispatch: three forms each (lane terms by
//     reference / by value / as ints, arrays as pointers / references), listings changed (1-20 instructions re-ordered);
//   * the fused kernel's dv0 chain (the POSE reduction reads it between the product and the split): both POSE listings changed;
//   * the forward recompute in split-f16 (H from x; rgb from v0): five forms, all ten listings changed.
// How a function here takes its arguments (wgrad_dir0's lane terms by value, chain_gauss's as an int) is likewise what the audit
// accepted, not taste.
#pragma once
#include "render_t16.h"

namespace scanerf {

// A lane index the optimiser cannot trace back.  LDS addresses derived from the plain lane index are loop invariants: the
// ~60 distinct ones this kernel uses (operand slots in three 64 KB windows, bias rows, the XOR-swizzled staging slots of
// every block) get hoisted out of the tile loop and held -- or spilled -- for its whole duration.  Derived from an opaque
// copy they are recomputed where they are used (a handful of VALU per step).
__device__ __forceinline__ int fresh(int v)
{
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ T16Lane fresh_lane(const T16Lane &L)
{
    T16Lane r;
    r.lo16 = fresh(L.lo16);
    r.w1 = fresh(L.w1);
    r.r1 = fresh(L.r1);
    r.r2 = fresh(L.r2);
    r.pos8 = fresh(L.pos8);
    r.trp = fresh(L.trp);
    return r;
}
template <int N>
__device__ __forceinline__ void zero4(v4f (&v)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v4f{ 0, 0, 0, 0 };
}
// Gaussian activation of a block and its derivative factor G'(u) = -100 u G(u) as f16
__device__ __forceinline__ void act_deriv(v4f &u, t16_h4 &dg)
{
    v4f d;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float a = gauss_fast(u[g]);
        d[g] = -100.0f * u[g] * a;
        u[g] = a;
    }
    dg = t16_hi4(d);
}
__device__ __forceinline__ v4f mul_dg(const v4f &a, const t16_h4 &dg)
{
    return v4f{ a[0] * (float)dg[0], a[1] * (float)dg[1], a[2] * (float)dg[2], a[3] * (float)dg[3] };
}
__device__ __forceinline__ t16_h4 lo4(const t16_h8 &v) { return __builtin_shufflevector(v, v, 0, 1, 2, 3); }
__device__ __forceinline__ t16_h4 hi4(const t16_h8 &v) { return __builtin_shufflevector(v, v, 4, 5, 6, 7); }

// Weight-gradient blocks owned by this wave: acc[i] += sum over the 4 tile pairs of dY[yb] X[xb0 + i]^T (operands read back
// transposed from the pairs' staging images).  ROWSUM: also accumulate this lane's row sums of dY (bias gradients).
// SPLIT: hi and lo parts of both operands staged ({Y, X, Y lo, X lo} per wave), three products per term.
template <int NX, bool ROWSUM, int XSTRIDE = 1, bool SPLIT = false>
__device__ __forceinline__ void wgrad(v4f *acc, float &rowsum, const char *stage, const T16Lane &L, int yb, int x_mat_off, int xb0)
{
#ifdef T16_NO_WGRAD
    return;
#endif
    constexpr int kWave = SPLIT ? 2 * T16_STAGE_WAVE : T16_STAGE_WAVE, kLo = 2 * T16_STAGE_MAT;
#pragma unroll
    for (int P = 0; P < 4; ++P) {
        const char *pm = stage + P * 2 * kWave;
        const t16_h8 a = t16_stage_get(pm, L, yb);
        t16_h8 b[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) b[i] = t16_stage_get(pm + x_mat_off, L, xb0 + i * XSTRIDE);
        if (ROWSUM) rowsum = t16_sum8(a, rowsum);
        if constexpr (SPLIT) {
            const t16_h8 alo = t16_stage_get(pm + kLo, L, yb);
            if (ROWSUM) rowsum = t16_sum8(alo, rowsum);
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const t16_h8 blo = t16_stage_get(pm + x_mat_off + kLo, L, xb0 + i * XSTRIDE);
                acc[i] = t16_mfma(alo, b[i], acc[i]);
                acc[i] = t16_mfma(a, blo, acc[i]);
                acc[i] = t16_mfma(a, b[i], acc[i]);
            }
            __builtin_amdgcn_sched_barrier(0);   // (bounds the operands in flight: the pairs' reads are not hoisted over each other; freeing them changed nothing)
        } else {
#pragma unroll
            for (int i = 0; i < NX; ++i) acc[i] = t16_mfma(a, b[i], acc[i]);
        }
    }
}
// a split operand (hi, lo) of this lane's sample into blocks b, b + 1 of a staged matrix and of its lo twin
__device__ __forceinline__ void stage_put2(char *mat, const T16Lane &L, int b, const T16HL &v)
{
    t16_stage_put(mat, L, b, __builtin_shufflevector(v.hi, v.hi, 0, 1, 2, 3));
    t16_stage_put(mat, L, b + 1, __builtin_shufflevector(v.hi, v.hi, 4, 5, 6, 7));
    t16_stage_put(mat + 2 * T16_STAGE_MAT, L, b, __builtin_shufflevector(v.lo, v.lo, 0, 1, 2, 3));
    t16_stage_put(mat + 2 * T16_STAGE_MAT, L, b + 1, __builtin_shufflevector(v.lo, v.lo, 4, 5, 6, 7));
}
// G'(u) = -100 u G(u) of a block, f32, from its pre-activation (the activation is formed again: 4 exponentials against 4 more
// registers held across the weight-gradient products)
__device__ __forceinline__ v4f gauss_deriv(const v4f &u)
{
    v4f d;
#pragma unroll
    for (int g = 0; g < 4; ++g) d[g] = -100.0f * u[g] * gauss_fast(u[g]);
    return d;
}
// the Gaussian activations of a layer (64 units from their pre-activations), split and staged as blocks 0..3 of X and X lo
__device__ __forceinline__ void stage_act(char *stX, const T16Lane &L, const v4f u[4])
{
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        v4f a0, a1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            a0[g] = gauss_fast(u[2 * t][g]);
            a1[g] = gauss_fast(u[2 * t + 1][g]);
        }
        stage_put2(stX, L, 2 * t, t16_split(a0, a1));
    }
}

// ---- barrier-free segments of the t16s layer steps.  Both kernels run them in this order with their workgroup barriers (A1 B1 A2
// B2 A3 B3 A4 B4 A5) in between: a step stages its operands for the owners' weight-gradient products (.. A ..), then runs those
// products and chains the gradient to the layer below (.. B ..).

// dY of a 64-unit layer (split, two k-step operands) into blocks 0..3 of Y and Y lo
__device__ __forceinline__ void stage_dy(char *stY, const T16Lane &L, const T16HL dyS[2])
{
    stage_put2(stY, L, 0, dyS[0]);
    stage_put2(stY, L, 2, dyS[1]);
}
// 16 more "units" of Directional_MLP.mlp.0's input, block 2 of X: SH[4q .. 4q+3] of this lane's sample
__device__ __forceinline__ void stage_sh(char *stX, const T16Lane &L, const v4f &sh4)
{
    const v4f zero = { 0, 0, 0, 0 };
    const T16HL shS = t16_split(sh4, zero);
    t16_stage_put(stX, L, 2, lo4(shS.hi));
    t16_stage_put(stX + 2 * T16_STAGE_MAT, L, 2, lo4(shS.lo));
}
// a 64-output layer's weight gradient, row block rb of dY: wave cb == 0 owns x blocks 0 .. NX-1 and the bias row sums, cb == 1
// x blocks NX .. 2NX-1
template <int NX>
__device__ __forceinline__ void wgrad_layer(v4f (&gW)[NX], float &gB, const char *stage, const T16Lane &L, int rb, int cb)
{
    if (cb == 0) wgrad<NX, true, 1, true>(gW, gB, stage, L, rb, T16_STAGE_MAT, 0);
    else { float dummy = 0.0f; wgrad<NX, false, 1, true>(gW, dummy, stage, L, rb, T16_STAGE_MAT, NX); }
}
// ... of Directional_MLP.mlp.0: cb == 0 owns x = H[32:48] and the SH block, cb == 1 x = H[48:64]
__device__ __forceinline__ void wgrad_dir0(v4f (&gW)[2], float &gB, const char *stage, T16Lane L, int rb, int cb)   // (L by value: see the top)
{
    if (cb == 0) wgrad<2, true, 2, true>(gW, gB, stage, L, rb, T16_STAGE_MAT, 0);
    else { float dummy = 0.0f; wgrad<1, false, 1, true>(gW, dummy, stage, L, rb, T16_STAGE_MAT, 1); }
}
// dv1 = (W_rgb^T gs3) * G'(v1); narS = the narrow block (heads and rgb rows) as a split k-step operand
__device__ __forceinline__ void chain_narrow_rgb(v4f (&dc)[4], const char *lds, const T16Lane &L, const T16HL &narS, const v4f kv1[4])
{
    zero4(dc);
    s16_chain_narrow<4>(dc, lds, S16T_D2, L.lo16, narS);
#pragma unroll
    for (int b = 0; b < 4; ++b) dc[b] *= gauss_deriv(kv1[b]);
}
// dc = (W^T dY) * G'(u) through a 64 -> 64 layer (its forward image at `base`), u = the pre-activations that feed it
__device__ __forceinline__ void chain_gauss(v4f (&dc)[4], const char *lds, int base, int trp, const T16HL dyS[2], const v4f u[4])
{
    zero4(dc);
    s16_chain<4, 2, 2>(dc, lds, base, trp, dyS);
#pragma unroll
    for (int b = 0; b < 4; ++b) dc[b] *= gauss_deriv(u[b]);
}
// dH[32:64] = W_D0[:, :32]^T dv0 (input k-step 0 of the D0 pairs), dH[0:32] = heads^T gh
__device__ __forceinline__ void chain_dH(v4f (&dH)[4], const char *lds, int trp, int lo16, const T16HL dyS[2], const T16HL &narS)
{
    zero4(dH);
    s16_chain<2, 2, 2>(&dH[2], lds, T16_D0, trp, dyS);
    s16_chain_narrow<2>(&dH[0], lds, S16T_HEAD, lo16, narS);
}

}  // namespace scanerf
