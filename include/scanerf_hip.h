/*
 * scanerf_hip.h -- C ABI of libscanerf_hip.so: the MI355X (gfx950) implementation of
 * ScaNeRF's per-tile volume-rendering hot path.
 *
 * Drop-in boundary: one entry point per op of the reference's two pybind modules
 * (CUDA_EXT: cuda/binding.cpp:10-54, HASHGRID: hashgrid/binding.cpp:9-44) that lies on
 * the hot path, plus the fused fast-path entry points.  Plain pointers and sizes only
 * (no torch types).  Every pointer is a DEVICE pointer unless marked [host].  All
 * tensors are contiguous row-major.  Outputs are pre-allocated and pre-filled by the
 * caller exactly as the reference's Python does (sentinel -1 / zeros); the library
 * never allocates and keeps no state between calls.
 *
 * Every function returns 0 on success, non-zero on failure; scanerf_last_error()
 * returns a thread-local message for the last failure.  Launches are asynchronous on
 * `stream` (a hipStream_t passed as void*; NULL = the null stream): every launch of a call
 * goes to that stream and to no other, and the call returns without waiting for it.  ONE
 * entry waits for its own stream before it returns (hipStreamSynchronize(stream); never the
 * device, never another stream): scanerf_mesh_filter_emit, which reads V' and F' back to
 * check them against the caller's.  tests/test_gpu_stream_contract.py holds the list
 * (SYNCHRONISES) and checks every entry against it under a side stream.
 *
 * Citations are file:line under the reference repository.
 */
#ifndef SCANERF_HIP_H_
#define SCANERF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *scanerf_stream_t; /* hipStream_t */

#define SCANERF_PARAMSIZE 13994 /* hashgrid/include/decoder.h:20 */

/* feature-table element types (scanerf_*: `feat_dtype`) */
#define SCANERF_F32 0
#define SCANERF_F16 1
#define SCANERF_BF16 2

const char *scanerf_last_error(void);
int scanerf_abi_version(void); /* 10 */
/* Options.  The library keeps no global or per-process state and reads no environment variable: what a caller may choose is an
 * argument of the call it affects --
 *   decoder arithmetic of the fused training kernels      scanerf_render_cfg.arith (SCANERF_ARITH_*)
 *   levels masked by the coarse-to-fine schedule          scanerf_render_cfg.skip_levels
 *   decoder arithmetic of the render-time inference ops   SCANERF_INFER_H3 / SCANERF_INFER_F32 in `sample_major`
 *   per-sample array layout of the render-time ops        `sample_major` (0 / 1 / 2), SCANERF_SKIP_UNSAMPLED
 *   table-gradient record format of the stand-alone op    `compact_records` (-1 default / 0 / 1 / 2)
 *   large-table route (dfeat + stand-alone scatter, or the backward's own records + split pass): which entry points are called
 * Launch shapes, alternative producers and timing builds of the A/B experiments exist only in a library built with
 * `make EXP=1` (-DSCANERF_EXPERIMENTS), where they are read from the environment; scanerf_experiments_enabled() tells which
 * build this is (0 = product build). */
int scanerf_experiments_enabled(void);

/* ---- CUDA_EXT surface ------------------------------------------------------------ */

/* cuda/compute_ray_kernel.cu:95-115 (compute_ray.h:9-14).  locs [B,3] i32 (view,px,py),
 * Ks [C,9], C2Ws [C,12] -> rays_o, rays_d [B,3] */
int scanerf_compute_ray_forward(float *rays_o, float *rays_d, const float *Ks, const float *C2Ws,
                                const int32_t *locs, int B, scanerf_stream_t stream);

/* cuda/compute_ray_kernel.cu:117-136 (compute_ray.h:16-21).  grad_C2Ws [C,12] is ACCUMULATED
 * into.  Implements the correct adjoint (per-ray gradients); the reference reads
 * grad_rays_*[view_idx] (compute_ray_kernel.cu:71-72), see DESIGN.md. */
int scanerf_compute_ray_backward(const float *grad_rays_o, const float *grad_rays_d, const float *Ks,
                                 float *grad_C2Ws, const int32_t *locs, int B, int num_cam,
                                 scanerf_stream_t stream);

/* cuda/helper_kernel.cu:130-148 (K=1) and :177-197 (v2).  center,size [K,3]; bounds [B,K,2] */
int scanerf_ray_aabb_intersection(const float *rays_o, const float *rays_d, const float *center,
                                  const float *size, float *bounds, int B, int K, scanerf_stream_t stream);

/* cuda/helper_kernel.cu:645-671: the live training sampler.  occ = bool grid [2^lx,2^ly,2^lz]
 * (1 byte/cell), log2dim [3] i32, corner/size [3] (all device); z_vals,dists [B,S] pre-filled -1. */
int scanerf_sample_points_grid(const float *rays_o, const float *rays_d, float *z_vals, float *dists,
                               const float *block_corner, const float *block_size, const uint8_t *occ,
                               const int32_t *log2dim, int B, int S, scanerf_stream_t stream);

/* cuda/sample_kernel.cu:102-126.  Rays that miss the box are left untouched (the reference
 * device-asserts); *missed (device i32, may be NULL) counts them. */
int scanerf_sample_insideout_block(const float *rays_o, const float *rays_d, int S, int S_bg,
                                   const float *block_center, const float *block_size, float far_,
                                   float *z_vals, float *z_vals_bg, int32_t *missed, int B,
                                   scanerf_stream_t stream);

/* cuda/sample_kernel.cu:48-68 */
int scanerf_background_sampling(const float *starts, const float *bg_depth, float *z_vals, int S,
                                float sample_range, int B, scanerf_stream_t stream);

/* cuda/adam_kernel.cu:72-94 / :147-169.  Arrays are [K,8] (index = row*8+dim, dim<param_dim);
 * `step` is the PREVIOUS step count (the kernel uses step+1: adam.h:16 `int &step` quirk).
 * Entries whose grad is exactly 0 are skipped (no moment decay).  fp16: moments are IEEE half. */
int scanerf_adam_step(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, float lr,
                      float beta1, float beta2, float eps, int step, int64_t K, int param_dim,
                      scanerf_stream_t stream);
int scanerf_adam_step_fp16(float *params, const float *grad, void *exp_avg, void *exp_avg_sq, float lr,
                           float beta1, float beta2, float eps, int step, int64_t K, int param_dim,
                           scanerf_stream_t stream);

/* ---- HASHGRID surface ------------------------------------------------------------ */

/* hashgrid/src/hashgrid_bg_kernel.cu:229-249.  points [N,3] in [-2,2]; features [L,T,2]
 * (feat_dtype); resolutions [L,3] i32; outputs [N,L,2] f32.  T must be a power of two. */
int scanerf_embedding_bg_forward(const float *points, float *outputs, const void *features,
                                 const int32_t *resolutions, int N, int L, int T, int feat_dtype,
                                 scanerf_stream_t stream);
/* hashgrid/src/hashgrid_bg_kernel.cu:251-275.  grad_points [N,3] and grad_features [L,T,2]
 * (f32) are ACCUMULATED into (caller zero-fills: PyHashGridBG.py:27-28).  Either may be NULL. */
int scanerf_embedding_bg_backward(const float *points, const float *grad_in, float *grad_points,
                                  float *grad_features, const float *features, const int32_t *resolutions,
                                  int N, int L, int T, scanerf_stream_t stream);
/* Domain: as the reference's kernels (hashgrid_bg_kernel.cu:107-150 does not clamp), every encoder op takes points in [-2, 2]^3.
 * Outside, the plain ops extrapolate like the reference (negative / > 1 interpolation weights); the binned table-gradient routes
 * (scanerf_embedding_bg_backward_binned[_adam] in every record format -- the compact 8- / 12-byte records store the x-weight as an
 * unsigned fraction in [0, 1), and the 16-byte default of 8-level point-major rows was measured wrong outside as well -- the fused
 * path behind SCANERF_ARITH_T16 / T16S, scanerf_table_grad_scatter_adam_rays) are defined for in-domain points only, which is what
 * the samplers and the two contractions produce.  The drop-in binding embedding_bg_backward_cuda goes beyond that precondition:
 * it sends points outside to scanerf_embedding_bg_backward, as the reference's kernel extrapolates them. */
/* The same table gradient without global atomics: radix partition of the contributions by
 * 2048-entry table bucket + LDS accumulation (csrc/scatter.hip).  grad_layout 0: grad_in is
 * [N][L][2] (binding surface), 1: [L][N][2].  workspace: caller-owned scratch of at least
 * scanerf_embedding_bwd_workspace_bytes(N,L,T) bytes, 16-byte aligned (0 => shape not
 * supported by the binned path; use scanerf_embedding_bg_backward).  Does not compute
 * grad_points (call scanerf_embedding_bg_backward with grad_features = NULL for that). */
size_t scanerf_embedding_bwd_workspace_bytes(int N, int L, int T);
int scanerf_embedding_bg_backward_binned(const float *points, const float *grad_in, float *grad_features,
                                         const int32_t *resolutions, int N, int L, int T, int grad_layout,
                                         void *workspace, size_t workspace_bytes,
                                         int compact_records /* record format: -1 = the layout's default (12-byte records for point-major
                                            rows of 16 levels, 16-byte ones for level-major gradients), 0 = 16-byte (exact products),
                                            1 = 8-byte (level-major only), 2 = 12-byte: csrc/scatter_common.h */,
                                         scanerf_stream_t stream);
/* The same ending in the fused sparse Adam (the bucket images are the touched-entry list: no gradient table, no zero-fill, no
 * scan; per element the IEEE sequence of scanerf_adam_step, `step` = previous count).  half_table (may be NULL): f16 / bf16
 * gather copy refreshed where params change.  overflow_grad: zero [L][T][2] f32 table, written (and consumed) only if the
 * workspace overflows.  compact_records (grad_layout 1): 1 = 8-byte records (13-bit significands, csrc/scatter_common.h) -- for
 * feature gradients that come out of the t16 backward's f16 products; 2 = 12-byte records (f32 components less 4 bits, 23-bit
 * weight: behind the t16s backward); 0 = 16-byte records, exact. */
int scanerf_embedding_bg_backward_binned_adam(const float *points, const float *grad_in, const int32_t *resolutions, int N,
                                              int L, int T, int grad_layout, void *workspace, size_t workspace_bytes,
                                              float *params, float *exp_avg, float *exp_avg_sq, void *half_table,
                                              int half_dtype, float *overflow_grad, float lr, float beta1, float beta2,
                                              float eps, int step, int compact_records, scanerf_stream_t stream);
/* The same scatter + sparse Adam for the samples of up to TWO render branches over the same B rays (a tile's foreground and
 * background, tile.py:639-692 -- one optimiser step for both, tile.py:1010), without materialising or concatenating contracted
 * points: point positions are formed from rays_o/rays_d [B,3] and each branch's depths z [B,S] exactly as the render kernels form
 * them (contract_mode 0 = contract_fore, 1 = contract_bg; min_bbox / bbox_size [3] on the HOST), gradients are each branch's
 * level-major dfeat [16][B*S][2] out of scanerf_render_backward; valid [B] u8 (may be NULL) masks rays out.  z2 = NULL: one branch.
 * Tables of >= 2^22 entries per level, L = 16, 12-byte records in 64-byte segments (csrc/scatter_common.h format 3); workspace
 * of scanerf_embedding_bwd_workspace_bytes(B*(S1+S2), 16, T).  Replaces hashgrid_bg_kernel.cu:152-226 + torch.optim.Adam. */
int scanerf_table_grad_scatter_adam_rays(const float *rays_o, const float *rays_d, int B, const float *z1, const float *dfeat1,
                                         const uint8_t *valid1, int S1, int contract_mode1, const float *z2, const float *dfeat2,
                                         const uint8_t *valid2, int S2, int contract_mode2, const float *min_bbox /*[host]*/,
                                         const float *bbox_size /*[host]*/, const int32_t *resolutions, int T, void *workspace,
                                         size_t workspace_bytes, float *params, float *exp_avg, float *exp_avg_sq, void *half_table,
                                         int half_dtype, float *overflow_grad, float lr, float beta1, float beta2, float eps, int step,
                                         int fp16_moments /* OPT-IN, default 0: exp_avg / exp_avg_sq are [16][T][2] HALF arrays and the
                                            update is adam_step_cuda_fp16's (cuda/adam_kernel.cu:98-144: gradient x 128, moments stored in
                                            half): 16 instead of 24 bytes of optimiser state moved per touched entry each way.  NOT what the
                                            reference's live code runs (torch.optim.Adam, fp32 state, tile.py:301) */,
                                         scanerf_stream_t stream);
/* hashgrid/src/hashgrid_kernel.cu:246-270 / :272-300 (world-space box variant) */
int scanerf_embedding_forward(const float *points, float *outputs, const float *features,
                              const float *block_corner, const float *block_size,
                              const int32_t *resolutions, int N, int L, int T, scanerf_stream_t stream);
int scanerf_embedding_backward(const float *points, const float *grad_in, float *grad_points,
                               float *grad_features, const float *features, const float *block_corner,
                               const float *block_size, const int32_t *resolutions, int N, int L, int T,
                               scanerf_stream_t stream);

/* ---- fused fast path -------------------------------------------------------------- */

/* One launch for hashgrid/__init__.py:512-596 (HashGrid.render_batch_rays): for each ray,
 * samples o+z*d -> contraction (mode 0: contract_fore :394-395, 1: contract_bg :397-411) ->
 * 16-level hash lookup -> ShallowMLP (network.py:172-190) -> cal_integrate_weight/accumulate
 * (:344-366).  Nothing per-sample is materialised except `weights`.
 *
 *   rays_o, rays_d [B,3]; z_vals, dists [B,S]; features [16,T,2] (feat_dtype);
 *   resolutions [16,3] i32; mlp_blob [13994] f32 in decoder.h blob order (rendering.py:101-112);
 *   weight_feature [32] f32 (hashgrid/__init__.py:228-235 repeated x2);
 *   min_bbox, bbox_size [3] [host] (the HashGrid 2x box);
 *   out_ray [B,16] f32: rgb(3, clamped) depth(1) T_left(1) diffuse(3) specular(3) tint(3)
 *                       sum_w_spec2 (1: sum_i w_i*|c_s,i|^2, the l2_reg_specular numerator) pad(1);
 *   weights [B,S] f32 (may be NULL).
 */
typedef struct {
    int contract_mode; /* 0 fore, 1 bg */
    int infinity;      /* dists[:, -1] = 1e10 (hashgrid/__init__.py:349-350) */
    float min_bbox[3];
    float bbox_size[3];
    int arith; /* decoder arithmetic: SCANERF_ARITH_F32 (f32-input MFMA, exact f32), SCANERF_ARITH_H3 (f16 MFMA
                  on hi/lo-split operands, three products per term: f32-equivalent results, csrc/render_h3.h) or
                  SCANERF_ARITH_T16 (forward as H3; backward on 16-sample tiles at two waves per SIMD with the
                  forward recompute in H3 and the gradient products on one f16 MFMA per term, csrc/render_t16.h;
                  needs the x-stash) or SCANERF_ARITH_T16S (the T16 kernel with every gradient product split as well --
                  three MFMAs per term, G' in f32, f32 table-gradient records: f32-equivalent gradients at the T16
                  structure's speed; needs the x-stash).  plan / backward / accumulate of one step must be given the same value */
    unsigned skip_levels; /* bit l set: level l's inputs meet exactly-zero first-layer weights (the coarse-to-fine mask,
                             hashgrid/__init__.py:228-235, folded into the packed decoder), so scanerf_render_forward* may
                             leave the level's table alone (its encoder outputs become 0: same results bit for bit).  0 = none */
} scanerf_render_cfg;
#define SCANERF_ARITH_F32 0
#define SCANERF_ARITH_H3 1
#define SCANERF_ARITH_T16 2
#define SCANERF_ARITH_T16S 3

/* Packs the decoder blob (+ weight_feature folded into the first layer) into the LDS image
 * the fused kernels stage (csrc/render_common.h).  workspace: scanerf_render_workspace_floats()
 * f32, 16-byte aligned, caller-owned; re-pack whenever the blob or weight_feature changes. */
int scanerf_render_workspace_floats(void);
int scanerf_pack_decoder(const float *mlp_blob, const float *weight_feature, float *workspace,
                         scanerf_stream_t stream);

/* ray_valid [B] u8 (may be NULL): rays with 0 render as zeros with T_left = 1
 * (hashgrid/__init__.py:427-431) and are skipped.  tile_T [B, ceil(S/16)] (may be NULL): the
 * transmittance entering each 16-sample tile, saved for scanerf_render_backward.  xstash [B*S,32] f32
 * (may be NULL): the encoder outputs in register order, so the backward can skip the re-gather. */
int scanerf_render_forward_packed(const float *rays_o, const float *rays_d, const float *z_vals,
                                  const float *dists, const void *features, int feat_dtype,
                                  const int32_t *resolutions, const float *workspace,
                                  const scanerf_render_cfg *cfg /*[host]*/, const uint8_t *ray_valid,
                                  float *out_ray, float *weights, float *tile_T, float *xstash, int B, int S,
                                  int T, scanerf_stream_t stream);
/* scanerf_render_forward_packed that ALSO does scanerf_render_scatter_plan's work for the t16 backward of the same rays: the
 * record counts come out of the forward kernel (its hash indices are the plan's), then the scans run.  Call it INSTEAD of
 * scanerf_render_scatter_plan, with that function's workspace and cfg->arith = SCANERF_ARITH_T16; only for shapes where
 * scanerf_render_forward_plan_supported() is non-zero (forward and backward kernels visit the same rays per workgroup). */
int scanerf_render_forward_packed_plan(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                                       const void *features, int feat_dtype, const int32_t *resolutions, const float *workspace,
                                       const scanerf_render_cfg *cfg, const uint8_t *ray_valid, float *out_ray, float *weights,
                                       float *tile_T, float *xstash, void *jstash /* [B,ceil(S/32),8,4,64] u32: six 20-bit significands + one exponent per (sample, level), or NULL (fp32 tables) */,
                                       int B, int S, int T, void *scatter_ws, size_t scatter_ws_bytes, scanerf_stream_t stream);
int scanerf_render_forward_plan_supported(int B, int S, int T);

/* Adjoint of scanerf_render_forward_packed (hashgrid/__init__.py:512-596 under autograd).
 *   out_ray, tile_T: the forward's outputs;  grad_out [B,16]: dL/d(out_ray) (columns as out_ray;
 *   the sum_w_spec2 column is differentiated with the weights detached, as the reference's
 *   l2_reg_specular, hashgrid/__init__.py:593);
 *   dfeat [16][B*S][2] f32 (out): dL/d(hash features), level-major -> feed to
 *   scanerf_embedding_bg_backward_binned(grad_layout = 1) with the contracted sample points; may be
 *   NULL when scatter_ws is given;
 *   scatter_ws / scatter_ws_bytes / grad_features (may be NULL/0/NULL): FUSED table-gradient path.  The
 *   kernel then appends the scatter records itself (no dfeat round trip, no separate producer pass):
 *     scanerf_render_scatter_plan(...)        -- before: reserves each workgroup's record ranges
 *     scanerf_render_backward(..., ws, ...)   -- emits
 *     scanerf_render_scatter_accumulate(...)  -- after: grad_features [16][T][2] += records
 *   all three on the same (B, S, T), rays, z_vals, cfg, ray_valid and stream; grad_features is written
 *   by the backward only if the workspace overflows;
 *   dw_partial [4*scanerf_render_backward_grid(B)][13994] f32 scratch;
 *   grad_blob [13994] f32: dL/d(decoder blob), ACCUMULATED into (deterministic reduction). */
int scanerf_render_backward_grid(int B);
int scanerf_render_backward(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                            const void *features, int feat_dtype, const int32_t *resolutions,
                            const float *workspace, const float *weight_feature,
                            const scanerf_render_cfg *cfg /*[host]*/, const uint8_t *ray_valid,
                            const float *out_ray, const float *tile_T, const float *grad_out,
                            const float *xstash /* forward's, or NULL */, float *dfeat, float *dw_partial,
                            float *grad_blob, float *g_dnorm /* [B,ceil(S/32)] or NULL */,
                            float *g_rowsum /* [B,2,64] or NULL */,
                            const void *jstash /* forward's position Jacobians [B,ceil(S/32),8,4,64] u32, or NULL */,
                            float *g_raypos /* [B,6] dL/d(rays_o), dL/d(rays_d) through the sample positions (t16, needs jstash,
                                               g_dnorm and g_rowsum; zero-filled by the caller), or NULL */,
                            void *scatter_ws, size_t scatter_ws_bytes,
                            float *grad_features, int B, int S, int T, scanerf_stream_t stream);
/* Fused table-gradient path (replaces the atomicAdd scatter of hashgrid_bg_kernel.cu:196-201 for the
 * samples of a render batch).  workspace_bytes == 0 => shape unsupported, use dfeat + the binned op.
 * Precision of the sum: records are added in 64-bit fixed point (bit-reproducible).  Tables of at most 2^21 entries per level:
 * the records carry what the emitting backward wrote (f32 behind SCANERF_ARITH_F32 / H3, 19-bit-mantissa f32 behind T16S,
 * 13-bit behind T16).  Tables ABOVE 2^21 entries, when the workspace has the size scanerf_render_scatter_workspace_bytes
 * returns (it then holds the split pass's second record area): every record -- also an f32 one out of the F32 / H3 backward
 * -- is re-encoded by the split pass as a 12-byte record (gradient components rounded to 19 mantissa bits, x-weight to 23
 * bits: ~2^-21 relative per record against the window path), and the second entry of an x-neighbour pair that crosses a
 * 2^13-entry window (levels with a resolution above 8 192 only) is added to grad_features / overflow_grad with float atomics,
 * i.e. NOT bit-reproducibly; a smaller caller-owned workspace (or SCANERF_NO_SPLIT=1 in an experiments build) keeps the window
 * re-reads (f32 records, reproducible, slower). */
size_t scanerf_render_scatter_workspace_bytes(int B, int S, int T);
int scanerf_render_scatter_plan(const float *rays_o, const float *rays_d, const float *z_vals,
                                const int32_t *resolutions, const scanerf_render_cfg *cfg /*[host]*/,
                                const uint8_t *ray_valid, int B, int S, int T, void *workspace,
                                size_t workspace_bytes, scanerf_stream_t stream);
/* The three accumulate entries take `arith` (ABI 10): the SCANERF_ARITH_* the plan was made for (cfg->arith of
 * scanerf_render_scatter_plan / of the planning forward).  It selects a launch shape only -- the kernel decodes the records by the
 * format word the plan left in the workspace -- so a value other than the plan's gives the same bits, possibly slower; a value
 * outside SCANERF_ARITH_* is refused.  The library keeps no note of a plan between the calls. */
int scanerf_render_scatter_accumulate(float *grad_features, int B, int S, int T, void *workspace,
                                      size_t workspace_bytes, int arith, scanerf_stream_t stream);
/* accumulate + fused sparse Adam in one pass (replaces scanerf_render_scatter_accumulate + scanerf_adam_step on the table:
 * the bucket images ARE the touched-entry list, so no gradient table, no zero-fill, no scan; same per-element IEEE sequence as
 * scanerf_adam_step / cuda/adam_kernel.cu:24-69, `step` = the previous step count).  params / exp_avg / exp_avg_sq [16][T][2]
 * f32; half_table (may be NULL): f16 / bf16 (half_dtype = SCANERF_F16 / SCANERF_BF16) gather copy of params, refreshed where
 * params change; overflow_grad (may be NULL): the table given to scanerf_render_backward as grad_features -- consulted and
 * re-zeroed only if the record workspace overflowed, so it is allocated zero once and never filled per step. */
int scanerf_render_scatter_accumulate_adam(float *params, float *exp_avg, float *exp_avg_sq, void *half_table,
                                           int half_dtype, float *overflow_grad, float lr, float beta1, float beta2,
                                           float eps, int step, int B, int S, int T, void *workspace,
                                           size_t workspace_bytes, int arith, scanerf_stream_t stream);
/* ... over TWO record sets (a tile's foreground and background branch, each planned / emitted on its own workspace over the
 * same B rays and table, S1 / S2 samples): both gradients meet in one bucket image and ONE Adam step (tile.py:880-1015). */
int scanerf_render_scatter_accumulate_adam2(float *params, float *exp_avg, float *exp_avg_sq, void *half_table,
                                            int half_dtype, float *overflow_grad, float lr, float beta1, float beta2,
                                            float eps, int step, int B, int T, int S1, void *workspace1,
                                            size_t workspace1_bytes, int S2, void *workspace2, size_t workspace2_bytes,
                                            int arith, scanerf_stream_t stream);
/* Valid-ray compaction of a training batch (hashgrid/__init__.py:419-434: valid = all(z_vals != -1), then rays_o[valid],
 * rays_d[valid], z_vals[valid], dists[valid]; tile.py gathers the targets the same way), without torch's nonzero + gathers:
 * scanerf_ray_valid writes the flags, scanerf_compact_rays moves the valid rays' entries, in their original order, to rows
 * [0, *count) of the out_* buffers (each sized for B rays; count: device int32).  target / out_t and out_index [B] i32 (source
 * ray of each output row) may be NULL.  valid: 16-byte aligned.  Wave ballot + popcount prefix sums, no atomics. */
int scanerf_ray_valid(const float *z_vals, uint8_t *valid, int B, int S, scanerf_stream_t stream);
int scanerf_compact_rays(const uint8_t *valid, int B, int S, const float *rays_o, const float *rays_d, const float *target,
                         const float *z_vals, const float *dists, float *out_o, float *out_d, float *out_t, float *out_z,
                         float *out_dist, int32_t *out_index, int32_t *count, scanerf_stream_t stream);

/* Photometric loss of the training step and dL/d(out_ray) in two launches (criterions.py:90,142-144 MSE over the valid
 * rays' rgb + tile.py:999 reg_weight * l2_reg_specular = mean over valid rays x 3 of out_ray[:,14]):
 *   loss [1] = (sum_valid |rgb - target|^2 + reg_weight * sum_valid out_ray[:,14]) / (3 * n_valid)
 *   grad_out [B,16] = its gradient w.r.t. out_ray (all 16 columns written; invalid rays zero)
 * scratch: scanerf_photometric_loss_scratch_floats() f32.  Deterministic (fixed reduction order). */
/* Ray gradients of a scanerf_render_backward call that produced g_raypos (render.py ray_gradients_fused; replaces autograd through
 * network.py:38-77 sh_encoding and the direction normalisation of :177): g_o = g_raypos[:,0:3]; g_d = g_raypos[:,3:6] + the |d|
 * path (g_dnorm [B,ceil(S/32)] summed) + the SH path (g_rowsum [B,2,64] x Directional_MLP.mlp.0 weight rows 32..47 of mlp_blob).
 * Rays with ray_valid == 0 get zeros. */
int scanerf_ray_grad_epilogue(const float *rays_d, const float *mlp_blob, const float *g_raypos, const float *g_dnorm,
                              const float *g_rowsum, const uint8_t *ray_valid, float *g_o, float *g_d, int B, int S,
                              scanerf_stream_t stream);
/* Alpha compositing of per-sample decoder outputs along rays and its adjoint, as stand-alone ops: HashGrid.cal_integrate_weight
 * (hashgrid/__init__.py:344-360) + the accumulate calls and the l2_reg_specular sum of render_batch_rays (:362-366, :564-574,
 * :591-594) in one launch each way, for callers that keep the decoder outputs as tensors (the op-by-op route).
 *   sigma [B*S], diffuse / specular / tint [B*S,3], z_vals / dists [B,S], rays_d [B,3]; infinity: the last sample's delta is 1e10;
 *   out_ray [B,16]: the columns scanerf_render_forward_packed writes (rgb, depth, T_left = transmittance BEFORE the last sample,
 *   diffuse, specular, tint, sum w |c_s|^2); weights [B,S] (may be NULL).
 * Backward: grad_out [B,16] (column 14 differentiates sum w |c_s|^2 with w detached, as :593), grad_weights [B,S] (may be NULL) ->
 *   dL/d(sigma) [B*S], dL/d(diffuse / specular / tint) [B*S,3], g_dnorm [B] (may be NULL) = dL/d|rays_d| through delta. */
int scanerf_composite_forward(const float *sigma, const float *diffuse, const float *specular, const float *tint, const float *z_vals,
                              const float *dists, const float *rays_d, float *out_ray, float *weights, int B, int S, int infinity,
                              scanerf_stream_t stream);
int scanerf_composite_backward(const float *sigma, const float *diffuse, const float *specular, const float *tint, const float *z_vals,
                               const float *dists, const float *rays_d, const float *out_ray, const float *grad_out,
                               const float *grad_weights, float *g_sigma, float *g_diffuse, float *g_specular, float *g_tint,
                               float *g_dnorm, int B, int S /* <= 512 */, int infinity, scanerf_stream_t stream);
int scanerf_photometric_loss_scratch_floats(void);
int scanerf_photometric_loss_grad(const float *out_ray, const float *target /*[B,3]*/, const uint8_t *ray_valid,
                                  float reg_weight, float *grad_out, float *loss, float *scratch, int B,
                                  scanerf_stream_t stream);
/* The same for the complete per-tile render (tile.py:666-690 merge, tile.py:880-1015 loss): pred = fg.rgb + fg.T_left * bg.rgb,
 * loss [1] = mean over the rays valid in either branch (criterions.py:121-138: valid = fore_valid | bg_valid) x 3 of
 * (pred - target)^2 + reg_weight * (l2_reg_specular of the fg-valid rays + of the bg-valid rays); rays invalid in both
 * branches get zero gradients; grad_fg / grad_bg [B,16] = its gradients w.r.t. the two branches' out_ray (fg: rgb, T_left and column 14;
 * bg: rgb and column 14).  scratch as above. */
int scanerf_photometric_loss_grad_fgbg(const float *out_fg, const float *out_bg, const float *target,
                                       const uint8_t *valid_fg, const uint8_t *valid_bg, float reg_weight, float *grad_fg,
                                       float *grad_bg, float *loss, float *scratch, int B, scanerf_stream_t stream);
/* Device self-test of the split-f16 backward primitives (csrc/render_h3.h; test infrastructure, one wave):
 * workspace from scanerf_pack_decoder; dy, x [64][32] f32 -> out_dx [2][64][32] (W^T dy of Spatial_MLP.mlp.2, and
 * of the H part of Directional_MLP.mlp.0 in rows 0..31 of the second slab), out_dw [64][64] = dy x^T, out_rs [64]
 * = row sums of dy. */
int scanerf_h3_selftest(const float *workspace, const float *dy, const float *x, float *out_dx, float *out_dw,
                        float *out_rs, scanerf_stream_t stream);
/* Test infrastructure: one launch of ~300 KB of straight-line code on every CU, after which no other kernel's instructions are
 * left in the instruction caches (no reference counterpart; tests/test_gpu_determinism.py, tools/fault_probe.py: faults that only
 * show on cold instruction caches). */
int scanerf_icache_sweep(scanerf_stream_t stream);
/* Measurement infrastructure (no reference counterpart): blocks x 512 threads each issue loads_per_thread (multiple of 8) scattered
 * 8-byte loads over table[0 .. entries) (entries: power of two; make it far larger than the 32 MB of L2).  Timed by the caller,
 * loads / second = the chip's L2 <-> fabric request rate for scattered accesses (bench.py `roofline.fabric_requests`). */
int scanerf_gather_rate_probe(const void *table, long long entries, int blocks, int loads_per_thread, unsigned *sink,
                              scanerf_stream_t stream);
/* Test infrastructure: the 8-byte scatter-record codec (csrc/scatter_common.h Rec8) on n values.  words [n][2] = the packed
 * records; out [n][8] = l0, l1, the four contributions the accumulate adds (x, y to l0; x, y to l1), E - 25, t. */
int scanerf_rec8_selftest(const float *gx, const float *gy, const float *tx, const uint32_t *l0, const uint32_t *k, int n,
                          uint32_t *words, float *out, scanerf_stream_t stream);
/* For pose refinement (gradients w.r.t. the rays): g_dnorm = per-tile partials of dL/d|rays_d| through
 * delta = dist*|d| (hashgrid/__init__.py:347); g_rowsum = per-ray sums of dL/d(Directional_MLP.mlp.0
 * pre-activation) in two partial rows (their sum times W[:,32:48] is dL/dSH(viewdir)).  The gradient
 * through the sample positions comes from scanerf_embedding_bg_point_grad on dfeat. */
int scanerf_embedding_bg_point_grad(const float *points, const float *dfeat_level_major, float *grad_points,
                                    const float *features, const int32_t *resolutions, int N, int L, int T,
                                    scanerf_stream_t stream);

/* Encoder with an explicit mapping (for benchmarks and the two-kernel path):
 * variant 0 auto / 1 XCD-partitioned by level / 2 level-fastest; level_major_out != 0 writes
 * [L][N][2] instead of the binding surface's [N][L][2]. */
int scanerf_embedding_bg_forward_ex(const float *points, float *outputs, const void *features,
                                    const int32_t *resolutions, int N, int L, int T, int feat_dtype,
                                    int variant, int level_major_out, scanerf_stream_t stream);

/* ---- HASHGRID surface, render-time ops (hashgrid/include/rendering.h:20-182;
 *      hashgrid/src/rendering_kernel.cu, file:line per function) --------------------------------
 * Tile set: corners/sizes [nb,3] f32; occ = concatenated bool grids; grid_starts [nb] i64;
 * log2dim [nb,3] i32; intersections [B,nb,2] f32 (1e7 = miss); tracing_blocks [B,nb] i32
 * (argsort of near); block indices are int16, 4 slots, -1 = none. */
int scanerf_ray_block_intersection(const float *rays_o, const float *rays_d, const float *corners,
                                   const float *sizes, float *intersections, int B, int nb,
                                   scanerf_stream_t stream);                                   /* :126-174 */
/* sample_major (the per-sample arrays of the render-time ops below): 0 = the reference's [B][S] arrays; 1 = [S][B] (z_vals,
 * dists, block_idxs [S][B][4], the per-sample outputs [S][B][3] / [S][B]): the renderer's own layout -- a wave's 32 samples are
 * then one depth index of 32 neighbouring rays (pixels), whose cells coincide down to the fine levels, instead of 32 depths of
 * one ray.  Same arithmetic per sample. */
int scanerf_render_sample_points(const float *rays_o, const float *rays_d, const float *corners,
                                 const float *sizes, const uint8_t *occ, const int64_t *grid_starts,
                                 const int32_t *log2dim, const int32_t *tracing_blocks,
                                 const float *intersections, int32_t *tracing_idx, float *z_start,
                                 float *z_vals, float *dists, int B, int S, int nb,
                                 int sample_major, scanerf_stream_t stream);                                     /* :179-382 */
int scanerf_prepare_points(const float *z_vals, const uint8_t *running_mask, const float *intersections,
                           int16_t *block_idxs, int B, int S, int nb, int sample_major, scanerf_stream_t stream); /* :391-449 */
/* images [nb][scanerf_render_workspace_floats()]: each tile's decoder blob packed by
 * scanerf_pack_decoder with weight_feature == 1; tables [nb,16,T,2] f16; resolution [nb,16,3] i32 */
int scanerf_pts_inference(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                          const int16_t *block_idxs, const void *tables_f16, const float *images,
                          const int32_t *resolution, const uint8_t *occ, const int64_t *grid_starts,
                          const int32_t *log2dim, const float *corners, const float *sizes, float *diffuse,
                          float *specular, float *alpha, int B, int S, int T, int nb,
                          int sample_major, scanerf_stream_t stream);                                            /* :467-621 */
/* SCANERF_SKIP_UNSAMPLED, OR-ed into `sample_major` of scanerf_pts_inference_tracing and scanerf_accumulate_color (the renderer's own
 * pair; no reference counterpart): a ray whose FIRST depth is -1 holds no sample in this tracing pass (sample_points fills a ray's
 * depths from index 0) -- the inference leaves its outputs unwritten and the accumulation does not read them, instead of 28 bytes
 * of zeros written and read per sample slot of such a ray.  Same per-ray results. */
#define SCANERF_SKIP_UNSAMPLED 4
/* Decoder arithmetic of scanerf_pts_inference / scanerf_pts_inference_tracing / scanerf_bg_pts_inference_v2, OR-ed into their
 * `sample_major` as well: none = 16-sample tiles at four waves per SIMD, every product on split-f16 MFMA (default);
 * SCANERF_INFER_H3 = the 32-sample-tile kernel at two waves per SIMD (same arithmetic, round 4's kernel);
 * SCANERF_INFER_F32 = the single-pass f32-input MFMA kernel (exact f32; [B][S] arrays only, also what > 64 tiles fall back to).
 * Measured per sample against a float64 evaluation (tests/test_gpu_render_infer_error.py, profiles/render_infer_error.md; diffuse,
 * specular and alpha, quantities bounded by 1): the default is within 3.2e-7 (median) and 4.6e-6 (largest sample) over every input
 * family there, 1.0 - 1.8 times what a float32 evaluation of the same formulas is off by; H3 and the plain images up to 2.3 times,
 * the f32 kernel up to 1.25 times.  Relative to a sample's own opacity the formula itself -- 1 - exp(-sigma delta) in float32 --
 * is good to 2^-24 / alpha only: 1e-3 (median) at alpha ~ 1e-5, for the kernels and for the float32 evaluation alike. */
#define SCANERF_INFER_H3 8
#define SCANERF_INFER_F32 16
/* SCANERF_INFER_FOLDED (16-sample-tile kernel only): `images` were packed by scanerf_pack_decoder from blobs whose three
 * Gaussian-activated layers -- Spatial_MLP.mlp.0, Directional_MLP.mlp.0 and .2, biases and weights: blob floats [0, 2112),
 * [6503, 9639), [9639, 13799) -- were multiplied by sqrt(50 log2 e) = 8.4932184 beforehand; the kernel then evaluates the
 * activation exp(-u^2 / 0.02) as exp2(-(u')^2): one vector instruction less per activation (48 per lane and 16-sample tile). */
#define SCANERF_INFER_FOLDED 32
/* prepare_points + pts_inference as ONE launch (no reference counterpart; the renderer's own route): the slot lists are derived
 * in the kernel from running_mask [B] and intersections [B,nb,2] at every use instead of being written and read back (8 bytes per
 * sample, once per tile step).  Same values as the two ops in sequence.  Needs the 16-sample-tile kernel (the default) and
 * nb <= 8; otherwise it fails and the caller runs the two ops. */
int scanerf_pts_inference_tracing(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                                  const uint8_t *running_mask, const float *intersections, const void *tables_f16,
                                  const float *images, const int32_t *resolution, const uint8_t *occ,
                                  const int64_t *grid_starts, const int32_t *log2dim, const float *corners,
                                  const float *sizes, float *diffuse, float *specular, float *alpha, int B, int S, int T,
                                  int nb, int sample_major, scanerf_stream_t stream);
int scanerf_accumulate_color(const float *pts_diffuse, const float *pts_specular, const float *pts_alpha,
                             float *transparency, const float *z_vals, float *diffuse, float *specular,
                             float *depth, int B, int S, int sample_major, scanerf_stream_t stream);             /* :624-702 */
int scanerf_render_inverse_z_sampling(const float *intersections, const int16_t *related_bidx, float *z_vals,
                                      float sample_range, int B, int S, int nb,
                                      int sample_major, scanerf_stream_t stream);                                /* :816-868 */
int scanerf_bg_pts_inference_v2(const float *rays_o, const float *rays_d, const float *z_vals,
                                const int16_t *bg_idxs, int step, const float *corners, const float *sizes,
                                const int32_t *resolution, const void *tables_f16, const float *images,
                                float *diffuse, float *specular, float *alpha, int B, int S, int T, int nb,
                                int sample_major, scanerf_stream_t stream);                                      /* :1012-1171 */
int scanerf_update_outgoing_bidx(const float *rays_o, const float *rays_d, const float *corners,
                                 const float *sizes, const int32_t *tracing_blocks, const float *intersections,
                                 int16_t *outgoing_bidxs, float *blend_weights, float ratio, int skip, int B,
                                 int nb, scanerf_stream_t stream);                             /* :1263-1401 */
int scanerf_update_outgoing_bidx_v2(const float *rays_o, const float *corners, const float *sizes,
                                    int16_t *inside_bidxs, float *blend_weights, int B, int nb,
                                    scanerf_stream_t stream);                                  /* :1406-1474 */
/* The tile order rendering.py:301 gets from torch.argsort(intersections[..., 0], dim=-1) (stable): order [B,nb] i32 = the
 * ray's tiles by entry distance (misses, 1e7, last; equal distances by tile index).  nb <= 64. */
int scanerf_sort_tracing_blocks(const float *inter, int32_t *order, int B, int nb, scanerf_stream_t stream);
int scanerf_get_last_block(const int32_t *tracing_blocks, int32_t *bidxs, const float *intersections, int B,
                           int nb, scanerf_stream_t stream);                                   /* :1212-1260 */
int scanerf_ray_firsthit_block(const float *rays_o, const float *rays_d, const float *corners, const float *sizes,
                               const uint8_t *occ, const int64_t *grid_starts, const int32_t *log2dim,
                               const int32_t *tracing_blocks, const float *intersections, int16_t *hit_blockIdxs,
                               int B, int nb, scanerf_stream_t stream);                        /* :705-813 */
int scanerf_process_occupied_grid(int bidx, int total_grid, const float *corners, const float *sizes,
                                  const uint8_t *occ, const int64_t *grid_starts, const int32_t *log2dim,
                                  uint8_t *tgt_occ, int nb, scanerf_stream_t stream);          /* :1479-1564 */

/* cuda/include/voxelize.h:12-119 (CUDA_EXT.voxelize_mesh after its PLY read: cuda/include/plyIO.h): mark the cells of the
 * sampler grid that the 1.5x-inflated boxes of the mesh faces overlap; init_out != 0 also marks (vis and outside) every
 * cell whose centre lies outside the union box of the faces that touch the grid.  vertices [V,3] f32, faces [F,3] i32,
 * vis / outside bool grids [2^lx,2^ly,2^lz], scratch6 6 x u32 -- device; log2dim [3], block_corner [3], block_size [3] --
 * HOST (the reference takes them as CPU tensors). */
int scanerf_voxelize_mesh(const float *vertices, const int32_t *faces, int V, int F, const int32_t *log2dim,
                          const float *block_corner, const float *block_size, uint8_t *vis, int init_out,
                          uint8_t *outside, uint32_t *scratch6, scanerf_stream_t stream);

/* ---- stand-alone decoder op (ABI 7): network.ShallowMLP.forward (network.py:172-190) and its adjoint, one launch each, on the
 * matrix cores at the fused kernels' arithmetic (split-f16 operands, three products per term, f32 accumulate: f32-equivalent).
 * What an unchanged HashGrid.render_batch_rays calls between the encoder op and its torch compositing
 * (hashgrid/__init__.py:545-548: decoder(cat([features, rays_d]), weight_feature=...)).
 *   feats / dirs: rows of 32 / 3 floats with row strides ld_feats / ld_dirs IN FLOATS -- for the reference's concatenated
 *     x [N,35]: feats = x, dirs = x + 32, both strides 35 (no slicing copy); the direction is normalised inside
 *     (d / (|d| + 1e-8), network.py:177);
 *   workspace: scanerf_pack_decoder(blob, weight_feature, workspace) -- weight_feature [32] is folded into the first layer;
 *   forward outputs: sigma [N] (= [N,1]), diffuse / specular / tint [N,3], contiguous; specular is the RAW sigmoid output
 *     (the caller multiplies by tint, hashgrid/__init__.py:568);
 *   backward: g_* = dL/d(those outputs) (contiguous; any may be NULL = zero) -> d_feats rows of 32 floats (stride ld_dfeats;
 *     dL/d(features), weight_feature applied), d_dirs rows of 3 floats (stride ld_ddirs; NULL = not wanted) -- for the
 *     gradient of x [N,35]: d_feats = gx, d_dirs = gx + 32, strides 35 -- and grad_blob [13994] += dL/d(blob) (deterministic
 *     reduction of one partial row per workgroup); dw_partial: scratch of scanerf_decoder_backward_grid(N) x 13994 floats. */
int scanerf_decoder_forward(const float *feats, int ld_feats, const float *dirs, int ld_dirs, const float *workspace,
                            float *sigma, float *diffuse, float *specular, float *tint, long long N, scanerf_stream_t stream);
int scanerf_decoder_backward_grid(long long N);
int scanerf_decoder_backward(const float *feats, int ld_feats, const float *dirs, int ld_dirs, const float *workspace,
                             const float *weight_feature, const float *g_sigma, const float *g_diffuse, const float *g_specular,
                             const float *g_tint, float *d_feats, int ld_dfeats, float *d_dirs, int ld_ddirs, float *dw_partial,
                             float *grad_blob, long long N, scanerf_stream_t stream);

/* ---- multi-view warp loss (csrc/warp.hip): warp_loss.py:147-660 WarpLoss.__call__ and cuda/view_selection_kernel.cu:19-349,
 * without the host round trips of the reference (its sample_neighbor_color indexes the images on the CPU every step).
 *   Rays: rays_o, rays_d [B,3]; ray_q [B,7] = (depth, diffuse[3], specular[3]) of the merged prediction (tile.py:666-690); the point
 *   is p = rays_o + depth * rays_d (warp_loss.py:548).  ray_valid [B] (NULL = all) marks the rays the loss counts (criterions.py:
 *   101-110: fore_valid | bg_valid).  Cameras: ks [N,3,3], rts [N,3,4] world-to-camera.  K slots per ray, 1 <= K <=
 *   scanerf_warp_max_neighbors() and K <= N (the reference's topk(k=10) raises when N < 10: callers pass min(10, N)).
 * scanerf_warp_select_views -- replaces computeViewcost (view_selection_kernel.cu:19-72) + topk + the 0.176 threshold
 *   (warp_loss.py:390-413): the K cameras of lowest cost per ray (ties: lower index first), cost in nei_cost [B,K], nei_valid [B,K]
 *   = cost <= 0.176 (0 for rays outside ray_valid).  No [N,B] cost matrix. */
int scanerf_warp_max_neighbors(void);
int scanerf_warp_select_views(const float *rays_o, const float *rays_d, const float *ray_q, const uint8_t *ray_valid,
                              const float *ks, const float *rts, int N, int H, int W, int K, int B, int *nei_views,
                              float *nei_cost, uint8_t *nei_valid, scanerf_stream_t stream);
/* scanerf_warp_project -- replaces proj2neighbor_forward (view_selection_kernel.cu:115-211, warp_loss.py:415-439) and
 *   sample_neighbor_color (warp_loss.py:441-521): per (ray, slot) grid [B,K,2] = K (R p + t) .xy / (.z + 1e-8) - 0.5,
 *   proj_depth [B,K] = .z, nei_origin / nei_direction [B,K,3] = the neighbour camera's centre and R^T (x/(z+1e-8), y/(z+1e-8), 1)
 *   of the camera-space point, nei_color [B,K,3] = bilinear from images [N,H,W,3] f32 with the top-left corner at trunc(grid),
 *   nei_valid = nei_valid_in AND occlusions [N,H,W] (NULL = all true) at trunc(grid + 0.5).  Invalid slots are zero-filled. */
int scanerf_warp_project(const float *rays_o, const float *rays_d, const float *ray_q, const float *ks, const float *rts,
                         const int *nei_views, const uint8_t *nei_valid_in, const float *images, const uint8_t *occlusions, int N,
                         int H, int W, int K, int B, float *grid, float *proj_depth, float *nei_origin, float *nei_direction,
                         float *nei_color, uint8_t *nei_valid, scanerf_stream_t stream);
/* scanerf_warp_loss_grad -- replaces compute_loss (warp_loss.py:332-337, :650-656) with its autograd and proj2neighbor_backward
 *   (view_selection_kernel.cu:214-349): loss [1] = scale / (n K) * sum over valid slots of score [B,K] * mean_c((clamp(diffuse +
 *   specular, 0, 1) - nei_color)^2), n = number of valid rays; grad_q [B,7] = dL/d(ray_q), grad_o / grad_d [B,3] = dL/d(rays_o,
 *   rays_d) through p, grad_rts [N,12] = dL/d(rts) (overwritten).  The colour's gradient reaches grid through the bilinear weights
 *   and p / rts through the projection Jacobian in the same launch.  grad_rts is summed in a fixed order (per-(ray, slot) partials,
 *   then per (camera, chunk) and chunk by chunk), not with the reference's float atomics: bit-reproducible.  scratch: scanerf_warp_scratch_floats
 *   (B, K, N) floats.  grid / nei_color / nei_valid as scanerf_warp_project wrote them. */
size_t scanerf_warp_scratch_floats(int B, int K, int N);
int scanerf_warp_loss_grad(const float *rays_o, const float *rays_d, const float *ray_q, const uint8_t *ray_valid, const float *ks,
                           const float *rts, const int *nei_views, const uint8_t *nei_valid, const float *grid,
                           const float *nei_color, const float *score, const float *images, int N, int H, int W, int K, int B,
                           float scale, float *loss, float *grad_q, float *grad_o, float *grad_d, float *grad_rts, float *scratch,
                           size_t scratch_floats, scanerf_stream_t stream);

/* ---- monocular prior losses (csrc/mono.hip): mono_loss.py DepthConsistencyLoss + DepthSmoothLoss (criterions.py:99-105,170-183)
 *   and their gradient w.r.t. the per-ray rendered depth, in one call.  depth [B] = the merged pred_depth (tile.py:666-690);
 *   ray_valid [B] (NULL = all): fore_valid | bg_valid; locs [B,3] int32 (view, px, py), integer pixel coordinates; a ray whose
 *   locs fall outside [0,N) x [0,W) x [0,H) counts as invalid.  Views are grouped by locs[:,0] (any ray order).
 *   Depth consistency (mono_depth [N,H,W], NULL or w_depth = 0: off): per view the scale / shift (h0, h1) of depth onto mono_depth
 *   from f64 moments (h = 0 when det = 0); L_depth = sum m (h0 p + h1 - t)^2 / sum m over all views (0 when no ray is valid);
 *   dL/dp = 2 m h0 (h0 p + h1 - t) / sum m (the gradient through h is 0 analytically).
 *   Depth smoothness (mono_normal [N,H,W,3], NULL or w_smooth = 0: off; needs kinv [N,9] = K^-1 row-major and B % 4 == 0): rays
 *   4k..4k+3 are a 2x2 patch (r = 2 dy + dx) of one view; valid iff all four rays are valid, share a view and n_r . mean(n) > 0.9;
 *   L_smooth = mean over valid patches of 0.25 sum |normalize(mean n) . normalize(edge)| (0, zero gradient, when none).
 *   loss [3] = (w_depth L_depth + w_smooth L_smooth, L_depth, L_smooth); grad_depth [B] = d loss[0] / d depth (overwritten).
 *   No allocation, no host synchronisation, no float atomics (every sum in a fixed order: bit-reproducible).  scratch:
 *   scanerf_mono_scratch_floats(B, N) floats, 8-byte aligned. */
size_t scanerf_mono_scratch_floats(int B, int N);
int scanerf_mono_loss_grad(const float *depth, const uint8_t *ray_valid, const int32_t *locs, const float *mono_depth,
                           const float *mono_normal, const float *kinv, int N, int H, int W, int B, float w_depth, float w_smooth,
                           float *loss, float *grad_depth, float *scratch, size_t scratch_floats, scanerf_stream_t stream);

/* ---- ray / triangle-mesh tracer (csrc/mesh.hip): the reference's third compiled module, fastMesh (fastMesh/binding.cpp:
 *   build / fisrtHit / firstEnter / getSceneBound).  A uniform grid of 2^log2dim cells per axis (4 <= log2dim <= 7; the reference's
 *   LOG2DIM is 6) over the cube [min_corner, min_corner + 2^log2dim * cell]; scene_info [4] f32 DEVICE = (min_corner, cell), cell =
 *   largest extent of the vertex bounds / 2^log2dim.  vertices [V,3] f32, faces [F,3] i32.  Cell index n = (x << 2 log2dim) |
 *   (y << log2dim) | z.  A face is registered in every cell its axis-aligned box overlaps (tile_structure.h:43-82); faces with a vertex
 *   index outside [0,V) are left out.
 * Build (replaces break_into_tiles, tile_structure.h:13-106, a host loop; here on the device, without atomics, bit-reproducible):
 *   scanerf_mesh_count_cells: counts [F] = number of cells of each face;
 *   scanerf_mesh_emit_keys: keys [n_keys] i64 = (cell << 32) | face for every (face, cell) pair, face f's from offsets [F] (the
 *     exclusive scan of counts); sorted by the caller they are cell_faces in the reference's order (ascending face inside a cell);
 *   scanerf_mesh_cell_boxes: cell_box [n_cells,6] = min xyz, max xyz over the vertices of the faces of each occupied cell (what
 *     singleRay_firstEnter recomputes per ray, fastMesh_kernel.cu:157-184); start_num [n_cells,2] i32 = (start, count) into
 *     cell_faces [n_entries] i32;
 *   scanerf_mesh_gather_triangles: tris [n_entries,9] = (A, B - A, C - A) per cell_faces entry (optional: first_hit without its two
 *     indirections).
 * Traces (replace firstHit_cuda / firstEnter_cuda, fastMesh_kernel.cu:195-329): rays_o, rays_d [B,3] (not assumed normalised: t in
 *   units of |d|), out [B] f32, 0 = nothing found.  bitmask [2^(3 log2dim) / 64] u64, rank [same] u32 = set bits in all earlier words.
 *   The ray is clipped to the grid cube first (origins outside the grid are valid).  lds != 0 stages bitmask and rank into the LDS
 *   (log2dim <= 6).
 *   scanerf_mesh_first_hit: nearest intersection t > 0, two-sided, edges inclusive; the candidate is carried across cells (the
 *     reference returns at the first cell with any hit, :284-290).  tris != NULL: pre-gathered triangles; else vertices / faces /
 *     cell_faces.
 *   scanerf_mesh_first_enter: the first occupied cell in ray order whose cell_box the ray hits: the slab entry distance (clamped
 *     at 0, so a ray that starts inside that box gives 0 = nothing, as the reference, :181-186). */
int scanerf_mesh_count_cells(const float *vertices, const int32_t *faces, int V, int F, int log2dim, const float *scene_info,
                             int32_t *counts, scanerf_stream_t stream);
int scanerf_mesh_emit_keys(const float *vertices, const int32_t *faces, int V, int F, int log2dim, const float *scene_info,
                           const int64_t *offsets, int64_t *keys, long long n_keys, scanerf_stream_t stream);
int scanerf_mesh_cell_boxes(const float *vertices, const int32_t *faces, const int32_t *start_num, const int32_t *cell_faces,
                            int n_cells, float *cell_box, scanerf_stream_t stream);
int scanerf_mesh_gather_triangles(const float *vertices, const int32_t *faces, const int32_t *cell_faces, long long n_entries,
                                  float *tris, scanerf_stream_t stream);
int scanerf_mesh_first_hit(const float *rays_o, const float *rays_d, int B, const float *vertices, const int32_t *faces,
                           const float *tris, const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                           const int32_t *cell_faces, const float *scene_info, int log2dim, int lds, float *out,
                           scanerf_stream_t stream);
int scanerf_mesh_first_enter(const float *rays_o, const float *rays_d, int B, const uint64_t *bitmask, const uint32_t *rank,
                             const int32_t *start_num, const float *cell_box, const float *scene_info, int log2dim, int lds,
                             float *out, scanerf_stream_t stream);

/* ---- tile allocation (csrc/coverage.hip): the one hot step of the reference's preprocess/build_tiles.py:129-156, fused.  For every
 *   camera c and every candidate tile box k: counts[k][c] = number of pixels of the reduced frame (h = H / scale, w = W / scale,
 *   integer division) whose ray enters box k before it meets the mesh.  Ks [C,9] and C2Ws [C,12] row-major f32.  Rays are the
 *   reference's get_rays_torch_v2 on K / scale (no +0.5 pixel centre): x = (i - cx / scale) / (fx / scale), y = (j - cy / scale) /
 *   (fy / scale), d = x R[:,0] + y R[:,1] + R[:,2] (not normalised), o = C2W[:,3].  Depth = scanerf_mesh_first_hit's, 0 -> 1e5; near =
 *   scanerf_ray_aabb_intersection's (box_sizes: full sides), a miss never counts; counted where near < depth.  The tracer's arrays are
 *   scanerf_mesh_first_hit's.  counts [K,C] i32 must be ZERO-FILLED by the caller: workgroups add into it (integer adds: exact,
 *   two launches give equal bits).  The boxes are walked in passes of scanerf_view_coverage_boxes_per_pass(); any K works.
 *   C == 0 or K == 0 is a no-op. */
int scanerf_view_coverage_boxes_per_pass(void);
int scanerf_view_coverage(const float *Ks, const float *C2Ws, int C, int H, int W, int scale, const float *box_centers,
                          const float *box_sizes, int K, const float *vertices, const int32_t *faces, const float *tris,
                          const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces,
                          const float *scene_info, int log2dim, int32_t *counts, scanerf_stream_t stream);

/* ---- surface normals (csrc/normals.hip): the density's position gradient, fused.  The reference forms it by torch
 *   autograd through encoder and decoder (hashgrid/__init__.py:374-392 compute_normal, :576-588 render_batch_rays(out_normal=True),
 *   tile.py:695-712 render_normals).  Here: one gather pass per sample (features and their three position tangents from the same
 *   eight corner values of each level), the 64 x 32 first-layer product on the f32-input matrix instruction, and the rest of the
 *   density path in closed form (it is linear behind the first layer).  16 levels, 32-channel decoder; tables f32 / f16.
 *     x = contracted position in [-2,2]^3, cells as scanerf_embedding_bg_forward;  f = feat * weight_feature [32];
 *     u0 = W0 f + b0;  s = ws . (W1[:32] G(u0) + b1[:32]) + bs;  sigma = softplus(s);  G(u) = exp(-50 u^2);
 *     g_k = d sigma / d p_k = sigmoid(s) sum_j a_j G'(u0_j) (W0 (weight_feature * d feat / d p_k))_j,  a = W1[:32]^T ws^T;
 *     d feat_l / d p_k = A_k (res_l,k - 1) / 4 * sum_c (d w_c / d t_k) table_l[idx_c];   n = -g / (|g| + 1e-8).
 *   mlp_blob: the flat decoder blob [SCANERF_PARAMSIZE] (not a packed image); weight_feature [32] f32.  Deterministic.
 * Point form: x = points [N,3] as given, A = axis_scale [3] (host).  -> sigma [N], grad [N,3] = g (may be NULL), normal [N,3]. */
int scanerf_sigma_normals_points(const float *points, const float *axis_scale /*[3] host*/, const void *features, int feat_dtype,
                                 const int32_t *resolutions /*[16,3]*/, const float *mlp_blob, const float *weight_feature,
                                 float *sigma, float *grad, float *normal, int N, int T, scanerf_stream_t stream);
/* Ray form: samples o + z d, x = contract_fore of the box min_bbox / bbox_size ([3] host each; A = 4 / bbox_size), weights w_i of
 *   hashgrid/__init__.py:344-360 (delta = dists |d|, T_i = prod_{j<i} (1 - alpha_j + 1e-6), infinity: the last delta is 1e10).
 *   -> out [B,4] = (sum_i w_i n_i, sum_i w_i), 16-byte aligned; sample_normals [B,S,3] = n_i (may be NULL).  Rays with
 *   ray_valid[b] == 0 (ray_valid may be NULL) write zeros.  The background contraction is not offered. */
int scanerf_render_normals(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists, const void *features,
                           int feat_dtype, const int32_t *resolutions, const float *mlp_blob, const float *weight_feature,
                           const float *min_bbox /*[3] host*/, const float *bbox_size /*[3] host*/, int infinity,
                           const uint8_t *ray_valid, float *out, float *sample_normals, int B, int S, int T,
                           scanerf_stream_t stream);

/* ---- normal maps of the multi-tile render (csrc/render_normals_tiles.hip).  The reference has no multi-tile
 *   normal; the definition is this comment.  Normals are blended exactly as scanerf_pts_inference blends colours
 *   (rendering_kernel.cu:467-581).  For sample t of ray i with slot list block_idxs[t][0..3] (int16; -1 ends the list), each listed
 *   tile b in turn, in float32:
 *     pts = (o + z d - corner_b) / size_b (corner / size of the render box);  dis = (0.5 - |pts - 0.5|) size_b;
 *     w_b = xz_weight(dis.x, dis.z), counted in W = sum_b w_b whether or not the cell is occupied;
 *     the tile contributes only if its occupancy cell (scanerf_pts_inference's loc / cell offset) is set; then
 *       p01 = pts / 2 + 0.25;  per level v = p01 (res - 1), i0 = int(v), t = v - i0 (scanerf_pts_inference's expression: a sample's
 *       normal and colour read the same cells);  tables f16, read as exported;  density and gradient by the closed form above with
 *       weight_feature == 1 and the contracted coordinate x = 2 pts - 1 (A = 2 / size_b per axis):  g_b = d sigma_b / d world
 *       position,  n_b = -g_b / (|g_b| + 1e-8);  pa_b = 1 - exp(-sigma_b dist |d|), |d| of the un-normalised direction;
 *     pts_normal[t] = sum_b w_b pa_b n_b (summed in slot order), divided by W when W > 0.
 *   Samples with no listed tile (z == -1 among them) give exactly (0, 0, 0).  EVERY sample is written.  blobs: the flat decoder blobs
 *   [nb][SCANERF_PARAMSIZE] (not packed images); resolution [nb,16,3]; tables_f16 [nb,16,T,2]; occ / grid_starts / log2dim / corners /
 *   sizes as scanerf_pts_inference.  pts_normal [B,S,3] and the per-sample inputs in the layout `sample_major` (0, 1 or 2, no flag
 *   bits).  Any nb that fits the int16 slots; B * S < 2^31.  Deterministic; a sample's bits do not depend on the layout. */
int scanerf_pts_normals(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists, const int16_t *block_idxs,
                        const void *tables_f16, const float *blobs, const int32_t *resolution, const uint8_t *occ,
                        const int64_t *grid_starts, const int32_t *log2dim, const float *corners, const float *sizes,
                        float *pts_normal, int B, int S, int T, int nb, int sample_major, scanerf_stream_t stream);
/* The same launch with four counters added into counts [4] u32 (caller-zeroed): [0] 64-sample groups that ran at least one tile,
 *   [1] stagings of a tile's operands in LDS, [2] passes of the per-tile loop (one gather and first-layer product of a whole wave
 *   each), [3] lanes that held a sample in those passes.  Measurement entry point (tools/bench_render_normals.py). */
int scanerf_pts_normals_counted(const float *rays_o, const float *rays_d, const float *z_vals, const float *dists,
                                const int16_t *block_idxs, const void *tables_f16, const float *blobs, const int32_t *resolution,
                                const uint8_t *occ, const int64_t *grid_starts, const int32_t *log2dim, const float *corners,
                                const float *sizes, float *pts_normal, unsigned int *counts, int B, int S, int T, int nb,
                                int sample_major, scanerf_stream_t stream);
/* Per-ray accumulation by scanerf_accumulate_color's rule: a ray whose transparency is < 1e-5 is skipped; otherwise per sample, in
 *   order, normal += T pts_normal[t], T <- T (1 - pts_alpha[t]), T starting at the ray's transparency, pts_alpha as
 *   scanerf_pts_inference wrote it.  transparency [B] is read, not written: run this BEFORE scanerf_accumulate_color of the same pass.
 *   normal [B,3] is added into (the raw accumulated vector, world coordinates; foreground only; a display mapping (n + 1) / 2 stays
 *   with the caller).  SCANERF_SKIP_UNSAMPLED OR-ed into sample_major: a ray whose first depth is -1 is not read (its pts_alpha is
 *   uninitialised memory behind scanerf_pts_inference_tracing). */
int scanerf_accumulate_normal(const float *pts_normal, const float *pts_alpha, const float *transparency, const float *z_vals,
                              float *normal, int B, int S, int sample_major, scanerf_stream_t stream);

/* ---- level-set mesh extraction (csrc/isosurface.hip).  The reference has no mesh extraction; the definition is
 *   this comment.  float32 unless said otherwise.
 *   Lattice: n = (nx, ny, nz) cells over the tile box (occ_corner / occ_size in world coordinates, [-1,1]^3 in contracted ones).
 *     Point (i,j,k), 0 <= i <= nx (likewise j, k), has the contracted position x = float(i) * h_x - 1, h_x = 2.0f / float(nx), the
 *     multiply and the subtract separately rounded; y and z alike.
 *   Field: v(i,j,k) = sigma(x) if the point is live, else 0.  sigma is what scanerf_sigma_normals_points returns for that x, bit
 *     for bit (16 levels, 32-channel decoder, f32 or f16 table, weight_feature).  With G = 2^log2dim per axis, point i lies in the
 *     CLOSED occupancy cell c (0 <= c < G) of an axis iff c n <= i G <= (c + 1) n (integers; at most two cells per axis, eight in
 *     all); the point is live iff any of those cells is set in occupied_grid [Gx,Gy,Gz].
 *   Inside: v > level, strict, level > 0 (sigma units): unoccupied space is outside.
 *   Surface nets: cell (i,j,k), 0 <= i < nx etc., is active when its 8 corners are neither all inside nor all outside.  An active
 *     cell owns one vertex, the mean of the crossing points of those of its 12 edges whose ends differ in `inside`.  On an edge
 *     along axis a from point p (value va) to p + e_a (value vb) the crossing has the lattice coordinate p_a + t,
 *     t = (level - va) / (vb - va), and integer coordinates otherwise.  Edges are summed in the order a = 0, 1, 2 and, within an
 *     axis, with o1 = (a+1)%3 and o2 = (a+2)%3, the offsets (d1,d2) along (o1,o2) in the order (0,0), (1,0), (0,1), (1,1);
 *     sequentially in float32, then divided by the count.  The vertex L (lattice coordinates) has the contracted position
 *     L * h - 1 and the world position occ_corner + L * (occ_size / n) (dense op: origin + L * spacing), separately rounded.
 *     A lattice edge along a from p to p + e_a whose ends differ and which is interior (1 <= p_o1 <= n_o1 - 1 and
 *     1 <= p_o2 <= n_o2 - 1) gives one quad over the vertices of the four cells p + (d1,d2), (d1,d2) = (-1,-1), (0,-1), (0,0),
 *     (-1,0) along (o1,o2), in this cyclic order q0..q3 -- reversed if p is outside -- split into the triangles (q0,q1,q2) and
 *     (q0,q2,q3): counter-clockwise seen from the outside.  Edges on the faces of the tile box give no quad: the mesh is open
 *     there, where the neighbouring tile continues.
 *   Two passes.  count: per brick of 8^3 cells the active-cell mask and the vertex / quad counts, then their exclusive sums, all in
 *     `scratch` (scanerf_isosurface_scratch_bytes(nx,ny,nz) bytes, 16-byte aligned: 72 bytes per brick + 72; 0 for a lattice that
 *     is refused); its first 16 bytes then hold int64 V and int64 F (triangles).  The caller reads them, allocates, and calls
 *     emit with the SAME arguments and the scratch as count left it:  vertices [V,3] f32 (world), faces [F,3] i32, cells [V,3] i32
 *     (the owning cell of each vertex), lattice [V,3] f32 (L; may be NULL).  Vertices are ordered by brick, then by cell within
 *     the brick; faces by brick, then edge.  No atomics: the same bits from launch to launch.  A brick whose entries would not fit
 *     V / F as passed is not written.  V == 0 is a no-op.  Nothing proportional to the lattice points is ever stored; the fused
 *     emit evaluates the density of the bricks that hold a vertex a second time.
 *   Refused before any launch: null pointers, level <= 0, n_k < 1, 2^31 or more cells or points, occ_cells (the elements of
 *     occupied_grid) != 2^(log2dim[0] + log2dim[1] + log2dim[2]), T not a power of two.
 * Dense op: the field is the caller's array values [nx+1, ny+1, nz+1] f32 (device); origin / spacing [3] host. */
size_t scanerf_isosurface_scratch_bytes(int nx, int ny, int nz);
int scanerf_isosurface_count_dense(const float *values, int nx, int ny, int nz, float level, void *scratch, size_t scratch_bytes,
                                   scanerf_stream_t stream);
int scanerf_isosurface_emit_dense(const float *values, int nx, int ny, int nz, float level, const float *origin /*[3] host*/,
                                  const float *spacing /*[3] host*/, const void *scratch, size_t scratch_bytes, float *vertices,
                                  int32_t *faces, int32_t *cells, float *lattice, int V, int F, scanerf_stream_t stream);
/* Fused: the field is the tile's density, evaluated brick by brick where the sampler is occupied.  features [16,T,2] f32 / f16,
 *   resolutions [16,3], mlp_blob (flat decoder blob), weight_feature [32], occupied_grid (u8 / bool) on the device; log2dim,
 *   occ_corner, occ_size [3] host. */
int scanerf_isosurface_count(const void *features, int feat_dtype, const int32_t *resolutions, const float *mlp_blob,
                             const float *weight_feature, int T, const uint8_t *occupied_grid, const int32_t *log2dim /*[3] host*/,
                             long long occ_cells, int nx, int ny, int nz, float level, void *scratch, size_t scratch_bytes,
                             scanerf_stream_t stream);
int scanerf_isosurface_emit(const void *features, int feat_dtype, const int32_t *resolutions, const float *mlp_blob,
                            const float *weight_feature, int T, const uint8_t *occupied_grid, const int32_t *log2dim /*[3] host*/,
                            long long occ_cells, int nx, int ny, int nz, float level, const float *occ_corner /*[3] host*/,
                            const float *occ_size /*[3] host*/, const void *scratch, size_t scratch_bytes, float *vertices,
                            int32_t *faces, int32_t *cells, float *lattice, int V, int F, scanerf_stream_t stream);
/* Scene mesh: ONE mesh of a tiled scene -- the level set of the field the multi-tile renderer draws, the tiles'
 *   densities blended per point with scanerf_pts_inference's xz-distance weights, on one lattice over a world box.  The reference has
 *   no counterpart; the definition is this comment.  float32, every product and every sum separately rounded, integers where named.
 *   Lattice: the world box box_corner / box_size ([3] host each, box_size > 0) with n = (nx, ny, nz) cells; step_k = box_size_k /
 *     float(n_k) (one division, on the host); point (i,j,k) lies at wp_k = box_corner_k + float(i_k) * step_k; a vertex with the
 *     lattice coordinate L at box_corner + L * step, as in the dense op.
 *   Tiles: the renderer's arrays as scanerf_pts_normals takes them -- tables_f16 [nb,16,T,2], blobs [nb][SCANERF_PARAMSIZE] (flat
 *     decoder blobs), resolution [nb,16,3], occ / grid_starts / log2dim (the tiles' OWN occupancy grids, the ones
 *     scanerf_pts_inference tests, not the dilated sampling grid), corners / sizes [nb,3] (the render boxes); weight_feature == 1.
 *   Per point, the tiles b = 0 .. nb-1 in ascending index:
 *     pts = (wp - corner_b) / size_b;  the point LISTS b iff 0 <= pts_c <= 1 on all three axes.  There is no cap of four: a lattice
 *       point has no slot list, every tile that holds it counts (prepare_points keeps the first four; a point of six coincident
 *       tiles lists six here);
 *     dis = (0.5 - |pts - 0.5|) size_b;  w_b = xz_weight(dis.x, dis.z);  W += w_b whether or not the cell is occupied;
 *     b CONTRIBUTES iff its occupancy cell (scanerf_pts_inference's loc = clamp(int(pts 2^log2dim_b)) and cell offset) is set; then
 *       sigma_b = the density at the contracted coordinate x_c = 2 pts_c - 1 -- the bits scanerf_sigma_normals_points returns for
 *       that x with tile b's table, blob and resolutions (the per-tile extraction's coordinate, not scanerf_pts_inference's
 *       p01 = pts / 2 + 0.25 locator: the two differ by one rounding at cell borders) -- and num += w_b sigma_b.
 *   Field: v = num * (W > 0 ? 1 / W : 1); 0 where no tile is listed or none contributes.  Inside: v > level, level > 0.
 *     Classification, vertices, quads, winding, output order and the two passes are those above, unchanged; the surface is open only
 *     at the faces of the world box.  The DENSITY blend is the small-step limit of the renderer's blend of the opacities
 *     1 - exp(-sigma_b delta) (as delta -> 0 it is delta sum_b w_b sigma_b / W): the level set is that of the density the rendered
 *     images integrate, with their seam behaviour.
 *   A point's sums are ordered by tile index alone: its bits do not depend on the brick that evaluates it nor on the launch.
 *   scratch: scanerf_isosurface_scratch_bytes(nx,ny,nz), unchanged.  Any nb >= 1.  Refused before any launch: null pointers, nb < 1,
 *     T not a power of two, box_size <= 0 or not finite, level <= 0, a lattice or scratch the dense op refuses. */
int scanerf_isosurface_count_tiles(const void *tables_f16, const float *blobs, const int32_t *resolution, const uint8_t *occ,
                                   const int64_t *grid_starts, const int32_t *log2dim, const float *corners, const float *sizes, int T,
                                   int nb, const float *box_corner /*[3] host*/, const float *box_size /*[3] host*/, int nx, int ny,
                                   int nz, float level, void *scratch, size_t scratch_bytes, scanerf_stream_t stream);
int scanerf_isosurface_emit_tiles(const void *tables_f16, const float *blobs, const int32_t *resolution, const uint8_t *occ,
                                  const int64_t *grid_starts, const int32_t *log2dim, const float *corners, const float *sizes, int T,
                                  int nb, const float *box_corner /*[3] host*/, const float *box_size /*[3] host*/, int nx, int ny,
                                  int nz, float level, const void *scratch, size_t scratch_bytes, float *vertices, int32_t *faces,
                                  int32_t *cells, float *lattice, int V, int F, scanerf_stream_t stream);
/* Blended density, its gradient and the normal at world points: the field of the scene mesh above and the gradient of
 *   exactly that function, weight terms included, at points [N,3] f32 (device, world units, any order) -- the scene mesh's vertices,
 *   for one.  The reference has no counterpart; the definition is this comment.  The tile arrays are those of
 *   scanerf_isosurface_count_tiles.  float32; every product and every sum below is separately rounded; the per-tile density terms
 *   carry the bits of scanerf_sigma_normals_points; tiles in ascending index, so a point's bits depend on its own position alone --
 *   not on its neighbours in the launch, on N or on the launch.
 *   Per point p and tile b (the expressions of the scene mesh):
 *     pt = (p - corner_b) / size_b;  the point LISTS b iff 0 <= pt_c <= 1 on all three axes (no cap of four);
 *     dis_c = (0.5 - |pt_c - 0.5|) size_b,c;  w_b = xz_weight(dis_x, dis_z);  W += w_b, whether or not the cell is occupied;
 *     the weight's gradient in world units: s_c = +1 if pt_c < 0.5, -1 if pt_c > 0.5, 0 if equal, and by the branch xz_weight takes
 *       gw_b = (s_x dis_z, 0, s_z dis_x) if dis_x != 0 and dis_z != 0;  (s_x, 0, 0) if only dis_x != 0;  (0, 0, s_z) if only
 *       dis_z != 0;  0 otherwise;  C += gw_b (every listed tile);
 *     b CONTRIBUTES iff it is listed and its occupancy cell (clamp(int(pt 2^log2dim_b))) is set; then sigma_b, gsigma_b = what
 *       scanerf_sigma_normals_points returns as sigma and grad at x_c = 2 pt_c - 1 with tile b's table, blob and resolutions,
 *       weight_feature == 1 and axis_scale_c = 2.0f / size_b,c;  num += w_b sigma_b;  A_k += w_b gsigma_b,k;  B_k += sigma_b gw_b,k.
 *   After the last tile, inv = (W > 0 ? 1 / W : 1):
 *     sigma = v = num inv;   grad_k = ((A_k + B_k) - v C_k) inv;   normal = grad * (-1 / (sqrt((g_x^2 + g_y^2) + g_z^2) + 1e-8)).
 *   A point that no tile contributes to gets +0.0 in all seven outputs; every element of sigma [N], grad [N,3] (may be null: not
 *   written) and normal [N,3] is written.  v has the bits of the scene mesh's field at that point.  The branch changes of xz_weight
 *   and its kink at pt = 0.5 are discontinuities of the renderer's own weight: kept as they are.  This is NOT scanerf_pts_normals'
 *   quantity: that op blends the tiles' UNIT normals by opacity per sample; this is the gradient of the blended density itself.
 *   Any nb >= 1.  Refused before any launch: null pointers (but grad), N < 0, nb < 1, T not a power of two >= 2.  N == 0: no launch. */
int scanerf_scene_sigma_normals_points(const float *points, const void *tables_f16, const float *blobs, const int32_t *resolution,
                                       const uint8_t *occ, const int64_t *grid_starts, const int32_t *log2dim, const float *corners,
                                       const float *sizes, int T, int nb, float *sigma, float *grad, float *normal, int N,
                                       scanerf_stream_t stream);

/* ---- connected components of a mesh and the filter by component (csrc/mesh_components.hip).  The reference has no
 *   counterpart; the definition is this comment.  Every quantity is an integer: every result is exact and reproducible bit for bit.
 *   Inputs: V vertices, faces [F,3] i32 with every index in [0, V) (the caller's duty; the Python layer checks it; a face that breaks it
 *     is never dereferenced: it joins nothing, counts for nothing and is not kept), optionally cells [V,3] i32 (Mesh.cells).
 *   Graph: the vertices are the nodes, a face joins its three vertices.  Degenerate faces (two equal indices) and duplicate faces are
 *     legal and join what they name.
 *   Label: labels[v] = the smallest vertex index of v's connected component.  It depends on the graph alone -- not on the order of the
 *     faces or of a face's corners, the launch geometry or timing.  A vertex that no face uses is its own component.
 *   Table, one row per component, the rows in ascending label order as this library writes them: label; n_vertices; n_faces, a face
 *     belonging to the component of its FIRST index; with cells, cell_min [3] / cell_max [3] over the component's vertices, and
 *     extent = max over the axes of (cell_max - cell_min + 1).  Without cells extent counts as 0.
 *     RANK: the row number after ordering the rows by n_faces descending, ties by label ascending (meshing.mesh_components returns the
 *     table in that order; the sort is the caller's, one key per row).
 *   Keep rule, the three conditions joined: a component is kept iff n_faces >= min_faces and extent >= min_extent and (keep_largest
 *     is None or rank < keep_largest).  Defaults 0, 0, None: everything is kept and the result is the input bit for bit.  min_faces = 1
 *     alone removes exactly the vertices no face uses.  min_extent > 0 without cells is refused.  The caller forms keep [C] u8 (by
 *     row, in the library's ascending-label row order) from the table.
 *   Filtered mesh: the kept vertices in their original relative order; the kept faces (a face is kept with the component of its first
 *     index, which is the component of all three) in their original relative order with their indices remapped; the per-vertex arrays
 *     gathered row for row; winding untouched.
 *   Calls, all on caller-owned memory and the caller's stream:
 *     scanerf_mesh_components_scratch_bytes(V, F): the scratch (16-byte aligned) all four calls below share: a 64-byte header, two
 *       [V] i32 arrays (the row of every root; the new index of every vertex) and one i32 per 256 vertices and per 256 faces.
 *       0 with scanerf_last_error set for sizes that are refused: V < 1, F < 0, V or 3 F within 256 of 2^31.
 *     scanerf_mesh_components_label: labels [V] i32 (every element written), and in the scratch the roots counted and numbered in
 *       ascending order; the header's first int64 is then C, the number of components: the caller reads it and allocates the table.
 *     scanerf_mesh_components_table: the C rows (label, n_vertices, n_faces [C] i32; cell_min, cell_max [C,3] i32, with cells: all
 *       three or none), exactly C rows written, with `labels` and the scratch as scanerf_mesh_components_label left them.  The sums
 *       are integer atomics aggregated per wave and per workgroup first: order-independent.
 *     scanerf_mesh_filter_count: keep [C] u8 -> the header's second and third int64 are V' and F', the kept vertices and faces; the
 *       caller reads them and allocates.
 *     scanerf_mesh_filter_emit: gathers vertices / cells / lattice / normals [V,3] (each may be NULL with its output: skipped) into
 *       out_* [V',3] and writes out_faces [F',3]; exactly V' and F' rows.  The call reads (V', F') back from the header (one 16-byte
 *       read that waits for the stream) and REFUSES, writing nothing, when Vout != V' or Fout != F'.
 *   Refused before any launch: null pointers, sizes scanerf_mesh_components_scratch_bytes refuses, a scratch that is missing, too
 *     small or not 16-byte aligned, C outside [1, V], negative Vout / Fout.  V == 0 has no call (meshing returns empty results). */
size_t scanerf_mesh_components_scratch_bytes(int V, int F);
int scanerf_mesh_components_label(const int32_t *faces, int V, int F, int32_t *labels, void *scratch, size_t scratch_bytes,
                                  scanerf_stream_t stream);
int scanerf_mesh_components_table(const int32_t *faces, const int32_t *cells, const int32_t *labels, int V, int F, const void *scratch,
                                  size_t scratch_bytes, int C, int32_t *label, int32_t *n_vertices, int32_t *n_faces, int32_t *cell_min,
                                  int32_t *cell_max, scanerf_stream_t stream);
int scanerf_mesh_filter_count(const int32_t *faces, const int32_t *labels, const uint8_t *keep, int V, int F, int C, void *scratch,
                              size_t scratch_bytes, scanerf_stream_t stream);
int scanerf_mesh_filter_emit(const int32_t *faces, const int32_t *labels, const uint8_t *keep, int V, int F, int C, void *scratch,
                             size_t scratch_bytes, const float *vertices, const int32_t *cells, const float *lattice,
                             const float *normals, float *out_vertices, int32_t *out_faces, int32_t *out_cells, float *out_lattice,
                             float *out_normals, int Vout, int Fout, scanerf_stream_t stream);

/* ---- closest point of a triangle mesh (csrc/mesh_distance.hip): the query behind the geometric evaluation of an
 *   extracted mesh against a scan.  The reference has no counterpart; the definition is this comment.
 *   Inputs: points [N,3] f32; the tracer's arrays exactly as scanerf_mesh_first_hit takes them (tris != NULL: pre-gathered triangles,
 *     else vertices / faces; cell_faces always: it names the faces) plus cell_box; log2dim 4..7; max_dist >= 0 (f32, +inf = no cut).
 *   Outputs: dist2 [N] f32, face [N] i32, closest [N,3] f32 (may be NULL: not written).
 *   Per face f = (A, B, C) and point p: q_f(p) = the closest point of the closed triangle, by Voronoi regions in this order -- the vertex
 *     regions A, B, C, then the edge regions AB, AC, BC, then the interior -- computed in float32 from (A, B - A, C - A), the operands
 *     `tris` stores, without FMA contraction; d2_f(p) = |p - q_f(p)|^2.  ONE device function computes both for every route below, so
 *     a (p, f) pair gives the same bits pre-gathered or indexed, through the grid or by brute force.
 *   A face is DEAD and never answers when n . n == 0 in float32, n = (B - A) x (C - A).  Faces the build does not register (a vertex
 *     index outside [0, V); a box wholly outside the grid cube, which rounding can do to a face lying in the cube's far side) do not
 *     answer either.
 *   dist2[i] = min over the live faces of d2_f; face[i] = the LOWEST face index attaining that float32 minimum (ties are common: shared
 *     edges and vertices); closest[i] = q of that face.  Where the minimum is > max_dist^2 (float32 product) or not finite, or no live
 *     face exists, or a coordinate of p is not finite: dist2 = +inf, face = -1, closest = p (for a non-finite p no search runs).
 *     Coordinates whose squares overflow float32 are outside the definition (the call still ends and writes every element).
 *   The search is exact: Chebyshev shells of cells around the cell of p (clamped into the grid: points outside the cube are valid),
 *     candidates compared as (d2, face), stopped by a bound on every face not yet seen, taken with a margin of 2^-18 (grid side + max
 *     |corner| + max |p|) for the float32 truncation of the build and of d2 itself (the argument: csrc/mesh_distance.hip).  The result does
 *     not depend on log2dim, the visiting order or the launch geometry.
 *   N == 0 launches nothing.  Every output element is written exactly once, nothing else is written.  Refused before any launch
 *     (nothing written): N < 0, log2dim outside 4..7, max_dist negative or NaN, null pointers.  No environment variable is read.
 *   scanerf_mesh_closest_point_brute: the same outputs from the same device function over every face 0..F-1, no grid (scene_info and
 *     log2dim only decide which faces the build registers); F == 0 is legal (nothing found).  The witness of the grid route.
 *   scanerf_mesh_closest_point_counted (measurement; optional): also counters [N,2] i32 = (occupied cells looked at, face tests). */
int scanerf_mesh_closest_point(const float *points, int N, const float *vertices, const int32_t *faces, const float *tris,
                               const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num, const int32_t *cell_faces,
                               const float *cell_box, const float *scene_info, int log2dim, float max_dist, float *dist2, int32_t *face,
                               float *closest, scanerf_stream_t stream);
int scanerf_mesh_closest_point_counted(const float *points, int N, const float *vertices, const int32_t *faces, const float *tris,
                                       const uint64_t *bitmask, const uint32_t *rank, const int32_t *start_num,
                                       const int32_t *cell_faces, const float *cell_box, const float *scene_info, int log2dim,
                                       float max_dist, float *dist2, int32_t *face, float *closest, int32_t *counters,
                                       scanerf_stream_t stream);
int scanerf_mesh_closest_point_brute(const float *points, int N, const float *vertices, const int32_t *faces, int V, int F,
                                     const float *scene_info, int log2dim, float max_dist, float *dist2, int32_t *face, float *closest,
                                     scanerf_stream_t stream);

#define SCANERF_RAY_OUT 16

#ifdef __cplusplus
}
#endif
#endif /* SCANERF_HIP_H_ */
