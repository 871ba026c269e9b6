"""Fused fast path: one launch per HashGrid.render_batch_rays (hashgrid/__init__.py:512-596)."""
import contextlib
import ctypes

import torch

from . import _capi
from ._capi import RAY_OUT, RenderCfg, check, dev_ptr, feat_dtype_code, lib, stream
from .network import sh3

_f32 = torch.float32
FORE, BG = 0, 1

# Decoder arithmetic of the fused kernels (module-level switch: set_arith(); it becomes scanerf_render_cfg.arith of every call):
#   "f32"  = the f32-input MFMA (exact f32);
#   "h3"   = f16 matrix cores on hi/lo-split operands, three products per term, f32 accumulate: results as close to fp64 as
#            the f32 evaluation (csrc/render_h3.h), forward and backward (32-sample tiles, one wave per SIMD);
#   "t16s" = (default) forward as "h3"; backward on 16-sample tiles at two waves per SIMD with EVERY product split like h3's
#            (csrc/render_t16.h): f32-equivalent gradients (4e-6 relative L2 against the oracle) at 5.5 instead of 6.2 ms;
#   "t16"  = the same backward with the gradient products on ONE f16 MFMA per term and 8-byte table-gradient records
#            (7e-4 relative L2): the fast, reduced-precision option (3.9 ms); converges like the others on the procedural
#            scene (tests/test_gpu_harness.py: 27.1 dB each) but is not what the reference computes.
#   Calls the 16-sample-tile kernels cannot serve (no x-stash) run the "h3" backward: see backward_arith().
_ARITH_CODES = {"f32": _capi.ARITH_F32, "h3": _capi.ARITH_H3, "t16": _capi.ARITH_T16, "t16s": _capi.ARITH_T16S}
ARITH_NAMES = tuple(_ARITH_CODES)
FP32_EQUIV_ARITH = "t16s"   # the fastest arithmetic whose gradients are f32-equivalent: what bench.py's headline runs
DEFAULT_ARITH = FP32_EQUIV_ARITH
ARITH = _ARITH_CODES[DEFAULT_ARITH]
# what each arithmetic computes in, for bench.py's `dtype`
ARITH_DTYPE = {
    "f32": "f32 throughout (f32-input MFMA; f32 table-gradient records summed in 64-bit fixed point)",
    "h3": "f32 tables / compositing / accumulate; every decoder product (forward, gradient chains, weight gradients) on f16 MFMA "
          "with hi+lo split operands (22-bit), three products per term, f32 accumulate; f32 table-gradient records summed in "
          "64-bit fixed point",
    "t16s": "f32 tables / compositing / accumulate; every decoder product (forward, gradient chains, weight gradients) on f16 MFMA "
            "with hi+lo split operands (22-bit), three products per term, f32 accumulate; G' in f32; f32 table-gradient records "
            "summed in 64-bit fixed point",
    "t16": "f32 tables / compositing; forward + backward recompute split-f16 x3 MFMA (22-bit operands); gradient products ONE f16 "
           "MFMA per term (11-bit operands); 13-bit table-gradient records summed in 64-bit fixed point -- REDUCED precision",
}


def set_arith(name):
    global ARITH
    ARITH = _ARITH_CODES[name]


def arith_name():
    return next(k for k, v in _ARITH_CODES.items() if v == ARITH)


def backward_arith(have_xstash=True, pose_grads=False):
    """The arithmetic code one training step's scatter_plan / render_backward / scatter_accumulate must agree on
    (t16 needs the forward's x-stash; it produces the pose-gradient sums as well)."""
    if ARITH in _capi.T16_FAMILY and not have_xstash:
        return _capi.ARITH_H3
    return ARITH


def compact_record_format(arith_code):
    """`compact_records` of scatter_table_grad_adam for feature gradients out of a backward run under `arith_code`:
    8-byte records behind t16 (its gradients are f16 products anyway), 12-byte ones behind t16s (f32-grade), else the
    16-byte ones."""
    return {_capi.ARITH_T16: 1, _capi.ARITH_T16S: 2}.get(arith_code, 0)


def tile_T_columns(S):
    """Columns of the forward's tile_T output: transmittance entering each 16-sample tile."""
    return (S + 15) // 16


# columns of out_ray [B,16]
RGB, DEPTH, T_LEFT, DIFFUSE, SPECULAR, TINT, W_SPEC2 = slice(0, 3), 3, 4, slice(5, 8), slice(8, 11), slice(11, 14), 14


class PackedDecoder:
    """Device workspace holding the decoder in the layout the fused kernels stage into LDS.
    Re-pack after every optimiser step on the decoder or when weight_feature changes."""

    def __init__(self, device):
        self.workspace = torch.empty(lib().scanerf_render_workspace_floats(), dtype=_f32, device=device)

    skip_levels = 0

    def pack(self, blob, weight_feature, skip_levels=0):
        """skip_levels: bit l = weight_feature is exactly zero on level l (network.skip_levels): render_forward then leaves
        that level's table alone."""
        if blob.numel() != _capi.PARAMSIZE or weight_feature.numel() != 32:
            raise RuntimeError(f"scanerf: blob must hold {_capi.PARAMSIZE} floats and weight_feature 32")
        self.skip_levels = int(skip_levels)
        check(lib().scanerf_pack_decoder(dev_ptr(blob, _f32, "mlp_blob"), dev_ptr(weight_feature, _f32, "weight_feature"),
                                         dev_ptr(self.workspace, _f32, "workspace"), stream()), "pack_decoder")
        return self


def _cfg(min_bbox, bbox_size, contract_mode, infinity, arith=None, skip_levels=0):
    c = RenderCfg()
    c.contract_mode, c.infinity = int(contract_mode), int(bool(infinity))
    c.arith = ARITH if arith is None else arith
    c.skip_levels = int(skip_levels)
    for k in range(3):
        c.min_bbox[k] = float(min_bbox[k])
        c.bbox_size[k] = float(bbox_size[k])
    return c


JSTASH_DTYPE = torch.int32


def jstash_shape(B, S):
    """Shape of render_forward's jstash output: per ray, 32-sample tile, level of the half-wave (8), word (4), forward lane (64):
    the six position Jacobians d(feature)/d(p) of a (sample, level) as 20-bit significands under one exponent, 16 bytes
    (csrc/render_device.h jst_pack)."""
    return (B, (S + 31) // 32, 8, 4, 64)


def forward_plan_supported(B, S, T):
    """render_forward(plan=True) can do scatter_plan's work for the t16 backward of the same rays (equal kernel grids)."""
    return bool(lib().scanerf_render_forward_plan_supported(B, S, T))


def render_forward(rays_o, rays_d, z_vals, dists, features, resolutions, packed, min_bbox, bbox_size, contract_mode,
                   infinity, ray_valid=None, want_weights=True, out_ray=None, weights=None, tile_T=None, xstash=None,
                   plan=False, plan_workspace=None, jstash=None):
    """-> out_ray [B,16] (see column constants), weights [B,S] or None.
    min_bbox / bbox_size: host sequences of 3 floats (the HashGrid 2x box).
    plan=True (only where forward_plan_supported): the launch also reserves the t16 backward's scatter-record ranges for these
    rays -- call it INSTEAD of scatter_plan; returns (out_ray, weights, workspace).
    jstash (fp32 tables): jstash_shape(B, S) JSTASH_DTYPE (packed words) that receives the encoder's position Jacobians, for
    render_backward(ray_pos_grad=...) (pose refinement without a second pass over the table)."""
    B, S = z_vals.shape
    if features.shape[0] != 16 or features.shape[2] != 2:
        raise RuntimeError("scanerf: fused path needs a [16,T,2] table (the reference hard-codes 16 levels)")
    if out_ray is None:
        out_ray = torch.empty((B, RAY_OUT), dtype=_f32, device=z_vals.device)
    if weights is None and want_weights:
        weights = torch.empty((B, S), dtype=_f32, device=z_vals.device)
    T = features.shape[1]
    args = (dev_ptr(rays_o, _f32, "rays_o"), dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(z_vals, _f32, "z_vals"),
            dev_ptr(dists, _f32, "dists"), dev_ptr(features, (torch.float32, torch.float16, torch.bfloat16), "features"),
            feat_dtype_code(features), dev_ptr(resolutions, torch.int32, "resolutions"),
            dev_ptr(packed.workspace, _f32, "workspace"))
    tail = (dev_ptr(ray_valid, (torch.bool, torch.uint8), "ray_valid", allow_none=True), dev_ptr(out_ray, _f32, "out_ray"),
            dev_ptr(weights, _f32, "weights", allow_none=True), dev_ptr(tile_T, _f32, "tile_T", allow_none=True),
            dev_ptr(xstash, _f32, "xstash", allow_none=True), B, S, T)
    if plan or jstash is not None:
        ws = None
        if plan:
            need = lib().scanerf_render_scatter_workspace_bytes(B, S, T)
            if not need or not forward_plan_supported(B, S, T):
                raise RuntimeError(f"scanerf: render_forward(plan=True) does not support B={B} S={S} T={T}")
            ws = _capi.workspace(z_vals.device, need) if plan_workspace is None else plan_workspace
        cfg = _cfg(min_bbox, bbox_size, contract_mode, infinity, ARITH if ARITH in _capi.T16_FAMILY else _capi.ARITH_T16,
                   getattr(packed, "skip_levels", 0))
        tail = tail[:5] + (dev_ptr(jstash, JSTASH_DTYPE, "jstash", allow_none=True),) + tail[5:]
        check(lib().scanerf_render_forward_packed_plan(*args, ctypes.byref(cfg), *tail, ws.data_ptr() if ws is not None else None,
                                                       ws.numel() if ws is not None else 0, stream()),
              "render_forward(plan)")
        return (out_ray, weights, ws) if plan else (out_ray, weights)
    cfg = _cfg(min_bbox, bbox_size, contract_mode, infinity, skip_levels=getattr(packed, "skip_levels", 0))
    check(lib().scanerf_render_forward_packed(*args, ctypes.byref(cfg), *tail, stream()), "render_forward")
    return out_ray, weights


# ---- surface normals: the density's position gradient, fused (csrc/normals.hip) --------------------------------
_TABLE_DTYPES = (torch.float32, torch.float16)   # (exported tiles are f16; bf16 gather copies keep the op-by-op route)


def _normals_common(features, resolutions, blob, weight_feature):
    """The checks both forms share, before any launch -> (T, the five leading pointers' tail)."""
    if features.dim() != 3 or features.shape[0] != 16 or features.shape[2] != 2:
        raise RuntimeError("scanerf: the fused normals need a [16,T,2] table (the reference hard-codes 16 levels)")
    T = int(features.shape[1])
    if T < 2 or T & (T - 1):
        raise RuntimeError(f"scanerf: the table size T={T} must be a power of two")
    if blob.numel() != _capi.PARAMSIZE or weight_feature.numel() != 32:
        raise RuntimeError(f"scanerf: blob must hold {_capi.PARAMSIZE} floats and weight_feature 32")
    if tuple(resolutions.shape) != (16, 3):
        raise RuntimeError(f"scanerf: resolutions must be [16,3], got {tuple(resolutions.shape)}")
    return T, (dev_ptr(features, _TABLE_DTYPES, "features"), feat_dtype_code(features), dev_ptr(resolutions, torch.int32, "resolutions"),
               dev_ptr(blob, _f32, "mlp_blob"), dev_ptr(weight_feature, _f32, "weight_feature"))


def _host3(v, name):
    v = [float(x) for x in v]
    if len(v) != 3:
        raise RuntimeError(f"scanerf: {name} must hold 3 floats")
    return (ctypes.c_float * 3)(*v)


def sigma_normals_points(points, features, resolutions, blob, weight_feature, axis_scale=(1.0, 1.0, 1.0), want_grad=False):
    """Density, its position gradient and the surface normal at contracted points [N,3] in [-2,2]^3 (hashgrid/__init__.py:374-392
    compute_normal, in closed form): -> sigma [N], grad [N,3] or None (d sigma / d p, with d x_k / d p_k = axis_scale[k]),
    normal [N,3] = -grad / (|grad| + 1e-8).  blob: the flat decoder blob; weight_feature [32]."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"scanerf: points must be [N,3], got {tuple(points.shape)}")
    T, mid = _normals_common(features, resolutions, blob, weight_feature)
    N = int(points.shape[0])
    p = dev_ptr(points, _f32, "points")
    sigma = torch.empty((N,), dtype=_f32, device=points.device)
    normal = torch.empty((N, 3), dtype=_f32, device=points.device)
    grad = torch.empty((N, 3), dtype=_f32, device=points.device) if want_grad else None
    check(lib().scanerf_sigma_normals_points(p, _host3(axis_scale, "axis_scale"), *mid, dev_ptr(sigma, _f32, "sigma"),
                                             dev_ptr(grad, _f32, "grad", allow_none=True), dev_ptr(normal, _f32, "normal"), N, T,
                                             stream()), "sigma_normals_points")
    return sigma, grad, normal


def render_normals(rays_o, rays_d, z_vals, dists, features, resolutions, blob, weight_feature, min_bbox, bbox_size, infinity=False,
                   ray_valid=None, want_sample_normals=False):
    """Normals composited along rays (hashgrid/__init__.py:576-588 / tile.py:695-712 as one launch): samples o + z d in
    contract_fore of the box -> out [B,4] = (sum_i w_i n_i, sum_i w_i) and, on request, the per-sample normals [B,S,3].
    Rays with ray_valid == 0 give zeros.  min_bbox / bbox_size: host sequences of 3 floats (the HashGrid 2x box)."""
    if z_vals.dim() != 2:
        raise RuntimeError(f"scanerf: z_vals must be [B,S], got {tuple(z_vals.shape)}")
    B, S = (int(v) for v in z_vals.shape)
    if S < 1:
        raise RuntimeError(f"scanerf: render_normals needs S >= 1, got S={S}")
    for t, name, shape in ((rays_o, "rays_o", (B, 3)), (rays_d, "rays_d", (B, 3)), (dists, "dists", (B, S))):
        if tuple(t.shape) != shape:
            raise RuntimeError(f"scanerf: {name} must be {list(shape)}, got {list(t.shape)}")
    if ray_valid is not None and tuple(ray_valid.shape) != (B,):
        raise RuntimeError(f"scanerf: ray_valid must be [{B}], got {list(ray_valid.shape)}")
    T, mid = _normals_common(features, resolutions, blob, weight_feature)
    head = (dev_ptr(rays_o, _f32, "rays_o"), dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(z_vals, _f32, "z_vals"), dev_ptr(dists, _f32, "dists"))
    valid = dev_ptr(ray_valid, (torch.bool, torch.uint8), "ray_valid", allow_none=True)
    out = torch.empty((B, 4), dtype=_f32, device=z_vals.device)
    sn = torch.empty((B, S, 3), dtype=_f32, device=z_vals.device) if want_sample_normals else None
    check(lib().scanerf_render_normals(*head, *mid, _host3(min_bbox, "min_bbox"), _host3(bbox_size, "bbox_size"), int(bool(infinity)),
                                       valid, dev_ptr(out, _f32, "out"), dev_ptr(sn, _f32, "sample_normals", allow_none=True), B, S, T,
                                       stream()), "render_normals")
    return out, sn


_KEEP_DW_PARTIAL = None


def render_backward(rays_o, rays_d, z_vals, dists, features, resolutions, packed, weight_feature, min_bbox, bbox_size,
                    contract_mode, infinity, out_ray, tile_T, grad_out, ray_valid=None, grad_blob=None, xstash=None,
                    ray_grad_buffers=None, scatter=None, want_dfeat=True, arith=None, jstash=None, ray_pos_grad=None):
    """Adjoint of render_forward -> (dfeat [16, B*S, 2] level-major, grad_blob [13994]).
    scatter = (workspace, grad_features) from scatter_plan(): the kernel emits the table-gradient records
    itself; finish with scatter_accumulate().  dfeat is then only produced if want_dfeat.
    arith: as given to scatter_plan (default: backward_arith() of this call's inputs).
    jstash + ray_pos_grad ([B,6] zeros; t16 kernel, with ray_grad_buffers): the kernel also writes dL/d(rays_o), dL/d(rays_d)
    through the sample positions, from the forward's position Jacobians (see ray_gradients_fused)."""
    B, S = z_vals.shape
    dev = z_vals.device
    if arith is None:
        arith = backward_arith(xstash is not None, ray_grad_buffers is not None)
    if scatter is None and not want_dfeat:
        raise ValueError("render_backward: nothing would receive the feature gradients")
    dfeat = torch.empty((16, B * S, 2), dtype=_f32, device=dev) if want_dfeat else None
    nblk = lib().scanerf_render_backward_grid(B)
    dw_partial = torch.empty((4 * nblk, _capi.PARAMSIZE), dtype=_f32, device=dev)
    if _KEEP_DW_PARTIAL is not None:   # investigation hook (tools/bwd_stamps.py: the -DT16_STAMPS build parks its cycle sums there)
        _KEEP_DW_PARTIAL[:] = [dw_partial, nblk]
    if grad_blob is None:
        grad_blob = torch.zeros(_capi.PARAMSIZE, dtype=_f32, device=dev)
    cfg = _cfg(min_bbox, bbox_size, contract_mode, infinity, arith)
    check(lib().scanerf_render_backward(
        dev_ptr(rays_o, _f32, "rays_o"), dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(z_vals, _f32, "z_vals"),
        dev_ptr(dists, _f32, "dists"), dev_ptr(features, (torch.float32, torch.float16, torch.bfloat16), "features"),
        feat_dtype_code(features), dev_ptr(resolutions, torch.int32, "resolutions"),
        dev_ptr(packed.workspace, _f32, "workspace"), dev_ptr(weight_feature, _f32, "weight_feature"),
        ctypes.byref(cfg), dev_ptr(ray_valid, (torch.bool, torch.uint8), "ray_valid", allow_none=True),
        dev_ptr(out_ray, _f32, "out_ray"), dev_ptr(tile_T, _f32, "tile_T"), dev_ptr(grad_out, _f32, "grad_out"),
        dev_ptr(xstash, _f32, "xstash", allow_none=True), dev_ptr(dfeat, _f32, "dfeat", allow_none=True), dev_ptr(dw_partial, _f32, "dw_partial"), dev_ptr(grad_blob, _f32, "grad_blob"),
        dev_ptr(ray_grad_buffers[0] if ray_grad_buffers else None, _f32, "g_dnorm", allow_none=True),
        dev_ptr(ray_grad_buffers[1] if ray_grad_buffers else None, _f32, "g_rowsum", allow_none=True),
        dev_ptr(jstash, JSTASH_DTYPE, "jstash", allow_none=True), dev_ptr(ray_pos_grad, _f32, "ray_pos_grad", allow_none=True),
        scatter[0].data_ptr() if scatter else None, scatter[0].numel() if scatter else 0,
        dev_ptr(scatter[1] if scatter else None, _f32, "grad_features", allow_none=True),
        B, S, features.shape[1], stream()), "render_backward")
    return dfeat, grad_blob


def photometric_loss_grad(out_ray, target, ray_valid=None, reg_weight=0.01, grad_out=None):
    """MSE over the valid rays' rgb + reg_weight * l2_reg_specular (criterions.py:142-144, tile.py:999) and its gradient
    w.r.t. out_ray, without a torch graph -> (loss [1] device tensor, grad_out [B,16])."""
    B = out_ray.shape[0]
    dev = out_ray.device
    if grad_out is None:
        grad_out = torch.empty((B, RAY_OUT), dtype=_f32, device=dev)
    loss = torch.empty(1, dtype=_f32, device=dev)
    scratch = torch.empty(lib().scanerf_photometric_loss_scratch_floats(), dtype=_f32, device=dev)
    check(lib().scanerf_photometric_loss_grad(
        dev_ptr(out_ray, _f32, "out_ray"), dev_ptr(target, _f32, "target"),
        dev_ptr(ray_valid, (torch.bool, torch.uint8), "ray_valid", allow_none=True), reg_weight,
        dev_ptr(grad_out, _f32, "grad_out"), dev_ptr(loss, _f32, "loss"), dev_ptr(scratch, _f32, "scratch"), B,
        stream()), "photometric_loss_grad")
    return loss, grad_out


def photometric_loss_grad_fgbg(out_fg, out_bg, target, valid_fg=None, valid_bg=None, reg_weight=0.01):
    """Loss of the complete per-tile render (tile.py:666-690: pred = fg.rgb + fg.T_left * bg.rgb; MSE over the rays valid in either branch, criterions.py:121-138, +
    reg_weight * both branches' l2_reg_specular, tile.py:999) and its gradients w.r.t. the two branches' out_ray, without a
    torch graph -> (loss [1], grad_fg [B,16], grad_bg [B,16])."""
    B = out_fg.shape[0]
    dev = out_fg.device
    gfg, gbg = torch.empty((B, RAY_OUT), dtype=_f32, device=dev), torch.empty((B, RAY_OUT), dtype=_f32, device=dev)
    loss = torch.empty(1, dtype=_f32, device=dev)
    scratch = torch.empty(lib().scanerf_photometric_loss_scratch_floats(), dtype=_f32, device=dev)
    vt = (torch.bool, torch.uint8)
    check(lib().scanerf_photometric_loss_grad_fgbg(
        dev_ptr(out_fg, _f32, "out_fg"), dev_ptr(out_bg, _f32, "out_bg"), dev_ptr(target, _f32, "target"),
        dev_ptr(valid_fg, vt, "valid_fg", allow_none=True), dev_ptr(valid_bg, vt, "valid_bg", allow_none=True),
        reg_weight, dev_ptr(gfg, _f32, "grad_fg"), dev_ptr(gbg, _f32, "grad_bg"), dev_ptr(loss, _f32, "loss"),
        dev_ptr(scratch, _f32, "scratch"), B, stream()), "photometric_loss_grad_fgbg")
    return loss, gfg, gbg


def scatter_accumulate_adam2(ws1, S1, ws2, S2, params, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, B, half_table=None,
                             overflow_grad=None, arith=None):
    """scatter_accumulate_adam over the record sets of TWO fused backward launches on the same rays and table (a tile's
    foreground and background branches): both gradients meet in one Adam step.  arith: as given to both scatter_plan calls."""
    check(lib().scanerf_render_scatter_accumulate_adam2(
        dev_ptr(params, _f32, "params"), dev_ptr(exp_avg, _f32, "exp_avg"), dev_ptr(exp_avg_sq, _f32, "exp_avg_sq"),
        dev_ptr(half_table, (torch.float16, torch.bfloat16), "half_table", allow_none=True),
        feat_dtype_code(half_table) if half_table is not None else 0,
        dev_ptr(overflow_grad, _f32, "overflow_grad", allow_none=True), lr, beta1, beta2, eps, step, B, params.shape[1], S1,
        ws1.data_ptr(), ws1.numel(), S2, ws2.data_ptr(), ws2.numel(), backward_arith() if arith is None else arith, stream()),
        "scatter_accumulate_adam2")


def ray_valid(z_vals):
    """[B] uint8: every sample of the ray's row != -1 (hashgrid/__init__.py:419 torch.all(z_vals != -1, dim=-1))."""
    B, S = z_vals.shape
    n = (B + 15) // 16 * 16  # scanerf_compact_rays reads the flags 16 bytes at a time
    buf = torch.zeros(n, dtype=torch.uint8, device=z_vals.device)
    check(lib().scanerf_ray_valid(dev_ptr(z_vals, _f32, "z_vals"), dev_ptr(buf, torch.uint8, "valid"), B,
                                  S, stream()), "ray_valid")
    return buf[:B]


def compact_rays(valid, rays_o, rays_d, target, z_vals, dists, want_index=False):
    """Order-preserving compaction of the valid rays (hashgrid/__init__.py:419-434) in one launch (wave ballot / popcount
    prefix sums): -> (count, rays_o, rays_d, target, z_vals, dists[, index]) with the valid rays' rows first; the returned
    tensors are views of length `count` (one host read of the count, as torch's boolean-mask indexing needs too).
    valid: from ray_valid()."""
    B, S = z_vals.shape
    dev = z_vals.device
    if valid.dtype not in (torch.uint8, torch.bool) or valid.data_ptr() % 16:
        raise RuntimeError("scanerf: compact_rays needs the 16-byte aligned uint8 flags ray_valid() returns")
    o, d = torch.empty_like(rays_o), torch.empty_like(rays_d)
    t = torch.empty_like(target) if target is not None else None
    z, di = torch.empty_like(z_vals), torch.empty_like(dists)
    idx = torch.empty(B, dtype=torch.int32, device=dev) if want_index else None
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().scanerf_compact_rays(
        dev_ptr(valid, (torch.uint8, torch.bool), "valid"), B, S, dev_ptr(rays_o, _f32, "rays_o"),
        dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(target, _f32, "target", allow_none=True), dev_ptr(z_vals, _f32, "z_vals"),
        dev_ptr(dists, _f32, "dists"), dev_ptr(o, _f32, "out_o"), dev_ptr(d, _f32, "out_d"), dev_ptr(t, _f32, "out_t", allow_none=True),
        dev_ptr(z, _f32, "out_z"), dev_ptr(di, _f32, "out_dist"), dev_ptr(idx, torch.int32, "out_index", allow_none=True),
        dev_ptr(count, torch.int32, "count"), stream()), "compact_rays")
    n = int(count.item())
    res = (n, o[:n], d[:n], t[:n] if t is not None else None, z[:n], di[:n])
    return res + (idx[:n],) if want_index else res


def scatter_supported(B, S, T):
    return lib().scanerf_render_scatter_workspace_bytes(B, S, T) != 0


def scatter_plan(rays_o, rays_d, z_vals, resolutions, T, min_bbox, bbox_size, contract_mode, infinity, ray_valid=None,
                 arith=None, workspace=None, skip_levels=0):
    """Reserve the record ranges of the fused table-gradient path for this batch (count + scan).
    Returns the workspace tensor to hand to render_backward(scatter=(ws, grad_features)) and scatter_accumulate.
    The workspace is a per-(device, stream) cache: one plan/backward/accumulate sequence at a time.
    arith: the backward kernel that will emit the records (its ray -> workgroup map is reserved here); default
    backward_arith() = what render_backward picks when it is given an x-stash and no pose-gradient buffers."""
    B, S = z_vals.shape
    need = lib().scanerf_render_scatter_workspace_bytes(B, S, T)
    if not need:
        raise RuntimeError(f"scanerf: fused scatter does not support B={B} S={S} T={T}")
    # (workspace: a caller-owned uint8 tensor instead of the cached one; smaller than `need` = overflow records take the
    # atomic path -- tests)
    ws = _capi.workspace(z_vals.device, need) if workspace is None else workspace
    # skip_levels (PackedDecoder.skip_levels): masked levels get no records; the plan notes it in the workspace for the backward
    cfg = _cfg(min_bbox, bbox_size, contract_mode, infinity, backward_arith() if arith is None else arith, skip_levels)
    check(lib().scanerf_render_scatter_plan(
        dev_ptr(rays_o, _f32, "rays_o"), dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(z_vals, _f32, "z_vals"),
        dev_ptr(resolutions, torch.int32, "resolutions"), ctypes.byref(cfg),
        dev_ptr(ray_valid, (torch.bool, torch.uint8), "ray_valid", allow_none=True), B, S,
        T, ws.data_ptr(), ws.numel(), stream()), "scatter_plan")
    return ws


def scatter_accumulate(ws, grad_features, B, S, arith=None):
    """grad_features [16,T,2] += the records the fused backward emitted into ws.
    arith: as given to scatter_plan (default: the same backward_arith()).  It picks the launch shape for the record format that
    plan chose and nothing else: the kernel reads the format from ws, so another value gives the same bits, possibly slower."""
    check(lib().scanerf_render_scatter_accumulate(
        dev_ptr(grad_features, _f32, "grad_features"), B, S, grad_features.shape[1], ws.data_ptr(), ws.numel(),
        backward_arith() if arith is None else arith, stream()), "scatter_accumulate")
    return grad_features


def scatter_accumulate_adam(ws, params, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, B, S, half_table=None,
                            overflow_grad=None, arith=None):
    """The records the fused backward emitted into ws applied straight to the table: accumulate + fused sparse Adam in one
    pass (no gradient table, no zero-fill, no scan of it).  `step` = the previous step count (cuda/adam_kernel.cu:83).
    half_table: optional f16 / bf16 gather copy of params, refreshed where params change; overflow_grad: the zero table
    handed to render_backward as grad_features (touched only if the record workspace overflows); arith: as scatter_accumulate's."""
    check(lib().scanerf_render_scatter_accumulate_adam(
        dev_ptr(params, _f32, "params"), dev_ptr(exp_avg, _f32, "exp_avg"), dev_ptr(exp_avg_sq, _f32, "exp_avg_sq"),
        dev_ptr(half_table, (torch.float16, torch.bfloat16), "half_table", allow_none=True),
        feat_dtype_code(half_table) if half_table is not None else 0,
        dev_ptr(overflow_grad, _f32, "overflow_grad", allow_none=True), lr, beta1, beta2, eps, step, B, S, params.shape[1],
        ws.data_ptr(), ws.numel(), backward_arith() if arith is None else arith, stream()),
        "scatter_accumulate_adam")


def scatter_table_grad(points, dfeat, grad_features, resolutions, compact_records=-1):
    """grad_features [16,T,2] += binned scatter of level-major dfeat at contracted `points` [N,3].
    compact_records: -1 = the layout's default (16-byte records for level-major gradients), 0 / 1 / 2 = 16- / 8- / 12-byte records."""
    N, (L, T) = points.shape[0], grad_features.shape[:2]
    need = lib().scanerf_embedding_bwd_workspace_bytes(N, L, T)
    if not need:
        raise RuntimeError("scanerf: shape not supported by the binned scatter")
    ws = _capi.workspace(points.device, need, "scatter")
    check(lib().scanerf_embedding_bg_backward_binned(
        dev_ptr(points, _f32, "points"), dev_ptr(dfeat, _f32, "dfeat"), dev_ptr(grad_features, _f32, "grad_features"),
        dev_ptr(resolutions, torch.int32, "resolutions"), N, L, T, 1, ws.data_ptr(), ws.numel(), int(compact_records), stream()),
        "scatter_table_grad")
    return grad_features


def scatter_table_grad_adam(points, dfeat, resolutions, params, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step,
                            half_table=None, overflow_grad=None, compact_records=0):
    """scatter_table_grad ending in the fused sparse Adam (no gradient table): the table path of tables too large for the
    backward kernel's own record emission.  overflow_grad: zero table like params (required by the C ABI).
    compact_records: 1 = 8-byte records (for dfeat out of the t16 backward; scatter_common.h Rec8), 2 = 12-byte records
    (f32-grade, behind the t16s backward; Rec12), 0 = 16-byte records."""
    N, (L, T) = points.shape[0], params.shape[:2]
    need = lib().scanerf_embedding_bwd_workspace_bytes(N, L, T)
    if not need:
        raise RuntimeError("scanerf: shape not supported by the binned scatter")
    ws = _capi.workspace(points.device, need, "scatter")
    check(lib().scanerf_embedding_bg_backward_binned_adam(
        dev_ptr(points, _f32, "points"), dev_ptr(dfeat, _f32, "dfeat"), dev_ptr(resolutions, torch.int32, "resolutions"), N, L, T,
        1, ws.data_ptr(), ws.numel(), dev_ptr(params, _f32, "params"), dev_ptr(exp_avg, _f32, "exp_avg"),
        dev_ptr(exp_avg_sq, _f32, "exp_avg_sq"),
        dev_ptr(half_table, (torch.float16, torch.bfloat16), "half_table", allow_none=True),
        feat_dtype_code(half_table) if half_table is not None else 0, dev_ptr(overflow_grad, _f32, "overflow_grad"), lr, beta1,
        beta2, eps, step, int(compact_records), stream()), "scatter_table_grad_adam")


def scatter_rays_supported(T, arith_code):
    """scatter_table_grad_adam_rays applies: tables of 2^22 to 2^24 entries per level behind the f32-grade backward (12-byte
    records).  Both bounds are csrc/scatter.hip binned_backward's seg_route, which the rays entry requires: one level's
    counters in the producer's LDS at a time (L * NB * 4 > 64 KiB), and NB <= 2048 buckets of 2^13 entries."""
    return (1 << 22) <= T <= (1 << 24) and compact_record_format(arith_code) == 2


def contracted_points(rays_o, rays_d, z_vals, min_bbox, bbox_size, contract_mode):
    """[B*S,3] hash-grid coordinates of the samples o + z d (device tensors min_bbox / bbox_size: the 2x box):
    (p - min) / size * 4 - 2, and for the background branch the L-inf fold p (2 - 1/|p|inf) / |p|inf (contract_bg)."""
    pts = ((rays_o[:, None, :] + z_vals[:, :, None] * rays_d[:, None, :]).reshape(-1, 3) - min_bbox) / bbox_size * 4.0 - 2.0
    if contract_mode == BG:
        linf = pts.abs().amax(-1, keepdim=True)
        pts = pts * ((2.0 - 1.0 / linf) / linf)
    return pts.contiguous()


def scatter_table_grad_adam_rays(rays_o, rays_d, branches, min_bbox, bbox_size, resolutions, params, exp_avg, exp_avg_sq, lr, beta1,
                                 beta2, eps, step, overflow_grad, half_table=None, fp16_moments=False):
    """The table gradient of one or two render branches over the same rays, scattered and applied by ONE sparse Adam step
    (scanerf_table_grad_scatter_adam_rays; tile.py:639-692, :1010).  branches: [(z [B,S], dfeat [16,B*S,2], ray_valid [B] or None,
    contract mode FORE / BG), ...] -- no contracted-point tensors, no concatenation.  overflow_grad: zero table like params.
    fp16_moments (opt-in): exp_avg / exp_avg_sq are float16 tensors, the update is adam_step_cuda_fp16's (cuda/adam_kernel.cu:98-144)."""
    mdt = torch.float16 if fp16_moments else _f32
    B, T = rays_o.shape[0], params.shape[1]
    if not 1 <= len(branches) <= 2 or params.shape[0] != 16:
        raise RuntimeError("scanerf: scatter_table_grad_adam_rays takes one or two branches and 16 levels")
    N = sum(B * z.shape[1] for z, _, _, _ in branches)
    need = lib().scanerf_embedding_bwd_workspace_bytes(N, 16, T)
    if not need:
        raise RuntimeError("scanerf: shape not supported by the binned scatter")
    ws = _capi.workspace(rays_o.device, need, "scatter")
    args = []
    for k in range(2):
        if k < len(branches):
            z, dfeat, valid, mode = branches[k]
            if tuple(dfeat.shape) != (16, B * z.shape[1], 2) or z.shape[0] != B:
                raise RuntimeError(f"scanerf: branch {k}: dfeat {tuple(dfeat.shape)} does not match z {tuple(z.shape)}")
            args += [dev_ptr(z, _f32, f"z{k}"), dev_ptr(dfeat, _f32, f"dfeat{k}"),
                     dev_ptr(valid, (torch.bool, torch.uint8), f"valid{k}", allow_none=True), z.shape[1], int(mode)]
        else:
            args += [None, None, None, 0, 0]
    mn, sz = (ctypes.c_float * 3)(*[float(v) for v in min_bbox]), (ctypes.c_float * 3)(*[float(v) for v in bbox_size])
    check(lib().scanerf_table_grad_scatter_adam_rays(
        dev_ptr(rays_o, _f32, "rays_o"), dev_ptr(rays_d, _f32, "rays_d"), B, *args, mn, sz,
        dev_ptr(resolutions, torch.int32, "resolutions"), T, ws.data_ptr(), ws.numel(), dev_ptr(params, _f32, "params"),
        dev_ptr(exp_avg, mdt, "exp_avg"), dev_ptr(exp_avg_sq, mdt, "exp_avg_sq"),
        dev_ptr(half_table, (torch.float16, torch.bfloat16), "half_table", allow_none=True),
        feat_dtype_code(half_table) if half_table is not None else 0, dev_ptr(overflow_grad, _f32, "overflow_grad"), lr, beta1,
        beta2, eps, step, 1 if fp16_moments else 0, stream()), "scatter_table_grad_adam_rays")


def ray_gradients_fused(rays_o, rays_d, blob, ray_pos_grad, g_dnorm, g_rowsum, ray_valid=None):
    """dL/d(rays_o), dL/d(rays_d) when the backward kernel produced the position path itself (render_backward(jstash=...,
    ray_pos_grad=...)): adds the two per-ray paths -- |d| through delta = dist * |d| and SH(d / |d|) of the decoder -- in one
    launch (scanerf_ray_grad_epilogue).  Same result as ray_gradients() / ray_gradients_fused_autograd()."""
    B = rays_d.shape[0]
    g_o, g_d = torch.empty_like(rays_o, dtype=_f32), torch.empty_like(rays_d, dtype=_f32)
    S = g_dnorm.shape[1] * 32
    check(lib().scanerf_ray_grad_epilogue(
        dev_ptr(rays_d, _f32, "rays_d"), dev_ptr(blob.detach(), _f32, "mlp_blob"), dev_ptr(ray_pos_grad, _f32, "ray_pos_grad"),
        dev_ptr(g_dnorm, _f32, "g_dnorm"), dev_ptr(g_rowsum, _f32, "g_rowsum"),
        dev_ptr(ray_valid, (torch.bool, torch.uint8), "ray_valid", allow_none=True), dev_ptr(g_o, _f32, "g_o"), dev_ptr(g_d, _f32, "g_d"),
        B, S, stream()), "ray_grad_epilogue")
    return g_o, g_d


def ray_gradients_fused_autograd(rays_o, rays_d, blob, ray_pos_grad, g_dnorm, g_rowsum, ray_valid=None):
    """ray_gradients_fused by torch autograd on [B]-sized tensors (what it was before the epilogue kernel: ~150 small launches);
    kept as the reference the tests compare the kernel with."""
    d = rays_d.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        dn = d.norm(2, dim=-1, keepdim=True)
        sh = sh3(d / (dn + 1e-8))
    w_sh = blob[6503 + 64 + 32 * 64: 6503 + 64 + 48 * 64].reshape(16, 64)  # Directional_MLP.mlp.0 weight^T rows 32..47
    g_sh = g_rowsum.sum(1) @ w_sh.t()
    g_dn = g_dnorm.sum(1, keepdim=True)
    g_o, g_dpos = ray_pos_grad[:, 0:3], ray_pos_grad[:, 3:6]
    if ray_valid is not None:
        keep = ray_valid[:, None].to(_f32)
        g_sh, g_dn, g_o, g_dpos = g_sh * keep, g_dn * keep, g_o * keep, g_dpos * keep
    torch.autograd.backward([sh, dn], [g_sh, g_dn])
    return g_o.contiguous(), d.grad + g_dpos


def ray_gradients(rays_o, rays_d, z_vals, features, resolutions, blob, min_bbox, bbox_size, contract_mode, dfeat,
                  g_dnorm, g_rowsum, ray_valid=None):
    """dL/d(rays_o), dL/d(rays_d) of a fused render (for pose refinement: tile.py trains se3_refine through
    the rays).  Three paths: the sample positions (hash-encoder point gradient kernel on dfeat, then the
    contraction's Jacobian by torch autograd), |d| through delta = dist*|d|, and SH(d/|d|) of the decoder."""
    B, S = z_vals.shape
    dev = z_vals.device
    mn = torch.as_tensor(min_bbox, dtype=_f32, device=dev)
    sz = torch.as_tensor(bbox_size, dtype=_f32, device=dev)
    o = rays_o.detach().clone().requires_grad_(True)
    d = rays_d.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        x = ((o[:, None, :] + z_vals[..., None] * d[:, None, :]).reshape(-1, 3) - mn) / sz * 4.0 - 2.0
        if contract_mode == BG:
            linf = torch.max(torch.abs(x), dim=-1, keepdim=True)[0]
            x = x * ((2 - 1.0 / linf) / linf)
        dn = d.norm(2, dim=-1, keepdim=True)
        sh = sh3(d / (dn + 1e-8))
    gp = torch.zeros(B * S, 3, dtype=_f32, device=dev)
    xd = x.detach().contiguous()
    check(lib().scanerf_embedding_bg_point_grad(dev_ptr(xd, _f32, "points"), dev_ptr(dfeat, _f32, "dfeat"),
                                                dev_ptr(gp, _f32, "grad_points"), dev_ptr(features, _f32, "features"),
                                                dev_ptr(resolutions, torch.int32, "resolutions"), B * S,
                                                16, features.shape[1], stream()),
          "embedding_bg_point_grad")
    w_sh = blob[6503 + 64 + 32 * 64: 6503 + 64 + 48 * 64].reshape(16, 64)  # Directional_MLP.mlp.0 weight^T rows 32..47
    g_sh = g_rowsum.sum(1) @ w_sh.t()
    g_dn = g_dnorm.sum(1, keepdim=True)
    if ray_valid is not None:
        keep = ray_valid[:, None].to(_f32)
        gp = gp * keep.repeat_interleave(S, dim=0)
        g_sh, g_dn = g_sh * keep, g_dn * keep
    torch.autograd.backward([x, sh, dn], [gp, g_sh, g_dn])
    return o.grad, d.grad


# ---------------------------------------------------------------------------------------------------------------------
# One render branch, forward to table gradient: what the training steps (tile_model) and the autograd boundary below both run.
# Table-gradient routes (table_grad_route):
RECORDS_ADAM = "records_adam"    # the backward kernel emits the records; accumulate + sparse Adam (adam2 for two branches)
RECORDS_TABLE = "records_table"  # the backward kernel emits the records; accumulate into a gradient table
RAYS_ADAM = "rays_adam"          # dfeat -> scatter_table_grad_adam_rays (places the samples itself; large tables)
POINTS_ADAM = "points_adam"      # dfeat at contracted points built in torch -> scatter_table_grad_adam
POINTS_TABLE = "points_table"    # dfeat at contracted points -> scatter_table_grad into a gradient table (then table_adam)
_TABLE_ROUTES = (RECORDS_TABLE, POINTS_TABLE)
# ... and the entry points asking for one
SINGLE, FGBG_STEP, FGBG_GRADIENTS, AUTOGRAD = "single", "fgbg_step", "fgbg_gradients", "autograd"


def table_grad_route(entry, T, B, S, arith, half_table=False, fused_adam=True, fused_scatter=None, large_t_route="dfeat"):
    """How a training step's feature gradients reach the table -> (routes: one per branch sample count in S, the
    `compact_records` of a contracted-points scatter).  Pure: no allocation, no launch.  arith: the backward's arithmetic;
    half_table: a half-precision gather copy is resident; large_t_route: the steps' switch tile_model.LARGE_T_ROUTE (the
    tile_model wrapper of this function passes it).  Each entry point keeps the choice it made before this was one place
    (tests/test_table_grad_route_cpu.py gives each row's reason):
      SINGLE: records where fused_scatter (default: T <= 2^21 or LARGE_T_ROUTE "fused") and the workspace allow, f32 included;
        else rays / points ending in the Adam, or with fused_adam=False points into a gradient table (compact above 2^21 only);
      FGBG_STEP: records + adam2 as SINGLE but never under f32; above 2^21 (not f32, no half table) ONE rays / points scatter
        over both branches; else FGBG_GRADIENTS' gradient table;
      FGBG_GRADIENTS: per branch, records into the table at T <= 2^21 (LARGE_T_ROUTE ignored), else points with -1;
      AUTOGRAD (only asked when the table needs a gradient): records at T <= 2^21, else points with -1."""
    # records emitted by the backward kernel need the level's cursors in ITS LDS (256 buckets per level): above 2^21 entries
    # they outgrow the accumulate's LDS image.  The split pass in front of the accumulate (csrc/scatter.hip k_bin_split) serves
    # larger tables, but the stand-alone scatter from dfeat (2^13-entry buckets) is still ahead there (T = 2^24, 16 384 rays:
    # 5.6 against 6.1 ms per step): LARGE_T_ROUTE = "fused" selects the split pass
    small = T <= (1 << 21)
    records = all(scatter_supported(B, s, T) for s in S)
    compact = compact_record_format(arith)
    if entry == SINGLE:
        if fused_scatter is None:
            fused_scatter = small or large_t_route == "fused"
        if fused_scatter and records:
            route = RECORDS_ADAM if fused_adam else RECORDS_TABLE
        elif not fused_adam:
            route, compact = POINTS_TABLE, (-1 if small else compact)
        else:
            route = RAYS_ADAM if scatter_rays_supported(T, arith) and not half_table else POINTS_ADAM
        return (route,), compact
    if entry == FGBG_STEP:
        if (small or large_t_route == "fused") and records and arith != _capi.ARITH_F32:
            return (RECORDS_ADAM,) * len(S), compact
        if not small and arith != _capi.ARITH_F32 and not half_table:
            return (RAYS_ADAM if scatter_rays_supported(T, arith) else POINTS_ADAM,) * len(S), compact
        entry = FGBG_GRADIENTS
    if entry == FGBG_GRADIENTS:
        return tuple(RECORDS_TABLE if small and scatter_supported(B, s, T) else POINTS_TABLE for s in S), -1
    if entry == AUTOGRAD:
        return (RECORDS_TABLE if small and records else POINTS_TABLE,), -1
    raise ValueError(f"table_grad_route: unknown entry point {entry!r}")


def _sec(timer, name, alg_bytes=0, alg_flops=0):
    """A section of `timer` (tile_model.KernelTimer), or nothing to enter without one."""
    return timer.section(name, alg_bytes, alg_flops) if timer is not None else contextlib.nullcontext()


MLP_FLOPS_PER_SAMPLE = 2 * 13728  # 27 456 FLOP per sample forward


class _Branch:
    """One render branch on the fused kernels: the forward with its stashes, the record plan of the table-gradient route, the
    backward, the ray gradients and the finish of a route into a gradient table.
    resolution, packed, blob: the grid's level resolutions, the PackedDecoder this pass packed (its skip_levels go to the plan)
    and the decoder blob; box: the 2x box as host (min_bbox, bbox_size); route / compact: from table_grad_route (route None:
    no table gradient, dfeat only).  sized=False (fgbg_gradients): only the backward is a timer section, without byte and FLOP
    counts; workspace: the branch's own record workspace (default: the per-stream one); master: the fp32 table the point
    gradients of ray_gradients read (default: the gather table, converted); box_dev: the box as device tensors for points()
    (default: uploaded when asked)."""

    def __init__(self, resolution, packed, blob, box, rays_o, rays_d, z, dist, valid, mode, infinity, route, compact, timer=None,
                 sized=True, workspace=None, master=None, box_dev=None):
        self.resolution, self.packed, self.blob, self.master, self.box_dev = resolution, packed, blob, master, box_dev
        self.rays_o, self.rays_d, self.z, self.dist, self.valid = rays_o, rays_d, z, dist, valid
        self.box = (*box, mode, infinity)
        self.route, self.compact, self.timer, self.sized, self.workspace = route, compact, timer, sized, workspace
        self.records = route in (RECORDS_ADAM, RECORDS_TABLE)
        self.B, self.S = z.shape
        self.ws = self.tile_T = self.xstash = self.jstash = self.dfeat = self.arith = None

    def _sec(self, name, *counts):
        return _sec(self.timer if self.sized else None, name, *counts)

    def forward(self, table, plan=False, jstash=False, want_weights=False, stash=True):
        """plan: the launch also reserves the backward's record ranges (forward_plan_supported); jstash: it stashes the encoder's
        position Jacobians, so that the backward chains the feature gradients to the rays without a second pass over the table;
        stash=False (nothing needs a gradient): no tile_T / x-stash, no backward.  -> out_ray (weights in self.weights)."""
        B, S, dev = self.B, self.S, self.z.device
        self.table = table
        if stash:
            self.tile_T = torch.empty((B, tile_T_columns(S)), device=dev)
            self.xstash = torch.empty((B * S, 32), device=dev)  # encoder outputs: 1 GB at 65 536 x 128, saves the re-gather
        if jstash:
            self.jstash = torch.empty(jstash_shape(B, S), dtype=JSTASH_DTYPE, device=dev)
        with self._sec("render_forward", B * (24 + 20 + S * 16 * 8 * 2 * table.element_size()), B * S * MLP_FLOPS_PER_SAMPLE):
            r = render_forward(self.rays_o, self.rays_d, self.z, self.dist, table, self.resolution, self.packed, *self.box,
                               ray_valid=self.valid, want_weights=want_weights, tile_T=self.tile_T, xstash=self.xstash,
                               plan=plan, plan_workspace=self.workspace, jstash=self.jstash)
        if plan:
            self.ws = r[2]
        self.out, self.weights = r[0], r[1]
        return self.out

    def points(self):
        mn, sz = self.box_dev or (torch.as_tensor(v, dtype=_f32, device=self.z.device) for v in self.box[:2])
        return contracted_points(self.rays_o, self.rays_d, self.z, mn, sz, self.box[2])

    def backward(self, grad_out, weight_feature, grad_blob, grad_table, pose_grads):
        """The backward of dL/d(out_ray) = grad_out; the record routes emit into grad_table (the gradient table, or the
        overflow table of a route ending in the sparse Adam), the *_TABLE routes finish into it.  -> (g_o, g_d) with pose_grads."""
        B, S, dev = self.B, self.S, self.z.device
        self.arith = backward_arith(True, pose_grads)   # of the plan, the backward and the accumulate alike
        if self.records and self.ws is None:   # count + scan of the scatter records (depends on the sample positions only)
            with self._sec("scatter_plan", B * S * 4):
                self.ws = scatter_plan(self.rays_o, self.rays_d, self.z, self.resolution, self.table.shape[1], *self.box,
                                       ray_valid=self.valid, arith=self.arith, workspace=self.workspace,
                                       skip_levels=self.packed.skip_levels)
        bufs = (torch.zeros(B, (S + 31) // 32, device=dev), torch.zeros(B, 2, 64, device=dev)) if pose_grads else None
        ray_pos = torch.zeros(B, 6, device=dev) if self.jstash is not None else None
        # forward recompute + activation gradients + weight gradients = 3x the forward MLP FLOPs
        counts = (B * (24 + 20 + S * 16 * 8 * 2 * 4 + S * 16 * 8), 3 * B * S * MLP_FLOPS_PER_SAMPLE) if self.sized else ()
        with _sec(self.timer, "render_backward", *counts):
            self.dfeat, _ = render_backward(
                self.rays_o, self.rays_d, self.z, self.dist, self.table, self.resolution, self.packed, weight_feature,
                *self.box, self.out, self.tile_T, grad_out, ray_valid=self.valid, grad_blob=grad_blob, xstash=self.xstash,
                ray_grad_buffers=bufs, scatter=(self.ws, grad_table) if self.records else None,
                want_dfeat=not self.records or (pose_grads and self.jstash is None),
                arith=self.arith, jstash=self.jstash, ray_pos_grad=ray_pos)
        g = None
        if pose_grads and self.jstash is not None:
            g = ray_gradients_fused(self.rays_o, self.rays_d, self.blob, ray_pos, *bufs, ray_valid=self.valid)
        elif pose_grads:
            master = self.master if self.master is not None else self.table.to(_f32)
            g = ray_gradients(self.rays_o, self.rays_d, self.z, master, self.resolution, self.blob, *self.box[:3], self.dfeat,
                              *bufs, ray_valid=self.valid)
        if self.route == RECORDS_TABLE:
            with self._sec("table_grad_accumulate", B * S * 16 * 64):
                scatter_accumulate(self.ws, grad_table, B, S, arith=self.arith)
        elif self.route == POINTS_TABLE:
            pts = self.points()
            with self._sec("table_grad_scatter", B * S * 16 * (8 + 16 * 8)):
                scatter_table_grad(pts, self.dfeat, grad_table, self.resolution, compact_records=self.compact)
        return g


# ---------------------------------------------------------------------------------------------------------------------
# Autograd boundary of the fused path: HashGrid.render_batch_rays (hashgrid/__init__.py:512-596) as ONE differentiable op.
# A caller that keeps the reference's loss code -- depth / smoothness / ADMM penalty terms on the per-ray outputs, summed
# and sent through loss.backward() (tile.py:954-1011, criterions.py:122-196) -- reaches the fused kernels through it.
FORWARD_PLAN_IN_AUTOGRAD = True   # (False: FusedRenderRays plans in its backward, as rounds 1-5 did: A/B and tests)


class FusedRenderRays(torch.autograd.Function):
    """out_ray [B,16], weights [B,S] = render(rays, samples; table, decoder blob).

    forward  = scanerf_render_forward_packed (+ x-stash, + position-Jacobian stash when the rays need gradients);
    backward = scanerf_render_backward on an ARBITRARY dL/d(out_ray) [B,16], returning the gradient of the hash table (dense
               [16,T,2]: fused record emission + scanerf_render_scatter_accumulate up to 2^21 entries per level, dfeat + the
               binned scatter above), of the decoder blob [13994] and of rays_o / rays_d.
    Both run through one _Branch, on table_grad_route's AUTOGRAD row.
    Not differentiated: z_vals / dists (the sampler runs under no_grad in the reference, hashgrid/__init__.py:278-285) and the
    `weights` output (returned for inspection: gradients flowing into it are ignored, as for l2_reg_specular's detached
    weights, hashgrid/__init__.py:593).  The out_ray column W_SPEC2 is differentiated with the weights detached (ibid.)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, z_vals, dists, features, blob, resolutions, weight_feature, min_bbox, bbox_size,
                contract_mode, infinity, ray_valid, skip_levels, want_weights):
        B, S = z_vals.shape
        dev = z_vals.device
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        z_vals, dists = z_vals.contiguous(), dists.contiguous()
        ctx.wf = weight_feature.reshape(-1).contiguous()
        packed = PackedDecoder(dev).pack(blob.detach().contiguous(), ctx.wf, skip_levels)
        need_rays = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        need_grad = need_rays or ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        table = features.detach()
        if ray_valid is not None and ray_valid.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("scanerf: ray_valid must be bool / uint8")
        T = table.shape[1]
        arith = backward_arith(True, need_rays)
        route = compact = None   # (no table gradient wanted: no route)
        if ctx.needs_input_grad[4]:
            (route,), compact = table_grad_route(AUTOGRAD, T, B, [S], arith)
        # The forward launch counts the backward's record ranges (its hash indices are the plan's: no separate count launch, 0.27 ms at
        # configs[1]) where the table gradient will go through the fused records -- into a workspace this call OWNS until its
        # backward has run (other render calls may come between the two and use the per-stream one).
        ctx.plan_ws = None
        if (FORWARD_PLAN_IN_AUTOGRAD and route == RECORDS_TABLE and forward_plan_supported(B, S, T)
                and arith in _capi.T16_FAMILY):
            ctx.plan_ws = torch.empty(lib().scanerf_render_scatter_workspace_bytes(B, S, T), dtype=torch.uint8, device=dev)
        br = _Branch(resolutions, packed, blob.detach(), (list(min_bbox), list(bbox_size)), rays_o, rays_d, z_vals, dists, ray_valid,
                     int(contract_mode), bool(infinity), route, compact, workspace=ctx.plan_ws)
        out = br.forward(table, plan=ctx.plan_ws is not None, want_weights=want_weights, stash=need_grad,
                         jstash=need_rays and table.dtype == torch.float32 and ARITH in _capi.T16_FAMILY)
        # what the launch wrote goes through save_for_backward: freed with the graph, and `out` will carry this node
        ctx.save_for_backward(out, br.tile_T, br.xstash, br.jstash)
        br.out = br.tile_T = br.xstash = br.jstash = None
        ctx.branch = br
        weights = br.weights if br.weights is not None else out.new_empty(0)
        ctx.mark_non_differentiable(weights)
        return out, weights

    @staticmethod
    def backward(ctx, grad_out, _grad_weights):
        br = ctx.branch
        dev = br.z.device
        need_rays = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        grad_out = grad_out.contiguous().to(_f32)
        gtab = torch.zeros((16, br.table.shape[1], 2), dtype=_f32, device=dev) if ctx.needs_input_grad[4] else None
        gblob = torch.zeros(_capi.PARAMSIZE, dtype=_f32, device=dev)
        br.out, br.tile_T, br.xstash, br.jstash = ctx.saved_tensors
        g_o, g_d = br.backward(grad_out, ctx.wf, gblob, gtab, need_rays) or (None, None)
        br.out = br.tile_T = br.xstash = br.jstash = None
        if gtab is not None and br.table.dtype != _f32:
            gtab = gtab.to(br.table.dtype)
        return (g_o if ctx.needs_input_grad[0] else None, g_d if ctx.needs_input_grad[1] else None, None, None, gtab,
                gblob if ctx.needs_input_grad[5] else None, None, None, None, None, None, None, None, None, None)


def fused_render_rays(rays_o, rays_d, z_vals, dists, features, blob, resolutions, weight_feature, min_bbox, bbox_size,
                      contract_mode, infinity, ray_valid=None, skip_levels=0, want_weights=True):
    """FusedRenderRays.apply with keyword defaults -> (out_ray [B,16], weights [B,S])."""
    return FusedRenderRays.apply(rays_o, rays_d, z_vals, dists, features, blob, resolutions, weight_feature, min_bbox, bbox_size,
                                 contract_mode, infinity, ray_valid, skip_levels, want_weights)


COMPOSITE_BACKWARD_MAX_S = 512   # csrc/composite.hip k_composite_bwd: Tin[8]


class CompositeRays(torch.autograd.Function):
    """Alpha compositing of per-sample decoder outputs along rays as ONE op each way (csrc/composite.hip): what
    HashGrid.cal_integrate_weight + accumulate x 4 + the l2_reg_specular sum do in ~35 torch kernels (hashgrid/__init__.py:344-366,
    :564-574, :591-594).  sigma [B,S,1] or [B,S]; diffuse / specular / tint [B,S,3]; z_vals / dists [B,S]; rays_d [B,3] ->
    out_ray [B,16] (columns as the fused forward's: RGB, DEPTH, T_LEFT, DIFFUSE, SPECULAR, TINT, W_SPEC2), weights [B,S].
    Gradients flow to sigma, diffuse, specular, tint and (through delta = dists |d|) rays_d; z_vals / dists are sampler outputs.
    The forward takes any S; the adjoint keeps one transmittance per round of 64 samples in registers and stops at
    COMPOSITE_BACKWARD_MAX_S, so composite_rays() refuses a differentiable call beyond it, instead of loss.backward() failing later."""

    @staticmethod
    def forward(ctx, sigma, diffuse, specular, tint, z_vals, dists, rays_d, infinity):
        B, S = z_vals.shape
        dev = z_vals.device
        sg = sigma.reshape(B * S).contiguous()
        cd, cs, tn = (t.reshape(B * S, 3).contiguous() for t in (diffuse, specular, tint))
        z, dd, rd = z_vals.contiguous(), dists.contiguous(), rays_d.detach().contiguous()
        out = torch.empty((B, _capi.RAY_OUT), dtype=_f32, device=dev)
        w = torch.empty((B, S), dtype=_f32, device=dev)
        check(lib().scanerf_composite_forward(
            dev_ptr(sg, _f32, "sigma"), dev_ptr(cd, _f32, "diffuse"), dev_ptr(cs, _f32, "specular"), dev_ptr(tn, _f32, "tint"),
            dev_ptr(z, _f32, "z_vals"), dev_ptr(dd, _f32, "dists"), dev_ptr(rd, _f32, "rays_d"), dev_ptr(out, _f32, "out_ray"),
            dev_ptr(w, _f32, "weights"), B, S, 1 if infinity else 0, stream()), "composite_forward")
        ctx.save_for_backward(sg, cd, cs, tn, z, dd, rd, out)
        ctx.infinity, ctx.shapes = bool(infinity), (sigma.shape, diffuse.shape)
        return out, w

    @staticmethod
    def backward(ctx, g_out, g_w):
        sg, cd, cs, tn, z, dd, rd, out = ctx.saved_tensors
        B, S = z.shape
        dev = z.device
        g_sigma = torch.empty_like(sg)
        g_cd, g_cs, g_tn = torch.empty_like(cd), torch.empty_like(cs), torch.empty_like(tn)
        g_dn = torch.empty(B, dtype=_f32, device=dev)
        go = g_out.contiguous().to(_f32) if g_out is not None else torch.zeros_like(out)
        gw = g_w.contiguous().to(_f32) if g_w is not None else None
        check(lib().scanerf_composite_backward(
            dev_ptr(sg, _f32, "sigma"), dev_ptr(cd, _f32, "diffuse"), dev_ptr(cs, _f32, "specular"), dev_ptr(tn, _f32, "tint"),
            dev_ptr(z, _f32, "z_vals"), dev_ptr(dd, _f32, "dists"), dev_ptr(rd, _f32, "rays_d"), dev_ptr(out, _f32, "out_ray"),
            dev_ptr(go, _f32, "grad_out"), dev_ptr(gw, _f32, "grad_weights", allow_none=True), dev_ptr(g_sigma, _f32, "g_sigma"),
            dev_ptr(g_cd, _f32, "g_diffuse"), dev_ptr(g_cs, _f32, "g_specular"), dev_ptr(g_tn, _f32, "g_tint"),
            dev_ptr(g_dn, _f32, "g_dnorm"), B, S, 1 if ctx.infinity else 0, stream()),
            "composite_backward")
        g_rd = None
        if ctx.needs_input_grad[6]:   # |d| at d = 0: the subgradient 0, as torch's own norm backward (not 0 / 0)
            n = rd.norm(dim=-1, keepdim=True)
            g_rd = torch.where(n == 0, torch.zeros_like(rd), g_dn[:, None] * rd / n)
        sshape, cshape = ctx.shapes
        return g_sigma.reshape(sshape), g_cd.reshape(cshape), g_cs.reshape(cshape), g_tn.reshape(cshape), None, None, g_rd, None


def composite_rays(sigma, diffuse, specular, tint, z_vals, dists, rays_d, infinity=False):
    """-> (out_ray [B,16], weights [B,S]); see CompositeRays."""
    S = z_vals.shape[1]
    if S > COMPOSITE_BACKWARD_MAX_S and torch.is_grad_enabled() and any(t.requires_grad for t in (sigma, diffuse, specular, tint, rays_d)):
        raise RuntimeError(f"composite_rays: S={S} with a differentiable input: scanerf_composite_backward takes S <= "
                           f"{COMPOSITE_BACKWARD_MAX_S} (composite in torch beyond it, or call under torch.no_grad())")
    return CompositeRays.apply(sigma, diffuse, specular, tint, z_vals, dists, rays_d, infinity)


def render_batch_rays_dict(out_ray, weights, train):
    """The dictionary HashGrid.render_batch_rays returns (hashgrid/__init__.py:564-596) from the fused op's outputs:
    diffuse / tint / specular / rgb [B,3], depth [B,1], T_left [B], weights [B,S,1], and in TRAIN mode l2_reg_specular =
    mean over rays and channels of sum_s w_s c_s^2 (:593: torch.mean over [B,3]; out_ray holds the channel sum)."""
    out = {"diffuse": out_ray[:, DIFFUSE], "tint": out_ray[:, TINT], "specular": out_ray[:, SPECULAR],
           "rgb": out_ray[:, RGB], "depth": out_ray[:, DEPTH, None], "T_left": out_ray[:, T_LEFT],
           "weights": weights[..., None] if weights is not None and weights.numel() else None}
    if train:
        out["l2_reg_specular"] = out_ray[:, W_SPEC2].sum() / (3.0 * out_ray.shape[0])
    return out
