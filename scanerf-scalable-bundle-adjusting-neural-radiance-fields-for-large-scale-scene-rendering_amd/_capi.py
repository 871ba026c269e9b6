"""ctypes view of libscanerf_hip.so (the C ABI declared in include/scanerf_hip.h).

There is no CPU fallback: if the HIP library is missing, or a tensor is not a
contiguous tensor of the expected dtype on a HIP device, the call raises.
"""
import ctypes
import os
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCANERF_LIB") or os.path.join(_HERE, "lib", "libscanerf_hip.so")

F32, F16, BF16 = 0, 1, 2
RAY_OUT = 16
PARAMSIZE = 13994

_lib = None

# Every export include/scanerf_hip.h declares -- name: (return type, argument types, required) -- one letter per C type:
#   P  any pointer, array or scanerf_stream_t     I  int        U  unsigned       F  float
#   Z  size_t                                     L  int64_t / long long          S  const char * (return only)
# lib() sets each export's argtypes / restype from this table; tests/test_capi_cpu.py checks it against the header.
# OPT: test / measurement entry points, NOT required -- a lean product build may drop csrc/h3_selftest.hip and the probes;
# their users (tests, bench.py's live ceiling) check has_symbol() first.
REQ, OPT = True, False
PROTOTYPES = {
    "scanerf_last_error": ("S", "", REQ),
    "scanerf_abi_version": ("I", "", REQ),
    "scanerf_experiments_enabled": ("I", "", REQ),
    "scanerf_compute_ray_forward": ("I", "PPPPPIP", REQ),
    "scanerf_compute_ray_backward": ("I", "PPPPPIIP", REQ),
    "scanerf_ray_aabb_intersection": ("I", "PPPPPIIP", REQ),
    "scanerf_sample_points_grid": ("I", "PPPPPPPPIIP", REQ),
    "scanerf_sample_insideout_block": ("I", "PPIIPPFPPPIP", REQ),
    "scanerf_background_sampling": ("I", "PPPIFIP", REQ),
    "scanerf_adam_step": ("I", "PPPPFFFFILIP", REQ),
    "scanerf_adam_step_fp16": ("I", "PPPPFFFFILIP", REQ),
    "scanerf_embedding_bg_forward": ("I", "PPPPIIIIP", REQ),
    "scanerf_embedding_bg_backward": ("I", "PPPPPPIIIP", REQ),
    "scanerf_embedding_bwd_workspace_bytes": ("Z", "III", REQ),
    "scanerf_embedding_bg_backward_binned": ("I", "PPPPIIIIPZIP", REQ),
    "scanerf_embedding_bg_backward_binned_adam": ("I", "PPPIIIIPZPPPPIPFFFFIIP", REQ),
    "scanerf_table_grad_scatter_adam_rays": ("I", "PPIPPPIIPPPIIPPPIPZPPPPIPFFFFIIP", REQ),
    "scanerf_embedding_forward": ("I", "PPPPPPIIIP", REQ),
    "scanerf_embedding_backward": ("I", "PPPPPPPPIIIP", REQ),
    "scanerf_render_workspace_floats": ("I", "", REQ),
    "scanerf_pack_decoder": ("I", "PPPP", REQ),
    "scanerf_render_forward_packed": ("I", "PPPPPIPPPPPPPPIIIP", REQ),
    "scanerf_render_forward_packed_plan": ("I", "PPPPPIPPPPPPPPPIIIPZP", REQ),
    "scanerf_render_forward_plan_supported": ("I", "III", REQ),
    "scanerf_render_backward_grid": ("I", "I", REQ),
    "scanerf_render_backward": ("I", "PPPPPIPPPPPPPPPPPPPPPPPZPIIIP", REQ),
    "scanerf_render_scatter_workspace_bytes": ("Z", "III", REQ),
    "scanerf_render_scatter_plan": ("I", "PPPPPPIIIPZP", REQ),
    "scanerf_render_scatter_accumulate": ("I", "PIIIPZIP", REQ),
    "scanerf_render_scatter_accumulate_adam": ("I", "PPPPIPFFFFIIIIPZIP", REQ),
    "scanerf_render_scatter_accumulate_adam2": ("I", "PPPPIPFFFFIIIIPZIPZIP", REQ),
    "scanerf_ray_valid": ("I", "PPIIP", REQ),
    "scanerf_compact_rays": ("I", "PIIPPPPPPPPPPPPP", REQ),
    "scanerf_ray_grad_epilogue": ("I", "PPPPPPPPIIP", REQ),
    "scanerf_composite_forward": ("I", "PPPPPPPPPIIIP", REQ),
    "scanerf_composite_backward": ("I", "PPPPPPPPPPPPPPPIIIP", REQ),
    "scanerf_photometric_loss_scratch_floats": ("I", "", REQ),
    "scanerf_photometric_loss_grad": ("I", "PPPFPPPIP", REQ),
    "scanerf_photometric_loss_grad_fgbg": ("I", "PPPPPFPPPPIP", REQ),
    "scanerf_h3_selftest": ("I", "PPPPPPP", OPT),
    "scanerf_icache_sweep": ("I", "P", OPT),
    "scanerf_gather_rate_probe": ("I", "PLIIPP", OPT),
    "scanerf_rec8_selftest": ("I", "PPPPPIPPP", OPT),
    "scanerf_embedding_bg_point_grad": ("I", "PPPPPIIIP", REQ),
    "scanerf_embedding_bg_forward_ex": ("I", "PPPPIIIIIIP", REQ),
    "scanerf_ray_block_intersection": ("I", "PPPPPIIP", REQ),
    "scanerf_render_sample_points": ("I", "PPPPPPPPPPPPPIIIIP", REQ),
    "scanerf_prepare_points": ("I", "PPPPIIIIP", REQ),
    "scanerf_pts_inference": ("I", "PPPPPPPPPPPPPPPPIIIIIP", REQ),
    "scanerf_pts_inference_tracing": ("I", "PPPPPPPPPPPPPPPPPIIIIIP", REQ),
    "scanerf_accumulate_color": ("I", "PPPPPPPPIIIP", REQ),
    "scanerf_render_inverse_z_sampling": ("I", "PPPFIIIIP", REQ),
    "scanerf_bg_pts_inference_v2": ("I", "PPPPIPPPPPPPPIIIIIP", REQ),
    "scanerf_update_outgoing_bidx": ("I", "PPPPPPPPFIIIP", REQ),
    "scanerf_update_outgoing_bidx_v2": ("I", "PPPPPIIP", REQ),
    "scanerf_sort_tracing_blocks": ("I", "PPIIP", REQ),
    "scanerf_get_last_block": ("I", "PPPIIP", REQ),
    "scanerf_ray_firsthit_block": ("I", "PPPPPPPPPPIIP", REQ),
    "scanerf_process_occupied_grid": ("I", "IIPPPPPPIP", REQ),
    "scanerf_voxelize_mesh": ("I", "PPIIPPPPIPPP", REQ),
    "scanerf_decoder_forward": ("I", "PIPIPPPPPLP", REQ),
    "scanerf_decoder_backward_grid": ("I", "L", REQ),
    "scanerf_decoder_backward": ("I", "PIPIPPPPPPPIPIPPLP", REQ),
    "scanerf_warp_max_neighbors": ("I", "", REQ),
    "scanerf_warp_select_views": ("I", "PPPPPPIIIIIPPPP", REQ),
    "scanerf_warp_project": ("I", "PPPPPPPPPIIIIIPPPPPPP", REQ),
    "scanerf_warp_scratch_floats": ("Z", "III", REQ),
    "scanerf_warp_loss_grad": ("I", "PPPPPPPPPPPPIIIIIFPPPPPPZP", REQ),
    "scanerf_mono_scratch_floats": ("Z", "II", REQ),
    "scanerf_mono_loss_grad": ("I", "PPPPPPIIIIFFPPPZP", REQ),
    "scanerf_mesh_count_cells": ("I", "PPIIIPPP", REQ),
    "scanerf_mesh_emit_keys": ("I", "PPIIIPPPLP", REQ),
    "scanerf_mesh_cell_boxes": ("I", "PPPPIPP", REQ),
    "scanerf_mesh_gather_triangles": ("I", "PPPLPP", REQ),
    "scanerf_mesh_first_hit": ("I", "PPIPPPPPPPPIIPP", REQ),
    "scanerf_mesh_first_enter": ("I", "PPIPPPPPIIPP", REQ),
    "scanerf_view_coverage_boxes_per_pass": ("I", "", REQ),
    "scanerf_view_coverage": ("I", "PPIIIIPPIPPPPPPPPIPP", REQ),
    "scanerf_sigma_normals_points": ("I", "PPPIPPPPPPIIP", REQ),
    "scanerf_render_normals": ("I", "PPPPPIPPPPPIPPPIIIP", REQ),
    "scanerf_pts_normals": ("I", "PPPPPPPPPPPPPPIIIIIP", REQ),
    "scanerf_pts_normals_counted": ("I", "PPPPPPPPPPPPPPPIIIIIP", OPT),
    "scanerf_accumulate_normal": ("I", "PPPPPIIIP", REQ),
    "scanerf_isosurface_scratch_bytes": ("Z", "III", REQ),
    "scanerf_isosurface_count_dense": ("I", "PIIIFPZP", REQ),
    "scanerf_isosurface_emit_dense": ("I", "PIIIFPPPZPPPPIIP", REQ),
    "scanerf_isosurface_count": ("I", "PIPPPIPPLIIIFPZP", REQ),
    "scanerf_isosurface_emit": ("I", "PIPPPIPPLIIIFPPPZPPPPIIP", REQ),
    "scanerf_isosurface_count_tiles": ("I", "PPPPPPPPIIPPIIIFPZP", REQ),
    "scanerf_isosurface_emit_tiles": ("I", "PPPPPPPPIIPPIIIFPZPPPPIIP", REQ),
    "scanerf_scene_sigma_normals_points": ("I", "PPPPPPPPPIIPPPIP", REQ),
    "scanerf_mesh_components_scratch_bytes": ("Z", "II", REQ),
    "scanerf_mesh_components_label": ("I", "PIIPPZP", REQ),
    "scanerf_mesh_components_table": ("I", "PPPIIPZIPPPPPP", REQ),
    "scanerf_mesh_filter_count": ("I", "PPPIIIPZP", REQ),
    "scanerf_mesh_filter_emit": ("I", "PPPIIIPZPPPPPPPPPIIP", REQ),
    "scanerf_mesh_closest_point": ("I", "PIPPPPPPPPPIFPPPP", REQ),
    "scanerf_mesh_closest_point_counted": ("I", "PIPPPPPPPPPIFPPPPP", OPT),
    "scanerf_mesh_closest_point_brute": ("I", "PIPPIIPIFPPPP", REQ),
}
SYMBOLS = [n for n, (_, _, required) in PROTOTYPES.items() if required]
OPTIONAL_SYMBOLS = [n for n, (_, _, required) in PROTOTYPES.items() if not required]
# The exports of the second public header, include/scanerf_mesh_tools_hip.h (ops that came after ABI version 10 pinned the first
# header's set): the same letters, typed the same way, reached through tool(name) and not through lib().  All of them are required.
# tests/test_mesh_visibility_cpu.py checks this table against that header.
TOOL_PROTOTYPES = {
    "scanerf_mesh_point_views_cameras_per_pass": ("I", ""),
    "scanerf_mesh_point_views": ("I", "PIPPIIIFFFPPPPPPPPIPPP"),
    "scanerf_mesh_point_views_counted": ("I", "PIPPIIIFFFPPPPPPPPIPPPP"),
    "scanerf_tsdf_cameras_per_pass": ("I", ""),
    "scanerf_tsdf_integrate": ("I", "PPPIIIPPIIIFFFPP"),
    "scanerf_tsdf_integrate_counted": ("I", "PPPIIIPPIIIFFFPPP"),
    "scanerf_tsdf_values": ("I", "PIFPPP"),
    "scanerf_tsdf_cell_support": ("I", "PIIIPIPP"),
    "scanerf_tsdf_integrate_color": ("I", "PPPPIIIPPIIIFFFPPP"),
    "scanerf_tsdf_integrate_color_counted": ("I", "PPPPIIIPPIIIFFFPPPP"),
    "scanerf_tsdf_vertex_colors": ("I", "PIIIPPIPPP"),
    "scanerf_tsdf_vertex_normals": ("I", "PPIIIPPPIPPP"),
    "scanerf_mesh_simplify_scratch_bytes": ("I", "IIP"),
    "scanerf_mesh_simplify_cluster": ("I", "PPPPIIPFPZP"),
    "scanerf_mesh_simplify_emit": ("I", "PPPPIIPFPZPPPPPPIIP"),
    "scanerf_mesh_trace": ("I", "PPIPPPPPPPPIPPPP"),
    "scanerf_mesh_trace_brute": ("I", "PPIPPIIPIPPPP"),
    "scanerf_mesh_render_views": ("I", "PPIIIPPPPPPPPIPPPPPPP"),
    "scanerf_mesh_project_colors": ("I", "PPIPPPIIIFFFFPPPPPPPPIPPP"),
    "scanerf_mesh_project_colors_counted": ("I", "PPIPPPIIIFFFFPPPPPPPPIPPPP"),
    "scanerf_mesh_resolve_colors": ("I", "PIPPPP"),
}
CTYPES = {"P": ctypes.c_void_p, "I": ctypes.c_int, "U": ctypes.c_uint, "F": ctypes.c_float, "Z": ctypes.c_size_t,
          "L": ctypes.c_int64, "S": ctypes.c_char_p}


def has_symbol(name):
    return hasattr(lib(), name)


class RenderCfg(ctypes.Structure):
    _fields_ = [("contract_mode", ctypes.c_int), ("infinity", ctypes.c_int),
                ("min_bbox", ctypes.c_float * 3), ("bbox_size", ctypes.c_float * 3), ("arith", ctypes.c_int),
                ("skip_levels", ctypes.c_uint)]


ARITH_F32, ARITH_H3, ARITH_T16, ARITH_T16S = 0, 1, 2, 3
T16_FAMILY = (ARITH_T16, ARITH_T16S)   # backward on 16-sample tiles: x-stash, plan counted by the forward, in-kernel pose path


def _typed(fn, name, ret, args):
    """fn with the prototype's types; a call with the wrong number of arguments raises TypeError (ctypes itself passes
    extra arguments through)."""
    fn.restype = CTYPES[ret]
    fn.argtypes = [CTYPES[a] for a in args]
    n = len(args)

    def call(*a):
        if len(a) != n:
            raise TypeError(f"{name}() takes {n} arguments ({len(a)} given)")
        return fn(*a)
    call.__name__ = name
    return call


_tools = {}


def tool(name):
    """The typed function of an export of include/scanerf_mesh_tools_hip.h (TOOL_PROTOTYPES); a library without it is an error."""
    fn = _tools.get(name)
    if fn is None:
        ret, args = TOOL_PROTOTYPES[name]
        lib()   # the checks and the warnings of the first load
        so = ctypes.CDLL(LIB_PATH)
        if not hasattr(so, name):
            raise RuntimeError(f"scanerf: {LIB_PATH} does not export {name}")
        fn = _tools[name] = _typed(getattr(so, name), name, ret, args)
    return fn


def lib():
    """Load the HIP library or fail loudly (no fallback): a namespace of the exports in PROTOTYPES, typed; an optional
    export the build does not have is absent (has_symbol)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"scanerf: HIP library not built: {LIB_PATH} is missing. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc, gfx950).")
        so = ctypes.CDLL(LIB_PATH)
        l = types.SimpleNamespace()
        for name, (ret, args, required) in PROTOTYPES.items():
            if hasattr(so, name):
                setattr(l, name, _typed(getattr(so, name), name, ret, args))
            elif required:
                raise RuntimeError(f"scanerf: {LIB_PATH} does not export {name}")
        _lib = l
        st = audit_state()
        if st["status"] != "passed":
            import warnings
            warnings.warn(f"scanerf: {LIB_PATH} is NOT the audited build (ISA audit: {st['status']}; {st.get('why', '')}).  Its kernels' "
                          "listings were not checked against the validated ones (csrc/isa_manifest.json, DESIGN.md §4.1 (last paragraph); profiles/DESIGN_r04_experiment_log.md §4.10: no "
                          "packed-f32 instructions, pinned listings): launch-to-launch reproducibility is not established for it.",
                          RuntimeWarning, stacklevel=2)
    return _lib


def audit_state():
    """What tools/isa_audit.py (run by `make`) said about the library file this process loads: {"status": "passed" | "unvalidated"
    (another compiler build than the validated one; no packed-f32 instruction found) | "skipped" (built with
    SCANERF_SKIP_ISA_AUDIT=1) | "failed" | "stale" (the file changed after the audit) | "missing"}."""
    import hashlib
    import json
    side = os.path.join(os.path.dirname(LIB_PATH), "isa_audit.json")
    if os.environ.get("SCANERF_LIB"):
        return {"status": "variant", "why": "SCANERF_LIB selects an investigation build (tools/build_variant.py)"}
    try:
        st = json.load(open(side))
    except (OSError, ValueError):
        return {"status": "missing", "why": f"{side} not found: the library was not built by csrc/Makefile's `all`"}
    sha = hashlib.sha256(open(LIB_PATH, "rb").read()).hexdigest()
    if st.get("library_sha256") != sha:
        return {"status": "stale", "why": "the library file is not the one the audit saw"}
    return {"status": st.get("status", "missing"), "why": "; ".join(st.get("detail") or [])[:400], "compiler": st.get("compiler")}


def audit_required():
    """True where an "unvalidated" library is NOT acceptable: SCANERF_REQUIRE_AUDITED=1 (the project's own CI / bench box), or the
    installed hipcc IS the compiler build csrc/isa_manifest.json was validated with -- then nothing excuses a library that was
    not built and audited by it.  Elsewhere (a downstream user's other ROCm) "unvalidated" stays a loud warning."""
    import json
    import subprocess
    if os.environ.get("SCANERF_REQUIRE_AUDITED") == "1":
        return True
    try:
        want = json.load(open(os.path.join(_HERE, "csrc", "isa_manifest.json"))).get("compiler", "")
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True, timeout=60).stdout
        have = " | ".join(ln.strip() for ln in out.splitlines() if ln.startswith(("HIP version", "AMD clang version")))
        return bool(want) and want == have
    except (OSError, ValueError, subprocess.SubprocessError):
        return False


SWEEP_ICACHE = False   # tests only: evict the instruction caches after every library call (scanerf_icache_sweep)


def check(status, what):
    if status != 0:
        msg = lib().scanerf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"scanerf {what} failed ({status}): {msg}")
    if SWEEP_ICACHE:
        if not has_symbol("scanerf_icache_sweep"):
            raise RuntimeError("scanerf: SWEEP_ICACHE needs scanerf_icache_sweep (a test entry point this build does not export)")
        if lib().scanerf_icache_sweep(stream()) != 0:
            raise RuntimeError("scanerf icache_sweep failed: " + lib().scanerf_last_error().decode("utf-8", "replace"))


def stream():
    return torch.cuda.current_stream().cuda_stream


_DT = {torch.float32: "f32", torch.int32: "i32", torch.bool: "bool", torch.uint8: "u8", torch.float16: "f16",
       torch.bfloat16: "bf16", torch.int64: "i64", torch.int16: "i16"}


def dev_ptr(t, dtypes, name, allow_none=False):
    """Device pointer of a contiguous GPU tensor; validates what the reference leaves unchecked
    (the reference casts data_ptr blindly and calls .contiguous() even on outputs, so a
    non-contiguous output silently receives nothing)."""
    if t is None:
        if allow_none:
            return None
        raise RuntimeError(f"scanerf: {name} is None")
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"scanerf: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"scanerf: {name} must live on the GPU (no CPU path exists); got device {t.device}")
    if not isinstance(dtypes, (tuple, list)):
        dtypes = (dtypes,)
    if t.dtype not in dtypes:
        raise RuntimeError(f"scanerf: {name} has dtype {t.dtype}, expected {[_DT.get(d, d) for d in dtypes]}")
    if not t.is_contiguous():
        raise RuntimeError(f"scanerf: {name} must be contiguous")
    return t.data_ptr()


def feat_dtype_code(t):
    return {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}[t.dtype]


def ordered_after(creator, seen):
    """For a device tensor the package builds lazily and keeps (one copy, too large to keep per stream): `creator` is the torch stream
    its first use filled it on.  A later use under ANOTHER stream first waits for that stream (once per stream: `seen` holds the
    handles already ordered), so the reader cannot run ahead of the fill.  On the creating stream itself -- the single-stream path --
    this is a comparison of two handles: no event, no launch."""
    cur = torch.cuda.current_stream(creator.device)
    if cur.cuda_stream != creator.cuda_stream and cur.cuda_stream not in seen:
        cur.wait_stream(creator)
        seen.add(cur.cuda_stream)


_workspaces = {}


def workspace(device, nbytes, tag="plan"):
    """Grow-only scratch buffer per (device, stream, tag) (torch's caching allocator owns the memory; the C ABI never
    allocates).  Keyed by the CURRENT stream: work queued on one stream never shares scratch with another stream's, and a
    buffer that is replaced by a larger one is released to the allocator on the stream all of its users were queued on,
    so it cannot be handed out again while they are still in flight.  tag: a fused plan lives in its buffer from
    scatter_plan / render_forward(plan=True) until the accumulate; the stand-alone scatter (one call, "scatter") has its own
    buffer so that it cannot land between the two."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream if str(device).startswith("cuda") else 0, tag)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _workspaces.pop(key, None)
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf
