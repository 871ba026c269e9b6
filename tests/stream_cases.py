"""A registry of small cases, one or more per op family, for the stream contract of include/scanerf_hip.h ("launches are asynchronous
on `stream`"; a helper module, not a test).  tests/test_stream_cases_cpu.py checks the registry itself (every stream-taking export is
claimed; the two seeds of a case differ in every float and are equally valid in every integer), tests/test_gpu_stream_contract.py
runs every case under a side stream.

A Case has
    name, entries   the scanerf_* exports the case is expected to call;
    build(seed)     CPU tensors for every input (a dict), from the generators the suite already has;
    to_device(inp)  the device-side state: a dict with "in" (the inputs on the GPU) plus whatever the case's `setup` adds
                    (fixtures that are no inputs: geometry, meshes, packed-decoder workspaces);
    refill(state, inp)   in-place copy_ of another seed's inputs (CPU or device tensors) into the same device tensors;
    run(state)      a tuple of output tensors, each cloned on the current stream.  Outputs are allocated and pre-filled by run itself
                    on the current stream; integer outputs that a later op of the same run indexes with are pre-filled with valid
                    values, so stale data is a wrong answer and never an out-of-range index;
    exact           True: launch-to-launch bit identity (the suite asserts it for the entry already); False: the two float-atomic
                    table gradients, judged by `compare(outputs, reference(inputs))`: their parity tests' oracle and tolerances;
    host_syncs      None, or the file:line of the wrapper's first host read-back (.item() / .tolist() / int()): the per-entry
                    "no call synchronises" rule then holds up to that read-back;
    int_ranges      key -> (lo, hi): every value of an integer input lies in [lo, hi) for both seeds (bool inputs need none).
"""
import os
import re

import numpy as np
import torch

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scanerf_hip.h")
DEV = "cuda:0"
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ the header
def stream_entries(path=HEADER):
    """Names of the declarations of include/scanerf_hip.h whose LAST parameter is a scanerf_stream_t, in header order."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for m in re.finditer(r"\b(scanerf_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        if params and re.match(r"scanerf_stream_t\s+\w+$", params[-1]):
            out.append(m.group(1))
    return out


# ------------------------------------------------------------------------------------------------------------------ the case type
class Case:
    def __init__(self, name, entries, build, run, setup=None, exact=True, host_syncs=None, int_ranges=None, optional=(),
                 reference=None, compare=None):
        self.name, self.entries, self.build, self._run, self._setup = name, frozenset(entries), build, run, setup
        self.exact, self.host_syncs, self.int_ranges, self.optional = exact, host_syncs, dict(int_ranges or {}), frozenset(optional)
        self.reference, self.compare = reference, compare
        assert self.optional <= self.entries

    def to_device(self, inputs):
        state = {"in": {k: v.to(DEV).contiguous() for k, v in inputs.items()}}
        if self._setup is not None:
            self._setup(state)
        return state

    def refill(self, state, inputs):
        for k, v in inputs.items():
            state["in"][k].copy_(v, non_blocking=True)

    def run(self, state):
        return tuple(t.clone() for t in self._run(state))

    def live_entries(self):
        """The entries this build of the library has (the optional test / measurement exports may be absent)."""
        from scanerf_amd import _capi
        return {e for e in self.entries if e not in self.optional or _capi.has_symbol(e)}

    def __repr__(self):
        return f"Case({self.name})"


def stage(inputs):
    """The inputs of one seed on the GPU (copied on the current stream): what refill() copies from without touching the host."""
    return {k: v.to(DEV).contiguous() for k, v in inputs.items()}


def _t(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _rng(seed, salt):
    return np.random.default_rng(1000 * salt + seed)


def _rays(rng, B, scale=4.0):
    from test_gpu_parity import rays
    return rays(rng, B, scale)


def _table(rng, L, T):
    from test_gpu_parity import _table as table
    return table(rng, L, T)


def _res16():
    return O.level_resolutions(torch.tensor([32, 32, 32]), torch.tensor([2048, 2048, 2048])).int().contiguous()


def _blob(seed):
    sd = O.init_mlp(seed=seed, bias_scale=0.05)
    sd["sigma_layer.mlp.0.bias"] = sd["sigma_layer.mlp.0.bias"] + 4.0   # visible densities, as render_scenes' decoders
    return O.pack_blob(sd).float().contiguous()


def _lib():
    from scanerf_amd import _capi
    return _capi.lib()


def _call(name, *args):
    """One export through _capi.lib() (fetched at call time) on the current stream, checked."""
    from scanerf_amd import _capi
    _capi.check(getattr(_capi.lib(), name)(*args, _capi.stream()), name)


def _p(t):
    return None if t is None else t.data_ptr()


def _new(shape, fill=0.0, dtype=torch.float32):
    return torch.full(tuple(shape), fill, dtype=dtype, device=DEV)


CASES = []


def case(*a, **k):
    CASES.append(Case(*a, **k))


# ------------------------------------------------------------------------------------------------------------------ rays, box, samplers
def _build_rays(seed):
    rng = _rng(seed, 1)
    C, B = 7, 1000
    Ks = np.tile(f32([500, 0, 320.3, 0, 510, 239.6, 0, 0, 1]), (C, 1)) + f32(rng.uniform(0, 1, (C, 1)))
    locs = np.stack([np.sort(rng.integers(0, C, B)), rng.integers(0, 640, B), rng.integers(0, 480, B)], 1).astype(np.int32)
    return {"Ks": _t(Ks, torch.float32), "C2Ws": _t(rng.normal(size=(C, 12)).astype(f32)), "locs": _t(locs),
            "go": _t(rng.normal(size=(B, 3)).astype(f32)), "gd": _t(rng.normal(size=(B, 3)).astype(f32))}


def _run_rays(st):
    from scanerf_amd.cuda import compute_ray_backward, compute_ray_forward
    i = st["in"]
    B, C = i["locs"].shape[0], i["Ks"].shape[0]
    ro, rd, gC = _new((B, 3)), _new((B, 3)), _new((C, 12))
    compute_ray_forward(ro, rd, i["Ks"], i["C2Ws"], i["locs"])
    compute_ray_backward(i["go"], i["gd"], i["Ks"], gC, i["locs"])
    return ro, rd, gC


case("rays", {"scanerf_compute_ray_forward", "scanerf_compute_ray_backward"}, _build_rays, _run_rays,
     int_ranges={"locs": [(0, 7), (0, 640), (0, 480)]})


def _build_box(seed):
    rng = _rng(seed, 2)
    o, d = _rays(rng, 1000, 12.0)
    d[::17, 0] = 0.0
    return {"o": _t(o), "d": _t(d), "c": _t(rng.uniform(-1, 1, 3).astype(f32)), "s": _t(rng.uniform(6, 10, 3).astype(f32))}


def _run_box(st):
    from scanerf_amd.cuda import ray_aabb_intersection
    i = st["in"]
    b = _new((i["o"].shape[0], 2), -1.0)
    ray_aabb_intersection(i["o"], i["d"], i["c"], i["s"], b)
    return (b,)


case("box", {"scanerf_ray_aabb_intersection"}, _build_box, _run_box)


def _build_samplers(seed):
    rng = _rng(seed, 3)
    B = 1000
    o, d = _rays(rng, B, 5.0)
    return {"o": _t(o), "d": _t(d), "corner": _t(f32([-4, -4, -4]) + rng.uniform(-0.1, 0.1, 3).astype(f32)),
            "size": _t(f32([8, 8, 8]) + rng.uniform(-0.1, 0.1, 3).astype(f32)), "occ": _t(rng.random((16, 16, 16)) < 0.5),
            "o_in": _t(rng.uniform(-1, 1, (B, 3)).astype(f32)), "c": _t(rng.uniform(-0.1, 0.1, 3).astype(f32)),
            "s": _t(f32([4, 4, 4]) + rng.uniform(0, 0.1, 3).astype(f32)), "st": _t(rng.uniform(0, 3, B).astype(f32)),
            "bd": _t(rng.uniform(1, 20, B).astype(f32))}


def _run_samplers(st):
    from scanerf_amd.cuda import background_sampling_cuda, sample_insideout_block, sample_points_grid
    i = st["in"]
    B = i["o"].shape[0]
    z, dist = _new((B, 33), -1.0), _new((B, 33), -1.0)
    sample_points_grid(i["o"], i["d"], z, dist, i["corner"], i["size"], i["occ"], st["l2d"])
    zi, zb = _new((B, 64)), _new((B, 32))
    sample_insideout_block(i["o_in"], i["d"], 64, 32, i["c"], i["s"], 200.0, zi, zb)
    zz = _new((B, 48))
    background_sampling_cuda(i["o"], i["d"], i["st"], i["bd"], zz, 48, 1.6)
    return z, dist, zi, zb, zz


def _setup_samplers(st):
    st["l2d"] = torch.tensor([4, 4, 4], dtype=torch.int32, device=DEV)


case("samplers", {"scanerf_sample_points_grid", "scanerf_sample_insideout_block", "scanerf_background_sampling"},
     _build_samplers, _run_samplers, setup=_setup_samplers)


# ------------------------------------------------------------------------------------------------------------------ Adam
def _build_adam(seed):
    rng = _rng(seed, 4)
    K = 4099
    gr = (rng.normal(size=(K, 8)) * 1e-3).astype(f32)
    keep = rng.random((K, 8)) < 0.3
    gr = np.where(keep, gr, 0).astype(f32)
    gr[0, 0] = f32(1e-3 * seed)
    m = (rng.normal(size=(K, 8)) * 1e-2).astype(f32)
    v = (np.abs(rng.normal(size=(K, 8))) * 1e-3).astype(f32)
    return {"p": _t(rng.normal(size=(K, 8)).astype(f32)), "g": _t(gr), "m": _t(m), "v": _t(v),
            "m16": _t(m.astype(np.float16)), "v16": _t(v.astype(np.float16))}


def _run_adam(st):
    from scanerf_amd.cuda import adam_step_cuda, adam_step_cuda_fp16
    i = st["in"]
    P, M, V = i["p"].clone(), i["m"].clone(), i["v"].clone()
    adam_step_cuda(P, i["g"], M, V, 1e-3, 0.9, 0.99, 1e-15, 3)
    P2, M2, V2 = i["p"].clone(), i["m16"].clone(), i["v16"].clone()
    adam_step_cuda_fp16(P2, i["g"], M2, V2, 1e-3, 0.9, 0.99, 1e-15, 3)
    return P, M, V, P2, M2, V2


case("adam", {"scanerf_adam_step", "scanerf_adam_step_fp16"}, _build_adam, _run_adam)


# ------------------------------------------------------------------------------------------------------------------ encoders
ENC_N, ENC_T = 1024, 2 ** 13


def _build_enc_bg(seed):
    rng = _rng(seed, 5)
    pts = rng.uniform(-2, 2, (ENC_N, 3)).astype(f32)
    pts[0] = [2.0, -2.0, 0.0]
    return {"pts": _t(pts), "feat": _t(_table(rng, 16, ENC_T)), "gin": _t(rng.normal(size=(ENC_N, 16, 2)).astype(f32)),
            "dfeat": _t(rng.normal(size=(16, ENC_N, 2)).astype(f32))}


def _setup_res(st):
    st["res"] = _res16().to(DEV)


def _run_enc_bg(st):
    from scanerf_amd.hashgrid import embedding_bg_forward_cuda
    i, res = st["in"], st["res"]
    N, T = ENC_N, ENC_T
    out = _new((N, 16, 2))
    embedding_bg_forward_cuda(i["pts"], out, i["feat"], res)
    half = i["feat"].to(torch.float16)
    outs = []
    for feat, code, variant, lm in ((i["feat"], 0, 1, 1), (half, 1, 2, 0)):
        o = _new((16, N, 2) if lm else (N, 16, 2))
        _call("scanerf_embedding_bg_forward_ex", _p(i["pts"]), _p(o), _p(feat), _p(res), N, 16, T, code, variant, lm)
        outs.append(o)
    gp = _new((N, 3))
    _call("scanerf_embedding_bg_point_grad", _p(i["pts"]), _p(i["dfeat"]), _p(gp), _p(i["feat"]), _p(res), N, 16, T)
    return (out, *outs, gp)


case("encoder_bg", {"scanerf_embedding_bg_forward", "scanerf_embedding_bg_forward_ex", "scanerf_embedding_bg_point_grad"},
     _build_enc_bg, _run_enc_bg, setup=_setup_res)


def _run_enc_bg_atomic(st):
    from scanerf_amd.hashgrid import embedding_bg_backward_cuda
    i = st["in"]
    gp, gf = _new((ENC_N, 3)), _new((16, ENC_T, 2))
    embedding_bg_backward_cuda(i["pts"], i["gin"], gp, gf, i["feat"], st["res"])   # N < 4096: the atomic kernel
    return gp, gf


def _ref_enc_bg(inp):
    gp, gf = O.embedding_backward(inp["pts"].numpy(), inp["gin"].numpy(), inp["feat"].numpy(), _res16().numpy())
    return gp, gf


def _cmp_table_grad(got, ref):
    """tests/test_gpu_parity.py test_embedding_bg_backward / test_embedding_box_variant_and_autograd_modules: their bounds."""
    gp, gf = (t.cpu().numpy() for t in got)
    np.testing.assert_allclose(gf, ref[1], rtol=1e-3, atol=2e-4)
    scale = np.abs(ref[0]).max()
    np.testing.assert_allclose(gp / scale, ref[0] / scale, rtol=1e-4, atol=2e-6)


case("encoder_bg_atomic", {"scanerf_embedding_bg_backward"}, _build_enc_bg, _run_enc_bg_atomic, setup=_setup_res, exact=False,
     reference=_ref_enc_bg, compare=_cmp_table_grad)

BOX_L, BOX_T = 8, 2 ** 10


def _box_res():
    return O.level_resolutions(torch.tensor([16, 16, 16]), torch.tensor([256, 256, 256]), BOX_L).int().contiguous()


def _build_enc_box(seed):
    rng = _rng(seed, 6)
    corner, size = f32([-1, 0, 2]) + rng.uniform(0, 0.1, 3).astype(f32), f32([4, 6, 5]) + rng.uniform(0, 0.1, 3).astype(f32)
    pts = (rng.uniform(-0.05, 1.05, (ENC_N, 3)) * size + corner).astype(f32)
    return {"pts": _t(pts), "feat": _t(_table(rng, BOX_L, BOX_T)), "gin": _t(rng.normal(size=(ENC_N, BOX_L, 2)).astype(f32)),
            "corner": _t(corner), "size": _t(size)}


def _setup_box_res(st):
    st["res"] = _box_res().to(DEV)


def _run_enc_box(st):
    from scanerf_amd.hashgrid import embedding_forward_cuda
    i = st["in"]
    out = _new((ENC_N, BOX_L, 2))
    embedding_forward_cuda(i["pts"], out, i["feat"], i["corner"], i["size"], st["res"])
    return (out,)


def _run_enc_box_atomic(st):
    from scanerf_amd.hashgrid import embedding_backward_cuda
    i = st["in"]
    gp, gf = _new((ENC_N, 3)), _new((BOX_L, BOX_T, 2))
    embedding_backward_cuda(i["pts"], i["gin"], gp, gf, i["feat"], i["corner"], i["size"], st["res"])
    return gp, gf


def _ref_enc_box(inp):
    return O.embedding_backward(inp["pts"].numpy(), inp["gin"].numpy(), inp["feat"].numpy(), _box_res().numpy(), inp["corner"].numpy(),
                                inp["size"].numpy())


case("encoder_box", {"scanerf_embedding_forward"}, _build_enc_box, _run_enc_box, setup=_setup_box_res)
case("encoder_box_atomic", {"scanerf_embedding_backward"}, _build_enc_box, _run_enc_box_atomic, setup=_setup_box_res, exact=False,
     reference=_ref_enc_box, compare=_cmp_table_grad)


# ------------------------------------------------------------------------------------------------------------------ binned table gradient
def _build_binned(seed):
    rng = _rng(seed, 7)
    N = 4096
    pts = rng.uniform(-2, 2, (N, 3)).astype(f32)
    pts[:50] = 2.0
    gin = (rng.normal(size=(N, 16, 2)) * np.exp(rng.uniform(-6, 0, (N, 16, 1)))).astype(f32)
    return {"pts": _t(pts), "gin": _t(gin), "dfeat": _t(np.ascontiguousarray(gin.transpose(1, 0, 2)))}


def _run_binned(st):
    from scanerf_amd import render
    from scanerf_amd._capi import workspace
    i, res = st["in"], st["res"]
    N, T = i["pts"].shape[0], ENC_T
    gf0 = _new((16, T, 2))
    need = _lib().scanerf_embedding_bwd_workspace_bytes(N, 16, T)
    ws = workspace(DEV, need, "scatter")
    _call("scanerf_embedding_bg_backward_binned", _p(i["pts"]), _p(i["gin"]), _p(gf0), _p(res), N, 16, T, 0, _p(ws), ws.numel(), -1)
    gf1 = render.scatter_table_grad(i["pts"], i["dfeat"], _new((16, T, 2)), res)
    outs = [gf0, gf1]
    for fmt in (0, 1, 2):
        params, m1, m2, over = (_new((16, T, 2)) for _ in range(4))
        render.scatter_table_grad_adam(i["pts"], i["dfeat"], res, params, m1, m2, 1e-2, 0.9, 0.99, 1e-15, 0, overflow_grad=over,
                                       compact_records=fmt)
        outs += [params, m1, m2]
    return outs


case("binned", {"scanerf_embedding_bg_backward_binned", "scanerf_embedding_bg_backward_binned_adam"}, _build_binned, _run_binned,
     setup=_setup_res)

RAYS_B, RAYS_S1, RAYS_S2, RAYS_T = 256, 33, 16, 2 ** 22


def _build_rays_scatter(seed):
    """tests/test_gpu_parity.py test_ray_source_scatter_equals_points_and_concatenation's draws at B = 256, T = 2^22 (the smallest
    table the route accepts)."""
    gen = torch.Generator().manual_seed(77 + seed)
    B, S1, S2 = RAYS_B, RAYS_S1, RAYS_S2
    return {"o": torch.rand(B, 3, generator=gen) * 8 - 4, "d": torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1),
            "z1": torch.rand(B, S1, generator=gen) * 3, "z2": 8 + torch.rand(B, S2, generator=gen) * 50,
            "v1": torch.rand(B, generator=gen) > 0.2, "d1": torch.randn(16, B * S1, 2, generator=gen),
            "d2": torch.randn(16, B * S2, 2, generator=gen)}


def _setup_rays_scatter(st):
    _setup_res(st)
    st["tables"] = [torch.empty(16, RAYS_T, 2, device=DEV) for _ in range(4)]


def _run_rays_scatter(st):
    from scanerf_amd import render
    i = st["in"]
    params, m1, m2, over = st["tables"]
    for t in st["tables"]:
        t.zero_()
    br = [(i["z1"], i["d1"], i["v1"], render.FORE), (i["z2"], i["d2"], None, render.BG)]
    render.scatter_table_grad_adam_rays(i["o"], i["d"], br, [-8.0, -8.0, -8.0], [16.0, 16.0, 16.0], st["res"], params, m1, m2, 1e-2, 0.9,
                                        0.99, 1e-15, 0, overflow_grad=over)
    # (the tables are 512 MB each: the touched entries are what differs; every 2^22-entry level is compared through its moments)
    return params, m1, over[:, ::64]


case("large_table_rays", {"scanerf_table_grad_scatter_adam_rays"}, _build_rays_scatter, _run_rays_scatter, setup=_setup_rays_scatter)


# ------------------------------------------------------------------------------------------------------------------ fused training path
TILE = dict(corner=[-4.0, -4.0, -4.0], size=[8.0, 8.0, 8.0])


def _tile(log2_T):
    return O.Tile(TILE["corner"], TILE["size"], log2_T=log2_T)


def _build_fused(B, T, seed, salt):
    rng = _rng(seed, salt)
    o, d = _rays(rng, B, 4.0)
    return {"o": _t(o), "d": _t(d), "feat": _t(_table(rng, 16, T)), "blob": _blob(seed), "gout": _t((rng.normal(size=(B, 16)) / B).astype(f32)),
            "target": _t(rng.random((B, 3)).astype(f32))}


def _setup_fused(log2_T):
    def setup(st):
        from scanerf_amd import network, render
        tile = _tile(log2_T)
        on = lambda a: _t(a).to(DEV).contiguous()
        st.update(occ_corner=on(tile.occ_corner), occ_size=on(tile.occ_size), occ=on(tile.occ), l2d=on(tile.log2dim).int(),
                  res=on(tile.res).int(), box=(tile.min_bbox.tolist(), tile.bbox_size.tolist(), render.FORE, False),
                  packed=render.PackedDecoder(DEV), wf=network.weight_feature(20000, DEV))
    return setup


def _sample(st, S):
    from scanerf_amd.cuda import sample_points_grid
    i = st["in"]
    B = i["o"].shape[0]
    z, dist = _new((B, S), -1.0), _new((B, S), -1.0)
    sample_points_grid(i["o"], i["d"], z, dist, st["occ_corner"], st["occ_size"], st["occ"], st["l2d"])
    return z, dist


def _fused_step(arith, S, plan):
    """One training step's library calls, lowest-level wrappers: sampler, pack, forward (with the plan, or scatter_plan), loss, backward
    emitting records, accumulate into a gradient table, accumulate + Adam."""
    def run(st):
        from scanerf_amd import render
        i = st["in"]
        render.set_arith(arith)
        try:
            B, T = i["o"].shape[0], i["feat"].shape[1]
            z, dist = _sample(st, S)
            valid = torch.all(z != -1, dim=-1)
            pk = st["packed"].pack(i["blob"], st["wf"])
            tile_T, xs = _new((B, render.tile_T_columns(S))), _new((B * S, 32))
            code = render.backward_arith(True, False)
            if plan:
                out, w, ws = render.render_forward(i["o"], i["d"], z, dist, i["feat"], st["res"], pk, *st["box"], ray_valid=valid,
                                                   out_ray=_new((B, 16)), weights=_new((B, S)), tile_T=tile_T, xstash=xs, plan=True)
            else:
                out, w = render.render_forward(i["o"], i["d"], z, dist, i["feat"], st["res"], pk, *st["box"], ray_valid=valid,
                                               out_ray=_new((B, 16)), weights=_new((B, S)), tile_T=tile_T, xstash=xs)
                ws = render.scatter_plan(i["o"], i["d"], z, st["res"], T, *st["box"], ray_valid=valid, arith=code)
            loss, g = render.photometric_loss_grad(out, i["target"], valid, 0.01, grad_out=_new((B, 16)))
            g = g + i["gout"]
            over = _new((16, T, 2))
            dfeat, gblob = render.render_backward(i["o"], i["d"], z, dist, i["feat"], st["res"], pk, st["wf"], *st["box"], out, tile_T, g,
                                                  ray_valid=valid, xstash=xs, scatter=(ws, over), want_dfeat=True, arith=code)
            gtab = render.scatter_accumulate(ws, _new((16, T, 2)), B, S, arith=code)
            P, M, V = i["feat"].clone(), _new((16, T, 2)), _new((16, T, 2))
            render.scatter_accumulate_adam(ws, P, M, V, 1e-2, 0.9, 0.99, 1e-15, 0, B, S, overflow_grad=over, arith=code)
            return z, dist, out, w, loss, dfeat, gblob, gtab, P, M, V
        finally:
            render.set_arith(render.DEFAULT_ARITH)
    return run


_FUSED_COMMON = {"scanerf_sample_points_grid", "scanerf_pack_decoder", "scanerf_photometric_loss_grad", "scanerf_render_backward",
                 "scanerf_render_scatter_accumulate", "scanerf_render_scatter_accumulate_adam"}
case("fused_h3", _FUSED_COMMON | {"scanerf_render_forward_packed", "scanerf_render_scatter_plan"},
     lambda seed: _build_fused(1000, 2 ** 13, seed, 8), _fused_step("h3", 33, False), setup=_setup_fused(13))
case("fused_t16", _FUSED_COMMON | {"scanerf_render_forward_packed", "scanerf_render_scatter_plan"},
     lambda seed: _build_fused(1024, 2 ** 13, seed, 9), _fused_step("t16", 16, False), setup=_setup_fused(13))
# (the forward counts the plan only where its grid equals the backward's: 256 workgroups of four rays each, full from 2048 rays on)
case("fused_t16s_plan", _FUSED_COMMON | {"scanerf_render_forward_packed_plan"},
     lambda seed: _build_fused(2048, 2 ** 13, seed, 10), _fused_step("t16s", 64, True), setup=_setup_fused(13))


def _run_fgbg(st):
    """Two branches over the same rays: each planned and emitted on its own workspace, both losses, the pose path (Jacobian stash,
    ray-gradient epilogue), one Adam over both record sets."""
    from scanerf_amd import render
    i = st["in"]
    B, T, S1, S2 = i["o"].shape[0], i["feat"].shape[1], 33, 16
    code = render.backward_arith(True, True)
    z1, dist1 = _sample(st, S1)
    v1 = torch.all(z1 != -1, dim=-1)
    z2 = (9.0 + 60.0 * torch.linspace(0, 1, S2, device=DEV)[None, :] * (1.0 + i["o"][:, :1].abs())).contiguous()
    dist2 = torch.cat([z2[:, 1:] - z2[:, :-1], _new((B, 1), 1e-6)], 1).contiguous()
    v2 = i["target"][:, 0] > 0.2
    pk = st["packed"].pack(i["blob"], st["wf"])
    mn, sz = st["box"][0], st["box"][1]
    need = lambda S: _lib().scanerf_render_scatter_workspace_bytes(B, S, T)
    fw = []
    for z, dist, v, S, mode, inf in ((z1, dist1, v1, S1, render.FORE, False), (z2, dist2, v2, S2, render.BG, True)):
        tile_T, xs = _new((B, render.tile_T_columns(S))), _new((B * S, 32))
        js = torch.zeros(render.jstash_shape(B, S), dtype=render.JSTASH_DTYPE, device=DEV)
        out, _ = render.render_forward(i["o"], i["d"], z, dist, i["feat"], st["res"], pk, mn, sz, mode, inf, ray_valid=v, want_weights=False,
                                       out_ray=_new((B, 16)), tile_T=tile_T, xstash=xs, jstash=js)
        ws = render.scatter_plan(i["o"], i["d"], z, st["res"], T, mn, sz, mode, inf, ray_valid=v, arith=code,
                                 workspace=torch.empty(need(S), dtype=torch.uint8, device=DEV))
        fw.append((z, dist, v, S, mode, inf, tile_T, xs, js, out, ws))
    loss, gfg, gbg = render.photometric_loss_grad_fgbg(fw[0][9], fw[1][9], i["target"], v1, v2, 0.01)
    over, gblob = _new((16, T, 2)), _new((13994,))
    outs = [fw[0][9], fw[1][9], loss]
    for (z, dist, v, S, mode, inf, tile_T, xs, js, out, ws), g in zip(fw, (gfg, gbg)):
        bufs = (_new((B, (S + 31) // 32)), _new((B, 2, 64)))
        ray_pos = _new((B, 6))
        render.render_backward(i["o"], i["d"], z, dist, i["feat"], st["res"], pk, st["wf"], mn, sz, mode, inf, out, tile_T, g, ray_valid=v,
                               grad_blob=gblob, xstash=xs, ray_grad_buffers=bufs, scatter=(ws, over), want_dfeat=False, arith=code,
                               jstash=js, ray_pos_grad=ray_pos)
        outs += list(render.ray_gradients_fused(i["o"], i["d"], i["blob"], ray_pos, *bufs, ray_valid=v))
    P, M, V = i["feat"].clone(), _new((16, T, 2)), _new((16, T, 2))
    render.scatter_accumulate_adam2(fw[0][10], S1, fw[1][10], S2, P, M, V, 1e-2, 0.9, 0.99, 1e-15, 0, B, overflow_grad=over, arith=code)
    return outs + [gblob, P, M, V]


case("fused_fgbg_pose", {"scanerf_sample_points_grid", "scanerf_pack_decoder", "scanerf_render_forward_packed_plan",
                         "scanerf_render_scatter_plan", "scanerf_photometric_loss_grad_fgbg", "scanerf_render_backward",
                         "scanerf_ray_grad_epilogue", "scanerf_render_scatter_accumulate_adam2"},
     lambda seed: _build_fused(512, 2 ** 13, seed, 11), _run_fgbg, setup=_setup_fused(13))


def _build_compact(seed):
    rng = _rng(seed, 12)
    B, S = 1000, 33
    o, d = _rays(rng, B)
    z = rng.uniform(0.1, 5, (B, S)).astype(f32)
    z[rng.random(B) < 0.4, -1] = -1.0
    return {"o": _t(o), "d": _t(d), "z": _t(z), "dist": _t(rng.uniform(0.01, 0.1, (B, S)).astype(f32)), "target": _t(rng.random((B, 3)).astype(f32))}


def _run_compact(st):
    from scanerf_amd import render
    i = st["in"]
    valid = render.ray_valid(i["z"])
    n, *rest = render.compact_rays(valid, i["o"], i["d"], i["target"], i["z"], i["dist"], want_index=True)
    return (valid, *rest)


case("compact", {"scanerf_ray_valid", "scanerf_compact_rays"}, _build_compact, _run_compact,
     host_syncs="render.py:356 (compact_rays reads the count of valid rays)")


# ------------------------------------------------------------------------------------------------------------------ compositing, decoder
def _build_composite(seed):
    from per_ray_reference import family_inputs, upstream
    B, S = 261, 65
    names = ("sigma", "dif", "spec", "tint", "z", "dists", "rays_d")
    inp = dict(zip(names, family_inputs("mixed", B, S, 2000 + seed)))
    inp["sigma"] = inp["sigma"] + 1e-3 * seed     # ("mixed" zeroes a quarter of the rays' densities in every seed)
    inp["go"], inp["gw"] = upstream(B, S, seed=7 + seed)
    inp["go"][:, 15] = 1e-3 * seed
    inp["rays_d"][B - 1] = 1e-3 * seed
    return inp


def _run_composite(st):
    from scanerf_amd import render
    i = st["in"]
    ins = [i[k].detach().clone().requires_grad_(k in ("sigma", "dif", "spec", "tint", "rays_d"))
           for k in ("sigma", "dif", "spec", "tint", "z", "dists", "rays_d")]
    out, w = render.composite_rays(*ins, True)
    ((out * i["go"]).sum() + (w * i["gw"]).sum()).backward()
    return [out.detach(), w.detach()] + [ins[j].grad for j in (0, 1, 2, 3, 6)]


case("composite", {"scanerf_composite_forward", "scanerf_composite_backward"}, _build_composite, _run_composite)


def _build_decoder(seed):
    rng = _rng(seed, 13)
    N = 1000
    return {"feats": _t(rng.normal(size=(N, 32)).astype(f32) * 0.5), "dirs": _t(_rays(rng, N)[1]), "blob": _blob(seed),
            "wf": _t(rng.uniform(0.5, 1.0, 32).astype(f32)), "gw": _t(rng.normal(size=(N, 10)).astype(f32))}


def _run_decoder(st):
    from scanerf_amd import decoder_op
    i = st["in"]
    feats, dirs, blob = (i[k].detach().clone().requires_grad_(True) for k in ("feats", "dirs", "blob"))
    sigma, dif, spec, tint = decoder_op.decoder_apply_parts(feats, dirs, blob, i["wf"])
    allo = torch.cat([sigma.reshape(-1, 1), dif, spec, tint], 1)
    (allo * i["gw"]).sum().backward()
    return allo.detach(), feats.grad, dirs.grad, blob.grad


case("decoder", {"scanerf_decoder_forward", "scanerf_decoder_backward"}, _build_decoder, _run_decoder)


# ------------------------------------------------------------------------------------------------------------------ render-time ops
RT_B, RT_S, RT_SB = 512, 33, 16


def _build_render_time(seed):
    from test_gpu_render_time import _rays as rt_rays
    from test_gpu_render_time import _scene
    rng = _rng(seed, 14)
    sc = _scene(rng)
    o, d = rt_rays(rng, RT_B)
    return {"o": _t(o), "d": _t(d), "occ": _t(sc["occ"]), "tables": _t(sc["tables"]),
            "params": _t(sc["params"] * f32(1.0 + 0.01 * seed)), "T0": _t(rng.uniform(0.2, 1.0, (RT_B, 1)).astype(f32))}


def _setup_render_time(st):
    from test_gpu_render_time import _scene
    sc = _scene(np.random.default_rng(0))      # the geometry of every seed: three overlapping tiles
    on = lambda a: _t(a).to(DEV).contiguous()
    st.update(C=on(sc["corners"]), Z=on(sc["sizes"]), ST=on(sc["starts"]), L2=on(sc["l2d"]), RES=on(sc["res"]), nb=3,
              total=int(sc["occ"].size), cells=[int(np.prod(2 ** sc["l2d"][b])) for b in range(3)])


def _run_render_time(st):
    from scanerf_amd import _capi
    from scanerf_amd import hashgrid as H
    i = st["in"]
    B, S, Sb, nb = RT_B, RT_S, RT_SB, st["nb"]
    RO, RD, OCC, TAB, PAR = i["o"], i["d"], i["occ"], i["tables"], i["params"]
    C, Z, ST, L2, RES = st["C"], st["Z"], st["ST"], st["L2"], st["RES"]
    inter = _new((B, nb, 2), 1e7)
    H.ray_block_intersection(RO, RD, C, Z, inter)
    TB = H.sort_tracing_blocks(inter)
    last = _new((B,), 0, torch.int32)
    H.get_last_block(TB, last, inter)
    hit = _new((B,), 0, torch.int16)
    H.ray_firsthit_block(RO, RD, C, Z, OCC, ST, L2, TB, inter, hit)
    TI, ZS = _new((B,), 0, torch.int32), _new((B,))
    z, dd = _new((B, S), -1.0), _new((B, S), -1.0)
    H.sample_points(RO, RD, C, Z, OCC, ST, L2, TB, inter, TI, ZS, z, dd)
    running = (torch.arange(B, device=DEV) % 3 != 1).contiguous()
    bi = _new((B, S, 4), -1, torch.int16)
    H.prepare_points(z, running, inter, bi)
    fg = [_new((B, S, 3)), _new((B, S, 3)), _new((B, S, 1))]
    H.pts_inference(RO, RD, z, dd, bi, TAB, PAR, RES, OCC, ST, L2, C, Z, *fg)
    tr = [_new((B, S, 3)), _new((B, S, 3)), _new((B, S, 1))]
    H.pts_inference_tracing(RO, RD, z, dd, running, inter, TAB, PAR, RES, OCC, ST, L2, C, Z, *tr)
    pn = _new((B, S, 3))
    H.pts_normals(RO, RD, z, dd, bi, TAB, PAR, RES, OCC, ST, L2, C, Z, pn)
    pn2, counts = _new((B, S, 3)), _new((4,), 0, torch.int32)
    if _capi.has_symbol("scanerf_pts_normals_counted"):
        H.pts_normals(RO, RD, z, dd, bi, TAB, PAR, RES, OCC, ST, L2, C, Z, pn2, counts=counts)
    T0 = i["T0"].clone()
    nm = _new((B, 3))
    H.accumulate_normal(pn, fg[2], T0, z, nm)
    acc = [_new((B, 3)), _new((B, 3)), _new((B, 1))]
    H.accumulate_color(*fg, T0, z, *acc)
    ob, bw = _new((B, 4), -1, torch.int16), _new((B, 4))
    H.update_outgoing_bidx(RO, RD, C, Z, TB, inter, ob, bw, 0.12, False)
    ob2, bw2 = _new((B, 4), -1, torch.int16), _new((B, 4))
    H.update_outgoing_bidx_v2(RO, RD, C, Z, TB, inter, ob2, bw2)
    zb = _new((B, Sb), -1.0)
    H.inverse_z_sampling(inter, ob[:, 0].contiguous(), zb, 1e6)
    bg = [_new((B, Sb, 3)), _new((B, Sb, 3)), _new((B, Sb, 1))]
    H.bg_pts_inference_v2(RO, RD, zb, ob, 0, C, Z, RES, TAB, PAR, *bg)
    tgt = OCC.clone()
    for b in range(nb):
        H.process_occupied_grid(b, st["cells"][b], C, Z, OCC, ST, L2, tgt)
    return [inter, TB, last, hit, TI, ZS, z, dd, bi, *fg, *tr, pn, pn2, counts, T0, nm, *acc, ob, bw, ob2, bw2, zb, *bg, tgt]


case("render_time", {"scanerf_ray_block_intersection", "scanerf_sort_tracing_blocks", "scanerf_get_last_block", "scanerf_ray_firsthit_block",
                     "scanerf_render_sample_points", "scanerf_prepare_points", "scanerf_pts_inference", "scanerf_pts_inference_tracing",
                     "scanerf_pts_normals", "scanerf_pts_normals_counted", "scanerf_accumulate_normal", "scanerf_accumulate_color",
                     "scanerf_update_outgoing_bidx", "scanerf_update_outgoing_bidx_v2", "scanerf_render_inverse_z_sampling",
                     "scanerf_bg_pts_inference_v2", "scanerf_process_occupied_grid", "scanerf_pack_decoder"},
     _build_render_time, _run_render_time, setup=_setup_render_time, optional={"scanerf_pts_normals_counted"})


# ------------------------------------------------------------------------------------------------------------------ normals at points and along rays
def _normals_case(seed):
    import normals_reference as NR
    return NR.Case("base", 261, 33, 12, False, False, "all", 500 + seed)


def _build_normals(seed):
    import normals_reference as NR
    ins = NR.case_inputs(_normals_case(seed))
    rng = _rng(seed, 15)
    return {"o": _t(ins["o"]).float(), "d": _t(ins["d"]).float(), "z": _t(ins["z"]).float(), "dist": _t(ins["dist"]).float(),
            "table": _t(ins["table"]).float(), "blob": O.pack_blob(ins["sd"]).float(), "x": _t(rng.uniform(-2, 2, (1000, 3)).astype(f32))}


def _setup_normals(st):
    import normals_reference as NR
    ins = NR.case_inputs(_normals_case(1))
    st.update(res=ins["res"].to(DEV).contiguous(), wf=NR.case_mask(ins).to(DEV), mn=ins["mn"].tolist(), sz=ins["sz"].tolist(),
              ascale=NR.ascale_of(ins["sz"]).tolist())


def _run_normals(st):
    from scanerf_amd import render
    i = st["in"]
    out, sn = render.render_normals(i["o"], i["d"], i["z"], i["dist"], i["table"], st["res"], i["blob"], st["wf"], st["mn"], st["sz"], False,
                                    want_sample_normals=True)
    sigma, grad, normal = render.sigma_normals_points(i["x"], i["table"], st["res"], i["blob"], st["wf"], axis_scale=st["ascale"], want_grad=True)
    return out, sn, sigma, grad, normal


case("normals", {"scanerf_render_normals", "scanerf_sigma_normals_points"}, _build_normals, _run_normals, setup=_setup_normals)


# ------------------------------------------------------------------------------------------------------------------ scene arrays (3 tiles)
def _build_scene(seed):
    from test_gpu_render_time import _scene
    rng = _rng(seed, 16)
    sc = _scene(rng)
    pts = np.stack([rng.uniform(-4, 6, 1000), rng.uniform(-2, 2, 1000), rng.uniform(-2, 2, 1000)], 1).astype(f32)
    return {"tables": _t(sc["tables"]), "params": _t(sc["params"] * f32(1.0 + 0.01 * seed)), "occ": _t(sc["occ"]), "pts": _t(pts)}


def _scene_tiles(st):
    i = st["in"]
    return (i["tables"], st["RES"], i["params"], st["C"], st["Z"], i["occ"], st["ST"], st["L2"])


def _run_scene_normals(st):
    from scanerf_amd import meshing
    sigma, grad, normal = meshing.scene_sigma_normals_points(st["in"]["pts"], *_scene_tiles(st), want_grad=True)
    return sigma, grad, normal


case("scene_normals", {"scanerf_scene_sigma_normals_points"}, _build_scene, _run_scene_normals, setup=_setup_render_time)

SYNC_TOTALS = "meshing.py:51 (_totals reads V and F between the count and the emit pass)"


def _mesh_out(m):
    return [m.vertices, m.faces, m.cells, m.lattice] + ([m.normals] if m.normals is not None else [])


def _setup_scene_mesh(st):
    _setup_render_time(st)
    from scanerf_amd import meshing
    corner, size, n = [-4.0, -2.0, -2.0], [10.0, 4.0, 4.0], (24, 16, 16)
    field = meshing._scene_field_dense(*_scene_tiles(st), corner, size, n)
    live = field[field > 0]
    st.update(corner=corner, size=size, n=n, level=float(np.median(live)))


def _run_scene_mesh(st):
    from scanerf_amd import meshing
    m = meshing.extract_scene_mesh(*_scene_tiles(st), st["corner"], st["size"], st["n"], st["level"])
    return _mesh_out(m)


case("scene_mesh", {"scanerf_isosurface_count_tiles", "scanerf_isosurface_emit_tiles"}, _build_scene, _run_scene_mesh,
     setup=_setup_scene_mesh, host_syncs=SYNC_TOTALS)


# ------------------------------------------------------------------------------------------------------------------ isosurface of one tile, dense op
def _build_iso_dense(seed):
    import surface_nets_reference as SR
    return {"values": _t(SR.sphere_values((19, 18, 17), (8.0 + 0.25 * seed, 8.0, 8.0), 5.3))}


def _run_iso_dense(st):
    from scanerf_amd import meshing
    return _mesh_out(meshing.surface_nets(st["in"]["values"], 1.0, (1.5, -2.0, 0.25), (0.5, 0.25, 2.0)))


case("isosurface_dense", {"scanerf_isosurface_count_dense", "scanerf_isosurface_emit_dense"}, _build_iso_dense, _run_iso_dense,
     host_syncs=SYNC_TOTALS)


def _iso_case(seed):
    import surface_nets_reference as SR
    return SR.ModelCase("base", False, (20, 18, 16), (4, 4, 4), "half", 0.5, 700 + seed)


def _build_iso_model(seed):
    import surface_nets_reference as SR
    ins = SR.model_inputs(_iso_case(seed))
    return {"table": _t(ins["table"]).float(), "blob": O.pack_blob(ins["sd"]).float()}


def _setup_iso_model(st):
    import surface_nets_reference as SR
    from scanerf_amd import meshing, render
    c = _iso_case(1)
    ins = SR.model_inputs(c)
    st.update(res=ins["res"].to(DEV).contiguous(), wf=SR.NR.case_mask(ins).to(DEV), occ=torch.from_numpy(ins["occ"]).to(DEV),
              l2d=list(c.log2dim), corner=ins["occ_corner"].tolist(), size=ins["occ_size"].tolist(), n=list(c.n))
    sigma, _, _ = render.sigma_normals_points(meshing.lattice_positions(st["n"], DEV), st["in"]["table"], st["res"], st["in"]["blob"], st["wf"])
    st["level"] = max(float(sigma.median()), 1e-6)


def _run_iso_model(st):
    from scanerf_amd import meshing
    i = st["in"]
    m = meshing.extract_mesh(i["table"], st["res"], i["blob"], st["wf"], st["occ"], st["l2d"], st["corner"], st["size"], st["n"], st["level"])
    return _mesh_out(m)


case("isosurface_model", {"scanerf_isosurface_count", "scanerf_isosurface_emit"}, _build_iso_model, _run_iso_model,
     setup=_setup_iso_model, host_syncs=SYNC_TOTALS)


# ------------------------------------------------------------------------------------------------------------------ mesh components and filter
def _build_components(seed):
    """The surface-nets mesh of two spheres and a floater (tests/mesh_components_reference.py's lattices are built the same way); the
    seeds move the spheres, so the face list, its length and every label differ."""
    import surface_nets_reference as SR
    n = (22, 20, 18)
    v = np.maximum(SR.sphere_values(n, (6.0 + seed, 7.0, 8.0), 4.2), SR.sphere_values(n, (16.0, 12.0 + seed, 9.0), 3.1))
    v = np.maximum(v, SR.sphere_values(n, (19.0, 3.0, 3.0 + seed), 1.2))
    m = SR.surface_nets(v, 1.0, dtype=np.float32)
    V, F = len(m.vertices), len(m.faces)
    VMAX, FMAX = 1600, 3200
    assert V <= VMAX and F <= FMAX, (V, F)
    pad = lambda a, rows, dt: np.concatenate([np.asarray(a, dt), np.zeros((rows - len(a), 3), dt)])
    # (fixed shapes for refill: the rows behind V / F are unused vertices and degenerate faces on vertex 0, both legal)
    return {"vertices": _t(pad(m.vertices, VMAX, f32) + f32(1e-3 * seed)), "lattice": _t(pad(m.lattice, VMAX, f32) + f32(1e-3 * seed)),
            "cells": _t(pad(m.cells, VMAX, np.int32)), "faces": _t(pad(m.faces, FMAX, np.int32))}


def _run_components(st):
    from scanerf_amd import meshing
    i = st["in"]
    V = i["vertices"].shape[0]
    comps = meshing.mesh_components(i["faces"], V, i["cells"])
    mesh = meshing.Mesh(i["vertices"], i["faces"], i["cells"], i["lattice"], None)
    kept = meshing.filter_mesh(mesh, min_faces=8, keep_largest=2)
    return list(comps) + _mesh_out(kept)


case("mesh_components", {"scanerf_mesh_components_label", "scanerf_mesh_components_table", "scanerf_mesh_filter_count",
                         "scanerf_mesh_filter_emit"}, _build_components, _run_components,
     int_ranges={"cells": (0, 64), "faces": (0, 1600)},
     host_syncs="meshing.py:397 (the public functions' range check of the face indices reads their minimum and maximum)")


# ------------------------------------------------------------------------------------------------------------------ mesh tracer, coverage, distances
def _terrain(seed):
    import fastmesh_reference as FR
    return FR.terrain_fixture(seed=7 + seed)


def _build_mesh_build(seed):
    V, F, _ = _terrain(seed)
    return {"V": _t(V), "F": _t(F)}


def _run_mesh_build(st):
    from scanerf_amd.fastmesh import FastMesh
    i = st["in"]
    fm = FastMesh.from_arrays(i["V"], i["F"], DEV, log2dim=5, pregather=True)
    return fm.cell_faces, fm.start_num, fm.bitmask, fm.rank, fm.cell_box, fm.tris


case("mesh_build", {"scanerf_mesh_count_cells", "scanerf_mesh_emit_keys", "scanerf_mesh_cell_boxes", "scanerf_mesh_gather_triangles"},
     _build_mesh_build, _run_mesh_build, int_ranges={"F": (0, 2497)},
     host_syncs="fastmesh.py:78 (_build reads the number of (face, cell) pairs)")


def _build_mesh_trace(seed):
    import tile_allocation_reference as TR
    _, _, rays = _terrain(seed)
    (o, d), (oo, dd) = rays["inside"], rays["outside"]
    ks, c2ws = TR.cameras()
    rng = _rng(seed, 17)
    f = TR.fixture()
    centers = f["corners"] + f["tile_size"] / 2 + rng.uniform(-0.5, 0.5, (len(f["corners"]), 3)).astype(f32)
    return {"o": _t(np.concatenate([o[:768], oo[:256]])), "d": _t(np.concatenate([d[:768], dd[:256]])), "pts": _t(o[:1024] + f32(0.01 * seed)),
            "ks": _t(ks * f32(1.0 + 0.01 * seed), torch.float32), "c2ws": _t(c2ws + f32(0.01 * seed), torch.float32), "centers": _t(centers, torch.float32),
            "sizes": _t(np.tile(f["tile_size"][None], (len(centers), 1)) + f32(0.01 * seed), torch.float32)}


def _setup_mesh_trace(st):
    import tile_allocation_reference as TR
    from scanerf_amd.fastmesh import FastMesh
    V, F = TR.mesh()
    st["fm"] = FastMesh.from_arrays(V, F, DEV)
    st["fm_indexed"] = FastMesh.from_arrays(V, F, DEV, log2dim=5, pregather=False)
    st["H"], st["W"] = TR.H, TR.W


def _run_mesh_trace(st):
    from scanerf_amd import _capi, allocation
    i, fm = st["in"], st["fm"]
    hit, enter = fm.first_hit(i["o"], i["d"]), fm.first_enter(i["o"], i["d"])
    hit2 = st["fm_indexed"].first_hit(i["o"], i["d"])
    counts = allocation.view_coverage(fm, i["ks"], i["c2ws"], st["H"], st["W"], i["centers"], i["sizes"], scale=4)
    d1, f1, q1 = fm.closest_point(i["pts"])
    d2, f2, q2 = fm.closest_point(i["pts"], route="brute", max_dist=3.0)
    outs = [hit, enter, hit2, counts, d1, f1, q1, d2, f2, q2]
    if _capi.has_symbol("scanerf_mesh_closest_point_counted"):
        N = i["pts"].shape[0]
        dist2, face, closest, cnt = _new((N,)), _new((N,), 0, torch.int32), _new((N, 3)), _new((N, 2), 0, torch.int32)
        _call("scanerf_mesh_closest_point_counted", _p(i["pts"]), N, _p(fm.vertices), _p(fm.faces), _p(fm.tris), _p(fm.bitmask), _p(fm.rank),
              _p(fm.start_num), _p(fm.cell_faces), _p(fm.cell_box), _p(fm.scene_info), fm.log2dim, float("inf"), _p(dist2), _p(face),
              _p(closest), _p(cnt))
        outs += [dist2, face, closest, cnt]
    return outs


case("mesh_trace", {"scanerf_mesh_first_hit", "scanerf_mesh_first_enter", "scanerf_view_coverage", "scanerf_mesh_closest_point",
                    "scanerf_mesh_closest_point_brute", "scanerf_mesh_closest_point_counted"}, _build_mesh_trace, _run_mesh_trace,
     setup=_setup_mesh_trace, optional={"scanerf_mesh_closest_point_counted"})


def _build_voxelize(seed):
    V, F, _ = _terrain(seed)
    return {"V": _t(V), "F": _t(F)}


def _run_voxelize(st):
    import ctypes
    i = st["in"]
    vis, outside = _new((16, 16, 16), False, torch.bool), _new((16, 16, 16), False, torch.bool)
    scratch = _new((6,), 0, torch.int32)
    _call("scanerf_voxelize_mesh", _p(i["V"]), _p(i["F"]), i["V"].shape[0], i["F"].shape[0], (ctypes.c_int32 * 3)(4, 4, 4),
          (ctypes.c_float * 3)(-8.0, -8.0, -4.0), (ctypes.c_float * 3)(16.0, 16.0, 8.0), _p(vis), 1, _p(outside), _p(scratch))
    return vis, outside


case("voxelize", {"scanerf_voxelize_mesh"}, _build_voxelize, _run_voxelize, int_ranges={"F": (0, 2497)})


# ------------------------------------------------------------------------------------------------------------------ warp and mono losses
WARP_N, WARP_B, WARP_K = 12, 512, 10


def _build_warp(seed):
    import warp_cases as WC
    sc = WC.scene(WARP_N, WARP_B, seed=300 + seed, ray_valid="mixed")
    score = torch.rand(WARP_B, WARP_K, generator=torch.Generator().manual_seed(seed))
    return {"ks": sc.ks.reshape(-1, 9) * (1.0 + 1e-3 * seed), "rts": sc.rts.reshape(-1, 12), "images": sc.images, "occ": sc.occlusions, "o": sc.rays_o,
            "d": sc.rays_d, "q": sc.q, "valid": sc.ray_valid, "score": score}


def _run_warp(st):
    i = st["in"]
    N, B, K, H, W = WARP_N, WARP_B, WARP_K, i["images"].shape[1], i["images"].shape[2]
    views, cost, nv = _new((B, K), 0, torch.int32), _new((B, K)), _new((B, K), 0, torch.uint8)
    _call("scanerf_warp_select_views", _p(i["o"]), _p(i["d"]), _p(i["q"]), _p(i["valid"]), _p(i["ks"]), _p(i["rts"]), N, H, W, K, B,
          _p(views), _p(cost), _p(nv))
    grid, pd, no, nd, col, pv = _new((B, K, 2)), _new((B, K)), _new((B, K, 3)), _new((B, K, 3)), _new((B, K, 3)), _new((B, K), 0, torch.uint8)
    _call("scanerf_warp_project", _p(i["o"]), _p(i["d"]), _p(i["q"]), _p(i["ks"]), _p(i["rts"]), _p(views), _p(nv), _p(i["images"]),
          _p(i["occ"]), N, H, W, K, B, _p(grid), _p(pd), _p(no), _p(nd), _p(col), _p(pv))
    n = _lib().scanerf_warp_scratch_floats(B, K, N)
    scratch = _new((n,))
    loss, gq, go, gd, grts = _new((1,)), _new((B, 7)), _new((B, 3)), _new((B, 3)), _new((N, 3, 4))
    _call("scanerf_warp_loss_grad", _p(i["o"]), _p(i["d"]), _p(i["q"]), _p(i["valid"]), _p(i["ks"]), _p(i["rts"]), _p(views), _p(pv),
          _p(grid), _p(col), _p(i["score"]), _p(i["images"]), N, H, W, K, B, 1.0, _p(loss), _p(gq), _p(go), _p(gd), _p(grts), _p(scratch), n)
    return views, cost, nv, grid, pd, no, nd, col, pv, loss, gq, go, gd, grts


case("warp", {"scanerf_warp_select_views", "scanerf_warp_project", "scanerf_warp_loss_grad"}, _build_warp, _run_warp)

MONO_N, MONO_H, MONO_W = 8, 24, 32


def _build_mono(seed):
    from test_gpu_mono import random_batch
    depth, locs, valid, md, mn, kinv = random_batch(N=MONO_N, Bc=64, H=MONO_H, W=MONO_W, seed=seed)
    return {"depth": depth.float(), "locs": locs.int(), "valid": valid, "md": md.float(), "mn": mn.float(),
            "kinv": kinv.reshape(MONO_N, 9).float() * (1.0 + 1e-3 * seed)}


def _run_mono(st):
    i = st["in"]
    B = i["depth"].shape[0]
    n = _lib().scanerf_mono_scratch_floats(B, MONO_N)
    loss, grad, scratch = _new((3,)), _new((B,)), _new((n,))
    _call("scanerf_mono_loss_grad", _p(i["depth"]), _p(i["valid"]), _p(i["locs"]), _p(i["md"]), _p(i["mn"]), _p(i["kinv"]), MONO_N, MONO_H,
          MONO_W, B, 0.7, 0.3, _p(loss), _p(grad), _p(scratch), n)
    return loss, grad


case("mono", {"scanerf_mono_loss_grad"}, _build_mono, _run_mono, int_ranges={"locs": [(0, MONO_N), (0, MONO_W), (0, MONO_H)]})


# ------------------------------------------------------------------------------------------------------------------ test-infrastructure exports
def _build_infra(seed):
    rng = _rng(seed, 18)
    n = 2000
    gx = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(f32)
    return {"blob": _blob(seed), "dy": _t(rng.normal(size=(64, 32)).astype(f32)),
            "x": _t((rng.normal(size=(64, 32)) * rng.uniform(0.01, 2.0, (64, 1))).astype(f32)), "gx": _t(gx),
            "gy": _t((rng.normal(size=n) * np.abs(gx)).astype(f32)), "tx": _t(rng.uniform(0, 1, size=n).astype(f32)),
            "l0": _t(rng.integers(0, 8192, size=n).astype(np.int32)), "k": _t(rng.integers(0, 13, size=n).astype(np.int32)),
            "table": torch.zeros(1 << 16, 2, dtype=torch.int32)}


def _setup_infra(st):
    from scanerf_amd import render
    st["packed"] = render.PackedDecoder(DEV)
    st["ones"] = torch.ones(32, device=DEV)


def _run_infra(st):
    import ctypes

    from scanerf_amd import _capi
    i = st["in"]
    outs = []
    if _capi.has_symbol("scanerf_h3_selftest"):
        pk = st["packed"].pack(i["blob"], st["ones"])
        dx, dw, rs = _new((2, 64, 32)), _new((64, 64)), _new((64,))
        _call("scanerf_h3_selftest", _p(pk.workspace), _p(i["dy"]), _p(i["x"]), _p(dx), _p(dw), _p(rs))
        outs += [dx, dw, rs]
    if _capi.has_symbol("scanerf_rec8_selftest"):
        n = i["gx"].shape[0]
        words, out = _new((n, 2), 0, torch.int32), _new((n, 8))
        _call("scanerf_rec8_selftest", _p(i["gx"]), _p(i["gy"]), _p(i["tx"]), _p(i["l0"]), _p(i["k"]), n, _p(words), _p(out))
        outs += [words, out]
    if _capi.has_symbol("scanerf_gather_rate_probe"):
        sink = _new((64,), 0, torch.int32)
        _call("scanerf_gather_rate_probe", _p(i["table"]), i["table"].shape[0], 8, 8, ctypes.c_void_p(sink.data_ptr()))
        outs.append(sink)
    if _capi.has_symbol("scanerf_icache_sweep"):
        _call("scanerf_icache_sweep")
    return outs


case("test_infrastructure", {"scanerf_h3_selftest", "scanerf_rec8_selftest", "scanerf_gather_rate_probe", "scanerf_icache_sweep",
                             "scanerf_pack_decoder"}, _build_infra, _run_infra, setup=_setup_infra,
     int_ranges={"l0": (0, 8192), "k": (0, 16), "table": (0, 1 << 30)},
     optional={"scanerf_h3_selftest", "scanerf_rec8_selftest", "scanerf_gather_rate_probe", "scanerf_icache_sweep"})

# Entries that truly cannot be called at a small shape: name -> one sentence.  None.
EXEMPT = {}

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
