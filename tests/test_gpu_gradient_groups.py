"""Training gradients judged PER GROUP -- every table level, every named decoder tensor -- against the position-pinned float64
reference (tests/gradient_reference64.py), through every route a gradient takes to the table.  Needs an MI355X: `pytest -m gpu`.

Why per group: normalising by the global maximum or the global L2 lets a whole level or a small decoder tensor be wrong by
several per cent, and at the steps the other gradient tests run the coarse-to-fine mask hides the finest levels altogether.
Why float64: the float32 oracle's autograd is itself off by ~3.6e-6 relative L2 per level -- as much as the kernels.

Bounds (none taken from what the kernels give):
  * arith f32 / h3 / t16s: relative L2 of a group <= 8 * max(e32[group], e32 of that kind pooled), where e32 is the float32
    oracle's error against the same reference, computed here on the CPU for the same inputs.  8 = 4 (22-bit split-f16 operands
    against float32's 24) x 2 (another summation order).  e32[group] itself is in the max because a group that cancels (a bias
    whose sum nearly vanishes) is as ill-conditioned for the kernel as for the oracle.
  * arith t16 (one f16 product per gradient term): the project's 2e-3, flat, for every group against its own norm.  One group by
    name is measured against another scale, see CANCELLING_BIAS: sigma_layer.mlp.0.bias, the only scalar among the groups.
  * inputs: the foreground generator of the parity tests puts 1.7 % of its samples outside the encoder's domain [-2, 2]^3.
    render_backward's dfeat is judged on them as they are, and so is the default (16-byte-record) stand-alone scatter of
    test_backward_groups: include/scanerf_hip.h (Domain) declares the binned routes defined for in-domain points only, in every
    record format, so that one assertion records an observation -- today those records extrapolate like the reference, which
    tests/test_gpu_parity.py relies on for the same inputs -- not a documented property; should it stop holding, that step
    wants BackwardCase(in_domain=True) like the rest.  Every other table route (the stand-alone formats 0 / 1 / 2, atomics, the
    fused records, the rays scatter) gets the same inputs with the rays owning such a sample masked out through ray_valid.
  * compact record formats add their component widths (csrc/scatter_common.h) to the TABLE groups' bounds, see REC_EXTRA.
  * without an x-stash the 16-sample-tile kernels cannot run and the h3 backward serves the call under every arithmetic: the
    re-gather backward is judged under h3 and f32, once, not again under t16s / t16.
  * a masked level (weight_feature exactly 0) is exactly zero; through the Adam routes its parameters and moments keep their bits.
Each test prints its per-group table (pytest -s); profiles/gradient_error_by_group.md holds one copy."""
import functools

import numpy as np
import pytest
import torch

import gradient_reference64 as R64
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32_FACTOR = 8.0
T16_BOUND = 2e-3
LR, B1, B2, EPS = 1e-2, 0.9, 0.99, 1e-15
# What a compact record adds to a level's relative L2, beyond the 16-byte records' exact products (format 0, and -1 = the
# layout's default).  Documented component widths (csrc/scatter_common.h): 2^-13 (Rec8) and 2^-20 (Rec12) per record.
#   format 1 (Rec8): both components as 12-bit significands + sign under the exponent E of the larger one, m in [2^(E-1), 2^E):
#     one unit is 2^(E-12) <= 2^-11 m, half a unit (the documented "2^-13 .. 2^-12 of the larger component") bounds the rounding
#     error, which is uniform: rms <= 2^-11 m / sqrt(12) per component.  Two components against |g| >= m: the record is off by
#     <= 2^-11 / sqrt(6) of its norm in rms, i.e. squared 2^-26 * 8/3.  The 13-bit x-weight t: error uniform within 2^-14, rms
#     2^-14 / sqrt(3), moves g * dt from one entry of the pair to the other: 2 g^2 2^-28 / 3 against the record's
#     g^2 (w0^2 + w1^2) >= g^2 / 2: squared 2^-26 / 3.  Together 2^-26 * 3: sqrt(3) * 2^-13 = 2.11e-4 per record.  Records round
#     independently, and a level's reference norm adds up in quadrature over the same records (independent upstream gradients),
#     so a level carries at most the per-record figure.  The documented bare width 2^-13 = 1.22e-4 is NOT the term: it is the
#     rounding bound of ONE component at the top of its binade (half a unit 2^(E-13) against m -> 2^E).  A record has two rounded
#     components and a rounded weight, and m may sit at the bottom of the binade, where the same half unit is 2^-12 of it; the
#     rms over the three uniform errors at that worst position is the sqrt(3) * 2^-13 above.  With the bare width a correct
#     Rec8 encoder would be refused (f32-grade dfeat through format 1 gives 1.3e-4 .. 1.55e-4 against 8 * e32 + 1.22e-4 =
#     1.50e-4): the factor follows from the format's three rounded fields, it is not fitted to that figure.
#   format 2 (Rec12; also the 64-byte segments of the large-table producer, format 3): 19 stored mantissa bits, round to
#     nearest: the same argument gives 2^-19 / sqrt(6) for the components and 2^-24 * 2 / sqrt(3) for the 23-bit weight,
#     7.9e-7 together: below the documented 2^-20, which is used.
REC_EXTRA = {-1: 0.0, 0: 0.0, 1: 3.0 ** 0.5 * 2.0 ** -13, 2: 2.0 ** -20}
# The one group t16 is not judged against its own norm.  sigma_layer.mlp.0 has ONE output, so its bias gradient is one scalar:
# sum_n delta_n over every sample, of both signs.  Each term carries t16's relative rounding (one f16 product, 2^-11) of ITS
# size, so the sum's absolute error grows with sqrt(sum delta_n^2) whatever the sum cancels to -- and at fg, S = 128, step 12000
# it cancels to 0.019, 0.9 % of the layer's scale (the float32 oracle is 9.1e-5 off on it there against 2e-6 elsewhere, t16
# 9.3e-3; at every other case, and for every other group of all cases, t16 stays below 2e-3 of the group's own norm).  A bias
# is one more input column of its layer (x = 1), so the scale of its rounding is that of a typical column of the weight
# gradient sum_n delta_n x_n^T: the group is measured against the larger of its own norm and the weight gradient's rms column
# norm |dW| / sqrt(fan_in) -- the rule tests/test_gradient_reference_cpu.py holds the float32 oracle's biases to -- and the
# flat 2e-3 applies to that figure (the case above: 1.8e-4 absolute against 0.37, 5e-4).  Every vector bias keeps its own norm.
CANCELLING_BIAS = "decoder/sigma_layer.mlp.0.bias"


@pytest.fixture(scope="module")
def S():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    _capi.lib()  # fail loudly if the HIP library is missing
    return scanerf_amd


def g(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def _kinds(r, kinds=("dfeat", "table", "decoder")):
    conv = {"dfeat": lambda: R64.level_major(r["dfeat"]), "table": lambda: r["table"], "decoder": lambda: r["decoder"]}
    return {k: conv[k]() for k in kinds}


@functools.lru_cache(maxsize=None)
def _case(bg, S_, step, B=200, log2_T=12, invalid_every=0, table_dtype=torch.float32, in_domain=False):
    """(inputs, float64 reference, e32 = the float32 oracle's per-group error against it) -- computed once per input set."""
    case = R64.BackwardCase(bg, S_, step, B=B, log2_T=log2_T, invalid_every=invalid_every, table_dtype=table_dtype, in_domain=in_domain)
    assert case.valid.sum() > 0.7 * case.B
    ref = case.reference64()
    e32 = R64.group_errors(_kinds(case.oracle32()), _kinds(ref))
    return case, ref, e32


def _bounds(e32, names, arith, extra=0.0):
    """extra: what the record format adds -- to the table groups only, no other gradient passes through records."""
    out = {}
    for n in names:
        if not n.endswith("/*"):
            kind = e32[n]["kind"]
            pooled = e32[kind + "/*"]["rel_l2"]
            out[n] = T16_BOUND if arith == "t16" else F32_FACTOR * max(e32[n]["rel_l2"], pooled) + (extra if kind == "table" else 0.0)
    return out


def _judged(name, errs, arith):
    """The figure the bound applies to: the group's relative L2, but for CANCELLING_BIAS under t16 (see there)."""
    v = errs[name]
    if arith == "t16" and name == CANCELLING_BIAS:
        layer = name[len("decoder/"):-len(".bias")]
        fan_in = next(i for n, _, i in O.MLP_LAYERS if n == layer)
        return v["err_norm"] / max(v["ref_norm"], errs[f"decoder/{layer}.weight"]["ref_norm"] / fan_in ** 0.5)
    return v["rel_l2"]


def _judge(title, got, ref, e32, arith, masked=(), extra=0.0):
    """Print the per-group table of `got` against `ref` (kinds of got) and assert every group: masked levels exactly zero, every
    other group with a non-zero reference norm and within its bound.  The failure names the groups."""
    errs = R64.group_errors(got, {k: ref[k] for k in got})
    bounds = _bounds(e32, errs, arith, extra)
    print("\n" + R64.format_table(f"{title} [arith {arith}]", errs, bounds, e32))
    bad = []
    for name, v in errs.items():
        if name.endswith("/*"):
            continue
        lvl = int(name[-2:]) if "/L" in name else None
        if lvl is not None and lvl in masked:
            assert v["ref_norm"] == 0.0, name
            if v["err_norm"] != 0.0:
                bad.append(f"{name}: masked level is not exactly zero (norm {v['err_norm']:.3e})")
            continue
        assert v["ref_norm"] > 0.0, f"{title}: {name} has no reference gradient -- the case does not judge it"
        rel = _judged(name, errs, arith)
        if rel != v["rel_l2"]:
            print(f"{name}: judged against its layer's scale: {rel:.2e}")
        if not rel <= bounds[name]:
            bad.append(f"{name}: relative L2 {rel:.3e} > {bounds[name]:.3e} (e32 {e32[name]['rel_l2']:.2e})")
    assert not bad, f"{title} [arith {arith}]: " + "; ".join(bad)
    return errs


class _Gpu:
    """One BackwardCase on the device: forward (with or without the x-stash), then backward(...) as often as wanted."""

    def __init__(self, case, xstash=True, table=None):
        from scanerf_amd import network, render
        self.case, self.render = case, render
        B, S_ = case.B, case.S
        self.o, self.d, self.z, self.dist = g(case.o), g(case.d), g(case.z), g(case.dist)
        self.table = (case.table if table is None else table).to(DEV).contiguous()
        self.R = g(case.res.numpy())
        self.valid = None if case.valid.all() else g(case.valid)
        self.wf = network.weight_feature(case.step, DEV)
        assert torch.equal(self.wf.cpu()[::2], O.weight_feature(case.step))   # the mask values the reference pins
        self.skip = network.skip_levels(case.step)
        assert [l for l in range(16) if self.skip >> l & 1] == case.masked
        self.pk = render.PackedDecoder(DEV).pack(O.pack_blob(case.sd).to(DEV), self.wf, self.skip)
        self.box = (case.mn.tolist(), case.sz.tolist(), render.BG if case.bg else render.FORE, case.bg)
        self.tile_T = torch.empty(B, render.tile_T_columns(S_), device=DEV)
        self.xs = torch.empty(B * S_, 32, device=DEV) if xstash else None
        self.out, _ = render.render_forward(self.o, self.d, self.z, self.dist, self.table, self.R, self.pk, *self.box,
                                            ray_valid=self.valid, want_weights=False, tile_T=self.tile_T, xstash=self.xs)
        self.gout = torch.zeros(B, 16, device=DEV)
        self.gout[:, 0:3], self.gout[:, 3], self.gout[:, 4] = g(case.g_rgb), g(case.g_depth[:, 0]), g(case.g_T)
        self.gout[:, 14] = case.G_L2

    def backward(self, scatter=None, want_dfeat=True):
        return self.render.render_backward(self.o, self.d, self.z, self.dist, self.table, self.R, self.pk, self.wf, *self.box,
                                           self.out, self.tile_T, self.gout, ray_valid=self.valid, xstash=self.xs, scatter=scatter,
                                           want_dfeat=want_dfeat)

    def plan(self, own=False):
        """Reserve the fused records' ranges for this batch (own: a workspace of this call's own, for two plans alive at once)."""
        render, c = self.render, self.case
        assert render.scatter_supported(c.B, c.S, c.T)
        ws = None
        if own:
            ws = torch.empty(render.lib().scanerf_render_scatter_workspace_bytes(c.B, c.S, c.T), dtype=torch.uint8, device=DEV)
        return render.scatter_plan(self.o, self.d, self.z, self.R, c.T, *self.box, ray_valid=self.valid, workspace=ws,
                                   skip_levels=self.skip)

    def points(self):
        """The contracted sample points, pinned: the oracle's own float32 values."""
        c = self.case
        return g(R64.pinned_points(c.o, c.d, c.z, c.bg, c.mn, c.sz))

    def valid_samples(self, dfeat):
        """(points, dfeat) of the valid rays' samples only: what a stand-alone scatter of in-domain points is handed."""
        keep = g(np.repeat(self.case.valid, self.case.S))
        return self.points()[keep].contiguous(), dfeat[:, keep].contiguous()


def _decoder(gblob):
    return {k: v.clone() for k, v in O.unpack_blob(gblob.detach().cpu()).items()}


def _with_arith(arith, fn, *a):
    from scanerf_amd import render
    render.set_arith(arith)
    try:
        return fn(*a)
    finally:
        render.set_arith(render.DEFAULT_ARITH)


def _moment_gradient(m1):
    """The gradient an Adam route saw: its first moment after one step from zero moments is (1 - beta1) * g."""
    return m1.detach().cpu().double() / (1.0 - B1)


def _assert_masked_untouched(case, P, P0, M, V, what):
    for l in case.masked:
        assert torch.equal(P[l], P0[l]), f"{what}: parameters of masked level {l} moved"
        assert not bool(M[l].any()) and not bool(V[l].any()), f"{what}: moments of masked level {l} moved"
    open_levels = [l for l in range(16) if l not in case.masked]
    assert all(bool(M[l].any()) for l in open_levels), f"{what}: an open level got no update"


# --------------------------------------------------------------------------------------------------- backward: dfeat, decoder
SHAPES = {"fg64": (False, 64), "bg40": (True, 40), "fg128": (False, 128)}
BACKWARD_CASES = [(k, step, {}) for k in SHAPES for step in (12000, 5600, 0)] + \
    [("fg33odd", 12000, dict(B=37, invalid_every=5)), ("bg33odd", 12000, dict(B=37, invalid_every=5))]
SHAPES.update(fg33odd=(False, 33), bg33odd=(True, 33))


def _backward_groups(shape, step, kw, arith):
    case, ref, e32 = _case(*SHAPES[shape], step, **kw)
    tag = f"{shape} step {step} table {str(case.table.dtype)[6:]}"
    refk = _kinds(ref)
    results = {}
    # without an x-stash the 16-sample-tile kernels cannot run: the h3 backward serves the call under t16s / t16 as well, the
    # same computation as under h3, where it is judged
    for xstash in ((False, True) if arith in ("h3", "f32") else (True,)):
        run = _Gpu(case, xstash=xstash)
        dfeat, gblob = run.backward()
        how = "x-stash" if xstash else "re-gather"
        _judge(f"render_backward dfeat + decoder, {how}, {tag}", {"dfeat": dfeat, "decoder": _decoder(gblob)}, refk, e32, arith,
               case.masked)
        results[xstash] = (run, dfeat)
    # the table gradient through the stand-alone binned scatter (default records), from the x-stash backward's dfeat
    run, dfeat = results[True]
    gF = run.render.scatter_table_grad(run.points(), dfeat, torch.zeros(16, case.T, 2, device=DEV), run.R)
    _judge(f"table gradient, stand-alone binned scatter, {tag}", {"table": gF}, refk, e32, arith, case.masked)


@pytest.mark.parametrize("arith", ["h3", "t16s", "t16"])
@pytest.mark.parametrize("shape,step,kw", BACKWARD_CASES, ids=[f"{k}-{s}" for k, s, _ in BACKWARD_CASES])
def test_backward_groups(S, shape, step, kw, arith):
    """render_backward's dfeat per level BEFORE any scatter (with the x-stash, and under h3 without), the decoder gradient per named
    tensor, and the table gradient per level through the stand-alone scatter: step 12000 (all 16 levels at full weight), 5600
    (level 12 at 0.47, 13-15 masked), 0 (8-15 masked), and B = 37, S = 33 with a ray_valid mask."""
    _with_arith(arith, _backward_groups, shape, step, kw, arith)


def test_backward_groups_f32_arith(S):
    _with_arith("f32", _backward_groups, "fg64", 12000, {}, "f32")
    _with_arith("f32", _backward_groups, "bg40", 5600, {}, "f32")


@pytest.mark.parametrize("arith", ["h3", "t16s", "t16"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_backward_groups_half_tables(S, dtype, arith):
    """bf16 / f16 gather tables: the table IS the rounded values (the reference upcasts them exactly), so the same bounds hold."""
    _with_arith(arith, _backward_groups, "fg64", 12000, dict(table_dtype=dtype), arith)
    _with_arith(arith, _backward_groups, "bg40", 5600, dict(table_dtype=dtype), arith)


# --------------------------------------------------------------------------------------------------- table routes, small table
def _standalone_routes(shape, step, arith):
    from scanerf_amd.hashgrid.lib import HASHGRID as HG
    case, ref, e32 = _case(*SHAPES[shape], step, in_domain=True)
    refk = _kinds(ref, ("table",))
    run = _Gpu(case)
    pts, dfeat = run.valid_samples(run.backward()[0])
    for fmt in (0, 1, 2):
        gF = run.render.scatter_table_grad(pts, dfeat, torch.zeros(16, case.T, 2, device=DEV), run.R, compact_records=fmt)
        _judge(f"table gradient, stand-alone binned scatter, record format {fmt}, {shape} step {step}", {"table": gF}, refk, e32, arith,
               case.masked, REC_EXTRA[fmt])
    gF = torch.zeros(16, case.T, 2, device=DEV)
    route, HG.TABLE_GRAD_ROUTE = HG.TABLE_GRAD_ROUTE, "atomics"
    try:
        HG.embedding_bg_backward_cuda(pts, dfeat.permute(1, 0, 2).contiguous(), None, gF, run.table, run.R)
    finally:
        HG.TABLE_GRAD_ROUTE = route
    _judge(f"table gradient, atomic kernel, {shape} step {step}", {"table": gF}, refk, e32, arith, case.masked)
    # ... and ending in the sparse Adam, every record format
    for fmt in (0, 1, 2):
        P0 = run.table.clone()
        P, M, V, over = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0), torch.zeros_like(P0)
        run.render.scatter_table_grad_adam(pts, dfeat, run.R, P, M, V, LR, B1, B2, EPS, 0, overflow_grad=over, compact_records=fmt)
        assert not bool(over.any())
        _judge(f"first moment / (1 - beta1), stand-alone scatter + Adam, record format {fmt}, {shape} step {step}",
               {"table": _moment_gradient(M)}, refk, e32, arith, case.masked, REC_EXTRA[fmt])
        _assert_masked_untouched(case, P, P0, M, V, f"scatter_table_grad_adam format {fmt}")


@pytest.mark.parametrize("arith", ["h3", "t16s", "t16"])
@pytest.mark.parametrize("shape,step", [("fg64", 12000), ("fg64", 5600), ("bg40", 5600)])
def test_standalone_scatter_formats_and_atomics_groups(S, shape, step, arith):
    """The x-stash backward's dfeat through the stand-alone binned scatter in record formats 0 / 1 / 2, through the reference-style
    atomic kernel, and through the scatter ending in the sparse Adam: the table gradient per level, foreground and background."""
    _with_arith(arith, _standalone_routes, shape, step, arith)


def _fused_records(bg, S_, step, arith):
    from scanerf_amd import render
    case, ref, e32 = _case(bg, S_, step, log2_T=14, in_domain=True)
    refk = _kinds(ref, ("table",))
    extra = REC_EXTRA[render.compact_record_format(render.backward_arith())]
    run = _Gpu(case)
    ws = run.plan()
    gF = torch.zeros(16, case.T, 2, device=DEV)
    _, gblob = run.backward(scatter=(ws, gF), want_dfeat=False)
    render.scatter_accumulate(ws, gF, case.B, case.S)
    tag = f"{'bg' if bg else 'fg'}{S_} step {step} T 2^14"
    _judge(f"table gradient, fused records -> scatter_accumulate, {tag}", {"table": gF, "decoder": _decoder(gblob)},
           _kinds(ref, ("table", "decoder")), e32, arith, case.masked, extra)
    # the same records through the accumulate's Adam epilogue: no gradient is ever materialised
    over = torch.zeros(16, case.T, 2, device=DEV)
    ws = run.plan()
    run.backward(scatter=(ws, over), want_dfeat=False)
    P0 = run.table.clone()
    P, M, V = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    render.scatter_accumulate_adam(ws, P, M, V, LR, B1, B2, EPS, 0, case.B, case.S, overflow_grad=over)
    torch.cuda.synchronize()
    assert not bool(over.any())
    _judge(f"first moment / (1 - beta1), accumulate_adam, {tag}", {"table": _moment_gradient(M)}, refk, e32, arith, case.masked, extra)
    _assert_masked_untouched(case, P, P0, M, V, "scatter_accumulate_adam")


@pytest.mark.parametrize("arith", ["f32", "h3", "t16s", "t16"])
@pytest.mark.parametrize("bg,S_,step", [(False, 64, 12000), (False, 64, 5600), (True, 40, 12000), (True, 40, 0)])
def test_fused_records_and_accumulate_adam_groups(S, bg, S_, step, arith):
    """T = 2^14: the backward kernel emits the table-gradient records itself (16-byte under f32 / h3, 12-byte under t16s, 8-byte
    under t16); scatter_accumulate into a gradient table, and scatter_accumulate_adam read back through the first moment."""
    _with_arith(arith, _fused_records, bg, S_, step, arith)


def _two_branches(step, log2_T, B=200):
    """A foreground and a background branch over the SAME rays, table and decoder (the generator draws the rays first, so the two
    cases share them): -> (fg, bg) cases, then (reference, e32) of the foreground's table gradient alone and of the two summed."""
    fg = R64.BackwardCase(False, 64, step, B=B, log2_T=log2_T, in_domain=True)
    bg = R64.BackwardCase(True, 40, step, B=B, log2_T=log2_T)
    assert np.array_equal(fg.o, bg.o) and np.array_equal(fg.d, bg.d)
    bg.table = fg.table
    ref1, o1 = {"table": fg.reference64()["table"]}, fg.oracle32()["table"].astype(np.float64)
    ref2, o2 = {"table": ref1["table"] + bg.reference64()["table"]}, o1 + bg.oracle32()["table"]
    return fg, bg, (ref1, R64.group_errors({"table": o1}, ref1)), (ref2, R64.group_errors({"table": o2}, ref2))


def _adam2(step, arith):
    from scanerf_amd import render
    fg, bg, _, (ref, e32) = _two_branches(step, 14)
    extra = REC_EXTRA[render.compact_record_format(render.backward_arith())]
    over = torch.zeros(16, fg.T, 2, device=DEV)
    runs = [_Gpu(fg), _Gpu(bg)]
    wss = [r.plan(own=True) for r in runs]
    for r, ws in zip(runs, wss):
        r.backward(scatter=(ws, over), want_dfeat=False)
    P0 = runs[0].table.clone()
    P, M, V = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    render.scatter_accumulate_adam2(wss[0], fg.S, wss[1], bg.S, P, M, V, LR, B1, B2, EPS, 0, fg.B, overflow_grad=over)
    torch.cuda.synchronize()
    assert not bool(over.any())
    _judge(f"first moment / (1 - beta1), accumulate_adam2 over fg64 + bg40, step {step} T 2^14", {"table": _moment_gradient(M)}, ref,
           e32, arith, fg.masked, extra)
    _assert_masked_untouched(fg, P, P0, M, V, "scatter_accumulate_adam2")


@pytest.mark.parametrize("arith", ["h3", "t16s", "t16"])
@pytest.mark.parametrize("step", [12000, 5600])
def test_accumulate_adam2_groups(S, step, arith):
    """Two branches' records meeting in ONE Adam step: the first moment against the sum of the two float64 table gradients."""
    _with_arith(arith, _adam2, step, arith)


# --------------------------------------------------------------------------------------------------- large table (2^22)
def _large_table(step):
    """T = 2^22, 1280 rays (the large-table producer wants >= 2^16 points): the segment route of the stand-alone scatter into a
    gradient table, the same ending in the sparse Adam, and scatter_table_grad_adam_rays over one and over two branches."""
    from scanerf_amd import render
    arith = "t16s"
    assert render.scatter_rays_supported(2 ** 22, render.backward_arith())
    fg, bg, (ref1, e32_1), (ref2, e32_2) = _two_branches(step, 22, B=1280)
    runs = [_Gpu(fg), _Gpu(bg, table=fg.table)]
    dfeats = [r.backward()[0] for r in runs]
    run, T = runs[0], fg.T
    pts, df = run.valid_samples(dfeats[0])
    assert pts.shape[0] >= 1 << 16
    for fmt in (-1, 2):
        gF = render.scatter_table_grad(pts, df, torch.zeros(16, T, 2, device=DEV), run.R, compact_records=fmt)
        _judge(f"table gradient, stand-alone scatter (compact_records {fmt}; 2 = 64-byte segments), fg64 B 1280 step {step} T 2^22",
               {"table": gF}, ref1, e32_1, arith, fg.masked, REC_EXTRA[fmt])
        del gF
    for branches, ref, e32, what in (((0,), ref1, e32_1, "fg64"), ((0, 1), ref2, e32_2, "fg64 + bg40")):
        P0 = run.table.clone()
        P, M, V, over = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0), torch.zeros_like(P0)
        render.scatter_table_grad_adam_rays(run.o, run.d, [(runs[k].z, dfeats[k], runs[k].valid, runs[k].box[2]) for k in branches],
                                            *run.box[:2], run.R, P, M, V, LR, B1, B2, EPS, 0, over)
        torch.cuda.synchronize()
        assert not bool(over.any())
        _judge(f"first moment / (1 - beta1), scatter_table_grad_adam_rays over {what}, B 1280 step {step} T 2^22",
               {"table": _moment_gradient(M)}, ref, e32, arith, fg.masked, REC_EXTRA[2])
        _assert_masked_untouched(fg, P, P0, M, V, f"scatter_table_grad_adam_rays ({what})")
        del P, M, V, over, P0


@pytest.mark.parametrize("step", [12000, 5600])
def test_large_table_segment_route_and_rays_adam_groups(S, step):
    _with_arith("t16s", _large_table, step)


# --------------------------------------------------------------------------------------------------- fg + bg, autograd boundary
def _fgbg(step, arith):
    from scanerf_amd import render
    from scanerf_amd.tile_model import TileModel, fgbg_gradients
    rng = np.random.default_rng(31)
    B, Sf, Sb = 256, 64, 40
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=12, seed=4)
    with torch.no_grad():
        m.features.mul_(200.0)
    occ = rng.random((16, 16, 16)) < 0.6
    m.set_occupancy(g(occ))
    o = rng.uniform(-3.9, 3.9, (B, 3)).astype(np.float32)
    d = rng.normal(size=(B, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tgt = rng.random((B, 3)).astype(np.float32)
    loss, gtab, gblob = fgbg_gradients(m, g(o), g(d), g(tgt), Sf, Sb, step, invalid_underground=True)
    tile = O.Tile([-4, -4, -4], [8, 8, 8], log2_T=12)
    tile.occ = torch.from_numpy(occ)
    table = m.features.detach().cpu()
    sd = {k: v.detach().cpu() for k, v in m.decoder.ref_state_dict().items()}
    r = R64.RenderRays64(tile, table, sd, o, d, Sf, Sb, step, invalid_underground=True)
    assert 0 < int(r.fore_valid.sum()) < B and 0 < int(r.bg_valid.sum()) < B
    ref = r.gradients(r.photometric_loss(tgt))
    o32 = R64.oracle32_render_rays(tile, table, sd, o, d, Sf, Sb, step, tgt, invalid_underground=True)
    kinds = lambda q: {"table": q["table"], "decoder": q["decoder"]}
    e32 = R64.group_errors(kinds(o32), kinds(ref))
    np.testing.assert_allclose(float(loss), ref["loss"], rtol=2e-5)
    masked = [l for l in range(16) if float(O.weight_feature(step)[l]) == 0.0]
    # (T = 2^12: each branch's backward emits its records into the one gradient table, format by arithmetic)
    extra = REC_EXTRA[render.compact_record_format(render.backward_arith())]
    _judge(f"fgbg_gradients, partly empty occupancy, step {step}", {"table": gtab, "decoder": _decoder(gblob)}, kinds(ref), e32, arith,
           masked, extra)


@pytest.mark.parametrize("arith", ["h3", "t16s", "t16"])
@pytest.mark.parametrize("step", [12000, 5600])
def test_fgbg_gradients_groups(S, step, arith):
    """The complete per-tile render (fg + T_left * bg, tile.py's loss over the rays valid in either branch) on a small tile whose
    occupancy grid is 40 % empty: table gradient per level, decoder gradient per tensor."""
    _with_arith(arith, _fgbg, step, arith)


def _autograd(bg, S_, step, arith):
    from scanerf_amd import render
    case, ref, e32 = _case(bg, S_, step, in_domain=True)
    run = _Gpu(case)
    feats = run.table.clone().requires_grad_(True)
    blob = O.pack_blob(case.sd).to(DEV).requires_grad_(True)
    out, _ = render.fused_render_rays(run.o, run.d, run.z, run.dist, feats, blob, run.R, run.wf, *run.box, ray_valid=run.valid,
                                      skip_levels=run.skip)
    (out * run.gout).sum().backward()
    # (T = 2^12: the table gradient goes through the fused records, format by arithmetic)
    extra = REC_EXTRA[render.compact_record_format(render.backward_arith())]
    _judge(f"FusedRenderRays loss.backward(), {'bg' if bg else 'fg'}{S_} step {step}", {"table": feats.grad, "decoder": _decoder(blob.grad)},
           _kinds(ref, ("table", "decoder")), e32, arith, case.masked, extra)


@pytest.mark.parametrize("arith", ["h3", "t16s", "t16"])
@pytest.mark.parametrize("bg,S_,step", [(False, 64, 12000), (True, 40, 5600)])
def test_fused_render_rays_autograd_groups(S, bg, S_, step, arith):
    """The autograd boundary: loss.backward() through FusedRenderRays gives the table and decoder gradients."""
    _with_arith(arith, _autograd, bg, S_, step, arith)
