"""The stream contract of include/scanerf_hip.h on the GPU: every export launches on the stream it is given and nowhere else, no
call synchronises (but the ones SYNCHRONISES lists), per-stream workspaces do not meet, and what the Python package caches is ordered
for a second stream.  Every case of tests/stream_cases.py runs under a stream from torch.cuda.Stream() (non-blocking: the null stream
does not order against it) that a delay kernel holds busy while the host enqueues the case.

How a wrong stream shows.  The device tensors hold seed 2's values (Y) when the side-stream run starts; the refill with seed 1's (X)
and the case's launches are queued on the side stream BEHIND the delay.  A launch that went to any other stream runs at once, on Y's
inputs or Y's intermediates, so the run's outputs differ from the default-stream run on X -- and the recorder, which wraps every
attribute of _capi.lib(), shows the handle the call carried.  Stale data is always valid data (tests/test_stream_cases_cpu.py).

`pytest -s` prints the table profiles/stream_contract.md holds."""
import collections
import time

import pytest
import torch

import stream_cases as SC

pytestmark = pytest.mark.gpu
DEV = SC.DEV

# Entries that synchronise THEIR OWN stream, read from the code (not found by trial): name -> file:line of the synchronising call.
SYNCHRONISES = {"scanerf_mesh_filter_emit": "csrc/mesh_components.hip:525 (hipStreamSynchronize after the read-back of V' and F')"}

DELAY_FLOOR_MS, DELAY_CAP_MS = 5.0, 500.0
Call = collections.namedtuple("Call", "name stream before after rearmed")
TABLE = []          # rows of the printed table
STREAM_NOTE = []    # check (b): which stream index was needed


def _capi():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    return _capi


# ------------------------------------------------------------------------------------------------------------------ delay
class Delay:
    """A kernel that keeps one stream busy and leaves the GPU otherwise free: torch.cuda._sleep (a spin on the clock in one thread),
    or a chain of dependent 64x64 matmuls where torch has none.  Calibrated once with two events."""

    def __init__(self):
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.a = torch.eye(64, device=DEV) * 0.5
        probe = 20_000_000 if self.sleep else 2000
        self._enqueue(probe)          # (the first launch loads the kernel)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._enqueue(probe)
        e1.record()
        torch.cuda.synchronize()
        self.units_per_ms = probe / max(e0.elapsed_time(e1), 1e-3)

    def _enqueue(self, units):
        if self.sleep:
            self.sleep(int(units))
        else:
            x = self.a
            for _ in range(int(units)):
                x = x @ self.a

    def __call__(self, ms):
        """Enqueue `ms` milliseconds of delay on the current stream -> the event recorded right behind it."""
        assert ms <= DELAY_CAP_MS * 1.001, f"a delay of {ms:.0f} ms: the case is too big, shrink it"
        self._enqueue(ms * self.units_per_ms)
        ev = torch.cuda.Event()
        ev.record()
        return ev


@pytest.fixture(scope="module")
def delay():
    return Delay()


# ------------------------------------------------------------------------------------------------------------------ recorder
class Recorder:
    """Every attribute of _capi.lib() replaced (callers fetch lib().scanerf_x at call time).  A stream-taking export's call is
    recorded as (name, last argument, delay pending before the call, delay pending right after it returned, re-armed).
    rearm: where the delay has run out before a call -- a wrapper read a count back, or an entry synchronised -- a new delay is
    queued on the current stream first, so that every call is judged, also the ones behind a host read-back."""

    def __init__(self, monkeypatch):
        api = _capi()
        self.calls, self.event, self.rearm_ms, self.delay, self.null_for = [], None, None, None, None
        streamy = set(SC.stream_entries())
        ns = api.lib()
        for name, fn in list(vars(ns).items()):
            if callable(fn) and name in streamy:
                monkeypatch.setattr(ns, name, self._wrap(name, fn))

    def _pending(self):
        return None if self.event is None else not self.event.query()

    def _wrap(self, name, fn):
        def call(*a):
            before, rearmed = self._pending(), False
            if before is False and self.rearm_ms is not None:
                self.event = self.delay(self.rearm_ms)
                before, rearmed = self._pending(), True
            handle = a[-1]
            if self.null_for == name:
                a, self.null_for = a[:-1] + (None,), None        # check (b): this one call goes to the null stream
                handle = None
            rc = fn(*a)
            self.calls.append(Call(name, int(handle or 0), before, self._pending(), rearmed))
            return rc
        call.__name__ = name
        return call

    def take(self):
        out, self.calls = self.calls, []
        return out


def _bits(t):
    if t.dtype.is_floating_point:
        return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def side_run(c, state, Xd, s, ms, rec, delay, rearm=True):
    """Step 3 of check (a): under `s`, the delay, the refill with X, the run; then s.synchronize() -> (outputs, calls)."""
    torch.cuda.synchronize()
    rec.take()
    rec.delay, rec.rearm_ms = delay, (ms if rearm else None)
    with torch.cuda.stream(s):
        rec.event = delay(ms)
        c.refill(state, Xd)
        R = c.run(state)
    s.synchronize()
    rec.event = rec.rearm_ms = None
    torch.cuda.synchronize()
    return R, rec.take()


def judge_calls(c, calls, handle):
    """Steps 5-7 -> (problems, number of re-armed delays, whether the delay ran out before a call of a case without host reads)."""
    bad = []
    wrong = [k for k in calls if k.stream != handle]
    if wrong:
        bad.append(f"calls on another stream than the caller's {handle:#x}: " + ", ".join(f"{k.name}@{k.stream:#x}" for k in wrong))
    missing = c.live_entries() - {k.name for k in calls}
    if missing:
        bad.append(f"entries the case claims but did not call: {sorted(missing)}")
    ran_out, after_sync = False, False
    for k in calls:
        if k.rearmed and not (c.host_syncs or after_sync):
            ran_out = True
        if k.before is False:
            bad.append(f"{k.name}: the delay could not be kept pending before the call")
        elif (k.after is False) != (k.name in SYNCHRONISES):
            bad.append(f"{k.name}: delay pending after the call = {k.after}, but the entry is "
                       f"{'' if k.name in SYNCHRONISES else 'not '}listed in SYNCHRONISES")
        after_sync = after_sync or k.name in SYNCHRONISES
    return bad, sum(k.rearmed for k in calls), ran_out


def baseline(c, rec):
    """Steps 1 and 2: the default-stream runs on X, then on Y (which leaves every output, scratch buffer and cache with Y's values).
    -> state, X and Y on the device, R_X, R_Y, the host enqueue time of the (warm) second run in ms, the default-stream call names."""
    X, Y = c.build(1), c.build(2)
    state = c.to_device(X)
    Xd, Yd = SC.stage(X), SC.stage(Y)
    torch.cuda.synchronize()
    rec.take()
    R_X = c.run(state)
    torch.cuda.synchronize()
    names = [k.name for k in rec.take()]
    c.refill(state, Yd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    R_Y = c.run(state)
    enqueue_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    rec.take()
    return X, state, Xd, Yd, R_X, R_Y, enqueue_ms, names


def delay_for(enqueue_ms):
    ms = max(DELAY_FLOOR_MS, 20.0 * enqueue_ms)
    assert ms <= DELAY_CAP_MS, f"host enqueue time {enqueue_ms:.1f} ms needs a delay of {ms:.0f} ms: the case is too big, shrink it"
    return ms


def check_case(c, s, rec, delay, null_for=None):
    """Check (a) for one case on stream `s` -> dict(problems, differs: step 4 found a difference, row)."""
    X, state, Xd, Yd, R_X, R_Y, enqueue_ms, _ = baseline(c, rec)
    assert not same_bits(R_X, R_Y), f"{c.name}: seeds 1 and 2 give the same outputs: a stale read would not show"
    ms = delay_for(enqueue_ms)
    for attempt in (0, 1):
        rec.null_for = null_for
        R, calls = side_run(c, state, Xd, s, ms, rec, delay)
        bad, rearmed, ran_out = judge_calls(c, calls, s.cuda_stream)
        if not ran_out or attempt == 1 or null_for is not None:
            break
        ms = min(2.0 * ms, DELAY_CAP_MS)          # the run proved nothing: once more, with the delay doubled
        c.refill(state, Yd)
        c.run(state)
    if ran_out and null_for is None:
        bad.append(f"the delay ({ms:.0f} ms) ran out before the case's last call: the run proves nothing")
    if c.exact:
        differs = not same_bits(R, R_X)
    else:
        ref = c.reference(X)
        c.compare(R_X, ref)
        try:
            c.compare(R, ref)
            differs = False
        except AssertionError as e:
            differs = str(e)[:400]
    row = dict(case=c.name, entries=sorted(c.live_entries()), enqueue_ms=enqueue_ms, delay_ms=ms, exact=c.exact,
               synchronises=sorted(set(SYNCHRONISES) & {k.name for k in calls}), host_syncs=c.host_syncs, rearmed=rearmed)
    return dict(problems=bad, differs=differs, row=row, calls=calls)


# ------------------------------------------------------------------------------------------------------------------ the side stream: check (b)
Side = collections.namedtuple("Side", "stream index log")


@pytest.fixture(scope="module")
def side(delay):
    """A stream that demonstrably runs concurrently with the null stream: the cheapest case with ONE call sent to the null stream must
    come out different (the mis-streamed kernel ran on stale inputs while the side stream was held).  If it does not, the stream
    shares a hardware queue with the null stream: another one, four tries at the most.  index None: none was found."""
    mp = pytest.MonkeyPatch()
    log = []
    try:
        rec = Recorder(mp)
        c = SC.BY_NAME["box"]
        for index in range(4):
            s = torch.cuda.Stream()
            r = check_case(c, s, rec, delay, null_for="scanerf_ray_aabb_intersection")
            flagged = any("another stream" in p for p in r["problems"])
            log.append(dict(index=index, flagged=flagged, differs=bool(r["differs"])))
            if flagged and r["differs"]:
                return Side(s, index, log)
            del s
        return Side(torch.cuda.Stream(), None, log)
    finally:
        mp.undo()


def test_b_the_harness_detects_a_call_on_the_wrong_stream(side):
    """ray_aabb_intersection sent to the null stream (a legal launch on valid, stale inputs): step 5 flags the handle, step 4 differs."""
    STREAM_NOTE.append(f"check (b): stream index {side.index} of {len(side.log)} tried; log {side.log}")
    assert all(t["flagged"] for t in side.log), f"the recorder did not flag the substituted call: {side.log}"
    assert side.index is not None, ("two concurrently running streams could not be established: on each of four streams from "
                                    f"torch.cuda.Stream() a kernel sent to the null stream waited for the side stream's delay: {side.log}")


# ------------------------------------------------------------------------------------------------------------------ check (a), (f)
@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.name)
def test_a_ordering_on_one_side_stream(c, side, delay, monkeypatch):
    """Steps 1-7 of check (a), and (f): the delay is still pending after every call of an entry if and only if the entry is not in
    SYNCHRONISES."""
    rec = Recorder(monkeypatch)
    r = check_case(c, side.stream, rec, delay)
    TABLE.append(r["row"])
    assert not r["differs"], f"{c.name}: the side-stream run differs from the default-stream run on the same inputs: {r['differs']}"
    assert not r["problems"], "\n".join(r["problems"])


def test_f_synchronises_lists_entries_of_the_header():
    assert set(SYNCHRONISES) <= set(SC.stream_entries())
    assert set(SYNCHRONISES) <= set().union(*(c.entries for c in SC.CASES)), "a synchronising entry no case calls is never judged"


# ------------------------------------------------------------------------------------------------------------------ check (c): caches
def _two_streams(op_a, op_b, delay, ms=20.0):
    """sync; under s1: delay, op_a(); straight away under s2: op_b(); sync both -> (result a, result b)."""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        delay(ms)
        ra = [t.clone() for t in op_a()]
    with torch.cuda.stream(s2):
        rb = [t.clone() for t in op_b()]
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    return ra, rb


def _cache_check(make, op, delay, what):
    """make() -> fresh objects; op(objects) -> outputs.  Baseline on the default stream, then s1 (delayed) populates and s2 hits;
    then the same with the roles of the two streams swapped on fresh objects (s2's op first in host order, undelayed; s1's hit behind
    a delay)."""
    base = [t.clone() for t in op(make())]
    torch.cuda.synchronize()
    obj = make()
    ra, rb = _two_streams(lambda: op(obj), lambda: op(obj), delay)
    assert same_bits(ra, base), f"{what}: the populating stream's result differs from the default-stream baseline"
    assert same_bits(rb, base), f"{what}: a second stream read the cache before the first stream had filled it"
    obj = make()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s2):
        delay(20.0)
        rb = [t.clone() for t in op(obj)]
    with torch.cuda.stream(s1):
        ra = [t.clone() for t in op(obj)]
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    assert same_bits(rb, base) and same_bits(ra, base), f"{what} (streams swapped): a second stream read the cache before it was filled"


def _inference_inputs():
    """The render-time case's arrays up to the two inference ops' inputs, on the default stream."""
    from scanerf_amd import hashgrid as H
    c = SC.BY_NAME["render_time"]
    X = c.build(1)
    st = c.to_device(X)
    i = st["in"]
    B, S, Sb = SC.RT_B, SC.RT_S, SC.RT_SB
    inter = torch.full((B, 3, 2), 1e7, device=DEV)
    H.ray_block_intersection(i["o"], i["d"], st["C"], st["Z"], inter)
    TB = H.sort_tracing_blocks(inter)
    TI, ZS = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, device=DEV)
    z, dd = torch.full((B, S), -1.0, device=DEV), torch.full((B, S), -1.0, device=DEV)
    H.sample_points(i["o"], i["d"], st["C"], st["Z"], i["occ"], st["ST"], st["L2"], TB, inter, TI, ZS, z, dd)
    bi = torch.full((B, S, 4), -1, dtype=torch.int16, device=DEV)
    H.prepare_points(z, torch.ones(B, dtype=torch.bool, device=DEV), inter, bi)
    ob, bw = torch.full((B, 4), -1, dtype=torch.int16, device=DEV), torch.zeros((B, 4), device=DEV)
    H.update_outgoing_bidx(i["o"], i["d"], st["C"], st["Z"], TB, inter, ob, bw, 0.12, False)
    zb = torch.full((B, Sb), -1.0, device=DEV)
    H.inverse_z_sampling(inter, ob[:, 0].contiguous(), zb, 1e6)
    torch.cuda.synchronize()
    return st, dict(z=z, dd=dd, bi=bi, ob=ob, zb=zb)


@pytest.mark.parametrize("folded", [True, False], ids=["folded", "plain"])
def test_c_packed_decoder_images_are_ordered_for_a_second_stream(folded, delay, monkeypatch):
    """hashgrid/lib/HASHGRID.py _packed_images: raw `params` packed on first use under stream A; a call under stream B with the same
    tensor must not run its inference before A's pack."""
    from scanerf_amd import hashgrid as H
    from scanerf_amd.hashgrid.lib import HASHGRID as HG
    monkeypatch.setattr(HG, "FOLD_ACTIVATION", folded)
    st, a = _inference_inputs()
    i = st["in"]
    B, S, Sb = SC.RT_B, SC.RT_S, SC.RT_SB
    new = lambda *shape: torch.zeros(shape, device=DEV)

    def op(params):
        fg = [new(B, S, 3), new(B, S, 3), new(B, S, 1)]
        H.pts_inference(i["o"], i["d"], a["z"], a["dd"], a["bi"], i["tables"], params, st["RES"], i["occ"], st["ST"], st["L2"], st["C"],
                        st["Z"], *fg)
        bg = [new(B, Sb, 3), new(B, Sb, 3), new(B, Sb, 1)]
        H.bg_pts_inference_v2(i["o"], i["d"], a["zb"], a["ob"], 0, st["C"], st["Z"], st["RES"], i["tables"], params, *bg)
        return fg + bg

    base = op(HG.PackedDecoders(i["params"]))
    assert float(base[2].max()) > 0.01 and float(base[5].max()) > 0.01
    _cache_check(lambda: i["params"].clone(), op, delay, f"_packed_images ({'folded' if folded else 'plain'})")
    torch.cuda.synchronize()
    assert same_bits([t.clone() for t in op(i["params"].clone())], base)


def test_c_hashgrid_converted_tensors_are_ordered_for_a_second_stream(delay):
    """hashgrid/grid.py _converted: the sampler's log2dim is converted on first use (a copy and a cast) and read by every later
    samplePoints, whatever its stream."""
    from scanerf_amd.hashgrid import HashGrid
    X = SC.BY_NAME["samplers"].build(1)
    o, d = X["o"].to(DEV), X["d"].to(DEV)

    def make():
        return HashGrid(DEV, [-4.0, -4.0, -4.0], [8.0, 8.0, 8.0], log2_hashmap_size=10)

    _cache_check(make, lambda g: g.samplePoints(o, d, 33), delay, "HashGrid._converted")


@pytest.mark.parametrize("which", ["weight_feature", "overflow_grad", "gather_table"])
def test_c_tile_model_lazy_tensors_are_ordered_for_a_second_stream(which, delay):
    """tile_model.TileModel builds weight_feature (_wf), overflow_grad (a zero fill) and the bf16 gather_table on first use, on
    whichever stream is current; each is read here by the lowest-level call that consumes it, on the other stream."""
    from scanerf_amd import render
    from scanerf_amd.tile_model import TileModel
    X = SC.BY_NAME["fused_h3"].build(1)
    o, d = X["o"].to(DEV), X["d"].to(DEV)
    B, S = o.shape[0], 33

    def make():
        m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=13, seed=3, table_dtype=torch.bfloat16 if which == "gather_table" else torch.float32)
        with torch.no_grad():
            m.features.mul_(100.0)
        z, dist = m.sample(o, d, S)
        ones = torch.ones(32, device=DEV)
        fixed_wf = m.weight_feature(20000).clone()
        torch.cuda.synchronize()
        m._wf_by_stream.clear()      # (the lazily built tensors start absent: this test is about their first use)
        return m, z, dist, ones, fixed_wf

    def op(obj):
        m, z, dist, ones, fixed_wf = obj
        box = (m.min_bbox.tolist(), m.bbox_size.tolist(), render.FORE, False)
        wf = m.weight_feature(3100) if which == "weight_feature" else fixed_wf
        table = m.gather_table() if which == "gather_table" else m.features.detach()
        pk = render.PackedDecoder(DEV).pack(m.decoder.blob().detach(), wf)
        tile_T, xs = torch.empty(B, render.tile_T_columns(S), device=DEV), torch.empty(B * S, 32, device=DEV)
        out, w = render.render_forward(o, d, z, dist, table, m.resolution, pk, *box, tile_T=tile_T, xstash=xs)
        if which != "overflow_grad":
            return out, w
        over = m.overflow_grad()
        ws = render.scatter_plan(o, d, z, m.resolution, table.shape[1], *box,
                                 workspace=torch.empty(render.lib().scanerf_render_scatter_workspace_bytes(B, S, table.shape[1]),
                                                       dtype=torch.uint8, device=DEV))
        g = torch.full((B, 16), 1.0 / B, device=DEV)
        render.render_backward(o, d, z, dist, table, m.resolution, pk, wf, *box, out, tile_T, g, xstash=xs, scatter=(ws, over), want_dfeat=False)
        P, M, V = m.features.detach().clone(), torch.zeros_like(m.features), torch.zeros_like(m.features)
        render.scatter_accumulate_adam(ws, P, M, V, 1e-2, 0.9, 0.99, 1e-15, 0, B, S, overflow_grad=over)
        return out, P, M, V, over

    _cache_check(make, op, delay, f"TileModel.{which}")


# ------------------------------------------------------------------------------------------------------------------ check (d): two plans
def _plan_models():
    c = SC.BY_NAME["fused_t16s_plan"]
    out = []
    for seed in (1, 2):
        X = c.build(seed)
        st = c.to_device(X)
        st["P"], st["M"], st["V"] = st["in"]["feat"].clone(), torch.zeros_like(st["in"]["feat"]), torch.zeros_like(st["in"]["feat"])
        st["over"] = torch.zeros_like(st["in"]["feat"])
        out.append(st)
    torch.cuda.synchronize()
    return out


def _plan_forward(st, S=16, workspace=None):
    from scanerf_amd import render
    i = st["in"]
    B = i["o"].shape[0]
    z, dist = SC._sample(st, S)
    pk = st["packed"].pack(i["blob"], st["wf"])
    tile_T, xs = torch.empty(B, render.tile_T_columns(S), device=DEV), torch.empty(B * S, 32, device=DEV)
    out, _, ws = render.render_forward(i["o"], i["d"], z, dist, st["P"], st["res"], pk, *st["box"], want_weights=False, tile_T=tile_T,
                                       xstash=xs, plan=True, plan_workspace=workspace)
    st["ctx"] = (z, dist, pk, tile_T, xs, out, ws)


def _plan_finish(st, S=16):
    from scanerf_amd import render
    i = st["in"]
    B = i["o"].shape[0]
    z, dist, pk, tile_T, xs, out, ws = st.pop("ctx")
    render.render_backward(i["o"], i["d"], z, dist, st["P"], st["res"], pk, st["wf"], *st["box"], out, tile_T, i["gout"], xstash=xs,
                           scatter=(ws, st["over"]), want_dfeat=False)
    render.scatter_accumulate_adam(ws, st["P"], st["M"], st["V"], 1e-2, 0.9, 0.99, 1e-15, 0, B, S, overflow_grad=st["over"])


def _plan_state(st):
    return [st["P"].clone(), st["M"].clone(), st["V"].clone()]


def test_d_two_streams_two_fused_plans(delay, monkeypatch):
    """_capi.workspace is keyed by the current stream: model A's plan must survive model B's whole step on another stream.  Device
    order, enforced: A's forward-with-plan runs on s1 and an event marks its end; a delay then holds s1; s2 waits for the event and
    runs B's forward-with-plan, backward and accumulate; the host waits for s2 and finds s1's delay still pending -- B's step is over
    and A's plan has not been consumed; only then A's backward and accumulate are queued on s1.  With one workspace for both streams
    B's plan and records would have replaced A's.  Tables and moments of both equal their single-stream baselines bit for bit.
    Control: the same interleaving on ONE stream with each model's plan in a workspace of its own -- the order of the calls alone
    changes nothing, so what the two-stream run adds is the per-stream workspace.  (The interleaving on one stream and ONE workspace
    is what the wrappers' documentation rules out: B's plan would replace A's under A's backward, whose record ranges are then no
    longer reserved; it is not run.)"""
    from scanerf_amd import render
    assert render.forward_plan_supported(2048, 16, 2 ** 13)
    A, B = _plan_models()
    for st in (A, B):
        _plan_forward(st)
        _plan_finish(st)
    torch.cuda.synchronize()
    base = [_plan_state(A), _plan_state(B)]
    assert int((base[0][1] != 0).sum()) > 1000 and not same_bits(base[0], base[1])

    rec = Recorder(monkeypatch)
    A, B = _plan_models()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    rec.take()
    with torch.cuda.stream(s1):
        _plan_forward(A)
        planned_a = torch.cuda.Event()
        planned_a.record()
        rec.event = delay(200.0)
    with torch.cuda.stream(s2):
        s2.wait_event(planned_a)
        _plan_forward(B)
        _plan_finish(B)
    s2.synchronize()
    assert planned_a.query() and not rec.event.query(), "B's step did not end between A's forward and A's backward: the run proves nothing"
    with torch.cuda.stream(s1):
        _plan_finish(A)
    s1.synchronize()
    rec.event = None
    torch.cuda.synchronize()
    calls = rec.take()
    planned = [k for k in calls if k.name == "scanerf_render_forward_packed_plan"]
    assert [k.stream for k in planned] == [s1.cuda_stream, s2.cuda_stream]
    assert {k.stream for k in calls} == {s1.cuda_stream, s2.cuda_stream}
    assert same_bits(_plan_state(A), base[0]), "model A's step changed when model B's step ran on another stream in between"
    assert same_bits(_plan_state(B), base[1]), "model B's step changed when it ran between model A's forward and backward"

    A, B = _plan_models()
    need = render.lib().scanerf_render_scatter_workspace_bytes(2048, 16, 2 ** 13)
    _plan_forward(A, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
    _plan_forward(B, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
    _plan_finish(B)
    _plan_finish(A)
    torch.cuda.synchronize()
    assert same_bits(_plan_state(A), base[0]) and same_bits(_plan_state(B), base[1]), "control: the interleaved order alone changed a result"


# ------------------------------------------------------------------------------------------------------------------ check (e): autograd
def _autograd_cases():
    from scanerf_amd import decoder_op, render
    from scanerf_amd.hashgrid import HashEmbeddingBG

    def fused(seed=1):
        c = SC.BY_NAME["fused_fgbg_pose"]
        st = c.to_device(c.build(seed))
        i = st["in"]
        z, dist = SC._sample(st, 33)
        torch.cuda.synchronize()
        leaves = [i[k].detach().clone().requires_grad_(True) for k in ("o", "d", "feat", "blob")]

        def fwd():
            out, w = render.fused_render_rays(leaves[0], leaves[1], z, dist, leaves[2], leaves[3], st["res"], st["wf"], st["box"][0],
                                              st["box"][1], render.FORE, False)
            return (out * i["gout"]).sum()
        return leaves, fwd

    def encoder(seed=1):
        rng = SC._rng(seed, 19)
        N = 4096           # (from 4096 points on the table gradient takes the binned, bit-reproducible route)
        pts = torch.from_numpy(rng.uniform(-2, 2, (N, 3)).astype(SC.f32)).to(DEV)
        feat = torch.from_numpy(SC._table(rng, 16, SC.ENC_T)).to(DEV)
        gin = torch.from_numpy(rng.normal(size=(N, 16, 2)).astype(SC.f32)).to(DEV)
        res = SC._res16().to(DEV)
        leaves = [pts.requires_grad_(True), feat.requires_grad_(True)]
        return leaves, lambda: (HashEmbeddingBG(leaves[0], leaves[1], res).reshape(N, -1) * gin.reshape(N, -1)).sum()

    def decoder(seed=1):
        c = SC.BY_NAME["decoder"]
        i = c.to_device(c.build(seed))["in"]
        leaves = [i[k].detach().clone().requires_grad_(True) for k in ("feats", "dirs", "blob")]

        def fwd():
            sigma, dif, spec, tint = decoder_op.decoder_apply_parts(*leaves, i["wf"])
            return (torch.cat([sigma.reshape(-1, 1), dif, spec, tint], 1) * i["gw"]).sum()
        return leaves, fwd

    def composite(seed=1):
        c = SC.BY_NAME["composite"]
        i = c.to_device(c.build(seed))["in"]
        names = ("sigma", "dif", "spec", "tint", "z", "dists", "rays_d")
        ins = [i[k].detach().clone().requires_grad_(k in ("sigma", "dif", "spec", "tint", "rays_d")) for k in names]

        def fwd():
            out, w = render.composite_rays(*ins, True)
            return (out * i["go"]).sum() + (w * i["gw"]).sum()
        return [ins[j] for j in (0, 1, 2, 3, 6)], fwd

    return {"FusedRenderRays": fused, "HashEmbeddingBG": encoder, "decoder_op": decoder, "CompositeRays": composite}


@pytest.mark.parametrize("name", ["FusedRenderRays", "HashEmbeddingBG", "decoder_op", "CompositeRays"])
def test_e_autograd_backward_runs_on_the_forward_stream(name, side, monkeypatch):
    """The forward under `s`, .backward() from the default-stream context: the autograd engine runs a node's backward on the stream its
    forward ran on, so every backward library call must carry s's handle; after wait_stream the gradients equal the all-default run."""
    make = _autograd_cases()[name]
    leaves, fwd = make()
    fwd().backward()
    torch.cuda.synchronize()
    base = [t.grad.clone() for t in leaves]
    assert all(bool(torch.isfinite(g).all()) for g in base) and any(float(g.abs().max()) > 0 for g in base)

    rec = Recorder(monkeypatch)
    leaves, fwd = make()
    s = side.stream
    torch.cuda.synchronize()
    rec.take()
    with torch.cuda.stream(s):
        loss = fwd()
    n_forward = len(rec.calls)
    loss.backward()
    calls = rec.take()
    torch.cuda.current_stream().wait_stream(s)
    got = [t.grad.clone() for t in leaves]
    torch.cuda.synchronize()
    assert n_forward >= 1 and len(calls) > n_forward, "no library call in the backward"
    wrong = [k for k in calls if k.stream != s.cuda_stream]
    assert not wrong, f"{name}: library calls on another stream than the forward's: {[(k.name, hex(k.stream)) for k in wrong]}"
    assert same_bits(got, base), f"{name}: gradients differ from the all-default-stream run"


# ------------------------------------------------------------------------------------------------------------------ the default-stream call lists
STEP_CALLS = ["sample_points_grid", "ray_valid", "pack_decoder", "render_forward_packed_plan", "photometric_loss_grad", "render_backward",
              "render_scatter_accumulate_adam"]


def test_default_stream_call_lists(monkeypatch):
    """The launch sequence of the single-stream path, asserted: a change that adds a launch to it fails here (an added event or wait
    would be torch's, not the library's: the fixes add none on one stream, _capi.ordered_after compares two handles).  The registry's
    training-step and render-pass cases, then the package's own step -- tile_model.train_step_fused on an f32 and a bf16 table, two
    steps each: the code that builds TileModel.weight_feature, overflow_grad and gather_table lazily -- and HashGrid.samplePoints
    (HashGrid._converted).  Every call carries the null stream's handle."""
    from scanerf_amd.hashgrid import HashGrid
    from scanerf_amd.tile_model import TileModel, train_step_fused
    rec = Recorder(monkeypatch)
    lists = {}

    def record(name, fn):
        torch.cuda.synchronize()
        rec.take()
        fn()
        torch.cuda.synchronize()
        calls = rec.take()
        assert calls and all(k.stream == 0 for k in calls), [k for k in calls if k.stream != 0]
        lists[name] = [k.name.replace("scanerf_", "") for k in calls]

    for name in ("fused_t16s_plan", "fused_fgbg_pose", "render_time"):
        c = SC.BY_NAME[name]
        st = c.to_device(c.build(1))
        record(name, lambda: c.run(st))
    X = SC.BY_NAME["fused_t16s_plan"].build(1)
    o, d, tgt = (X[k].to(DEV) for k in ("o", "d", "target"))
    for tag, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=13, seed=1, table_dtype=dt)
        opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
        for i in range(2):
            record(f"train_step_fused {tag} step {i}", lambda: train_step_fused(m, opt, o, d, tgt, 16, 20000 + i))
    g = HashGrid(DEV, [-4.0, -4.0, -4.0], [8.0, 8.0, 8.0], log2_hashmap_size=10)
    for i in range(2):
        record(f"HashGrid.samplePoints call {i}", lambda: g.samplePoints(o, d, 16))
    for name, names in lists.items():
        print(f"\ndefault-stream calls of {name}: " + " ".join(names))
    assert lists["fused_t16s_plan"] == ["sample_points_grid", "pack_decoder", "render_forward_packed_plan", "photometric_loss_grad",
                                        "render_backward", "render_scatter_accumulate", "render_scatter_accumulate_adam"]
    assert lists["fused_fgbg_pose"] == ["sample_points_grid", "pack_decoder", "render_forward_packed_plan", "render_scatter_plan",
                                        "render_forward_packed_plan", "render_scatter_plan", "photometric_loss_grad_fgbg", "render_backward",
                                        "ray_grad_epilogue", "render_backward", "ray_grad_epilogue", "render_scatter_accumulate_adam2"]
    assert lists["render_time"] == ["ray_block_intersection", "sort_tracing_blocks", "get_last_block", "ray_firsthit_block",
                                    "render_sample_points", "prepare_points", "pack_decoder", "pack_decoder", "pack_decoder", "pts_inference",
                                    "pts_inference_tracing", "pts_normals"] + ["pts_normals_counted"] * _capi().has_symbol("scanerf_pts_normals_counted") + [
                                    "accumulate_normal", "accumulate_color", "update_outgoing_bidx", "update_outgoing_bidx_v2",
                                    "render_inverse_z_sampling", "bg_pts_inference_v2"] + ["process_occupied_grid"] * 3
    for name, names in lists.items():
        if name.startswith("train_step_fused"):
            assert names == STEP_CALLS, (name, names)
        if name.startswith("HashGrid"):
            assert names == ["sample_points_grid"], (name, names)


def test_zz_print_the_table():
    """`pytest -s`: the table of profiles/stream_contract.md (runs last in this file)."""
    print("\n| case | entries | host enqueue (ms) | delay (ms) | compared | synchronises | host read-back (delays re-armed) |")
    print("|---|---|---|---|---|---|---|")
    for r in TABLE:
        reads = f"{r['host_syncs']} ({r['rearmed']})" if r["host_syncs"] else "-"
        print(f"| {r['case']} | {' '.join(e.replace('scanerf_', '') for e in r['entries'])} | {r['enqueue_ms']:.2f} | {r['delay_ms']:.0f} | "
              f"{'bitwise' if r['exact'] else 'bounded'} | {' '.join(r['synchronises']) or '-'} | {reads} |")
    for line in STREAM_NOTE:
        print(line)
