"""The colour fusion on the GPU (csrc/tsdf.hip, scanerf_amd/fusion.py): cacc of the fused kernel against the composed
torch route against the numpy float32 restatement bit for bit at every point, against float64 within the derived bound on the judged
points; acc against the plain entries bit for bit; batch splits, a second run, a non-zero start, the counted entry; vertex_colors
against numpy; guard regions, refusals, empty calls; a side stream; and end to end on a traced icosphere, the small tile fixture and
the command."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import tsdf_color_reference as CR
import tsdf_reference as TR
from test_gpu_tsdf import DEV, GUARD, SENTINEL, _bits, _guarded, _guards_intact, _icosphere, _np, _trace_depth, tile_scene  # noqa: F401

pytestmark = pytest.mark.gpu
assert GUARD % 4 == 0      # a guarded cacc stays 16-byte aligned


def _inputs(c, cams=slice(None)):
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a[cams])).to(DEV)
    return g(c["depths"]), g(c["ks"]), g(c["c2ws"]), g(c["colors"])


def _volume(c, color=True):
    from scanerf_amd import fusion
    return fusion.TSDFVolume(c["origin"], c["spacing"], c["n"], c["trunc"], DEV, color=color)


def _integrate(c, route="fused", splits=(), start=None, cstart=None, counters=None, color=True):
    vol = _volume(c, color)
    if start is not None:
        vol.acc.copy_(torch.from_numpy(start).to(DEV))
    if cstart is not None:
        vol.cacc.copy_(torch.from_numpy(cstart).to(DEV))
    cuts = [0, *splits, len(c["ks"])]
    for a, b in zip(cuts[:-1], cuts[1:]):
        d, k, t, col = _inputs(c, slice(a, b))
        vol.integrate(d, k, t, near=c["near"], far=c["far"], route=route, counters=counters, colors=col if color else None)
    return vol


@functools.lru_cache(maxsize=None)
def fused(name):
    return _integrate(CR.case(name))


def _same_bits(vol, acc, cacc):
    return np.array_equal(_bits(_np(vol.acc)), _bits(acc)) and np.array_equal(_bits(_np(vol.cacc)), _bits(cacc))


# ---- the integration -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.CASES)
def test_fused_composed_and_numpy_float32_agree_in_every_bit(name):
    c = CR.case(name)
    got, witness = fused(name), _integrate(c, "composed")
    g, w, ref = _np(got.cacc), _np(witness.cacc), c["cref32"]["cacc"]
    assert g.dtype == np.float32 and g.shape == ref.shape
    d_np, d_w = _bits(g) != _bits(ref), _bits(g) != _bits(w)
    print(f"tsdf colour {name}: {g.shape[0]} points, sum Wc {g[:, 3].sum():.0f} of sum Wt {_np(got.acc)[:, 1].sum():.0f}; fused != numpy f32 in "
          f"{int(d_np.any(1).sum())} points, fused != composed in {int(d_w.any(1).sum())} points")
    assert not d_w.any(), "the fused kernel and the composed route (no skip) differ in cacc"
    assert not d_np.any(), "the fused kernel and the numpy float32 restatement differ in cacc"
    assert np.array_equal(_bits(_np(witness.acc)), _bits(_np(got.acc))) and np.array_equal(_bits(_np(got.acc)), _bits(c["cref32"]["acc"]))


@pytest.mark.parametrize("name", CR.CASES)
def test_fused_against_float64_on_the_judged_points(name):
    c = CR.case(name)
    got, a64, j, bound = _np(fused(name).cacc).astype(np.float64), c["cref64"]["cacc"], c["judged"], c["cref64"]["bound"]
    err = np.abs(got[:, :3] - a64[:, :3])
    print(f"tsdf colour {name}: judged {int(j.sum())} of {len(j)}; Wc mismatches on all points {int((got[:, 3] != a64[:, 3]).sum())}; "
          f"max |RGB - RGB64| judged {err[j].max() if j.any() else 0.0:.2e}, max error / bound {(err[j] / np.maximum(bound[j], 1e-300)).max() if j.any() else 0.0:.3f}")
    assert np.array_equal(got[j, 3], a64[j, 3])
    assert (err[j] <= bound[j]).all()


@pytest.mark.parametrize("name", CR.CASES)
def test_acc_of_the_colour_entries_equals_acc_of_the_plain_entries(name):
    c = CR.case(name)
    plain = _integrate(c, color=False)
    assert plain.cacc is None
    assert np.array_equal(_bits(_np(plain.acc)), _bits(_np(fused(name).acc)))
    counters = torch.zeros(4, dtype=torch.int64, device=DEV)
    assert np.array_equal(_bits(_np(plain.acc)), _bits(_np(_integrate(c, counters=counters).acc)))


@pytest.mark.parametrize("name", CR.CASES)
def test_batch_splits_and_a_second_run_give_equal_bits(name):
    from scanerf_amd import _capi
    c = CR.case(name)
    C, acc, cacc = len(c["ks"]), _np(fused(name).acc), _np(fused(name).cacc)
    per_pass = _capi.tool("scanerf_tsdf_cameras_per_pass")()
    if name == "sphere70":
        assert C > per_pass, "the case must take more than one pass"
    for k in sorted({1, per_pass, C - 1}):
        if 0 < k < C:
            assert _same_bits(_integrate(c, splits=(k,)), acc, cacc), (name, k)
    assert _same_bits(_integrate(c, splits=(C // 3, 2 * C // 3)), acc, cacc)
    assert _same_bits(_integrate(c), acc, cacc), "a second run differs"


@pytest.mark.parametrize("name", ["sphere40", "edges"])
def test_integrate_on_a_non_zero_start_of_both_accumulators(name):
    c = CR.case(name)
    rng = np.random.default_rng(12)
    P = c["cref32"]["acc"].shape[0]
    start = np.stack([rng.uniform(-3, 3, P), rng.integers(0, 5, P)], 1).astype(np.float32)
    cstart = np.concatenate([rng.uniform(-2, 2, (P, 3)), rng.integers(0, 5, (P, 1))], 1).astype(np.float32)
    want = CR.integrate(c, np.float32, acc=start, cacc=cstart)
    for route in ("fused", "composed"):
        assert _same_bits(_integrate(c, route, start=start, cstart=cstart), want["acc"], want["cacc"]), route
    untouched = c["cref32"]["cacc"][:, 3] == 0
    assert untouched.any() and np.array_equal(_bits(want["cacc"][untouched]), _bits(cstart[untouched]))


@pytest.mark.parametrize("name", CR.CASES)
def test_counted_entry_gives_the_same_sums_and_counts_the_coloured_pairs(name):
    c = CR.case(name)
    counters, plain = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    vol = _integrate(c, counters=counters)
    assert _same_bits(vol, _np(fused(name).acc), _np(fused(name).cacc))
    _integrate(c, counters=plain, color=False)
    pairs, skipped, updates, coloured = counters.tolist()
    print(f"tsdf colour {name}: pairs evaluated {pairs}, (block, camera) pairs skipped {skipped}, updates {updates}, coloured {coloured}")
    assert coloured == int(c["cref32"]["cacc"][:, 3].sum()) and updates == int(c["cref32"]["acc"][:, 1].sum())
    assert [pairs, skipped, updates] == plain.tolist()
    with pytest.raises(RuntimeError, match=r"counters must be a \[4\]"):
        _integrate(c, counters=plain)
    with pytest.raises(RuntimeError, match=r"counters must be a \[3\]"):
        _integrate(c, counters=counters, color=False)
    with pytest.raises(RuntimeError, match="counters belong to the fused route"):
        _integrate(c, "composed", counters=counters)


# ---- the colours at mesh vertices ------------------------------------------------------------------------------------------------------
HAND_CELLS = [[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1], [-1, 0, 0], [0, 2, 0], [0, 0, 2], [2, 2, 2], [0, 0, 0], [0, 0, 0], [1, 0, 1], [0, 1, 0]]
HAND_LATTICE = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1.5, 1.25, 1.75], [0.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 2.5], [2, 2, 2], [-3, 0, 0],
                [0, 7, math.nan], [1.3, 0.7, 1.1], [0.25, 1.0, 0.0]]


def _check_vertex_colors(vol, cacc, n, cells, lattice, what):
    from scanerf_amd import meshing
    mesh = meshing.Mesh(torch.zeros((len(cells), 3), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV),
                        torch.from_numpy(np.ascontiguousarray(cells, np.int32)).to(DEV),
                        torch.from_numpy(np.ascontiguousarray(lattice, np.float32)).to(DEV), None)
    rgb, weight = vol.vertex_colors(mesh, fill=-2.0)
    v32, v64 = CR.vertex_colors(cacc, n, cells, lattice, np.float32), CR.vertex_colors(cacc, n, cells, lattice, np.float64)
    none = v32["weight"] == 0
    want = np.where(none[:, None], np.float32(-2.0), v32["rgb"])
    got, w = _np(rgb), _np(weight)
    assert got.dtype == np.float32 and got.shape == (len(cells), 3) and w.shape == (len(cells),)
    err = np.abs(got.astype(np.float64) - v64["rgb"])[~none]
    print(f"tsdf colour {what}: V {len(cells)}, uncoloured {int(none.sum())}; rgb != numpy f32 in {int((_bits(got) != _bits(want)).any(1).sum())} vertices, "
          f"weight in {int((_bits(w) != _bits(v32['weight'])).sum())}; max |rgb - rgb64| {err.max() if err.size else 0.0:.2e}, max error / bound "
          f"{(err / np.maximum(v64['bound'][~none], 1e-300)).max() if err.size else 0.0:.3f}")
    assert np.array_equal(_bits(w), _bits(v32["weight"])) and np.array_equal(_bits(got), _bits(want))
    assert v64["judged"].all() and (err <= v64["bound"][~none]).all()
    assert (np.abs(w.astype(np.float64) - v64["weight"]) <= v64["weight_bound"]).all()
    return got, w


@pytest.mark.parametrize("name", CR.SPHERES)
def test_vertex_colors_against_numpy_on_the_culled_and_the_raw_mesh(name):
    from scanerf_amd import meshing
    c = CR.case(name)
    vol = fused(name)
    raw, mesh = CR.reference_mesh(c)
    for what, m in (("culled", mesh), ("raw", raw)):
        _check_vertex_colors(vol, c["cref32"]["cacc"], c["n"], m.cells, m.lattice, f"{name} {what}")
    # and on the library's own mesh: extract(colors=True) is vertex_colors on what extract() returns
    report = {}
    got, rgb = vol.extract(report=report, colors=True)
    plain = vol.extract()
    assert isinstance(got, meshing.Mesh) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, plain))
    want = CR.vertex_colors(c["cref32"]["cacc"], c["n"], _np(got.cells), _np(got.lattice), np.float32)
    assert report["color"] == 0 and (want["weight"] > 0).all() and np.array_equal(_bits(_np(rgb)), _bits(want["rgb"]))
    err = np.abs(_np(rgb).astype(np.float64) - CR.radial_answer(_np(got.vertices))).max(1)
    print(f"tsdf colour {name}: library mesh V {len(err)}, radial colour error max {err.max():.4f} mean {err.mean():.4f}")
    assert err.max() <= CR.RADIAL_MARGIN * CR.RADIAL_MAX[name]


def test_vertex_colors_on_hand_built_cells():
    c = CR.case("edges")
    n = c["n"]
    cacc = c["cref32"]["cacc"].copy()
    lone = TR.point_index(n, (2, 2, 2))      # cell (2, 2, 2) .. (3, 3, 3) loses every colour but one corner's: an all-uncoloured cell next to it
    for d in range(8):
        cacc[TR.point_index(n, (2 + (d >> 2), 2 + ((d >> 1) & 1), 2 + (d & 1)))] = 0
    assert cacc[lone].tolist() == [0, 0, 0, 0]
    vol = _volume(c)
    vol.cacc.copy_(torch.from_numpy(cacc).to(DEV))
    cells, lattice = np.asarray(HAND_CELLS, np.int32), np.asarray(HAND_LATTICE, np.float32)
    cells[5], cells[6] = (0, n[1], 0), (0, 0, n[2])      # one past the last cell on an axis
    got, w = _check_vertex_colors(vol, cacc, n, cells, lattice, "hand-built")
    assert (got[[4, 5, 6]] == -2.0).all() and not w[[4, 5, 6]].any()      # outside the lattice: nothing read, the fill
    assert (got[7] == -2.0).all() and w[7] == 0                              # the all-uncoloured cell
    p0, p7 = cacc[TR.point_index(n, (0, 0, 0))], cacc[TR.point_index(n, (1, 1, 1))]
    assert np.array_equal(got[0], p0[:3] / p0[3]) and w[0] == p0[3]          # t = 0 on every axis: corner 0 alone
    assert np.array_equal(got[1], p7[:3] / p7[3]) and w[1] == p7[3]          # t = 1: corner 7 alone
    assert np.array_equal(got[8], got[0])                                    # t clamped to 0
    # the default fill, and no vertex at all
    from scanerf_amd import meshing
    mesh = lambda cc, ll: meshing.Mesh(torch.zeros((len(cc), 3), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV),
                                       torch.from_numpy(cc).to(DEV), torch.from_numpy(ll).to(DEV), None)
    rgb, weight = vol.vertex_colors(mesh(cells[4:8], lattice[4:8]))
    assert (rgb == 0.5).all() and not weight.any()
    rgb, weight = vol.vertex_colors(mesh(cells[:0], lattice[:0]))
    assert rgb.shape == (0, 3) and weight.shape == (0,)


# ---- the C entries on guarded buffers ------------------------------------------------------------------------------------------------
def _head(c, acc, cacc):
    d, k, t, col = _inputs(c)
    k9, c12 = k.reshape(-1, 9).contiguous(), t.reshape(-1, 12).contiguous()
    o, s = (ctypes.c_float * 3)(*c["origin"]), (ctypes.c_float * 3)(*c["spacing"])
    keep = (d, col, k9, c12, o, s)
    return keep, dict(depths=d.data_ptr(), colors=col.data_ptr(), Ks=k9.data_ptr(), C2Ws=c12.data_ptr(), C=len(k9), H=d.shape[1], W=d.shape[2],
                      origin=o, spacing=s, nx=c["n"][0], ny=c["n"][1], nz=c["n"][2], trunc=c["trunc"], near=c["near"], far=c["far"],
                      acc=acc.data_ptr(), cacc=cacc.data_ptr())


@pytest.mark.parametrize("name", ["sphere40", "edges"])
def test_guard_regions_are_untouched_and_exactly_the_outputs_are_written(name):
    from scanerf_amd import _capi
    c = CR.case(name)
    ref = c["cref32"]
    P = ref["acc"].shape[0]
    abuf, acc = _guarded((P, 2), torch.float32, SENTINEL)
    cbuf, cacc = _guarded((P, 4), torch.float32, SENTINEL)
    assert cacc.data_ptr() % 16 == 0
    keep, head = _head(c, acc, cacc)
    st = torch.cuda.current_stream().cuda_stream
    integrate = _capi.tool("scanerf_tsdf_integrate_color")
    acc.zero_(), cacc.zero_()
    assert integrate(*head.values(), st) == 0
    assert np.array_equal(_bits(_np(acc)), _bits(ref["acc"])) and np.array_equal(_bits(_np(cacc)), _bits(ref["cacc"]))
    assert _guards_intact(abuf, SENTINEL) and _guards_intact(cbuf, SENTINEL)
    # a row no camera observes (coloured) keeps the caller's bits, a row one observes (colours) is replaced: nothing else is written
    acc.fill_(SENTINEL), cacc.fill_(SENTINEL)
    assert integrate(*head.values(), st) == 0
    a, ca = _np(acc), _np(cacc)
    seen, coloured = ref["acc"][:, 1] > 0, ref["cacc"][:, 3] > 0
    assert (~coloured).any() and (seen & ~coloured).any()
    assert (a[~seen] == SENTINEL).all() and (a[seen, 1] == SENTINEL + ref["acc"][seen, 1]).all()
    assert (ca[~coloured] == SENTINEL).all() and (ca[coloured, 3] == SENTINEL + ref["cacc"][coloured, 3]).all()
    assert _guards_intact(abuf, SENTINEL) and _guards_intact(cbuf, SENTINEL)
    # vertex colours: every element of rgb and weight written once, nothing outside, cacc not written
    cacc.copy_(torch.from_numpy(ref["cacc"]).to(DEV))
    rng = np.random.default_rng(2)
    V = 301
    cells = np.stack([rng.integers(-1, m + 1, V) for m in c["n"]], 1).astype(np.int32)
    lattice = (cells + rng.uniform(-0.1, 1.1, (V, 3))).astype(np.float32)
    rbuf, rgb = _guarded((V, 3), torch.float32, SENTINEL)
    wbuf, weight = _guarded((V,), torch.float32, SENTINEL)
    cd, ld = torch.from_numpy(cells).to(DEV), torch.from_numpy(lattice).to(DEV)
    assert _capi.tool("scanerf_tsdf_vertex_colors")(cacc.data_ptr(), *c["n"], cd.data_ptr(), ld.data_ptr(), V, rgb.data_ptr(), weight.data_ptr(), st) == 0
    want = CR.vertex_colors(ref["cacc"], c["n"], cells, lattice, np.float32)
    assert np.array_equal(_bits(_np(rgb)), _bits(want["rgb"])) and np.array_equal(_bits(_np(weight)), _bits(want["weight"]))
    outside = ((cells < 0) | (cells >= np.asarray(c["n"]))).any(1)
    assert outside.any() and not _np(rgb)[outside].any() and not _np(weight)[outside].any()
    assert _guards_intact(rbuf, SENTINEL) and _guards_intact(wbuf, SENTINEL) and _guards_intact(cbuf, SENTINEL)
    assert np.array_equal(_bits(_np(cacc)), _bits(ref["cacc"]))
    del keep


def test_refusals_with_device_pointers_write_nothing_and_empty_calls_launch_nothing():
    from scanerf_amd import _capi
    c = CR.case("edges")
    P = c["cref32"]["acc"].shape[0]
    abuf, acc = _guarded((P, 2), torch.float32, SENTINEL)
    cbuf, cacc = _guarded((P, 4), torch.float32, SENTINEL)
    keep, ok = _head(c, acc, cacc)
    st = torch.cuda.current_stream().cuda_stream
    integrate, counted = _capi.tool("scanerf_tsdf_integrate_color"), _capi.tool("scanerf_tsdf_integrate_color_counted")
    ctr = torch.zeros(4, dtype=torch.int64, device=DEV)
    for over in ({"C": -1}, {"H": 0}, {"W": -1}, {"nx": 0}, {"trunc": 0.0}, {"trunc": math.inf}, {"near": -1.0}, {"near": math.nan},
                 {"far": 0.125}, {"far": math.nan}, {"spacing": (ctypes.c_float * 3)(0.25, 0.0, 0.25)}, {"depths": None}, {"colors": None},
                 {"acc": None}, {"cacc": None}, {"cacc": cacc.data_ptr() + 4}, {"nx": 2047, "ny": 2047, "nz": 2047}):
        a = {**ok, **over}
        assert integrate(*a.values(), st) != 0, over
        assert counted(*a.values(), ctr.data_ptr(), st) != 0, over
    assert counted(*ok.values(), None, st) != 0
    assert integrate(*{**ok, "C": 0}.values(), st) == 0      # C == 0: nothing is launched, nothing written
    assert counted(*{**ok, "C": 0}.values(), ctr.data_ptr(), st) == 0
    colors = _capi.tool("scanerf_tsdf_vertex_colors")
    rbuf, rgb = _guarded((8, 3), torch.float32, SENTINEL)
    wbuf, weight = _guarded((8,), torch.float32, SENTINEL)
    cells, lattice = torch.zeros((8, 3), dtype=torch.int32, device=DEV), torch.zeros((8, 3), device=DEV)
    good = (cacc.data_ptr(), 4, 4, 4, cells.data_ptr(), lattice.data_ptr(), 8, rgb.data_ptr(), weight.data_ptr())
    for i, bad in ((0, None), (0, cacc.data_ptr() + 8), (1, 0), (2, -1), (4, None), (5, None), (6, -1), (7, None), (8, None)):
        args = list(good)
        args[i] = bad
        assert colors(*args, st) != 0, (i, bad)
    assert colors(cacc.data_ptr(), 2047, 2047, 2047, cells.data_ptr(), lattice.data_ptr(), 8, rgb.data_ptr(), weight.data_ptr(), st) != 0
    args = list(good)
    args[6] = 0
    assert colors(*args, st) == 0      # V == 0
    torch.cuda.synchronize()
    for b in (abuf, cbuf, rbuf, wbuf):
        assert bool((b == SENTINEL).all()), "a refused or empty call wrote something"
    assert not ctr.any()
    # the Python level: no camera
    vol = _volume(c)
    d, k, t, col = _inputs(c)
    vol.integrate(d[:0], k[:0], t[:0], near=c["near"], far=c["far"], colors=col[:0])
    assert not vol.acc.any() and not vol.cacc.any()
    report = {}
    empty, rgb0 = vol.extract(report=report, colors=True)
    assert empty.vertices.shape == (0, 3) and rgb0.shape == (0, 3) and report["color"] == 0
    del keep


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def test_stream_the_new_ops_run_on_the_callers_stream(monkeypatch):
    import stream_cases as SC
    from scanerf_amd import _capi
    from test_gpu_stream_contract import Delay, same_bits
    names = ("scanerf_tsdf_integrate_color", "scanerf_tsdf_vertex_colors")
    n = (24, 20, 28)

    def build(seed):
        c = TR.sphere("stream", 40, 48, 64, n, 600 + seed)
        colors = CR.radial_colors(c["ks"], c["c2ws"], c["depths"]) * np.float32(1.0 - 0.1 * seed)
        return {"depths": torch.from_numpy(c["depths"] * np.float32(1.0 + 0.01 * seed)), "ks": torch.from_numpy(c["ks"]),
                "c2ws": torch.from_numpy(c["c2ws"]), "colors": torch.from_numpy(colors)}

    def setup(state):
        from scanerf_amd import meshing
        rng = np.random.default_rng(9)
        cells = np.stack([rng.integers(0, m, 4000) for m in n], 1).astype(np.int32)
        lattice = (cells + rng.uniform(0, 1, cells.shape)).astype(np.float32)
        state["mesh"] = meshing.Mesh(torch.zeros((4000, 3), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV),
                                     torch.from_numpy(cells).to(DEV), torch.from_numpy(lattice).to(DEV), None)

    def run_(state):
        from scanerf_amd import fusion
        i = state["in"]
        vol = fusion.TSDFVolume([TR.BOX[0]] * 3, [TR.BOX[1] / m for m in n], n, TR.TRUNC, DEV, color=True)
        vol.integrate(i["depths"], i["ks"], i["c2ws"], near=TR.NEAR, far=TR.FAR, colors=i["colors"])
        rgb, weight = vol.vertex_colors(state["mesh"])
        return vol.acc, vol.cacc, rgb, weight

    c = SC.Case("tsdf_color", list(names), build, run_, setup=setup)
    X, Y = c.build(1), c.build(2)
    assert all(not torch.equal(X[k], Y[k]) and X[k].shape == Y[k].shape for k in X)
    state = c.to_device(X)
    Xd, Yd = SC.stage(X), SC.stage(Y)
    handles = []
    for name in names:
        real = _capi.tool(name)

        def recorded(*a, _real=real):
            handles.append(int(a[-1] or 0))
            return _real(*a)
        monkeypatch.setitem(_capi._tools, name, recorded)
    torch.cuda.synchronize()
    R_X = c.run(state)
    c.refill(state, Yd)
    R_Y = c.run(state)
    torch.cuda.synchronize()
    assert not same_bits(R_X, R_Y), "the two seeds give the same answer: a stale read would not show"
    assert not same_bits(R_X[1:2], R_Y[1:2]) and not same_bits(R_X[2:3], R_Y[2:3])      # cacc and rgb themselves differ
    assert handles == [torch.cuda.current_stream().cuda_stream] * 4
    delay = Delay()
    s = torch.cuda.Stream()
    del handles[:]
    with torch.cuda.stream(s):
        pending = delay(20.0)
        c.refill(state, Xd)           # queued behind the delay: a launch on any other stream reads Y
        R = c.run(state)
        still = not pending.query()
    s.synchronize()
    torch.cuda.synchronize()
    assert handles == [s.cuda_stream] * 2 and s.cuda_stream != 0, "a call did not carry the caller's stream"
    assert still, "a call waited for its stream (the delay ran out before it returned)"
    assert same_bits(R, R_X), "under a side stream an op read stale inputs: a launch went to another stream"


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_a_traced_icosphere_with_the_radial_colour_map():
    from scanerf_amd import fusion
    from scanerf_amd.fastmesh import FastMesh
    from test_gpu_mesh_components import _same
    c = TR.case("sphere40")
    V, F = _icosphere(TR.RADIUS, 3)
    fm = FastMesh.from_arrays(V, F, DEV)
    H, W = c["depths"].shape[1:]
    depths = _trace_depth(fm, c["ks"], c["c2ws"], H, W)
    colors = torch.from_numpy(CR.radial_colors(c["ks"], c["c2ws"], _np(depths))).to(DEV)
    kw = dict(trunc=TR.TRUNC, views_per_batch=7, near=TR.NEAR, far=TR.FAR)
    report = {}
    mesh, rgb = fusion.fuse_depth_maps(depths, c["ks"], c["c2ws"], c["origin"], [TR.BOX[1]] * 3, c["n"], report=report, colors=colors, **kw)
    plain = fusion.fuse_depth_maps(depths, c["ks"], c["c2ws"], c["origin"], [TR.BOX[1]] * 3, c["n"], **kw)
    _same(mesh, plain, "fuse_depth_maps with colours against the call without")
    assert rgb.shape == mesh.vertices.shape and rgb.dtype == torch.float32 and mesh.vertices.shape[0] > 100
    err = np.abs(_np(rgb).astype(np.float64) - CR.radial_answer(_np(mesh.vertices))).max(1)
    print(f"tsdf colour end to end: V {len(err)}, uncoloured {report['color']}, radial colour error max {err.max():.4f} mean {err.mean():.4f} "
          f"(the reference mesh: {CR.RADIAL_MAX['sphere40']})")
    assert report["color"] == 0 and report["components"] == 1
    assert err.max() <= CR.RADIAL_MARGIN * CR.RADIAL_MAX["sphere40"]


def _renders(rnd, cams, scale, max_transparency, source):
    from scanerf_amd import fusion
    ks, c2ws, H, W = cams
    h, w = H // scale, W // scale
    k2 = fusion.scale_cameras(ks, scale)
    maps, images = [], []
    for K, c2w in zip(k2, torch.as_tensor(c2ws)):
        diffuse, specular, depth, transp = rnd.render(h, w, K, c2w)
        maps.append(fusion.mask_depth(depth[..., 0], transp[..., 0], max_transparency))
        images.append(torch.clamp(diffuse + specular if source == "rgb" else diffuse, 0.0, 1.0))
    return k2, torch.stack(maps).contiguous(), torch.stack(images).contiguous()


@pytest.mark.parametrize("source", ["diffuse", "rgb"])
def test_fuse_mesh_with_colours_equals_fuse_depth_maps_on_its_renders(tile_scene, source):  # noqa: F811
    from scanerf_amd import fusion, meshing
    from test_gpu_mesh_components import _same
    rnd, cams = tile_scene["rnd"], tile_scene["cameras"]
    kw = dict(cells_per_axis=20, max_transparency=0.9, scale=2, views_per_batch=2)
    report = {}
    mesh, rgb = rnd.fuse_mesh(cams, report=report, colors=source, **kw)
    plain = rnd.fuse_mesh(cams, **kw)
    assert isinstance(plain, meshing.Mesh) and isinstance(mesh, meshing.Mesh)
    _same(mesh, plain, "fuse_mesh with colours against fuse_mesh without")
    k2, maps, images = _renders(rnd, cams, 2, 0.9, source)
    corner, size = rnd.scene_box()
    n = meshing.cells_per_axis(size, 20)
    want, want_rgb = fusion.fuse_depth_maps(maps, k2, cams[1], corner, size, n, views_per_batch=5, colors=images)
    _same(mesh, want, "fuse_mesh against fuse_depth_maps on the same masked renders")
    assert rgb.shape == mesh.vertices.shape and torch.equal(rgb.view(torch.int32), want_rgb.view(torch.int32))
    coloured = int(mesh.vertices.shape[0]) - report["color"]
    print(f"tsdf colour tile fixture ({source}): V {mesh.vertices.shape[0]}, coloured {coloured}; rgb in [{float(rgb.min()):.3f}, {float(rgb.max()):.3f}], "
          f"mean {[round(float(v), 3) for v in rgb.mean(0)]}")
    assert mesh.vertices.shape[0] > 100 and coloured > 0 and bool(torch.isfinite(rgb).all())
    assert float(images.min()) >= 0.0 and float(images.max()) <= 1.0
    if source == "rgb":      # recorded, not asserted: whether the fixture's specular part moves a colour at all
        diffuse_only = _renders(rnd, cams, 2, 0.9, "diffuse")[2]
        print(f"tsdf colour tile fixture: diffuse + specular differs from diffuse in {int((diffuse_only != images).any(-1).sum())} of {images[..., 0].numel()} pixels")


def test_the_command_writes_a_coloured_ply_that_reads_back(tile_scene, tmp_path, capsys):  # noqa: F811
    from scanerf_amd import formats
    from test_gpu_mesh_components import _tool
    out = str(tmp_path / "fused_colour.ply")
    assert _tool("fuse_mesh").main([tile_scene["path"], "--cameras", tile_scene["log"], "--out", out, "--cells-per-axis", "20", "--scale", "2",
                                    "--max-transparency", "0.9", "--views-per-batch", "2", "--colors", "diffuse"]) == 0
    want, rgb = tile_scene["rnd"].fuse_mesh(tile_scene["cameras"], cells_per_axis=20, max_transparency=0.9, scale=2, views_per_batch=2,
                                            colors="diffuse")
    v, f, col = formats.read_ply(out, colors=True)
    assert np.array_equal(np.asarray(v, np.float32).reshape(-1, 3), _np(want.vertices)) and np.array_equal(np.asarray(f, np.int32).reshape(-1, 3), _np(want.faces))
    quantised = np.floor(np.clip(_np(rgb).astype(np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    assert col.dtype == np.uint8 and np.array_equal(col, quantised) and len(np.unique(col)) > 3
    printed = capsys.readouterr().out
    assert "colours (diffuse)" in printed and "5 cameras" in printed
