"""tile_model.table_grad_route, the one decision of how a training step's feature gradients reach the table, pinned over
table sizes, arithmetics, half tables, fused_adam, LARGE_T_ROUTE, fused_scatter and every entry point.  `expected` restates,
per entry point, the conditions each step function carried inline before the decision moved into one place; the only
difference is the rays route's upper bound T <= 2^24 (csrc/scatter.hip seg_route: NB <= 2048), so that T = 2^25 takes the
contracted points instead of a rays entry that raises.  No GPU: the function allocates and launches nothing."""
import itertools

import pytest

import scanerf_amd  # noqa: F401
from scanerf_amd import _capi, render
from scanerf_amd import tile_model as tm

F32, H3, T16, T16S = _capi.ARITH_F32, _capi.ARITH_H3, _capi.ARITH_T16, _capi.ARITH_T16S
LOG2_T = (19, 21, 22, 24, 25)
B, S_FG, S_BG = 16384, 128, 64
RA, RT, YA, PA, PT = tm.RECORDS_ADAM, tm.RECORDS_TABLE, tm.RAYS_ADAM, tm.POINTS_ADAM, tm.POINTS_TABLE


def expected(entry, T, arith, half, fused_adam, large_t_route, fused_scatter, S):
    small = T <= 1 << 21
    supported = [render.scatter_supported(B, s, T) for s in S]
    fmt = {T16: 1, T16S: 2}.get(arith, 0)
    rays = 1 << 22 <= T <= 1 << 24 and arith == T16S
    if entry == tm.SINGLE:   # train_step_fused: not excluded under f32
        fused = (small or large_t_route == "fused") if fused_scatter is None else fused_scatter
        if fused and supported[0]:
            return (RA if fused_adam else RT,), fmt
        if not fused_adam:   # compact records only above 2^21
            return (PT,), (fmt if not small else -1)
        return (YA if rays and not half else PA,), fmt
    if entry == tm.FGBG_STEP:   # records need both branches' workspaces and a backward other than f32
        if (small or large_t_route == "fused") and all(supported) and arith != F32:
            return (RA, RA), fmt
        if not small and arith != F32 and not half:   # the binned scatter over both branches
            return ((YA, YA) if rays else (PA, PA)), fmt
    if entry in (tm.FGBG_STEP, tm.FGBG_GRADIENTS):   # per branch, LARGE_T_ROUTE ignored: records under f32 too
        return tuple(RT if small and ok else PT for ok in supported), -1
    return (RT if small and supported[0] else PT,), -1   # AUTOGRAD


CASES = list(itertools.product((tm.SINGLE, tm.FGBG_STEP, tm.FGBG_GRADIENTS, tm.AUTOGRAD), LOG2_T, (F32, H3, T16, T16S),
                               (False, True), (False, True), ("dfeat", "fused"), (None, False, True)))


def test_route_matches_the_step_functions_conditions(monkeypatch):
    wrong = []
    for entry, log2_T, arith, half, fused_adam, large_t_route, fused_scatter in CASES:
        monkeypatch.setattr(tm, "LARGE_T_ROUTE", large_t_route)
        T = 1 << log2_T
        S = [S_FG] if entry in (tm.SINGLE, tm.AUTOGRAD) else [S_FG, S_BG]
        got = tm.table_grad_route(entry, T, B, S, arith, half, fused_adam, fused_scatter)
        want = expected(entry, T, arith, half, fused_adam, large_t_route, fused_scatter, S)
        if got != want:
            wrong.append((entry, log2_T, arith, half, fused_adam, large_t_route, fused_scatter, got, want))
    assert not wrong, f"{len(wrong)} of {len(CASES)} cases differ, first: {wrong[:3]}"


# Explicit rows, one reason each.
ROWS = [
    # (entry, log2 T, arith, half, fused_adam, LARGE_T_ROUTE, fused_scatter) -> (routes, compact_records)
    ((tm.SINGLE, 19, T16S, False, True, "dfeat", None), ((RA,), 2)),      # the headline: records + accumulate_adam
    ((tm.SINGLE, 19, F32, False, True, "dfeat", None), ((RA,), 0)),       # single branch: f32 keeps the records
    ((tm.SINGLE, 19, T16S, False, False, "dfeat", None), ((RT,), 2)),     # fused_adam=False: records into a gradient table
    ((tm.SINGLE, 19, T16S, False, True, "dfeat", False), ((PA,), 2)),     # bench --scatter dfeat at a small table
    ((tm.SINGLE, 19, T16, False, False, "dfeat", False), ((PT,), -1)),    # ... without fused_adam: default records at 2^21 and below
    ((tm.SINGLE, 22, T16, False, False, "dfeat", None), ((PT,), 1)),      # ... the compact ones above
    ((tm.SINGLE, 24, T16S, False, True, "dfeat", None), ((YA,), 2)),      # large tables: the rays scatter
    ((tm.SINGLE, 24, T16S, False, True, "fused", None), ((RA,), 2)),      # LARGE_T_ROUTE = "fused": records + split pass
    ((tm.SINGLE, 24, T16S, True, True, "dfeat", None), ((PA,), 2)),       # a half table keeps the rays scatter off
    ((tm.SINGLE, 24, T16, False, True, "dfeat", None), ((PA,), 1)),       # 8-byte records: no rays scatter
    ((tm.SINGLE, 25, T16S, False, True, "dfeat", None), ((PA,), 2)),      # T = 2^25: past the segment producer -> points
    ((tm.SINGLE, 25, T16S, False, True, "fused", None), ((PA,), 2)),      # ... and no record workspace for the fused route
    ((tm.FGBG_STEP, 19, T16S, False, True, "dfeat", None), ((RA, RA), 2)),   # records + adam2
    ((tm.FGBG_STEP, 19, F32, False, True, "dfeat", None), ((RT, RT), -1)),   # f32: gradient table, records fill it
    ((tm.FGBG_STEP, 22, F32, False, True, "dfeat", None), ((PT, PT), -1)),   # f32 above 2^21: points into the table
    ((tm.FGBG_STEP, 22, T16S, False, True, "dfeat", None), ((YA, YA), 2)),   # one rays scatter over both branches
    ((tm.FGBG_STEP, 24, T16, False, True, "dfeat", None), ((PA, PA), 1)),    # one points scatter over both branches
    ((tm.FGBG_STEP, 24, T16S, True, True, "dfeat", None), ((PT, PT), -1)),   # half table: the gradient table
    ((tm.FGBG_STEP, 25, T16S, False, True, "dfeat", None), ((PA, PA), 2)),   # T = 2^25: points, not the rays entry
    ((tm.FGBG_GRADIENTS, 19, T16S, False, True, "fused", None), ((RT, RT), -1)),  # the reference: records into the table
    ((tm.FGBG_GRADIENTS, 22, T16S, False, True, "fused", None), ((PT, PT), -1)),  # ... LARGE_T_ROUTE ignored
    ((tm.AUTOGRAD, 21, T16S, False, True, "dfeat", None), ((RT,), -1)),
    ((tm.AUTOGRAD, 22, T16S, False, True, "fused", None), ((PT,), -1)),
]


@pytest.mark.parametrize("case,want", ROWS)
def test_route_rows(monkeypatch, case, want):
    entry, log2_T, arith, half, fused_adam, large_t_route, fused_scatter = case
    monkeypatch.setattr(tm, "LARGE_T_ROUTE", large_t_route)
    S = [S_FG] if entry in (tm.SINGLE, tm.AUTOGRAD) else [S_FG, S_BG]
    assert tm.table_grad_route(entry, 1 << log2_T, B, S, arith, half, fused_adam, fused_scatter) == want


def test_rays_route_stops_where_the_segment_producer_does():
    assert [render.scatter_rays_supported(1 << t, T16S) for t in LOG2_T] == [False, False, True, True, False]
    assert not any(render.scatter_rays_supported(1 << t, a) for t in LOG2_T for a in (F32, H3, T16))


def test_records_fill_a_per_branch_table_where_one_branch_has_no_workspace():
    # a batch whose foreground records do not fit while the background's do: each branch of the gradient-table route decides
    # for itself (B = 2^20 rays fit no record workspace at S = 128)
    big = 1 << 20
    assert [render.scatter_supported(big, s, 1 << 19) for s in (128, 2)] == [False, True]
    assert tm.table_grad_route(tm.FGBG_GRADIENTS, 1 << 19, big, [128, 2], T16S) == ((PT, RT), -1)
