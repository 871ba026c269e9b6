"""CPU checks of tests/warp_cases.py, on the reference alone: every case of tests/test_gpu_warp_edges.py contains the edge it is
named for, the rays a judgement leaves out stay under their caps, the float32 yardstick is finite and non-zero for every judged
quantity, and warp_reference.select breaks exact ties by the lower camera index (the rule the selection kernel is held to)."""
import math

import pytest
import torch

import warp_cases as WC
import warp_reference as WR

F64, F32 = torch.float64, torch.float32
ids = lambda cases: [WC.case_id(c) for c in cases]


# ---- the tie rule ---------------------------------------------------------------------------------------------------------
def test_reference_select_breaks_exact_ties_by_lower_index():
    """Hand-built cost rows with exact ties; the first is the example of the selection kernel's former defect (a carried entry that
    ties with the next one was dropped: [2, 1] instead of [2, 0])."""
    rows = [([0.1, 0.1, 0.05], 2, [2, 0]),
            ([0.5, 0.1, 0.1, 1.0, 0.05, 0.1], 3, [4, 1, 2]),
            ([0.1, 0.1, 0.1, 0.1], 2, [0, 1]),
            ([0.1, 0.05, 0.1, 0.05, 0.1], 4, [1, 3, 0, 2]),
            ([1.0, 1.0, 1.0], 2, [0, 1])]
    for row, k, want in rows:
        v, c, _ = WR.select(torch.tensor([row], dtype=F64), k)
        assert v[0].tolist() == want, (row, k)
        assert WC.tie_model(row, k, fixed=True) == want, (row, k)
    assert WC.tie_model(rows[0][0], 2, fixed=False) == [2, 1]     # what the strict < on the carried entry gave


def test_tie_model_of_the_fixed_insert_is_a_stable_sort():
    g = torch.Generator().manual_seed(0)
    values = torch.tensor([0.05, 0.1, 0.17, 1.0], dtype=F64)
    differs = 0
    for _ in range(2000):
        n = int(torch.randint(1, 9, (1,), generator=g))
        k = int(torch.randint(1, n + 1, (1,), generator=g))
        row = values[torch.randint(0, 4, (n,), generator=g)]
        want = WR.select(row[None], k)[0][0].tolist()
        assert WC.tie_model(row.tolist(), k, fixed=True) == want
        differs += WC.tie_model(row.tolist(), k, fixed=False) != want
    assert differs > 100   # the draws do reach the defect


# ---- selection cases ------------------------------------------------------------------------------------------------------
def test_selection_case_list_covers_the_edges():
    ns = {c.N for c in WC.CASES_SELECT}
    assert {1, 2, 9, 255, 256, 257, 513} <= ns
    assert {1, 255, 256, 257, 1000} <= {c.B for c in WC.CASES_SELECT}
    assert any(c.N == 16 and c.top_k == WC.MAX_NEIGHBORS for c in WC.CASES_SELECT)
    assert {c.ray_valid for c in WC.CASES_SELECT} == {None, "mixed", "none"}
    assert [(c.N, c.top_k, c.B) for c in WC.CASES_DUPLICATES] == [(24, 10, 1000), (24, 5, 1000), (24, 3, 1000), (40, 7, 1000)]


@pytest.mark.parametrize("c", WC.CASES_SELECT, ids=ids(WC.CASES_SELECT))
def test_selection_case_ambiguity_cap_and_edge(c):
    sc = WC.case_scene(c)
    K = WC.case_K(c)
    amb = WC.ambiguous_rays(sc, K)
    cap = WC.CAP_AMBIGUOUS_DUP if c.duplicates else WC.CAP_AMBIGUOUS
    print(f"{c.name}: {int(amb.sum())} of {c.B} rays ambiguous")
    assert int(amb.sum()) <= cap * c.B
    views, cost, valid = WC.select_reference(sc, K)
    if c.ray_valid == "none":
        assert not bool(valid.any())
        return
    assert int(valid.sum()) >= max(1, c.B // 2)          # the scene does produce neighbours
    m = valid & ~amb[:, None]
    f = WC.PR.figures(WC.costs(sc, F32).gather(1, views)[m][:, None], cost[m][:, None], torch.ones(int(m.sum()), dtype=F64))
    assert all(math.isfinite(x) and 0 < x < 1e-5 for x in f.values()), f          # the yardstick of the costs
    if c.ray_valid == "mixed" and c.B > 1:
        assert 0 < int(sc.ray_valid.sum()) < c.B
    # cameras past every LDS pass of 256 are among the neighbours
    for first in range(256, c.N, 256):
        assert bool((views[valid] >= first).any()), first
    if K == WC.MAX_NEIGHBORS:
        assert views.shape[1] == 16
    if c.N < 10:
        assert K == c.N


@pytest.mark.parametrize("c", WC.CASES_DUPLICATES, ids=ids(WC.CASES_DUPLICATES))
def test_duplicate_scenes_hold_exact_ties(c):
    sc = WC.case_scene(c)
    h, K = c.N // 2, WC.case_K(c)
    assert torch.equal(sc.ks[:h], sc.ks[h:]) and torch.equal(sc.rts[:h], sc.rts[h:])
    c64, c32 = WC.costs(sc, F64), WC.costs(sc, F32)
    assert torch.equal(c64[:, :h], c64[:, h:]) and torch.equal(c32[:, :h], c32[:, h:])     # bit-equal in both precisions
    views, _, valid = WC.select_reference(sc, K)
    pair = (views[:, 1:] == views[:, :-1] + h) & valid[:, 1:] & valid[:, :-1]
    assert float(pair.any(1).float().mean()) >= 0.30
    srt, idx = torch.sort(c64, dim=1, stable=True)
    straddle = (idx[:, K] == idx[:, K - 1] + h) & (srt[:, K] <= WR.VALID_COST)
    print(f"{c.name}: duplicate pair in the kept slots {float(pair.any(1).float().mean()):.3f}, straddling slot K "
          f"{float(straddle.float().mean()):.3f}")
    if c.top_k in (5, 3, 7):
        assert float(straddle.float().mean()) >= 0.05
    # the model of the kernel's insert: the former loop differs from the stable sort on these scenes, the fixed one nowhere
    amb = WC.ambiguous_rays(sc, K).tolist()
    order = kept = 0
    for b in range(0, c.B, 4):
        if amb[b]:
            continue
        row = c64[b].tolist()
        want = [v for v, ok in zip(views[b].tolist(), valid[b].tolist()) if ok]
        fixed = [v for v in WC.tie_model(row, K, True) if row[v] <= WR.VALID_COST]
        old = [v for v in WC.tie_model(row, K, False) if row[v] <= WR.VALID_COST]
        assert fixed == want
        order += old != want
        kept += set(old) != set(want)
    assert order > 0
    if c.top_k in (5, 3, 7):
        assert kept > 0


# ---- projection cases -----------------------------------------------------------------------------------------------------
def test_general_cameras_are_general():
    sc = WC.case_scene(WC.CASES_PROJECT[0])
    k, R = sc.ks.reshape(-1, 9), sc.rts[:, :, :3].reshape(-1, 9)
    assert bool((k[:, :6] != 0).all()) and bool((k[:, 6:] == torch.tensor([0.0, 0.0, 1.0])).all())
    assert bool((R.abs() > 1e-3).all())
    for row in torch.cat([k[:, :6], R], 1).tolist():
        assert len(set(row)) == len(row)
    assert bool(((k[:, 0] - k[:, 4]).abs() > 1.0).all())                           # fx != fy
    off = torch.stack([k[:, 2] - sc.W / 2, k[:, 5] - sc.H / 2], 1)
    assert bool((off.abs() > 1e-3).all())                                           # principal point off-centre
    Rm = sc.rts[:, :, :3].double()
    assert float((Rm @ Rm.transpose(1, 2) - torch.eye(3, dtype=F64)).abs().max()) < 1e-6
    assert float((torch.linalg.det(Rm) - 1).abs().max()) < 1e-6


@pytest.mark.parametrize("c", WC.CASES_PROJECT, ids=ids(WC.CASES_PROJECT))
def test_projection_case_edges_and_yardstick(c):
    sc = WC.case_scene(c)
    assert (sc.H, sc.W) == (c.H, c.W)
    if c.supplied:
        views, valid = WC.supplied_slots(c, sc)
        assert bool((views == -1).any()) and bool((views == c.N).any()) and bool(valid.all())
        inside = (views >= 0) & (views < c.N)
        ref = WC.project_reference(sc, views)
        assert bool((ref["proj_depth"][inside] < 0).any())                                    # behind a camera
        gx, gy = ref["grid"][..., 0], ref["grid"][..., 1]
        assert bool(((gx < -1) | (gx > c.W) | (gy < -1) | (gy > c.H))[inside].any())          # outside the image
        assert bool(torch.isfinite(ref["grid"]).all())
    else:
        views, _, valid = WC.select_reference(sc, 10)
        inside = valid
        assert int(valid.sum()) >= 50
    ref64, ref32, scales = WC.project_reference(sc, views, F64), WC.project_reference(sc, views, F32), WC.project_scales(sc, views)
    for name in ("grid", "proj_depth", "nei_origin", "nei_direction"):
        f = WC.PR.figures(ref32[name][inside].reshape(int(inside.sum()), -1), ref64[name][inside].reshape(int(inside.sum()), -1),
                          scales[name][inside])
        assert all(math.isfinite(x) and x > 0 for x in f.values()), (name, f)
        assert f["max"] < 1e-5, (name, f)          # the scales do scale: float32 stays a few ulp on them
    g32 = ref32["grid"]
    col64, fl64, cs = WC.color_reference(sc, g32, views, inside, F64)
    col32, fl32, _ = WC.color_reference(sc, g32, views, inside, F32)
    assert torch.equal(fl64, fl32) or not c.supplied
    f = WC.PR.figures(col32[inside], col64[inside], cs[inside])
    assert all(math.isfinite(x) and x > 0 for x in f.values()), f
    assert bool((inside & ~fl32).any())          # the occlusion masks remove slots


# ---- loss cases -----------------------------------------------------------------------------------------------------------
def test_loss_case_list_covers_the_edges():
    by = {c.name: c for c in WC.CASES_LOSS}
    bk = lambda c: c.B * WC.case_K(c)
    assert bk(by["BK4090"]) == 4090 and bk(by["BK4100"]) == 4100                    # 1 -> 2 chunks of 4096 entries
    assert bk(by["BK262150"]) == 262150 and math.ceil(262150 / 64) == 4097           # 64 chunks, each past 4096
    assert (by["K1-B4096"].N, by["K1-B4097"].N) == (1, 1) and bk(by["K1-B4097"]) == 4097
    assert by["N2-B65541"].B > 256 * 256 and WC.case_K(by["N2-B65541"]) == 2
    assert by["N1-B1048579"].B == 4096 * 256 + 3
    assert by["B1"].B == 1 and by["N300-B2000"].N == 300 and by["blind-N40"].N == 40
    assert {c.ray_valid for c in WC.CASES_LOSS} == {None, "mixed", "one", "none"}
    assert by["scale0.7"].scale == 0.7 and by["zero-scores"].zero_scores


@pytest.mark.parametrize("c", WC.CASES_LOSS, ids=ids(WC.CASES_LOSS))
def test_loss_case_edge_cap_and_yardstick(c):
    sc, views, flags, grid, score = WC.cpu_pipeline(c)
    Kn = WC.case_K(c)
    counts = flags if sc.ray_valid is None else flags & sc.ray_valid[:, None]
    if c.ray_valid == "none":
        assert c is WC.CASE_NO_VALID_RAY and not bool(counts.any())
    else:
        assert int(counts.sum()) >= 1
        assert float((score * counts).sum()) > 0
    if c.ray_valid == "one":
        assert int(sc.ray_valid.sum()) == 1 and int(counts.sum()) >= 1
    if c.zero_scores:
        assert bool(((score == 0) & counts).any()) and bool(((score > 0) & counts).any())
    keep = WC.untied_rays(sc)
    assert int((~keep).sum()) <= WC.TIE_CAP * c.B
    per_cam = torch.zeros(c.N, dtype=torch.long).index_add_(0, views[counts].long(), torch.ones(int(counts.sum()), dtype=torch.long))
    if c.kind == "blind":
        away = torch.arange(c.N - 1)[torch.arange(c.N - 1) % 3 == 1]
        assert away.numel() >= 10 and bool((per_cam[away] == 0).all())
        ref_views, _, ref_valid = WC.select_reference(sc, Kn)                          # under warp_reference.select itself
        assert not bool(torch.isin(ref_views[ref_valid], away).any())
        cam, ray = sc.special
        assert int((ref_views[ref_valid] == cam).sum()) == 1 and bool(ref_valid[ray, 0]) and int(ref_views[ray, 0]) == cam
        assert int(per_cam[cam]) == 1 and int(counts[ray].sum()) == 1
    if c.kind == "border":
        g64 = WC.project_reference(sc, views)["grid"]
        gx, gy = g64[..., 0][counts], g64[..., 1][counts]
        bands = [(gx > -0.5) & (gx < 0), (gx > sc.W - 2) & (gx < sc.W - 1.5), (gy > -0.5) & (gy < 0), (gy > sc.H - 2) & (gy < sc.H - 1.5)]
        print("border bands:", [int(b.sum()) for b in bands])
        assert all(int(b.sum()) >= 50 for b in bands)
    if c.kind == "clamp":
        s = sc.q[:, 1:4].double() + sc.q[:, 4:7].double()
        reg = WC.clamp_regime(c.B)
        tests = [(s > 0) & (s < 1), s > 1, s < 0, s == 0.0, s == 1.0]
        for i, t in enumerate(tests):
            assert bool(t[reg == i].all()) and float(t.float().mean()) >= 0.05, WC.REGIMES[i]
        assert bool((sc.q[:, 1:4][reg == 2] < 0).all())                                # negative diffuse
        exact = ((s == 0.0) | (s == 1.0)).any(1) & counts.any(1)
        assert int(exact.sum()) >= 20 and bool(keep[exact].all())
    if c.ray_valid == "none":
        return
    dev = "cpu"
    ref64 = WC.loss_reference(sc, views, flags, score, grid, c.scale, F64, dev)
    ref32 = WC.loss_reference(sc, views, flags, score, grid, c.scale, F32, dev)
    assert ref64["n_valid_slots"] == int(counts.sum())
    assert int(ref64["owned"].sum()) == int((per_cam > 0).sum())
    assert math.isfinite(ref64["loss"]) and ref64["loss"] > 0
    assert ref32["loss"] != ref64["loss"] or c.B == 1
    for name, (got, ref, scale) in WC.loss_quantities(ref32, ref64, keep).items():
        f = WC.PR.figures(got, ref, scale)
        print(c.name, name, f)
        assert all(math.isfinite(x) for x in f.values()), (name, f)
        assert f["max"] > 0 and f["pooled"] > 0, (name, f)
        assert f["p99"] < 1e-3, (name, f)          # the scales do scale: float32 stays near its rounding on them
    assert WC.judge_loss(c.name + " (yardstick against itself)", ref32, ref64, ref32, keep) == []


def test_loss_reference_matches_warp_loss_autograd():
    """The per-slot restatement of loss_reference gives what autograd of warp_reference.warp_loss on the whole batch gives."""
    c = WC.CASES_LOSS[0]
    sc, views, flags, grid, score = WC.cpu_pipeline(c)
    ref = WC.loss_reference(sc, views, flags, score, grid, 0.7)
    o, d, q, rts = (x.double().requires_grad_(True) for x in (sc.rays_o, sc.rays_d, sc.q, sc.rts))
    L = WR.warp_loss(o, d, q[:, 0], q[:, 1:4], q[:, 4:7], rts, sc.ks.double(), sc.images.double(), None, views, flags, score.double(),
                     scale=0.7, ray_valid=sc.ray_valid, corner_grid=grid.double())
    L.backward()
    assert abs(float(L.detach()) - ref["loss"]) <= 1e-13 * abs(float(L.detach()))
    for a, b in ((q.grad, ref["grad_q"]), (o.grad, ref["grad_o"]), (d.grad, ref["grad_d"]), (rts.grad, ref["grad_rts"])):
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    sc_ = ref["scale"]
    assert bool((sc_["grad_o"] >= ref["grad_o"].norm(dim=1) * (1 - 1e-12)).all())
    assert bool((sc_["grad_rts"] >= ref["grad_rts"].reshape(-1, 12).norm(dim=1) * (1 - 1e-12)).all())
