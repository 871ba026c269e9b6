"""GPU checks of the three warp-loss entry points (csrc/warp.hip) per ray, per slot and per camera, at their edges: the cases of
tests/warp_cases.py (general cameras, duplicate cameras, blind cameras, border rays, clamp regimes, every size at which a kernel
takes another path), judged by warp_cases.judge against the float64 restatement with the float32 restatement as the yardstick.
tests/test_warp_cases_cpu.py asserts on the reference alone that each case holds its edge.  The C entry points are called directly
so that every output can be prefilled (NaN / 0xFF) and the scratch buffer sized to the float."""
import collections
import functools

import pytest
import torch

import warp_cases as WC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
ids = lambda cases: [WC.case_id(c) for c in cases]
TAIL_BITS = 0x7FC5A5A5   # a NaN payload: the pattern behind the scratch the loss entry point is given


def _capi():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    return _capi


DevScene = collections.namedtuple("DevScene", "ks rts images occlusions rays_o rays_d q ray_valid N H W B")


@functools.lru_cache(maxsize=4)
def dev_scene(c):
    sc = WC.case_scene(c)
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    return DevScene(d(sc.ks.reshape(-1, 9)), d(sc.rts.reshape(-1, 12)), d(sc.images), d(sc.occlusions), d(sc.rays_o), d(sc.rays_d),
                    d(sc.q), d(sc.ray_valid), sc.ks.shape[0], sc.H, sc.W, sc.rays_o.shape[0])


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def _ff(*shape):
    return torch.full(shape, 0xFF, dtype=torch.uint8, device=DEV)


def run_select(ds, K, B=None):
    """scanerf_warp_select_views into poisoned outputs -> status, views [B,K] int32, cost [B,K], valid [B,K] uint8."""
    api = _capi()
    B = ds.B if B is None else B
    rows = max(B, 1)
    views = torch.full((rows, K), -7, dtype=torch.int32, device=DEV)
    cost, valid = _nan(rows, K), _ff(rows, K)
    rc = api.lib().scanerf_warp_select_views(_p(ds.rays_o), _p(ds.rays_d), _p(ds.q), _p(ds.ray_valid), _p(ds.ks), _p(ds.rts), ds.N,
                                             ds.H, ds.W, K, B, _p(views), _p(cost), _p(valid), api.stream())
    torch.cuda.synchronize()
    return rc, views, cost, valid


def run_project(ds, views, valid_in):
    """scanerf_warp_project into poisoned outputs -> dict (valid: uint8)."""
    api = _capi()
    B, K = views.shape
    r = {"grid": _nan(B, K, 2), "proj_depth": _nan(B, K), "nei_origin": _nan(B, K, 3), "nei_direction": _nan(B, K, 3),
         "color": _nan(B, K, 3), "valid": _ff(B, K), "views": views}
    vin = valid_in.to(torch.uint8).contiguous()
    rc = api.lib().scanerf_warp_project(_p(ds.rays_o), _p(ds.rays_d), _p(ds.q), _p(ds.ks), _p(ds.rts), _p(views), _p(vin),
                                        _p(ds.images), _p(ds.occlusions), ds.N, ds.H, ds.W, K, B, _p(r["grid"]), _p(r["proj_depth"]),
                                        _p(r["nei_origin"]), _p(r["nei_direction"]), _p(r["color"]), _p(r["valid"]), api.stream())
    api.check(rc, "warp_project")
    torch.cuda.synchronize()
    return r


def run_loss(ds, proj, score, scale, short=0, tail=1024):
    """scanerf_warp_loss_grad into NaN outputs, with scratch of exactly scanerf_warp_scratch_floats (less `short`) at the front of a
    buffer whose tail holds TAIL_BITS -> status, dict, the tail as int32."""
    api = _capi()
    B, K = proj["views"].shape
    n = api.lib().scanerf_warp_scratch_floats(B, K, ds.N)
    buf = torch.full((n + tail,), TAIL_BITS, dtype=torch.int32, device=DEV)
    buf[:n] = 0x7FC00000
    r = {"loss": _nan(1), "grad_q": _nan(B, 7), "grad_o": _nan(B, 3), "grad_d": _nan(B, 3), "grad_rts": _nan(ds.N, 3, 4)}
    valid = proj["valid"].to(torch.uint8).contiguous()
    score = score.to(DEV, F32).contiguous()
    rc = api.lib().scanerf_warp_loss_grad(_p(ds.rays_o), _p(ds.rays_d), _p(ds.q), _p(ds.ray_valid), _p(ds.ks), _p(ds.rts),
                                          _p(proj["views"]), _p(valid), _p(proj["grid"]), _p(proj["color"]), _p(score),
                                          _p(ds.images), ds.N, ds.H, ds.W, K, B, float(scale), _p(r["loss"]), _p(r["grad_q"]),
                                          _p(r["grad_o"]), _p(r["grad_d"]), _p(r["grad_rts"]), _p(buf.view(F32)), n - short,
                                          api.stream())
    torch.cuda.synchronize()
    return rc, r, buf[n:]


def _rows(t, m):
    t = t.detach().cpu()
    return t[m].reshape(int(m.sum()), -1)


# ---- selection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", WC.CASES_SELECT, ids=ids(WC.CASES_SELECT))
def test_selection_per_ray(c):
    """Every ray float32 can decide: its list of valid slots equals the stable sort's, order included (ties by the lower camera
    index -- bit-identical duplicate cameras are decided, not left out), costs per slot within the bound; rays outside ray_valid
    get views 0, cost 1, valid 0."""
    sc, ds, K = WC.case_scene(c), dev_scene(c), WC.case_K(c)
    rc, views, cost, valid = run_select(ds, K)
    assert rc == 0
    views, cost, valid = views.cpu().long(), cost.cpu(), valid.cpu()
    assert bool(((valid == 0) | (valid == 1)).all()) and not bool(torch.isnan(cost).any())
    valid = valid.bool()
    rv, rc64, rvalid = WC.select_reference(sc, K)
    live = torch.ones(c.B, dtype=torch.bool) if sc.ray_valid is None else sc.ray_valid
    assert bool((views[~live] == 0).all()) and bool((cost[~live] == 1.0).all()) and not bool(valid[~live].any())
    if c.ray_valid == "none":
        assert not bool(valid.any())
        return
    judged = live & ~WC.ambiguous_rays(sc, K)
    assert int(judged.sum()) >= 0.9 * int(live.sum())
    same_flags = (valid == rvalid).all(1)
    same_order = same_flags & ((views == rv) | ~rvalid).all(1)
    member = lambda a, am, b, bm: ((a[:, :, None] == b[:, None, :]) & bm[:, None, :]).any(2) | ~am
    same_set = same_flags & member(views, valid, rv, rvalid).all(1) & member(rv, rvalid, views, valid).all(1)
    n_order, n_set = int((judged & ~same_order).sum()), int((judged & ~same_set).sum())
    print(f"{c.name}: {int(judged.sum())} rays judged; valid slots in another order on {n_order}, another set on {n_set}")
    assert n_set == 0, f"{n_set} rays keep another set of neighbours than the stable sort"
    assert n_order == 0, f"{n_order} rays list their neighbours in another order than the stable sort (ties: lower index first)"
    m = rvalid & judged[:, None]
    assert int(m.sum()) > 0
    c32 = WC.costs(sc, F32).gather(1, rv)
    one = torch.ones(int(m.sum()), dtype=F64)
    assert WC.judge(f"{c.name} cost", _rows(cost, m), _rows(rc64, m), _rows(c32, m), scale=one) == []


def test_selection_of_no_rays_touches_nothing():
    c = WC.CASES_SELECT[2]
    rc, views, cost, valid = run_select(dev_scene(c), WC.case_K(c), B=0)
    assert rc == 0
    assert bool((views == -7).all()) and bool(torch.isnan(cost).all()) and bool((valid == 0xFF).all())


# ---- projection -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", WC.CASES_PROJECT, ids=ids(WC.CASES_PROJECT))
def test_projection_per_slot(c):
    """The five outputs per slot on general cameras: slots from the selection kernel, or caller-supplied ones (views in [-1, N],
    points behind cameras and outside the images).  Flags exact on the kernel's grid; every slot that is not live is zero-filled."""
    sc, ds = WC.case_scene(c), dev_scene(c)
    if c.supplied:
        views, valid_in = WC.supplied_slots(c, sc)
    else:
        rc, v, _, ok = run_select(ds, 10)
        assert rc == 0
        views, valid_in = v.cpu(), ok.cpu().bool()
        assert int(valid_in.sum()) >= 50
    pr = run_project(ds, views.to(DEV).contiguous(), valid_in.to(DEV))
    live = valid_in & (views >= 0) & (views < c.N)
    out = {k: pr[k].cpu() for k in ("grid", "proj_depth", "nei_origin", "nei_direction", "color", "valid")}
    for k, t in out.items():
        assert bool((t[~live] == 0).all()), k                       # zero-filled, flag 0 (views of -1 and N among them)
        assert k == "valid" or bool(torch.isfinite(t).all()), k
    if c.supplied:
        assert bool((~live).any()) and bool(((views == -1) | (views == c.N)).any())
    ref64, ref32, scales = WC.project_reference(sc, views, F64), WC.project_reference(sc, views, F32), WC.project_scales(sc, views)
    bad = []
    for k in ("grid", "proj_depth", "nei_origin", "nei_direction"):
        bad += WC.judge(f"{c.name} {k}", _rows(out[k], live), _rows(ref64[k], live), _rows(ref32[k], live), scale=scales[k][live])
    col64, _, cs = WC.color_reference(sc, out["grid"], views, live, F64)
    col32, flags, _ = WC.color_reference(sc, out["grid"], views, live, F32)
    assert bool(((out["valid"] == 0) | (out["valid"] == 1)).all())
    assert torch.equal(out["valid"].bool(), flags)
    assert bool((live & ~flags).any()) and bool(flags.any())
    bad += WC.judge(f"{c.name} color", _rows(out["color"], live), _rows(col64, live), _rows(col32, live), scale=cs[live])
    assert bad == []


# ---- loss and gradients -----------------------------------------------------------------------------------------------------
def _loss_pipeline(c):
    sc, ds, K = WC.case_scene(c), dev_scene(c), WC.case_K(c)
    rc, views, _, valid = run_select(ds, K)
    assert rc == 0
    pr = run_project(ds, views, valid)
    score = WC.case_scores(c, pr["valid"].bool())
    return sc, ds, pr, score


def _bits(r):
    return [r[k].view(torch.int32) for k in ("loss", "grad_q", "grad_o", "grad_d", "grad_rts")]


@pytest.mark.parametrize("c", WC.CASES_LOSS, ids=ids(WC.CASES_LOSS))
def test_loss_and_gradients_per_ray_and_camera(c):
    """warp_cases.judge_loss on every case: grad_q's depth column, its colour columns, grad_o and grad_d per ray, grad_rts per
    camera, the loss.  All outputs start as NaN: grad_rts is overwritten, cameras without a slot and rays outside ray_valid are
    exactly 0.  The scratch is exactly scanerf_warp_scratch_floats long and what lies behind it stays bit-unchanged; a second
    launch gives the same bits."""
    sc, ds, pr, score = _loss_pipeline(c)
    rc, res, tail = run_loss(ds, pr, score, c.scale)
    assert rc == 0
    assert bool((tail == TAIL_BITS).all())
    for k, t in res.items():
        assert bool(torch.isfinite(t).all()), k
    rc2, res2, _ = run_loss(ds, pr, score, c.scale)
    assert rc2 == 0 and all(torch.equal(a, b) for a, b in zip(_bits(res), _bits(res2)))
    if sc.ray_valid is not None:
        dead = ~ds.ray_valid
        assert all(bool((res[k][dead] == 0).all()) for k in ("grad_q", "grad_o", "grad_d"))
    if c.ray_valid == "none":
        assert float(res["loss"]) == 0.0
        assert all(bool((t == 0).all()) for t in res.values())
        return
    dev = DEV if c.on_device else "cpu"
    args = (sc, pr["views"].cpu(), pr["valid"].bool().cpu(), score, pr["grid"].cpu(), c.scale)
    ref64, ref32 = WC.loss_reference(*args, F64, dev), WC.loss_reference(*args, F32, dev)
    assert ref64["n_valid_slots"] >= 1 and ref64["loss"] > 0
    owned = ref64["owned"].to(DEV)
    assert bool((res["grad_rts"][~owned] == 0).all())
    if c.kind == "blind":
        assert int((~owned).sum()) >= 10
        cam, ray = sc.special
        slots = (pr["views"] == cam) & pr["valid"].bool()
        assert int(slots.sum()) == 1 and bool(slots[ray].any())      # the one-slot camera
    res["loss"] = float(res["loss"])
    assert WC.judge_loss(c.name, res, ref64, ref32, WC.untied_rays(sc)) == []


def test_loss_refuses_short_scratch():
    """One float short of scanerf_warp_scratch_floats: an error with a message, and no launch (the outputs keep their NaN)."""
    c = WC.CASES_LOSS[0]
    sc, ds, pr, score = _loss_pipeline(c)
    rc, res, tail = run_loss(ds, pr, score, 1.0, short=1)
    assert rc != 0
    msg = _capi().lib().scanerf_last_error().decode("utf-8", "replace")
    assert "scratch" in msg and "needs" in msg, msg
    assert all(bool(torch.isnan(t).all()) for t in res.values())
    assert bool((tail == TAIL_BITS).all())
