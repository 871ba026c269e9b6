"""GPU parity of the render-time ops at the tile counts and overlaps of a large scene: 2-D grids of 8 to 65 overlapping tiles
and stacks of coincident tiles (tests/render_scenes.py; what those inputs contain is checked in test_render_scenes_cpu.py),
every op against the oracle's restatement at the bounds of test_gpu_render_time.test_render_loop_stage_by_stage: geometry and
integer outputs bit-equal, inference and accumulation rtol 1e-4 with atol 2e-6 (depth 2e-5).  Needs an MI355X.

The code paths only these shapes reach: slot lists derived in-kernel at nb = 8 and refused at 9; the high word of a chunk's
tile set (tiles >= 32, chunks that list no tile < 32, tile 63); the single-pass fallback above 64 tiles; the sort kernel and
its fallback beyond three entries; four slots per sample, four exit tiles per ray and the truncation of both lists at four.
"""
import functools

import numpy as np
import pytest
import torch

import render_scenes as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, S, SB = RS.B_RAYS, 32, 16
GRIDS = tuple(RS.GRIDS)


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def n(t):
    return t.detach().cpu().numpy()


def ops():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import hashgrid as H
    return H


def HG():
    import scanerf_amd  # noqa: F401
    from scanerf_amd.hashgrid.lib import HASHGRID
    return HASHGRID


@functools.lru_cache(maxsize=None)
def dev_scene(name):
    """The scene's arrays on the GPU, uploaded once (read-only for the tests).  The decoders are packed here and owned by this
    dict (PackedDecoders): a raw blob tensor kept alive by this cache would keep its entry in HASHGRID._images alive too, which
    test_packed_decoders_follow_their_owner_not_an_address expects to find empty."""
    sc, _ = RS.named(name)
    D = {k: g(sc[k]) for k in ("corners", "sizes", "occ", "starts", "l2d", "tables", "params", "res")}
    D["params"] = HG().PackedDecoders(D["params"])
    return D


def scene_tail(D):
    return D["tables"], D["params"], D["res"], D["occ"], D["starts"], D["l2d"], D["corners"], D["sizes"]


def filled(rows, cols, v=7.0):
    """outputs pre-filled with a value no sample has, so that one the kernel leaves unwritten shows"""
    return [torch.full((rows, cols, 3), v, device=DEV), torch.full((rows, cols, 3), v, device=DEV), torch.full((rows, cols, 1), v, device=DEV)]


def close(got, want, what, depth=False):
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 if depth else 2e-6, err_msg=what)


def pad32(a):
    """[B,...] -> [B rounded up to 32,...] with copies of the last ray, as the renderer pads"""
    pad = -a.shape[0] % 32
    return np.concatenate([a, np.repeat(a[-1:], pad, 0)]) if pad else a


def to_lay2(a):
    """[B,S,...] (B a multiple of 32) -> the ray-block layout [B/32,S,32,...] (scanerf_hip.h sample_major = 2)"""
    return np.ascontiguousarray(np.swapaxes(a.reshape(a.shape[0] // 32, 32, *a.shape[1:]), 1, 2))


def from_lay2(a):
    return np.swapaxes(a, 1, 2).reshape(a.shape[0] * 32, a.shape[1], *a.shape[3:])


@functools.lru_cache(maxsize=None)
def two_passes(name, order):
    """The first two tracing passes of the scene's rays on the ORACLE, every ray kept running (no decoder in the loop), and the
    oracle's inference of each: [(z, dists, block_idxs, (dif, spec, alpha))], computed once and shared."""
    sc, rays = RS.named(name)
    o, d = rays[order]
    out = []
    for z, dd, bi in RS.trace_samples(sc, o, d, S, passes=2):
        out.append((z, dd, bi, O.pts_inference(o, d, z, dd, bi, sc["tables"], sc["params"], sc["res"], sc["occ"], sc["starts"],
                                               sc["l2d"], sc["corners"], sc["sizes"])))
    return out


def run_pts_inference(name, order, z, dd, bi, lay):
    """pts_inference under the current INFER_ARITH in layout 0 or 2 -> (dif, spec, alpha) as [B,S,.] numpy"""
    H, D = ops(), dev_scene(name)
    _, rays = RS.named(name)
    o, d = rays[order]
    if lay == 0:
        out = filled(B, S)
        H.pts_inference(g(o), g(d), g(z), g(dd), g(bi), *scene_tail(D), *out)
        return [n(t) for t in out]
    Bp = B + -B % 32
    out = [t.reshape(Bp // 32, S, 32, -1) for t in filled(Bp, S)]
    H.pts_inference(g(pad32(o)), g(pad32(d)), g(to_lay2(pad32(z))), g(to_lay2(pad32(dd))), g(to_lay2(pad32(bi))), *scene_tail(D), *out,
                    sample_major=2)
    return [from_lay2(n(t))[:B] for t in out]


# ------------------------------------------------------------------ a. stage by stage
@pytest.mark.parametrize("name", GRIDS + tuple(RS.STACKS))
def test_stage_by_stage_over_every_scene(name):
    """The loop of test_render_loop_stage_by_stage on each scene: every tracing pass until no ray runs, then every background
    blend step -- four on the grids and STACK6 (rays that leave four tiles at one distance), three on STACK3."""
    H, D = ops(), dev_scene(name)
    sc, rays = RS.named(name)
    o, d = rays["shuffled"]
    nb = sc["corners"].shape[0]
    cn, sz, occ, st, l2 = sc["corners"], sc["sizes"], sc["occ"], sc["starts"], sc["l2d"]
    C, Z, OCC, ST, L2 = D["corners"], D["sizes"], D["occ"], D["starts"], D["l2d"]
    RO, RD = g(o), g(d)

    inter = torch.full((B, nb, 2), 1e7, device=DEV)
    H.ray_block_intersection(RO, RD, C, Z, inter)
    inter_ref = O.ray_block_intersection(o, d, cn, sz)
    assert np.array_equal(n(inter), inter_ref)
    tb_ref, max_tracing = RS.tracing_order(inter_ref)
    assert np.array_equal(n(H.sort_tracing_blocks(inter)), tb_ref)
    TB = g(tb_ref)
    assert max_tracing >= (4 if name in GRIDS else nb)

    last = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    H.get_last_block(TB, last, inter)
    assert np.array_equal(n(last), O.get_last_block(tb_ref, inter_ref))
    hit = torch.full((B,), -1, dtype=torch.int16, device=DEV)
    H.ray_firsthit_block(RO, RD, C, Z, OCC, ST, L2, TB, inter, hit)
    assert np.array_equal(n(hit), O.ray_firsthit_block(o, d, cn, sz, occ, st, l2, tb_ref, inter_ref))
    tgt, tgt_ref = OCC.clone(), occ.astype(np.uint8).copy()
    for b in range(nb):
        total = int(np.prod(2 ** l2[b]))
        H.process_occupied_grid(b, total, C, Z, OCC, ST, L2, tgt)
        O.process_occupied_grid(b, total, cn, sz, occ, st, l2, tgt_ref)
    assert np.array_equal(n(tgt).astype(np.uint8), tgt_ref) and (name not in GRIDS or tgt_ref.sum() > occ.sum())

    tracing_idx, z_start = np.zeros(B, np.int32), np.zeros(B, np.float32)
    TI, ZS = g(tracing_idx), g(z_start)
    transp, dif, spec, depth = (np.ones((B, 1), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32),
                                np.zeros((B, 1), np.float32))
    TR, DI, SP, DE = g(transp), g(dif), g(spec), g(depth)
    slots, n_pass, top_alpha = np.zeros(5, np.int64), 0, 0.0
    for step in range(max_tracing):
        running_ref = (tracing_idx < max_tracing) & (transp[:, 0] > 1e-5)
        if not running_ref.any():
            break
        n_pass += 1
        z = torch.full((B, S), -1.0, device=DEV)
        dd = torch.full((B, S), -1.0, device=DEV)
        H.sample_points(RO, RD, C, Z, OCC, ST, L2, TB, inter, TI, ZS, z, dd)
        z_ref, d_ref = O.render_sample_points(o, d, cn, sz, occ, st, l2, S, tb_ref, inter_ref, tracing_idx, z_start)
        assert np.array_equal(n(z), z_ref) and np.array_equal(n(dd), d_ref), f"step {step}"
        assert np.array_equal(n(TI), tracing_idx) and np.array_equal(n(ZS), z_start), f"step {step}"
        bi = torch.full((B, S, 4), -1, dtype=torch.int16, device=DEV)
        H.prepare_points(z, g(running_ref), inter, bi)
        bi_ref = O.prepare_points(z_ref, running_ref, inter_ref)
        assert np.array_equal(n(bi), bi_ref), f"step {step}"
        slots += np.bincount((bi_ref != -1).sum(-1).reshape(-1), minlength=5)
        pd, ps, pa = filled(B, S)
        H.pts_inference(RO, RD, z, dd, bi, *scene_tail(D), pd, ps, pa)
        rd_, rs_, ra_ = O.pts_inference(o, d, z_ref, d_ref, bi_ref, sc["tables"], sc["params"], sc["res"], occ, st, l2, cn, sz)
        top_alpha = max(top_alpha, float(ra_.max()))
        close(n(pa), ra_, f"alpha step {step}")
        close(n(pd), rd_, f"diffuse step {step}")
        close(n(ps), rs_, f"specular step {step}")
        H.accumulate_color(pd, ps, pa, TR, z, DI, SP, DE)
        O.accumulate_color(rd_, rs_, ra_, transp, z_ref, dif, spec, depth)
        np.testing.assert_allclose(n(TR), transp, rtol=1e-4, atol=1e-7)
        close(n(DI), dif, f"accumulated diffuse step {step}")
        close(n(SP), spec, f"accumulated specular step {step}")
        close(n(DE), depth, f"accumulated depth step {step}", depth=True)
    assert transp.min() < 0.5 and top_alpha > 0.05
    if name in GRIDS:   # (no three: render_scenes.py's docstring)
        assert n_pass >= 2 and slots[2] > 1000 and slots[4] > 300 and slots[3] == 0, slots
    else:
        assert slots[min(nb, 4)] > 5000 and slots[1:].sum() == slots[min(nb, 4)], slots

    # ---- background: exit tiles + blend weights (bit-exact), then every blend step
    ob = torch.full((B, 4), -1, dtype=torch.int16, device=DEV)
    bw = torch.zeros((B, 4), device=DEV)
    H.update_outgoing_bidx(RO, RD, C, Z, TB, inter, ob, bw, 0.12, False)
    ob_ref, bw_ref = O.update_outgoing_bidx(o, d, cn, sz, tb_ref, inter_ref, 0.12, False)
    assert np.array_equal(n(ob), ob_ref) and np.array_equal(n(bw), bw_ref)
    ob2 = torch.full((B, 4), -1, dtype=torch.int16, device=DEV)
    bw2 = torch.zeros((B, 4), device=DEV)
    H.update_outgoing_bidx_v2(RO, RD, C, Z, TB, inter, ob2, bw2)
    ob2_ref, bw2_ref = O.update_outgoing_bidx_v2(o, cn, sz)
    assert np.array_equal(n(ob2), ob2_ref) and np.array_equal(n(bw2), bw2_ref)
    assert (ob2_ref[:, min(nb, 4) - 1] != -1).sum() >= 20, "origins inside four tiles (three in STACK3)"
    with np.errstate(invalid="ignore", divide="ignore"):
        bwn = np.nan_to_num(bw_ref / bw_ref.sum(-1, keepdims=True))
    n_blend = int((bwn > 0).sum(-1).max())
    assert n_blend == min(nb, 4)
    n_exit = np.bincount((ob_ref != -1).sum(-1), minlength=5)
    if name in GRIDS:
        assert n_exit[2] >= 5 and n_exit[4] >= 5 and n_exit[3] == 0, n_exit
    bgd, bgs, bgz = np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 1), np.float32)
    BGD, BGS, BGZ = g(bgd), g(bgs), g(bgz)
    for i in range(n_blend):
        zb = torch.full((B, SB), -1.0, device=DEV)
        H.inverse_z_sampling(inter, ob[:, i].contiguous(), zb, 1e6)
        zb_ref = O.render_inverse_z_sampling(inter_ref, ob_ref[:, i], SB, 1e6)
        assert np.array_equal(n(zb), zb_ref), f"blend step {i}"
        pd, ps, pa = filled(B, SB)
        H.bg_pts_inference_v2(RO, RD, zb, ob, i, C, Z, D["res"], D["tables"], D["params"], pd, ps, pa)
        rd_, rs_, ra_ = O.bg_pts_inference_v2(o, d, zb_ref, ob_ref, i, cn, sz, sc["res"], sc["tables"], sc["params"])
        assert ra_.max() > 0.05 and (ob_ref[:, i] != -1).sum() >= 5
        close(n(pa), ra_, f"bg alpha blend step {i}")
        close(n(pd), rd_, f"bg diffuse blend step {i}")
        close(n(ps), rs_, f"bg specular blend step {i}")
        t1, td, ts, tz = (np.ones((B, 1), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32),
                          np.zeros((B, 1), np.float32))
        T1, TD, TS, TZ = g(t1), g(td), g(ts), g(tz)
        H.accumulate_color(pd, ps, pa, T1, zb, TD, TS, TZ)
        O.accumulate_color(rd_, rs_, ra_, t1, zb_ref, td, ts, tz)
        np.testing.assert_allclose(n(T1), t1, rtol=1e-4, atol=1e-7)
        close(n(TD), td, f"bg accumulated diffuse {i}")
        close(n(TS), ts, f"bg accumulated specular {i}")
        close(n(TZ), tz, f"bg accumulated depth {i}", depth=True)
    # ---- bg_pts_inference (v1): all of a ray's exit tiles blended per sample with the op's own weights, on one set of depths
    zb = torch.full((B, SB), -1.0, device=DEV)
    H.inverse_z_sampling(inter, ob[:, 0].contiguous(), zb, 1e6)
    zb_ref = O.render_inverse_z_sampling(inter_ref, ob_ref[:, 0], SB, 1e6)
    pd, ps, pa = filled(B, SB, 5.0)
    H.bg_pts_inference(RO, RD, zb, ob, bw, C, Z, D["res"], D["tables"], D["params"], pd, ps, pa)
    rd_, rs_, ra_ = O.bg_pts_inference(o, d, zb_ref, ob_ref, bw_ref, cn, sz, sc["res"], sc["tables"], sc["params"])
    assert ra_.max() > 0.05
    close(n(pa), ra_, "bg v1 alpha")
    close(n(pd), rd_, "bg v1 diffuse")
    close(n(ps), rs_, "bg v1 specular")


# ------------------------------------------------------------------ b. tile order
@pytest.mark.parametrize("name", GRIDS)
def test_tile_order_equals_stable_argsort(name):
    """sort_tracing_blocks at nb = 8, 9, 36, 64 (the insertion-sort kernel) and 65 (torch.argsort above 64) equals
    torch.argsort(near, stable=True): on the scene's rays (up to 26 tiles met per ray, four equal entry distances of 0 for origins
    in a corner, rays that miss everything) and on random intervals where 60 % of the entries are live."""
    H, D = ops(), dev_scene(name)
    sc, rays = RS.named(name)
    nb = sc["corners"].shape[0]
    for order in ("shuffled", "sorted"):
        o, d = rays[order]
        inter = torch.full((B, nb, 2), 1e7, device=DEV)
        H.ray_block_intersection(g(o), g(d), D["corners"], D["sizes"], inter)
        near = inter[..., 0]
        assert int((near == 0).sum(-1).max()) == 4 and int((near != 1e7).sum(-1).max()) >= 4 and int((near == 1e7).all(-1).sum()) >= 20
        got = H.sort_tracing_blocks(inter)
        assert got.dtype == torch.int32 and got.is_contiguous()
        assert torch.equal(got, torch.argsort(near, dim=-1, stable=True).int())
    gen = torch.Generator(device=DEV).manual_seed(nb)
    Br = 4099
    inter = torch.rand(Br, nb, 2, device=DEV, generator=gen) * 20
    inter[torch.rand(Br, nb, device=DEV, generator=gen) < 0.4] = 1e7
    dup = torch.rand(Br, device=DEV, generator=gen) < 0.3
    inter[dup, nb - 1, 0] = inter[dup, 0, 0]
    inter[dup, nb // 2, 0] = inter[dup, 1, 0]
    inter[::97] = 1e7
    got = H.sort_tracing_blocks(inter.contiguous())
    assert torch.equal(got, torch.argsort(inter[..., 0], dim=-1, stable=True).int()), nb


# ------------------------------------------------------------------ c. slot lists derived in the kernel, at their limit
@pytest.mark.parametrize("lay", [0, 2])
@pytest.mark.parametrize("name", ["G8", "STACK3"])
def test_fused_slot_lists_equal_the_two_ops_at_eight_tiles(name, lay):
    """pts_inference_tracing at nb = 8 (kTracingMaxTiles) against prepare_points + pts_inference, bit for bit, with a third of the
    rays stopped: G8's samples list one, two and four tiles (a grid has no three), STACK3's exactly three."""
    H, D = ops(), dev_scene(name)
    sc, rays = RS.named(name)
    nb = sc["corners"].shape[0]
    assert H.tracing_fusable(nb)
    z, dd, _, _ = two_passes(name, "shuffled")[0]
    o, d = (pad32(a) for a in rays["shuffled"])
    z, dd = pad32(z), pad32(dd)
    Bp = o.shape[0]
    running = (np.arange(Bp) % 3 != 1)
    inter_ref = O.ray_block_intersection(o, d, sc["corners"], sc["sizes"])
    bi_ref = O.prepare_points(z, running, inter_ref)
    counts = np.bincount((bi_ref != -1).sum(-1).reshape(-1), minlength=5)
    if name == "G8":
        assert counts[1] > 1000 and counts[2] > 1000 and counts[4] > 300, counts
    else:
        assert counts[3] > 5000 and counts[1] == counts[2] == counts[4] == 0, counts
    shape = (lambda *t: (Bp, S, *t)) if lay == 0 else (lambda *t: (Bp // 32, S, 32, *t))
    lz, ldd = (g(a) if lay == 0 else g(to_lay2(a)) for a in (z, dd))
    RO, RD, RUN, INTER = g(o), g(d), g(running), g(inter_ref)
    bi = torch.full(shape(4), -1, dtype=torch.int16, device=DEV)
    H.prepare_points(lz, RUN, INTER, bi, sample_major=lay)
    assert np.array_equal(n(bi) if lay == 0 else from_lay2(n(bi)), bi_ref)
    two = [torch.full(shape(k), 7.0, device=DEV) for k in (3, 3, 1)]
    H.pts_inference(RO, RD, lz, ldd, bi, *scene_tail(D), *two, sample_major=lay)
    one = [torch.full(shape(k), -3.0, device=DEV) for k in (3, 3, 1)]
    H.pts_inference_tracing(RO, RD, lz, ldd, RUN, INTER, *scene_tail(D), *one, sample_major=lay)
    alpha = n(two[2]) if lay == 0 else from_lay2(n(two[2]))
    assert alpha.max() > 0.05 and np.abs(alpha[~running]).max() == 0.0
    assert (alpha[..., 0][(bi_ref != -1).sum(-1) == min(nb, 4)] > 0).mean() > 0.5
    for a, b in zip(one, two):
        assert torch.equal(a, b)


def test_fused_slot_lists_are_refused_at_nine_tiles():
    """nb = 9: tracing_fusable says no, and the C entry returns its error naming nb instead of running -- a refused argument;
    the outputs are untouched and the two-op route gives the oracle's values."""
    H, D = ops(), dev_scene("G9")
    sc, rays = RS.named("G9")
    assert not H.tracing_fusable(9) and H.tracing_fusable(8)
    o, d = rays["shuffled"]
    z, dd, bi, ref = two_passes("G9", "shuffled")[0]
    inter_ref = O.ray_block_intersection(o, d, sc["corners"], sc["sizes"])
    out = filled(B, S, -3.0)
    with pytest.raises(RuntimeError, match=r"nb=9"):
        H.pts_inference_tracing(g(o), g(d), g(z), g(dd), torch.ones(B, dtype=torch.bool, device=DEV), g(inter_ref), *scene_tail(D), *out)
    torch.cuda.synchronize()
    assert all(bool((t == -3.0).all()) for t in out)
    for got, want, what in zip(run_pts_inference("G9", "shuffled", z, dd, bi, 0), ref, ("diffuse", "specular", "alpha")):
        close(got, want, what)


# ------------------------------------------------------------------ d. the high word of a chunk's tile set
@pytest.mark.parametrize("lay", [0, 2])
@pytest.mark.parametrize("order", ["shuffled", "sorted"])
@pytest.mark.parametrize("name", ["G36", "G64"])
def test_tiles_from_32_on_render_in_both_chunk_kernels(name, order, lay, monkeypatch):
    """Tiles 32..35 / 32..63 through the 16-sample-tile kernel (default), the 32-sample-tile kernel ("h3") and, as a third
    witness on the same inputs, the single-pass f32 kernel (layout 0 only: it reads no other), each against the oracle.  In the
    sorted order the first 8192 samples -- a whole chunk of either kernel -- list tiles >= 32 only: the low word stays empty.
    Every tile must show: the samples whose first slot it is have opacity somewhere."""
    sc, _ = RS.named(name)
    nb = sc["corners"].shape[0]
    passes = two_passes(name, order)
    if order == "sorted":
        head = passes[0][2].reshape(-1, 4)[:8192]
        assert ((head >= 32) | (head == -1)).all() and (head[:, 0] >= 32).mean() > 0.9
    first = np.concatenate([p[2][..., 0].reshape(-1) for p in passes])
    for arith in ("t16", "h3", "f32"):
        monkeypatch.setattr(HG(), "INFER_ARITH", arith)
        alphas = []
        for k, (z, dd, bi, ref) in enumerate(passes):
            got = run_pts_inference(name, order, z, dd, bi, 0 if arith == "f32" else lay)
            for a, b, what in zip(got, ref, ("diffuse", "specular", "alpha")):
                close(a, b, f"{arith} {what} pass {k}")
            alphas.append(got[2].reshape(-1))
        alphas = np.concatenate(alphas)
        dark = [t for t in range(nb) if not (first == t).any() or not alphas[first == t].max() > 0]
        assert not dark, f"{arith}: tiles {dark} render nothing"
    monkeypatch.setattr(HG(), "INFER_ARITH", "t16")


# ------------------------------------------------------------------ e. above 64 tiles
@functools.lru_cache(maxsize=None)
def renderer(name):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import renderer as R
    return R.TileSetRenderer(DEV, RS.renderer_tiles(RS.named(name)[0]))


@functools.lru_cache(maxsize=None)
def oracle_image(name):
    o, d = RS.named(name)[1]["shuffled"]
    return RS.oracle_render_loop(renderer(name), o, d, S, SB)


def render(name, **kw):
    o, d = RS.named(name)[1]["shuffled"]
    return [n(t) for t in renderer(name).render_rays(g(o), g(d), num_sample=S, num_bg_sample=SB, **kw)]


def image_close(got, ref, what):
    """(dif, spec, depth, T) against the oracle's loop: colour atol 2e-6, depth 2e-5, rtol 1e-4; the transmittance at the atol of
    test_renderer_end_to_end_and_tile_formats"""
    close(got[0], ref["dif"], f"{what} diffuse")
    close(got[1], ref["spec"], f"{what} specular")
    close(got[2], ref["depth"], f"{what} depth", depth=True)
    np.testing.assert_allclose(got[3], ref["T"], rtol=1e-4, atol=1e-6, err_msg=f"{what} transmittance")


def count_calls(monkeypatch, op):
    """wrap renderer.<op>; -> the list its calls' ray counts and sample_major flags are appended to"""
    import scanerf_amd  # noqa: F401
    from scanerf_amd import renderer as R
    calls, real = [], getattr(R, op)

    def wrapped(ro, *a, **k):
        calls.append((ro.shape[0], k.get("sample_major", 0)))
        return real(ro, *a, **k)
    monkeypatch.setattr(R, op, wrapped)
    return calls


def test_above_64_tiles_everything_takes_the_single_pass_route(monkeypatch):
    """G65 (65 tiles): the ops choose the plain (unfolded) images and the single-pass f32 kernel under the DEFAULT INFER_ARITH --
    the oracle's values, and the very bits of INFER_ARITH = "f32" -- and the renderer drops to layout 0, unpadded, without the
    fused slot lists, and still renders the oracle's image."""
    H, D, hg = ops(), dev_scene("G65"), HG()
    sc, rays = RS.named("G65")
    o, d = rays["shuffled"]
    assert hg.INFER_ARITH == "t16" and hg.FOLD_ACTIVATION
    passes = two_passes("G65", "shuffled")
    assert not hg._infer_folded(65, g(passes[0][0])) and hg._infer_folded(64, g(passes[0][0]))
    first = np.concatenate([p[2][..., 0].reshape(-1) for p in passes])
    default = [run_pts_inference("G65", "shuffled", z, dd, bi, 0) for z, dd, bi, _ in passes]
    for k, (got, p) in enumerate(zip(default, passes)):
        for a, b, what in zip(got, p[3], ("diffuse", "specular", "alpha")):
            close(a, b, f"{what} pass {k}")
    alphas = np.concatenate([got[2].reshape(-1) for got in default])
    dark = [t for t in range(65) if not (first == t).any() or not alphas[first == t].max() > 0]
    assert not dark, f"tiles {dark} render nothing"
    # background, every blend step
    inter_ref = O.ray_block_intersection(o, d, sc["corners"], sc["sizes"])
    tb_ref, _ = RS.tracing_order(inter_ref)
    ob_ref, _ = O.update_outgoing_bidx(o, d, sc["corners"], sc["sizes"], tb_ref, inter_ref, 0.12, False)
    assert (ob_ref[:, 3] != -1).sum() >= 5 and ob_ref.max() == 64
    bg_default = []
    for i in range(4):
        zb_ref = O.render_inverse_z_sampling(inter_ref, ob_ref[:, i], SB, 1e6)
        out = filled(B, SB)
        H.bg_pts_inference_v2(g(o), g(d), g(zb_ref), g(ob_ref), i, D["corners"], D["sizes"], D["res"], D["tables"], D["params"], *out)
        ref = O.bg_pts_inference_v2(o, d, zb_ref, ob_ref, i, sc["corners"], sc["sizes"], sc["res"], sc["tables"], sc["params"])
        for a, b, what in zip(out, ref, ("diffuse", "specular", "alpha")):
            close(n(a), b, f"bg {what} blend step {i}")
        bg_default.append([n(t) for t in out])
    # the route is the f32 kernel's: bit for bit
    monkeypatch.setattr(hg, "INFER_ARITH", "f32")
    for got, (z, dd, bi, _) in zip(default, passes):
        for a, b in zip(got, run_pts_inference("G65", "shuffled", z, dd, bi, 0)):
            assert np.array_equal(a, b)
    monkeypatch.setattr(hg, "INFER_ARITH", "t16")
    # a layout the single-pass kernel cannot read is refused, not misread
    z, dd, bi, _ = passes[0]
    with pytest.raises(RuntimeError, match="sample-major"):
        run_pts_inference("G65", "shuffled", z, dd, bi, 2)
    # the renderer
    sampled, fused = count_calls(monkeypatch, "sample_points"), count_calls(monkeypatch, "pts_inference_tracing")
    got = render("G65")                       # (layout=2 asked for, as by default)
    assert sampled and all(sm == 0 for _, sm in sampled) and max(b for b, _ in sampled) == B and not fused
    image_close(got, oracle_image("G65"), "G65")
    assert oracle_image("G65")["T"].min() < 0.5 < oracle_image("G65")["T"].max()


# ------------------------------------------------------------------ f. renderer end to end
@pytest.mark.parametrize("name", ["G9", "G36", "G64"])
def test_renderer_end_to_end_on_grids(name, monkeypatch):
    """TileSetRenderer.render_rays on 9, 36 and 64 tiles: the oracle's loop, in the layouts 0 and 2 (on G9 also 1), twice the same
    bits, and the later tracing passes run on the compacted running rays."""
    sampled, fused = count_calls(monkeypatch, "sample_points"), count_calls(monkeypatch, "pts_inference_tracing")
    ref = oracle_image(name)
    assert ref["T"].min() < 1e-5 and ref["T"].max() == 1.0 and (ref["T"] < 0.5).mean() > 0.5
    lay2 = render(name)
    n2 = len(sampled)
    assert all(sm == 2 for _, sm in sampled) and sampled[0][0] == B + -B % 32 and not fused
    assert min(b for b, _ in sampled) < sampled[0][0], "no tracing pass ran on the compacted rays"
    image_close(lay2, ref, f"{name} layout 2")
    lay0 = render(name, layout=0)
    assert all(sm == 0 for _, sm in sampled[n2:]) and sampled[n2][0] == B
    image_close(lay0, ref, f"{name} layout 0")
    close(lay2[0], lay0[0], "layouts diffuse")
    close(lay2[1], lay0[1], "layouts specular")
    close(lay2[2], lay0[2], "layouts depth", depth=True)
    np.testing.assert_allclose(lay2[3], lay0[3], rtol=1e-4, atol=1e-6)
    for a, b in zip(lay2, render(name)):
        assert np.array_equal(a, b)
    for a, b in zip(lay0, render(name, layout=0)):
        assert np.array_equal(a, b)
    if name == "G9":   # the [S,B] layout, end to end here alone: unpadded like layout 0
        n01 = len(sampled)
        image_close(render(name, layout=1), ref, f"{name} layout 1")
        assert len(sampled) > n01 and all(sm == 1 for _, sm in sampled[n01:])
        assert sampled[n01][0] == B and all(b <= B for b, _ in sampled[n01:])


def test_renderer_fused_and_two_op_routes_give_the_same_bits_at_eight_tiles(monkeypatch):
    fused = count_calls(monkeypatch, "pts_inference_tracing")
    rnd = renderer("G8")
    assert rnd.fuse_slots
    on = render("G8")
    n_on = len(fused)
    monkeypatch.setattr(rnd, "fuse_slots", False)
    off = render("G8")
    assert n_on >= 2 and len(fused) == n_on, "the switch must switch"
    for a, b in zip(on, off):
        assert np.array_equal(a, b)
    image_close(on, oracle_image("G8"), "G8")


# ------------------------------------------------------------------ g. truncation at four
def test_lists_truncate_at_four_and_write_nothing_beyond():
    """STACK6: six tiles hold every sample and share every exit distance.  Slot lists and exit lists are the first four tiles (the
    oracle's clamp; the reference writes a fifth and sixth entry out of bounds), the blend weights the oracle's, and nothing lands
    outside the [.,4] arrays, which lie inside guard tensors here.  (Inference over the four decoders per sample and the four
    blend steps: test_stage_by_stage_over_every_scene[STACK6].)"""
    H, D = ops(), dev_scene("STACK6")
    sc, rays = RS.named("STACK6")
    o, d = rays["shuffled"]
    z, dd, bi_ref, ref = two_passes("STACK6", "shuffled")[0]
    inter_ref = O.ray_block_intersection(o, d, sc["corners"], sc["sizes"])
    tb_ref, _ = RS.tracing_order(inter_ref)
    hit = (inter_ref[..., 0] != 1e7).any(-1)
    RO, RD, INTER, TB = g(o), g(d), g(inter_ref), g(tb_ref)
    pad = 4096
    # exit lists
    guard_b = torch.full((pad + B * 4 + pad,), -1, dtype=torch.int16, device=DEV)
    guard_w = torch.zeros(pad + B * 4 + pad, device=DEV)
    ob, bw = guard_b[pad:pad + B * 4].view(B, 4), guard_w[pad:pad + B * 4].view(B, 4)
    H.update_outgoing_bidx(RO, RD, D["corners"], D["sizes"], TB, INTER, ob, bw, 0.12, False)
    ob_ref, bw_ref = O.update_outgoing_bidx(o, d, sc["corners"], sc["sizes"], tb_ref, inter_ref, 0.12, False)
    assert np.array_equal(n(ob), ob_ref) and np.array_equal(n(bw), bw_ref)
    assert (ob_ref[hit] == np.int16([0, 1, 2, 3])).all() and (ob_ref[~hit] == -1).all() and hit.sum() > 400
    assert (bw_ref[hit] > 0).all(1).mean() > 0.9
    for guard, fill in ((guard_b, -1), (guard_w, 0)):
        assert bool((guard[:pad] == fill).all()) and bool((guard[pad + B * 4:] == fill).all())
    # origins inside all six tiles
    guard_b.fill_(-1), guard_w.zero_()
    H.update_outgoing_bidx_v2(RO, RD, D["corners"], D["sizes"], TB, INTER, ob, bw)
    ob2_ref, bw2_ref = O.update_outgoing_bidx_v2(o, sc["corners"], sc["sizes"])
    assert np.array_equal(n(ob), ob2_ref) and np.array_equal(n(bw), bw2_ref) and (ob2_ref[:, 3] == 3).sum() > 100
    for guard, fill in ((guard_b, -1), (guard_w, 0)):
        assert bool((guard[:pad] == fill).all()) and bool((guard[pad + B * 4:] == fill).all())
    # slot lists
    guard_s = torch.full((pad + B * S * 4 + pad,), -1, dtype=torch.int16, device=DEV)
    bi = guard_s[pad:pad + B * S * 4].view(B, S, 4)
    H.prepare_points(g(z), torch.ones(B, dtype=torch.bool, device=DEV), INTER, bi)
    assert np.array_equal(n(bi), bi_ref)
    listed = bi_ref[..., 0] != -1
    assert listed.sum() > 5000 and (bi_ref[listed] == np.int16([0, 1, 2, 3])).all()
    assert bool((guard_s[:pad] == -1).all()) and bool((guard_s[pad + B * S * 4:] == -1).all())
    # four decoders per sample, in both chunk kernels' layouts
    for lay in (0, 2):
        for got, want, what in zip(run_pts_inference("STACK6", "shuffled", z, dd, bi_ref, lay), ref, ("diffuse", "specular", "alpha")):
            close(got, want, f"{what} layout {lay}")
