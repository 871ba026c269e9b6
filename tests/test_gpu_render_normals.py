"""Normal maps of the multi-tile renderer on the GPU (csrc/render_normals_tiles.hip; needs an MI355X): pts_normals per sample,
accumulate_normal per ray and TileSetRenderer.render_rays / render with normals=True, each against the float64 evaluation of
tests/render_normals_reference.py behind float32-pinned slots and cells, held to K = 8 times the float32 yardstick's own error per
statistic (floor 2^-24).  What the scenes contain is checked without a GPU in tests/test_render_normals_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import render_normals_reference as R
import render_scenes as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = RS.B_RAYS
BP = B + -B % 32
S_VIEW, S_BG = 33, 16
f32 = np.float32


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def n(t):
    return t.detach().cpu().numpy()


def ops():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import hashgrid as H
    return H


@functools.lru_cache(maxsize=None)
def dev_scene(name):
    sc, _ = R.scene(name)
    return tuple(g(sc[k]) for k in ("tables", "params", "res", "occ", "starts", "l2d", "corners", "sizes"))


def pad32(a):
    pad = -a.shape[0] % 32
    return np.concatenate([a, np.repeat(a[-1:], pad, 0)]) if pad else a


def to_layout(a, lay):
    """[B,S,...] -> the layout's array (scanerf_hip.h sample_major): 1 = [S,B,...], 2 = [B/32,S,32,...] with B padded to 32"""
    if lay == 0:
        return np.ascontiguousarray(a)
    if lay == 1:
        return np.ascontiguousarray(np.swapaxes(a, 0, 1))
    a = pad32(a)
    return np.ascontiguousarray(np.swapaxes(a.reshape(a.shape[0] // 32, 32, *a.shape[1:]), 1, 2))


def from_layout(a, lay):
    if lay == 0:
        return a
    if lay == 1:
        return np.swapaxes(a, 0, 1)
    return np.swapaxes(a, 1, 2).reshape(a.shape[0] * 32, a.shape[1], *a.shape[3:])[:B]


def run_pts_normals(name, ins, lay, counts=None):
    """pts_normals on the case's inputs in the layout, the output prefilled with NaN -> [B,S,3] numpy (counts: the counted launch)"""
    rays = (g(pad32(ins["o"])), g(pad32(ins["d"]))) if lay == 2 else (g(ins["o"]), g(ins["d"]))
    z, dd, bi = (g(to_layout(ins[k], lay)) for k in ("z", "dd", "bi"))
    out = torch.full(tuple(z.shape) + (3,), float("nan"), device=DEV)
    ops().pts_normals(*rays, z, dd, bi, *dev_scene(name), out, sample_major=lay, counts=counts)
    return from_layout(n(out), lay)


# ------------------------------------------------------------------------------------------------------------ per sample
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("name,S", R.SAMPLE_CASES)
def test_pts_normals_per_sample(name, S, order):
    """Every sample of the first tracing pass against float64, in the three layouts (B = 509, padded to 512 in the ray-block layout):
    every sample written, samples without a slot exactly zero, equal bits in the three layouts and on a second launch."""
    ins, r64, r32 = R.sample_reference(name, S, order)
    got = {lay: run_pts_normals(name, ins, lay) for lay in (0, 1, 2)}
    bad = R.judge_normals(f"pts_normals {name} S={S} {order}", got[2].reshape(-1, 3), r64["normal"], r32["normal"])
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any() and not np.isnan(got[2]).any(), "a sample was left unwritten"
    none = ~r64["pin"]["listed"][:, 0]
    assert none.sum() > 0 and not got[2].reshape(-1, 3)[none].any()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), "the layouts differ"
    assert np.array_equal(got[2], run_pts_normals(name, ins, 2)), "two launches differ"
    # the counted launch (the measurement entry point's own kernel instance) must give the same bits: that is the check.  The
    # counters (groups that ran a tile, stagings, passes of the tile loop, lanes with a sample in them) are only held to what any
    # correct count satisfies; a miscounted staging or pass inside these ranges would go unnoticed
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert np.array_equal(got[2], run_pts_normals(name, ins, 2, counts=counts)), "the counted launch differs"
    groups, stagings, passes, lanes = (int(c) for c in n(counts))
    pin = r64["pin"]
    assert 0 < groups <= -(-BP * S // 64) and 1 <= stagings <= passes and groups <= passes and 0 < lanes <= 64 * passes
    assert lanes >= int((pin["listed"] & pin["occ"]).sum()), "an occupied listed slot was not served"
    if name == "G9Z":   # the zero-table tile alone: no normal at all
        pin = r64["pin"]
        only = (pin["listed"].sum(1) == 1) & pin["occ"][:, 0] & (pin["b"][:, 0] == R.ZERO_TILE)
        assert only.sum() > 10 and not got[2].reshape(-1, 3)[only].any()
    assert not bad, bad


def test_pts_normals_refuses_what_it_cannot_read():
    H = ops()
    ins = R.sample_reference("G9", 16)[0]
    z, dd, bi = (g(ins[k]) for k in ("z", "dd", "bi"))
    out = torch.empty(B, 16, 3, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        H.pts_normals(g(ins["o"]), g(ins["d"]), z, dd, bi, *dev_scene("G9"), out, sample_major=2)
    with pytest.raises(RuntimeError, match="shape"):
        H.pts_normals(g(ins["o"]), g(ins["d"]), z, dd, bi, *dev_scene("G9"), out[:, :15].contiguous())
    with pytest.raises(RuntimeError, match="dtype"):
        H.pts_normals(g(ins["o"]), g(ins["d"]), z, dd, bi.int(), *dev_scene("G9"), out)


# ------------------------------------------------------------------------------------------------------------ per ray
@functools.lru_cache(maxsize=None)
def accumulate_case():
    """Per-sample normals (the float32 yardstick's) and the oracle's alpha of G9's first pass at S = 33; start transparencies with
    rays below the 1e-5 threshold and at it; a non-zero start normal; the oracle's and the float64 result."""
    ins, r64, r32 = R.sample_reference("G9", 33)
    sc = ins["sc"]
    S = ins["z"].shape[1]
    pn = r32["normal"].numpy().reshape(B, S, 3)
    pa = O.pts_inference(ins["o"], ins["d"], ins["z"], ins["dd"], ins["bi"], sc["tables"], sc["params"], sc["res"], sc["occ"], sc["starts"],
                         sc["l2d"], sc["corners"], sc["sizes"])[2]
    rng = np.random.default_rng(5)
    T0 = rng.uniform(0.2, 1.0, (B, 1)).astype(f32)
    T0[::7] = f32(5e-6)
    T0[3::7] = f32(1e-5)
    start = rng.normal(size=(B, 3)).astype(f32)
    ref32, T = start.copy(), T0.copy()
    O.accumulate_color(pn, np.zeros_like(pn), pa, T, ins["z"], ref32, np.zeros((B, 3), f32), np.zeros((B, 1), f32))
    ref64 = R.accumulate_normal(pn, pa, T0, start.astype(np.float64), np.float64)
    return ins["z"], pn, pa, T0, start, ref32, ref64


def run_accumulate(z, pn, pa, T0, start, lay, flags=0):
    """-> (normal [B,3], transparency after the call) numpy"""
    Bl = BP if lay == 2 else B
    tr, nm = g(pad32(T0) if lay == 2 else T0), g(pad32(start) if lay == 2 else start)
    assert tr.shape[0] == Bl
    ops().accumulate_normal(g(to_layout(pn, lay)), g(to_layout(pa, lay)), tr, g(to_layout(z, lay)), nm, sample_major=lay | flags)
    return n(nm)[:B], n(tr)[:B]


@pytest.mark.parametrize("lay", (0, 1, 2))
def test_accumulate_normal(lay):
    """Against O.accumulate_color with the normal as its diffuse array (the kernel sums in that order: the same bits) and against
    float64; rays below 1e-5 untouched, the start added into, the transparency not written; with SKIP_UNSAMPLED the rays without a
    sample are not read."""
    H = ops()
    z, pn, pa, T0, start, ref32, ref64 = accumulate_case()
    got, tr = run_accumulate(z, pn, pa, T0, start, lay)
    bad = R.judge_normals(f"accumulate_normal layout {lay}", got, ref64, ref32)
    assert np.array_equal(tr, T0), "the transparency was written"
    assert np.array_equal(got[::7], start[::7]) and not np.array_equal(got[3::7], start[3::7])
    assert np.array_equal(got, ref32)
    assert not bad, bad
    un = z[:, 0] == -1
    assert 10 < un.sum() < B // 2
    pn2, pa2 = pn.copy(), pa.copy()
    pn2[un], pa2[un] = np.nan, np.nan
    skip, tr = run_accumulate(z, pn2, pa2, T0, start, lay, H.SKIP_UNSAMPLED)
    assert np.isfinite(skip).all() and np.array_equal(skip, got) and np.array_equal(tr, T0)
    assert np.isnan(run_accumulate(z, pn2, pa2, T0, start, lay)[0][un & (T0[:, 0] >= 1e-5)]).all(), "the flag must be what skips them"


# ------------------------------------------------------------------------------------------------------------ the renderer
@functools.lru_cache(maxsize=None)
def renderer(name):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import renderer as RR
    return RR.TileSetRenderer(DEV, RS.renderer_tiles(RS.named(name)[0]))


@functools.lru_cache(maxsize=None)
def view_reference(name):
    o, d = RS.named(name)[1]["shuffled"]
    return R.render_loop(R.renderer_arrays(renderer(name)), o, d, S_VIEW, S_BG)


def render(name, **kw):
    o, d = RS.named(name)[1]["shuffled"]
    return [n(t) for t in renderer(name).render_rays(g(o), g(d), num_sample=S_VIEW, num_bg_sample=S_BG, **kw)]


def count_calls(monkeypatch, op):
    """wrap renderer.<op>; -> the list its calls' (size of the first argument, sample_major flags, whether the second argument -- where
    it is a mask: prepare_points' running rays -- is all true) are appended to"""
    import scanerf_amd  # noqa: F401
    from scanerf_amd import renderer as RR
    calls, real = [], getattr(RR, op)

    def wrapped(first, *a, **k):
        mask = a[0] if a and isinstance(a[0], torch.Tensor) and a[0].dtype == torch.bool else None
        calls.append((first.shape[0], k.get("sample_major", 0), None if mask is None else bool(mask.all())))
        return real(first, *a, **k)
    monkeypatch.setattr(RR, op, wrapped)
    return calls


@pytest.mark.parametrize("name", ("G9", "STACK3", "G65", "G8"))
def test_renderer_normals_per_ray(name, monkeypatch):
    """render_rays(normals=True) against the oracle's loop extended by the normal: G9 on the ray-block layout with slot lists, G65 on the
    layout-0 fallback, G8 and STACK3 on the fused tracing route.  The colour outputs are the bits of normals=False; the full-size and the
    compacted pass route, and the fused and the two-op slot route, give equal bits in the normal."""
    rnd = renderer(name)
    sampled, fused, listed, nrm = (count_calls(monkeypatch, op) for op in ("sample_points", "pts_inference_tracing", "prepare_points",
                                                                           "pts_normals"))
    ref = view_reference(name)
    plain = render(name)
    n_plain = (len(sampled), len(fused), len(listed))
    assert len(plain) == 4 and not nrm
    got = render(name, normals=True)
    assert len(got) == 5 and got[4].shape == (B, 3) and got[4].dtype == np.float32
    bad = R.judge_normals(f"render_rays {name}", got[4], ref["normal64"], ref["normal32"])
    for a, b, what in zip(plain, got, ("diffuse", "specular", "depth", "transparency")):
        assert np.array_equal(a, b), f"normals=True changed the {what}"
    # the colour route stays what it was; the slot lists come from prepare_points on either route
    assert len(sampled) == 2 * n_plain[0] and len(fused) == 2 * n_plain[1] and len(nrm) == n_plain[0]
    assert len(listed) - n_plain[2] == n_plain[0] if n_plain[1] else len(listed) == 2 * n_plain[2]
    assert bool(n_plain[1]) == (name in ("G8", "STACK3")), "up to eight tiles run the fused tracing route, more cannot"
    assert all(sm == (0 if name == "G65" else 2) for _, sm, _ in nrm)
    if name != "STACK3":   # rays that cross several tiles in sequence: more than one tracing pass each
        assert (ref["passes"] >= 2).sum() >= 50 and n_plain[0] >= 2, (ref["passes"] >= 2).sum()
        assert ref["T"].min() < 1e-5, "no ray saturates: the 1e-5 rule is not exercised"
    assert float(np.linalg.norm(ref["normal64"], axis=1).max()) > 0.3
    # both pass routes
    for tenths in (0, 11):
        monkeypatch.setattr(rnd, "compact_below_tenths", tenths)
        del listed[:]
        other = render(name, normals=True)
        # (a compacted pass hands prepare_points an all-true mask; the full-size pass's mask leaves out the rays that miss every tile)
        assert listed and all(every == (tenths == 11) for _, _, every in listed), (tenths, listed)
        assert np.array_equal(other[4], got[4]), f"compact_below_tenths={tenths} changed the normal"
    monkeypatch.setattr(rnd, "compact_below_tenths", 9)
    if n_plain[1]:
        monkeypatch.setattr(rnd, "fuse_slots", False)
        n_fused = len(fused)
        off = render(name, normals=True)
        assert len(fused) == n_fused, "the switch must switch"
        for a, b in zip(got, off):
            assert np.array_equal(a, b)
    assert not bad, bad


def test_render_returns_the_normal_map_of_its_rays():
    rnd = renderer("G9")
    H, W = 24, 40
    K = np.float32([[30, 0, 20], [0, 30, 12], [0, 0, 1]])
    c2w = np.float32([[0, 0, 1, -6], [0, 1, 0, 0.3], [-1, 0, 0, 5.2]])   # looking down +x from x = -6
    out = rnd.render(H, W, K, c2w, num_sample=S_VIEW, num_bg_sample=S_BG, normals=True)
    assert len(out) == 5 and tuple(out[4].shape) == (H, W, 3)
    rays = rnd.render_rays(*rnd.compute_rays(H, W, K, c2w), num_sample=S_VIEW, num_bg_sample=S_BG, normals=True)
    for a, b in zip(out, rays):
        assert torch.equal(a.reshape(b.shape), b)
    assert float(out[4].norm(dim=-1).max()) > 0.3 and torch.isfinite(out[4]).all()
    four = rnd.render(H, W, K, c2w, num_sample=S_VIEW, num_bg_sample=S_BG)
    assert len(four) == 4 and all(torch.equal(a, b) for a, b in zip(four, out))
