"""The reference of tests/test_gpu_render_infer_error.py judged on its own (CPU only): its float32 run against the C oracle, its
float64 run against the goldens, every family's stated condition and every cap -- for exactly the cases the GPU file runs
(tests/render_infer_reference.py holds the list).

How close "the float32 run reproduces the C oracle" can be: both are float32 evaluations of one formula with different rounding
(summation order, expf against torch.exp), each at its own distance from the exact value, so they differ by up to the SUM of the two
distances.  The oracle's own distance is not an input here; with the float32 run's own distance to float64 on the case as the unit
(printed), the pooled L2 difference is held to 2 units (two independent roundings give sqrt 2) and the largest element to 4 (the
sum of two maxima, the oracle's taken as at most 3 units).  A restatement that differs from the oracle in a formula differs by thousands of
units.  The pinned parts -- which samples run at all, and the blend weights -- are bit-equal."""
import os

import numpy as np
import pytest
import torch

import render_infer_reference as R
import render_normals_reference as RNR
import render_scenes as RS
from oracle import oracle as O

F64, F32 = R.F64, R.F32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ("tables", "params", "res", "occ", "starts", "l2d", "corners", "sizes")


def _against_oracle(name, C, r64, r32):
    for what, g in zip(("dif", "spec", "alpha"), C):
        g = np.asarray(g, np.float64).reshape(r64[what].shape)
        a32, a64 = r32[what].numpy().astype(np.float64), r64[what].numpy()
        assert np.isfinite(a64).all() and np.isfinite(a32).all(), f"{name} {what}: the reference is not finite"
        dC, unit = np.abs(g - a32), np.abs(a32 - a64)
        print(f"{name} {what}: float32 run to float64 max {unit.max():.2e} L2 {np.linalg.norm(unit):.2e} | to the oracle max {dC.max():.2e} "
              f"L2 {np.linalg.norm(dC):.2e}")
        assert np.array_equal(g == 0, a32 == 0), f"{name} {what}: the samples that come out exactly 0 differ"
        assert np.linalg.norm(dC) <= 2 * np.linalg.norm(unit) and dC.max() <= 4 * unit.max(), f"{name} {what}"


def _oracle_pts(ins):
    sc = ins["sc"]
    return O.pts_inference(ins["o"], ins["d"], ins["z"], ins["dd"], ins["bi"], *(sc[k] for k in TAIL))


@pytest.mark.parametrize("c", R.PTS_CASES, ids=R.case_id)
def test_float32_run_reproduces_the_oracle_pts_inference(c):
    ins, r64, r32 = R.pts_reference(c)
    _against_oracle(R.case_id(c), _oracle_pts(ins), r64, r32)
    zero = (r64["alpha"] == 0).numpy()
    assert zero.any() and not zero.all()
    for r in (r64, r32):    # a sample whose alpha is exactly 0 is exactly 0
        assert float(r["dif"][torch.from_numpy(zero)].abs().max()) == 0 and float(r["spec"][torch.from_numpy(zero)].abs().max()) == 0


@pytest.mark.parametrize("c", [R.Case("G9", 17, "base"), R.Case("STACK6", 33, "base"), R.Case("G9", 17, "face"), R.Case("STACK6", 33, "face")],
                         ids=R.case_id)
def test_pinned_weights_are_the_oracles_bits(c):
    """Decoders that are zero but for a density bias of 60 and intervals of 1: every occupied slot has pa == 1.0f and c_d == 0.5f in
    float32, so the oracle's alpha is (sum of the occupied slots' w) / (sum of the listed slots' w) and its diffuse half of that, formed
    from its own weights in slot order -- the float32 run must give the same BITS, which it can only from the same weights, lists
    and cells."""
    ins = dict(R.pts_reference(c)[0])
    sc = dict(ins["sc"])
    blob = np.zeros(O.PARAMSIZE, np.float32)
    sd = {k: v.clone() for k, v in O.unpack_blob(torch.from_numpy(blob)).items()}
    sd["sigma_layer.mlp.0.bias"] = sd["sigma_layer.mlp.0.bias"] + 60.0
    sc["params"] = np.stack([O.pack_blob(sd).numpy()] * sc["corners"].shape[0])
    ins.update(sc=sc, dd=np.ones_like(ins["dd"]))
    C = _oracle_pts(ins)
    r32 = R.pts_inference(sc, ins["o"], ins["d"], ins["z"], ins["dd"], ins["bi"], F32)
    pin = r32["pin"]
    mixed = (pin["listed"] & ~pin["occ"]).any(1) & pin["occ"].any(1)
    print(f"{R.case_id(c)}: {int(pin['occ'].any(1).sum())} samples run, {int(mixed.sum())} of them also list an unoccupied slot")
    assert mixed.sum() > 100
    assert np.array_equal(C[2].reshape(-1), r32["alpha"].numpy()) and np.array_equal(C[0].reshape(-1, 3), r32["dif"].numpy())
    # (the stack's tiles share one box, hence one weight: its ratios are k / 4 but for rounding)
    assert len(np.unique(C[2])) > (100 if c.scene == "G9" else 5)


@pytest.mark.parametrize("c", R.BG_CASES + R.BG_V1_CASES, ids=R.case_id)
def test_float32_run_reproduces_the_oracle_background(c):
    ins, r64, r32 = R.bg_reference(c)
    sc = ins["sc"]
    tail = (sc["corners"], sc["sizes"], sc["res"], sc["tables"], sc["params"])
    if c.step is None:
        C = O.bg_pts_inference(ins["o"], ins["d"], ins["z"], ins["ob"], ins["bw"], *tail)
        assert ((ins["ob"] != -1).sum(1) == min(4, sc["corners"].shape[0])).sum() >= 5
    else:
        C = O.bg_pts_inference_v2(ins["o"], ins["d"], ins["z"], ins["ob"], c.step, *tail)
        n_rays = int((ins["ob"][:, c.step] != -1).sum())
        assert 5 <= n_rays and (c.family == "axis" or n_rays < ins["o"].shape[0])   # some rays have no tile: they stay 0
    _against_oracle(R.case_id(c), C, r64, r32)


@pytest.mark.parametrize("c", R.RAY_CASES, ids=R.case_id)
def test_float32_accumulation_is_the_oracles_and_ties_stay_under_the_cap(c):
    """accumulate_color over each of the case's pass sequences: the float32 run gives the oracle's bits (the same products and sums in the
    same order), the float64 run differs from it by rounding only, and no more than TIE_CAP of the rays come within TIE_BAND of the
    skip threshold -- in the op's sequences and in the loop that TileSetRenderer.render_rays is judged against."""
    sc, o, d, loop = R.ray_reference(c)
    B = o.shape[0]
    print(f"{R.case_id(c)}: loop ties {int(loop['tied'].sum())} of {B} (cap {R.TIE_CAP * B:.2f}); {len(loop['passes'])} tracing passes, "
          f"{len(loop['bg'])} background steps; transmittance {loop['f64']['T'].min():.2e} .. {loop['f64']['T'].max():.2e}")
    assert loop["tied"].mean() <= R.TIE_CAP
    assert len(loop["passes"]) >= 2 and len(loop["bg"]) == 4
    skipped = 0
    for k, (seq, s64, s32, tied) in enumerate(R.accumulate_reference(c)):
        T, dif, spec, depth = np.ones((B, 1), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 1), np.float32)
        for pd, ps, pa, z in seq:
            skipped += int((T[:, 0] < 1e-5).sum())
            O.accumulate_color(pd, ps, pa[..., None], T, z, dif, spec, depth)
        print(f"  sequence {k}: {len(seq)} passes, ties {int(tied.sum())}; float32 to float64: T {np.abs(s32['T'] - s64['T']).max():.2e} "
              f"colour {np.abs(s32['dif'] - s64['dif']).max():.2e} depth rel {np.abs(s32['depth'][s64['depth'] > 0] / s64['depth'][s64['depth'] > 0] - 1).max():.2e}")
        assert tied.mean() <= R.TIE_CAP
        assert np.array_equal(T[:, 0], s32["T"]) and np.array_equal(dif, s32["dif"]) and np.array_equal(spec, s32["spec"])
        assert np.array_equal(depth[:, 0], s32["depth"])
        assert np.abs(s32["T"] - s64["T"]).max() < 1e-5 and np.abs(s32["dif"] - s64["dif"]).max() < 1e-5
    if c.scene == "G9" and c.family in ("base", "dense", "fresh"):
        assert skipped > 0, "no pass ever skipped a ray: the threshold is not exercised"
    for k in ("dif", "spec", "T"):
        assert np.abs(loop["f32"][k] - loop["f64"][k]).max() < 1e-4


# ------------------------------------------------------------------------------------------------------------ the families' conditions
def _occupied_alpha(r64):
    return r64["pa"][torch.from_numpy(r64["pin"]["occ"])]


@pytest.mark.parametrize("name,S", [("G9", 17), ("STACK6", 33)])
def test_every_family_is_what_it_is_called(name, S):
    """The conditions of the families, asserted of the float64 reference alone."""
    ref = {f: R.pts_reference(R.Case(name, S, f)) for f in R.FAMILIES}
    base = ref["base"][1]
    say = lambda f, what: print(f"{name}-{S}-{f}: {what}")

    say("base", f"largest alpha {float(base['alpha'].max()):.3f}")
    assert float(base["alpha"].max()) > 0.05

    a = _occupied_alpha(ref["dense"][1])
    say("dense", f"{float((a > 0.999).double().mean()):.3f} of the occupied samples above 0.999, {int((ref['dense'][2]['alpha'] == 1).sum())} samples are 1.0f")
    assert float((a > 0.999).double().mean()) > 0.5

    a = _occupied_alpha(ref["thin"][1])
    say("thin", f"median occupied alpha {float(a.median()):.2e}, largest {float(a.max()):.2e}")
    assert 1e-6 <= float(a.median()) <= 1e-3

    st, st0 = ref["bias"][1]["stats"], base["stats"]
    say("bias", f"{st.below_half / st.units:.3f} of the hidden units below 0.5 (base {st0.below_half / st0.units:.3f})")
    assert st.below_half / st.units > 0.1 and st.below_half / st.units > st0.below_half / st0.units + 0.1

    st = ref["wide"][1]["stats"]
    say("wide", f"{st.first_dead / st.first:.3f} of the first-layer units below 1e-6 (base {st0.first_dead / st0.first:.3f})")
    assert st.first_dead / st.first > 0.1

    ins, r64, _ = ref["fresh"]
    tab = np.abs(ins["sc"]["tables"].astype(np.float32))
    sub = ((tab > 0) & (tab < 2.0 ** -14)).mean()
    one = torch.from_numpy(r64["pin"]["occ"].sum(1) == 1)   # dif / alpha is then the one tile's c_d: the weights cancel
    colour = (r64["dif"][one] / r64["alpha"][one, None]).numpy()
    say("fresh", f"{sub:.3f} of the table entries are f16 subnormals; single-slot colours spread {colour.std(0).max():.2e} over {len(colour)} samples")
    assert sub > 0.1 and colour.std(0).max() > 1e-6 and float(r64["alpha"][one].std()) > 1e-3

    ins, r64, r32 = ref["zero"]
    z_tile = R.ZERO_TILE[name]
    hit = (r64["pin"]["occ"] & (r64["pin"]["b"] == z_tile)).sum()
    say("zero", f"{int(hit)} occupied slots read the zeroed table of tile {z_tile}")
    assert hit > 200 and not ins["sc"]["tables"][z_tile].any()
    for r in (r64, r32):
        assert all(bool(torch.isfinite(r[k]).all()) for k in ("dif", "spec", "alpha"))

    ins = ref["axis"][0]
    nz = (ins["d"] != 0).sum(1)
    say("axis", f"{int((nz == 1).sum())} rays along an axis, {int((nz == 2).sum())} with one zero component; {int(ref['axis'][1]['pin']['occ'].sum())} occupied slots")
    assert (nz == 1).sum() > 100 and (nz == 2).sum() > 100 and (nz == 3).sum() == 0 and ref["axis"][1]["pin"]["occ"].sum() > 2000

    ins, r64, _ = ref["face"]
    sc, pin = ins["sc"], r64["pin"]
    wp = (ins["o"][:, None, :] + ins["z"][..., None] * ins["d"][:, None, :]).astype(np.float32).reshape(-1, 1, 3)
    pts = ((wp - sc["corners"][pin["b"]]) / sc["sizes"][pin["b"]]).astype(np.float32)
    on_x, on_z = ((pts[..., k] == 0) | (pts[..., k] == 1) for k in (0, 2))
    both, one_ = (pin["listed"] & on_x & on_z).sum(), (pin["listed"] & (on_x ^ on_z)).sum()
    shared = (pin["listed"] & on_x).sum(1).max()
    say("face", f"listed slots on a face in x and z (weight 0): {int(both)}, in one of them (the one-distance branch): {int(one_)}; "
        f"up to {int(shared)} tiles share a sample's face; occupied slots of weight 0: {int((pin['occ'] & (pin['w'] == 0)).sum())}")
    assert one_ > 1000 and shared >= (4 if name == "STACK6" else 1)
    if name == "G9":
        assert both > 100 and (pin["occ"] & (pin["w"] == 0)).sum() > 50

    for f, k in (("long", R.SCALE_D), ("short", 1 / R.SCALE_D)):
        ins, r64, _ = ref[f]
        dn = np.linalg.norm(ins["d"].astype(np.float64), axis=1)
        delta, delta0 = ins["dd"].astype(np.float64) * dn[:, None], ref["base"][0]["dd"].astype(np.float64) * dn[:, None] / k
        say(f, f"|d| {dn.min():.3g} .. {dn.max():.3g}; dist |d| and alpha equal to base: {np.array_equal(delta, delta0)}, {bool(torch.equal(r64['alpha'], base['alpha']))}")
        assert np.array_equal(delta, delta0) and np.array_equal(r64["pin"]["i0"], base["pin"]["i0"]) and np.array_equal(r64["pin"]["t"], base["pin"]["t"])
        assert float((r64["alpha"] - base["alpha"]).abs().max()) < 1e-15 and float((r64["spec"] - base["spec"]).abs().max()) < 1e-14
        assert (dn.max() > 1e3) if f == "long" else (dn.min() < 1e-3)


def test_case_lists_are_the_issues():
    assert {(c.scene, c.S) for c in R.CASES_SCENES} == {("G9", 16), ("G9", 17), ("G9", 33), ("STACK6", 33), ("G36", 16), ("G65", 16)}
    assert {(c.S, c.step) for c in R.BG_CASES if c.family == "base" and c.scene == "G9"} == {(16, 0), (16, 1), (48, 0), (48, 1)}
    assert all(RS.named(c.scene)[1]["shuffled"][0].shape[0] == 509 for c in R.CASES_SCENES)
    assert RS.named(R.TRACING_CASE.scene)[0]["corners"].shape[0] <= 8 < RS.named(R.CROSS_CASE.scene)[0]["corners"].shape[0]
    for c in R.CASES_SCENES:   # every case lists one, two and four tiles per sample somewhere (the stack: four)
        counts = RNR.slot_counts(R.pts_reference(c)[0]["bi"])
        assert counts[4] > 300 and (c.scene == "STACK6" or (counts[1] > 1000 and counts[2] > 1000)), counts


# ------------------------------------------------------------------------------------------------------------ goldens
def test_float64_decoder_reproduces_golden_g1(golden):
    """G1: the reference's network.ShallowMLP.forward in float32 (unit-scale directions, a coarse-to-fine mask on the features).  The
    render-time decoder on the masked features is the same function but for the 1e-8 in the direction's norm."""
    g = golden("g1_mlp")
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}
    x = torch.from_numpy(g["x"])
    out = R.decoder(O.pack_blob(sd).numpy(), x[:, :32] * torch.from_numpy(g["weight_feature"]), x[:, 32:], F64)
    np.testing.assert_allclose(out["sigma"].numpy(), g["sigma"][:, 0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out["diffuse"].numpy(), g["diffuse"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out["specular"].numpy(), g["tint"] * g["specular"], rtol=1e-5, atol=1e-6)


def test_float64_run_reproduces_golden_g12(golden):
    """G12: a tile exported by the reference's writer and the blob its reader makes of decoder.pth.  The float64 decoder on that blob is
    oracle.mlp_forward on the state dict itself (float64, mask 1, unit directions: the 1e-8 is then 1e-8 of the direction), and on the
    tile as a one-tile scene -- its own box, grid, 64-entry tables and resolutions 8 .. 128 -- the float32 run reproduces the oracle.
    (G6 pins render_batch_rays, the TRAINING path: contracted positions, compositing weights with 1e-6, an epsilon in the direction;
    it does not apply to these ops.)"""
    exp = golden("g12_expected")
    f = np.load(os.path.join(ROOT, "tests", "golden", "g12_tile", "feature.npz"))
    sd = torch.load(os.path.join(ROOT, "tests", "golden", "g12_tile", "decoder.pth"), map_location="cpu")
    g = torch.Generator().manual_seed(12)
    feat = torch.randn(256, 32, generator=g, dtype=F64) * 0.6
    u = torch.nn.functional.normalize(torch.randn(256, 3, generator=g, dtype=F64), dim=1)
    mine = R.decoder(exp["blob"], feat, u, F64)
    ref = O.mlp_forward({k: v.double() for k, v in sd.items()}, torch.cat([feat, u], 1), torch.ones(1, 32, dtype=F64))
    for a, b in ((mine["sigma"], ref["sigma"][:, 0]), (mine["diffuse"], ref["diffuse"]), (mine["specular"], ref["tint"] * ref["specular"])):
        assert float((a - b).abs().max()) < 1e-7
    sc = dict(corners=exp["render_block_corner"][None], sizes=exp["render_block_size"][None], l2d=f["grid_log2dim"][None].astype(np.int32),
              starts=np.zeros(1, np.int64), occ=f["occupied_grid"].reshape(-1), tables=f["features"][None], params=exp["blob"][None],
              res=f["resolution"][None].astype(np.int32))
    rng = np.random.default_rng(12)
    B, S = 127, 16
    centre = sc["corners"][0] + sc["sizes"][0] / 2
    d = rng.normal(size=(B, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.7, 1.3, (B, 1))).astype(np.float32)
    o = (centre + rng.uniform(-0.3, 0.3, (B, 3)) * sc["sizes"][0] - 9.0 * d).astype(np.float32)
    z, dd, bi = RS.trace_samples(sc, o, d, S, passes=1)[0]
    ins = {"sc": sc, "o": o, "d": d, "z": z, "dd": dd, "bi": bi}
    r64, r32 = (R.pts_inference(sc, o, d, z, dd, bi, dt) for dt in (F64, F32))
    assert r64["pin"]["occ"].sum() > 300 and float(r64["alpha"].max()) > 0.01
    _against_oracle("G12 tile", _oracle_pts(ins), r64, r32)
