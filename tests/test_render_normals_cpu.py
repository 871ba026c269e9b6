"""The yardstick of the multi-tile normal maps (tests/render_normals_reference.py) checked on its own, without a GPU: its slot,
occupancy and weight restatement against the oracle's pts_inference, its accumulation against the oracle's accumulate_color, and
the conditions the scenes must meet for the GPU tests (tests/test_gpu_render_normals.py) to mean something."""
import numpy as np
import pytest
import torch

import render_normals_reference as R
from oracle import oracle as O

f32 = np.float32


def _oracle_alpha(ins):
    sc = ins["sc"]
    return O.pts_inference(ins["o"], ins["d"], ins["z"], ins["dd"], ins["bi"], sc["tables"], sc["params"], sc["res"], sc["occ"],
                           sc["starts"], sc["l2d"], sc["corners"], sc["sizes"])[2].reshape(-1)


@pytest.mark.parametrize("name,S", R.CPU_CASES)
def test_blended_alpha_is_the_oracles(name, S):
    """sum_b w_b pa_b occ_b / W of the helper (float64 and float32 behind the pinned slots) against O.pts_inference's alpha, 1e-6
    absolute on a quantity in [0,1] (measured: 2.2e-7 at worst): slots, occupancy cells, weights and densities are the oracle's."""
    ins, r64, r32 = R.sample_reference(name, S)
    ref = _oracle_alpha(ins)
    e64 = float(np.abs(r64["alpha"].numpy() - ref).max())
    e32 = float(np.abs(r32["alpha"].numpy() - ref).max())
    print(f"{name} S={S}: |alpha - oracle| max: float64 {e64:.2e}, float32 {e32:.2e}; oracle alpha max {ref.max():.3f}")
    assert ref.max() > 0.3 and (ref > 0).mean() > 0.1
    assert e64 <= 1e-6 and e32 <= 1e-6


def test_slot_counts_of_the_scenes():
    """samples with no / 1 / 2 / 3 / 4 listed tiles: grids never list three, STACK3 always three, STACK6 truncates at four"""
    g9, g65 = R.sample_reference("G9", 17)[0], R.sample_reference("G65", 16)[0]
    assert R.slot_counts(g9["bi"]).tolist() == [731, 2433, 3267, 0, 2222]
    assert R.slot_counts(g65["bi"]).tolist() == [544, 3883, 2715, 0, 1002]
    s3, s6 = R.sample_reference("STACK3", 16)[0], R.sample_reference("STACK6", 33)[0]
    c3, c6 = R.slot_counts(s3["bi"]), R.slot_counts(s6["bi"])
    assert c3[3] > 1000 and c3[1] == c3[2] == c3[4] == 0 and c3[0] == (s3["z"] == -1).sum()
    assert c6[4] > 1000 and c6[1] == c6[2] == c6[3] == 0 and c6[0] == (s6["z"] == -1).sum()
    assert int(s6["bi"].max()) == 3, "six coincident tiles: the list holds the first four"
    assert int(g65["bi"].max()) == 64


@pytest.mark.parametrize("name,S", R.CPU_CASES)
def test_conditions_the_gpu_tests_rely_on(name, S):
    """Every scene lists tiles in unoccupied cells (their weight counts, their normal does not); no occupied slot's normal is decided by
    the 1e-8 of its normalisation (|g| between 6.9 and 1.7e3 over the four scenes); the float32 yardstick's own error of the blended
    normal is a float32 rounding error (<= 2.5e-6 at worst, median <= 4.3e-8), so K times it is a tight bound."""
    ins, r64, r32 = R.sample_reference(name, S)
    pin = r64["pin"]
    assert (pin["listed"] & ~pin["occ"]).sum() > 100 and pin["occ"].sum() > 1000
    gn = r64["g"].norm(dim=-1).numpy()[pin["occ"]]
    err = (r32["normal"].double() - r64["normal"]).norm(dim=1).numpy()
    print(f"{name} S={S}: |g| in [{gn.min():.3g}, {gn.max():.3g}]; yardstick error median {np.median(err):.2e} max {err.max():.2e}; "
          f"|normal| max {float(r64['normal'].norm(dim=1).max()):.3f}")
    assert 6.8 <= gn.min() and gn.max() <= 1.75e3
    assert err.max() <= 2.5e-6 and np.median(err) <= 4.4e-8
    assert float(r64["normal"].norm(dim=1).max()) > 0.2
    # samples without a listed tile: exactly zero
    none = ~pin["listed"][:, 0]
    assert none.sum() > 0 and not r64["normal"][torch.from_numpy(none)].any() and not r32["normal"][torch.from_numpy(none)].any()


def test_single_slot_samples_give_that_tiles_opacity_times_normal():
    ins, r64, _ = R.sample_reference("G9", 17)
    pin = r64["pin"]
    one = torch.from_numpy((pin["listed"].sum(1) == 1) & pin["occ"][:, 0] & (pin["w"][:, 0] > 0))
    assert int(one.sum()) > 500
    want = r64["pa"][one, 0, None] * r64["n"][one, 0]
    assert torch.allclose(r64["normal"][one], want, rtol=1e-13, atol=0)
    assert torch.allclose(r64["n"][one, 0].norm(dim=1), torch.ones(int(one.sum()), dtype=R.F64), atol=1e-8)


def test_zero_table_tile_gives_no_normal_but_its_opacity():
    """G9Z: tile 4's table is zero, so its features are constant: g = 0, n = 0 exactly; its density is the decoder's at zero features,
    so its pa > 0 still enters the blended alpha."""
    ins, r64, r32 = R.sample_reference("G9Z", 17)
    pin = r64["pin"]
    z_slots = torch.from_numpy(pin["occ"] & (pin["b"] == R.ZERO_TILE))
    assert int(z_slots.sum()) > 100
    for r in (r64, r32):
        assert not r["g"][z_slots].any() and not r["n"][z_slots].any()
        assert float(r["pa"][z_slots].min()) > 0
    only = torch.from_numpy((pin["listed"].sum(1) == 1) & pin["occ"][:, 0] & (pin["b"][:, 0] == R.ZERO_TILE))
    assert int(only.sum()) > 10 and not r64["normal"][only].any() and float(r64["alpha"][only].min()) > 0
    assert np.abs(r64["alpha"].numpy() - _oracle_alpha(ins)).max() <= 1e-6
    base = R.sample_reference("G9", 17)[1]
    other = ~torch.from_numpy((pin["occ"] & (pin["b"] == R.ZERO_TILE)).any(1))
    assert torch.equal(base["normal"][other], r64["normal"][other])


def test_a_sample_of_weight_zero_is_not_divided():
    """A point on a vertical edge of tile 0's box (dis.x == dis.z == 0): listed, W == 0.  The sum is left undivided, finite."""
    sc, _ = R.scene("G9")
    o, d = f32([[0.0, -1.5, 0.0]]), f32([[0.0, 1.0, 0.0]])
    z = f32([[0.25, 0.5, 1.0, 1.5]])
    dd = np.full_like(z, 0.25)
    bi = np.full((1, 4, 4), -1, np.int16)
    bi[:, :, 0] = 0
    for dtype in (R.F64, R.F32):
        r = R.blend(sc, o, d, z, dd, bi, dtype)
        assert r["pin"]["listed"][:, 0].all() and not r["W"].any()
        assert torch.isfinite(r["normal"]).all() and not r["normal"].any() and not r["alpha"].any()
    assert not O.pts_inference(o, d, z, dd, bi, sc["tables"], sc["params"], sc["res"], sc["occ"], sc["starts"], sc["l2d"], sc["corners"],
                               sc["sizes"])[2].any()


def test_accumulation_is_the_oracles_accumulate_color_bit_for_bit():
    """accumulate_normal's float32 restatement against O.accumulate_color with pts_normal passed as the diffuse array: rays below
    1e-5 untouched, a non-zero start added into, the transparency the oracle's own afterwards."""
    ins, r64, r32 = R.sample_reference("G9", 33)
    B, S = ins["z"].shape
    pn = r32["normal"].numpy().reshape(B, S, 3)
    pa = _oracle_alpha(ins).reshape(B, S, 1)
    rng = np.random.default_rng(5)
    T0 = rng.uniform(0.2, 1.0, (B, 1)).astype(f32)
    T0[::7] = f32(5e-6)
    T0[3::7] = f32(1e-5)
    start = rng.normal(size=(B, 3)).astype(f32)
    mine = R.accumulate_normal(pn, pa, T0, start.copy())
    T, dif, spec, depth = T0.copy(), start.copy(), np.zeros((B, 3), f32), np.zeros((B, 1), f32)
    O.accumulate_color(pn, np.zeros_like(pn), pa, T, ins["z"], dif, spec, depth)
    assert np.array_equal(mine, dif)
    assert np.array_equal(mine[::7], start[::7]) and not np.array_equal(mine[3::7], start[3::7])
    assert (T[1::7] < T0[1::7]).any()
    # float64: the same rule, and the float32 result is a float32 rounding away from it
    m64 = R.accumulate_normal(r64["normal"].numpy().reshape(B, S, 3), pa, T0, start.astype(np.float64), np.float64)
    assert np.abs(m64 - mine).max() < 1e-5
    # rays marked unsampled are not read
    pn_nan, un = pn.copy(), np.arange(B) % 3 == 0
    pn_nan[un] = np.nan
    skipped = R.accumulate_normal(pn_nan, pa, T0, start.copy(), unsampled=un)
    assert np.isfinite(skipped).all() and np.array_equal(skipped[~un], mine[~un]) and np.array_equal(skipped[un], start[un])


def test_prototypes_of_the_new_exports():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    from scanerf_amd import hashgrid as H
    lib = _capi.lib()
    for name in ("scanerf_pts_normals", "scanerf_accumulate_normal"):
        assert name in _capi.SYMBOLS and hasattr(lib, name)
    assert "scanerf_pts_normals_counted" in _capi.OPTIONAL_SYMBOLS
    assert callable(H.pts_normals) and callable(H.accumulate_normal)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        H.accumulate_normal(torch.zeros(2, 4, 3), torch.zeros(2, 4, 1), torch.ones(2, 1), torch.zeros(2, 4), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        H.accumulate_normal(torch.zeros(1, 4, 32, 3), torch.zeros(1, 4, 32, 1), torch.ones(33, 1), torch.zeros(1, 4, 32), torch.zeros(33, 3),
                            sample_major=2)
    with pytest.raises(RuntimeError, match="shape"):
        H.accumulate_normal(torch.zeros(2, 4, 3), torch.zeros(2, 5, 1), torch.ones(2, 1), torch.zeros(2, 4), torch.zeros(2, 3))
