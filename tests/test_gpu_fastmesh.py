"""The HIP mesh tracer (scanerf_amd.fastmesh.FastMesh, csrc/mesh.hip) against the independent float64 brute force of
tests/fastmesh_reference.py: the structure's arrays, first_hit, first_enter, the composite methods, the "BS" background mode of
HashGrid / the fused training step, the occlusion masks, and launch-to-launch bit identity.

Bounds: |t - t64| <= 1e-4 * max(t64, 1e-3), the project's parity bound, on every ray that is not grazing (a face within
1.001 t_hit + 1e-3 whose barycentric margin is below 1e-4 in float64); grazing rays at most 1 % of a set; first_enter may disagree
(a cell corner grazed: another visited set) on at most 0.5 % of a set."""
import numpy as np
import pytest
import torch

import fastmesh_reference as FR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _fm(V, F, log2dim=6, **kw):
    import scanerf_amd  # noqa
    from scanerf_amd.fastmesh import FastMesh
    return FastMesh.from_arrays(V, F, DEV, log2dim=log2dim, **kw)


@pytest.fixture(scope="module")
def terrain():
    V, F, rays = FR.terrain_fixture()
    return V, F, rays, _fm(V, F)


def _within(t, t64):
    return np.abs(t - t64) <= 1e-4 * np.maximum(t64, 1e-3)


def _check_hits(name, t, t64, grazing, cap=0.01):
    """hit / miss agrees and the bound holds on every ray that is not grazing; -> the largest relative difference."""
    t = np.asarray(t, np.float64)
    plain = ~grazing
    miss = (t == 0) != (t64 == 0)
    rel = np.abs(t - t64) / np.maximum(t64, 1e-3)
    worst = float(rel[plain & ~miss].max()) if (plain & ~miss).any() else 0.0
    print(f"first_hit [{name}]: {len(t)} rays, {int((t64 > 0).sum())} hit, {int(grazing.sum())} grazing ({grazing.mean():.3%}), "
          f"{int((miss & plain).sum())} hit/miss disagreements off grazing, largest relative difference {worst:.3e} "
          f"(all rays: {float(rel.max()):.3e})")
    assert grazing.mean() <= cap
    assert not (miss & plain).any()
    assert _within(t, t64)[plain].all()
    return worst


# ---- 1. structure ---------------------------------------------------------------------------------------------------------------
def _same_structure(fm, g):
    assert np.array_equal(fm.scene_info.cpu().numpy(), g["scene_info"])
    assert np.array_equal(fm.get_sceneinfo().cpu().numpy(), g["scene_bound"])
    assert np.array_equal(fm.bitmask.cpu().numpy().view(np.uint64), g["bitmask"])
    assert np.array_equal(fm.rank.cpu().numpy().view(np.uint32), g["rank"])
    assert np.array_equal(fm.start_num.cpu().numpy(), g["start_num"])
    assert np.array_equal(fm.cell_faces.cpu().numpy(), g["cell_faces"])
    assert np.array_equal(fm.cell_box.cpu().numpy(), g["cell_box"])
    assert fm.num_cells == len(g["cells"])


@pytest.mark.parametrize("log2dim", [6, 4])
def test_structure_equals_the_numpy_build(terrain, log2dim, tmp_path):
    from scanerf_amd import formats
    from scanerf_amd.fastmesh import FastMesh
    V, F, _, fm6 = terrain
    g = FR.build_grid(V, F, log2dim)
    fm = fm6 if log2dim == 6 else _fm(V, F, log2dim)
    _same_structure(fm, g)
    again = _fm(V, F, log2dim)                      # a second build: bit-identical
    for name in ("bitmask", "rank", "start_num", "cell_faces", "cell_box", "scene_info", "tris"):
        assert torch.equal(getattr(fm, name), getattr(again, name)), name
    tri = V[F[g["cell_faces"]]]                     # the pre-gathered triangles: (A, B - A, C - A) per list entry
    want = np.concatenate([tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]], 1)
    assert np.array_equal(fm.tris.cpu().numpy(), want)
    if log2dim == 6:                                # the same mesh through a PLY file
        formats.write_ply(str(tmp_path / "mesh.ply"), V, F)
        _same_structure(FastMesh(str(tmp_path / "mesh.ply")), g)
        from scanerf_amd.fastmesh import fastMesh       # the pybind class's names, outputs written in place
        low = fastMesh()
        low.build(str(tmp_path / "mesh.ply"))
        o, d = (T(x) for x in terrain[2]["inside"])
        depth = torch.zeros(o.shape[0], 1, device=DEV)
        low.fisrtHit(o, d, depth)
        assert torch.equal(depth[:, 0], fm.first_hit(o, d)) and float(depth.max()) > 0
        low.firstEnter(o, d, depth)
        assert torch.equal(depth[:, 0], fm.first_enter(o, d)) and torch.equal(low.getSceneBound(), fm.get_sceneinfo())
    for bad in (3, 8):
        with pytest.raises(ValueError, match="log2dim"):
            _fm(V, F, bad)


# ---- 2. first_hit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["inside", "outside", "axial"])
def test_first_hit_matches_the_brute_force(terrain, name):
    V, F, rays, fm = terrain
    o, d = rays[name]
    t64, grazing = FR.nearest_hit(o, d, V, F)
    t = fm.first_hit(T(o), T(d)).cpu().numpy()
    _check_hits(name, t, t64, grazing)
    # every variant of the kernel computes the same bits: indexed faces, LDS-staged lookup
    indexed = _fm(V, F, pregather=False)
    assert indexed.tris is None and np.array_equal(indexed.first_hit(T(o), T(d)).cpu().numpy(), t)
    for m in (fm, indexed):
        m.lds = True
        try:
            assert np.array_equal(m.first_hit(T(o), T(d)).cpu().numpy(), t)
        finally:
            m.lds = False
    # unnormalised directions: t is in units of |d|
    t3 = fm.first_hit(T(o), T(d * np.float32(4.0))).cpu().numpy()
    _check_hits(name + ", |d| = 4", t3 * 4.0, t64, grazing)


def test_first_hit_log2dim_4_and_7(terrain):
    V, F, rays, _ = terrain
    o, d = rays["inside"]
    t64, grazing = FR.nearest_hit(o, d, V, F)
    for L in (4, 7):
        _check_hits(f"inside, log2dim {L}", _fm(V, F, L).first_hit(T(o), T(d)).cpu().numpy(), t64, grazing)


# ---- 3. first_enter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["inside", "outside", "axial"])
def test_first_enter_matches_the_definition(terrain, name):
    V, F, rays, fm = terrain
    o, d = rays[name]
    e64 = FR.first_enter(o, d, V, F, 6)
    e = fm.first_enter(T(o), T(d)).cpu().numpy().astype(np.float64)
    bad = ~_within(e, e64) | ((e == 0) != (e64 == 0))
    ok = ~bad
    worst = float((np.abs(e - e64) / np.maximum(e64, 1e-3))[ok].max())
    print(f"first_enter [{name}]: {len(e)} rays, {int((e64 > 0).sum())} nonzero, {int(bad.sum())} disagree with float64 "
          f"({bad.mean():.3%}), largest relative difference on the others {worst:.3e}")
    assert bad.mean() <= 0.005
    fm.lds = True
    try:
        assert np.array_equal(fm.first_enter(T(o), T(d)).cpu().numpy().astype(np.float64), e)
    finally:
        fm.lds = False


# ---- 4. the sloping plane --------------------------------------------------------------------------------------------------------
def test_first_hit_returns_the_box_over_the_sloping_plane():
    """Two triangles registered in every cell of the grid, far from their surface, and a box above them: a tracer that returns at
    the first cell with any hit (the reference's rule) reports the plane BEHIND the box for most of these rays."""
    V, F, (o, d), top = FR.sloping_plane_fixture()
    fm = _fm(V, F)
    t64, grazing = FR.nearest_hit(o, d, V, F)
    assert not grazing.any()
    t = fm.first_hit(T(o), T(d)).cpu().numpy()
    _check_hits("sloping plane", t, t64, grazing)
    np.testing.assert_allclose(o[:, 2] + t * d[:, 2], top, atol=1e-3)        # the box's top face, not the plane at z ~ 0
    _, early, _ = FR.walk(o, d, V, F, FR.build_grid(V, F, 6))
    assert (~_within(early, t64)).mean() > 0.5                                # what the early return would have given


# ---- 5. the composite methods ---------------------------------------------------------------------------------------------------
def _depths(fm, o, d, V, F):
    """Brute-force first_hit depths [B,1] float32 on the device, the kernel's own value substituted where the ray is grazing."""
    t64, grazing = FR.nearest_hit(o, d, V, F)
    t = fm.first_hit(T(o), T(d)).cpu().numpy()
    _check_hits("composite", t, t64, grazing)
    return T(np.where(grazing, t, t64).astype(np.float32))[:, None]


def _bounds(o, d, center, size):
    from scanerf_amd.cuda import ray_aabb_intersection
    b = torch.full((o.shape[0], 2), -1.0, device=DEV)
    ray_aabb_intersection(o, d, center, size, b)
    return b


def _clear(a, b):
    """Rows where a > b cannot flip under the parity bound on a."""
    return (a - b).abs() > 2e-4 * torch.maximum(a.abs(), torch.full_like(a, 1e-3))


def test_composite_methods_match_their_formulas(terrain):
    V, F, rays, fm = terrain
    center, size = T(np.array([0.5, -0.5, 0.5], np.float32)), T(np.array([6.0, 5.0, 3.0], np.float32))
    fm.set(center, size)
    o = np.concatenate([rays["inside"][0][:1024], rays["outside"][0][:1024]])
    d = np.concatenate([rays["inside"][1][:1024], rays["outside"][1][:1024]])
    to, td = T(o), T(d)
    near_far = _bounds(to, td, center, size)
    near = near_far[:, :1]
    inside = torch.all(torch.abs(to - center) < size / 2.0, dim=-1, keepdim=True)
    assert 0.05 < float((near_far[:, 1] != -1).float().mean()) < 0.95 and bool(inside.any()) and not bool(inside.all())
    # render_depth / render_mask(trust_mesh=True): first_hit
    depth = _depths(fm, o, d, V, F)
    got = fm.render_depth(to, td)
    assert got.shape == (len(o), 1) and _within(got.cpu().numpy().astype(np.float64), depth.cpu().numpy().astype(np.float64)).all()
    want = ((depth > near) & (near != -1)) | (depth == 0) | inside
    mask = fm.render_mask(to, td, trust_mesh=True)
    sure = _clear(depth, near) | (near == -1) | inside
    assert mask.dtype == torch.bool and mask.shape == (len(o), 1) and torch.equal(mask[sure], want[sure]) and float(sure.float().mean()) > 0.99
    assert 0.05 < float(want.float().mean()) < 0.95
    # render_mask(trust_mesh=False): first_enter
    e64 = FR.first_enter(o, d, V, F, 6)
    e = fm.first_enter(to, td).cpu().numpy().astype(np.float64)
    agree = _within(e, e64) & ((e == 0) == (e64 == 0))
    assert (~agree).mean() <= 0.005
    enter = T(np.where(agree, e64, e).astype(np.float32))[:, None]
    want = ((enter > near) & (near != -1)) | (enter == 0) | inside
    mask = fm.render_mask(to, td)
    sure = _clear(enter, near) | (near == -1) | inside
    assert torch.equal(mask[sure], want[sure]) and float(sure.float().mean()) > 0.99
    # compute_bgdepth_batch: first_hit again from the box exit
    valid = near_far[:, 1] != -1
    start = torch.where(valid[:, None], to + near_far[:, 1:] * td, to)
    behind = _depths(fm, start.cpu().numpy(), d, V, F)
    bg = torch.where(depth == 0, torch.full_like(behind, 1000.0), behind)
    has_bg = (bg[:, 0] > 0) & valid
    bg = torch.where(valid[:, None], bg + near_far[:, 1:], bg)
    o_before = to.clone()
    got_bg, got_has, got_bounds = fm.compute_bgdepth_batch(to, td)
    assert torch.equal(to, o_before)                                           # the caller's rays are left alone
    assert torch.equal(got_bounds, near_far) and torch.equal(got_has, has_bg)
    assert 0.05 < float(has_bg.float().mean()) < 0.95
    assert _within(got_bg.cpu().numpy().astype(np.float64), bg.cpu().numpy().astype(np.float64)).all()
    # background_sampling: the sampling op on those depths
    from scanerf_amd.cuda import background_sampling_cuda
    z_want = torch.full((len(o), 24), -1.0, device=DEV)
    background_sampling_cuda(to, td, got_bounds[:, 1:].contiguous(), got_bg, z_want, 24, 1.5)
    z, v = fm.background_sampling(to, td, 24, 1.5)
    assert torch.equal(z, z_want) and torch.equal(v, has_bg)


def test_compute_bgdepth_over_a_camera_set(terrain):
    from scanerf_amd.cameras import CameraSet
    V, F, _, fm = terrain
    H, W = 32, 48
    cams = [FR.look_at(e, [0.5, -0.5, 0.5], H, W, 40.0) for e in ([14.0, 3.0, 6.0], [-2.0, 1.0, 5.0])]
    c2ws, ks = np.stack([c for c, _ in cams]), np.stack([k for _, k in cams])
    poses = CameraSet(ks, c2ws, DEV)
    center, size = T(np.array([0.5, -0.5, 0.5], np.float32)), T(np.array([6.0, 5.0, 3.0], np.float32))
    fm.set(center, size)
    got = fm.compute_bgdepth(poses, H, W)
    assert got.shape == (2, H, W)
    for i, (c2w, K) in enumerate(cams):
        o, d = FR.camera_rays(c2w, K, H, W)
        to, td = T(o), T(d)
        b = _bounds(to, td, center, size)
        valid = b[:, 1] != -1
        start = torch.where(valid[:, None], to + b[:, 1:] * td, to)
        z = _depths(fm, start.cpu().numpy(), d, V, F)
        want = torch.where(z <= 0, torch.zeros_like(z), torch.where(valid[:, None], z + b[:, 1:], z))[:, 0]
        assert _within(got[i].reshape(-1).cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)).all()
        assert float((want > 0).float().mean()) > 0.2


# ---- 6. BG_MODE "BS" ------------------------------------------------------------------------------------------------------------
def _shell_scene(B, seed):
    """A tile [-4,4]^3 inside a closed shell mesh [-12,12]^3; rays from inside the tile; the target colour is a smooth function
    of the point where the ray meets the shell: a scene the background branch can explain."""
    V, F = FR.shell_fixture()
    fm = _fm(V, F)
    g = torch.Generator(device="cpu").manual_seed(seed)
    o = (torch.rand(B, 3, generator=g) * 7.0 - 3.5).to(DEV)
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1).to(DEV)
    hit = o + fm.first_hit(o, d)[:, None] * d
    tgt = (0.5 + 0.4 * torch.sin(0.3 * hit)).contiguous()
    return fm, o, d, tgt


def test_render_bg_rays_bs_mode_uses_the_tracer():
    import scanerf_amd  # noqa
    from scanerf_amd.hashgrid import HashGrid
    from scanerf_amd.hashgrid.grid import INFERENCE
    from scanerf_amd.tile_model import Decoder
    fm, o, d, _ = _shell_scene(1024, 3)
    o = torch.cat([o[:768], o[768:] + torch.tensor([8.0, 0, 0], device=DEV)]).contiguous()   # a quarter starts outside the tile box
    d = torch.cat([d[:768], d[768:].abs()]).contiguous()                                      # ... and points away from it: no background
    hg = HashGrid(DEV, torch.tensor([-4.0, -4, -4]), torch.tensor([8.0, 8, 8]), log2_hashmap_size=12, sampler_log2dim=3)
    with torch.no_grad():
        hg.HE.features.mul_(50.0)
    dec = Decoder(seed=2).to(DEV)
    fm.set(hg.bbox_center, hg.bbox_size / 2.0)                                       # tile.py:149-150
    S, step = 32, 5000
    assert hg.render_bg_rays(o, d, S, dec, INFERENCE, bg_mode="BS", global_step=step, invalid_underground=False) == (None, False)
    with torch.no_grad():
        out, ok = hg.render_bg_rays(o, d, S, dec, INFERENCE, bg_mode="BS", fmesh=fm, global_step=step, invalid_underground=False)
        assert ok is True and isinstance(out, dict)
        z, valid = fm.background_sampling(o, d, S, float(hg.bbox_size.max()) / 10)
        dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((z.shape[0], 1), 1e-6, device=DEV)], -1)
        assert 0.5 < float(valid.float().mean()) < 0.9 and bool((z[valid] > 0).all())
        ref, _ = hg.render_batch_rays(o[valid], d[valid], z[valid], dists[valid], dec, INFERENCE, hg.contract_bg, infinity=True,
                                      global_step=step)
    assert torch.equal(out["valid"], valid)
    rgb, depth = torch.zeros_like(o), torch.zeros_like(o[:, :1])
    rgb[valid], depth[valid] = ref["rgb"], ref["depth"]
    assert torch.equal(out["rgb"], rgb) and torch.equal(out["depth"], depth)
    assert float(out["rgb"][valid].std()) > 0 and float(out["depth"][valid].min()) > 0


def _run_steps(steps, **kw):
    from scanerf_amd.tile_model import TileModel, train_step_fgbg
    fm, o, d, tgt = _shell_scene(4096, 5)
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=14, seed=4)
    fm.set(m._center_dev, m._half_dev)
    opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
    if kw.pop("with_mesh", False):
        kw["fmesh"] = fm
    losses = [float(train_step_fgbg(m, opt, o, d, tgt, 32, 32, 6000 + i, **kw)) for i in range(steps)]
    return losses, m.features.detach().clone(), m.decoder.params.detach().clone()


def test_train_step_fgbg_bs_mode_learns_and_repeats():
    a = _run_steps(20, bg_mode="BS", with_mesh=True)
    b = _run_steps(20, bg_mode="BS", with_mesh=True)
    print("train_step_fgbg(bg_mode='BS') losses:", " ".join(f"{l:.5f}" for l in a[0]))
    assert all(np.isfinite(a[0])) and a[0][-1] < a[0][0]
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    iz = _run_steps(3, bg_mode="IZ")
    assert iz[0][0] != a[0][0]                       # the other sampler: another render
    with pytest.raises(ValueError, match="needs fmesh"):
        _run_steps(1, bg_mode="BS")


def test_defaults_are_bit_identical_to_a_call_without_the_new_arguments():
    from scanerf_amd.tile_model import TileModel, fgbg_gradients
    plain = _run_steps(4)
    explicit = _run_steps(4, bg_mode="IZ", fmesh=None, occlusion_mask=None)
    unused = _run_steps(4, bg_mode="IZ", with_mesh=True)      # a tracer that the "IZ" mode never calls
    for other in (explicit, unused):
        assert plain[0] == other[0] and torch.equal(plain[1], other[1]) and torch.equal(plain[2], other[2])
    # occlusion_mask: an all-true mask changes nothing; a mask is the same as dropping the masked rays from the loss' valid sets
    fm, o, d, tgt = _shell_scene(2048, 6)
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=14, seed=4)
    fm.set(m._center_dev, m._half_dev)
    base = fgbg_gradients(m, o, d, tgt, 32, 32, 6000)
    ones = torch.ones(2048, 1, dtype=torch.bool, device=DEV)
    same = fgbg_gradients(m, o, d, tgt, 32, 32, 6000, occlusion_mask=ones)
    assert all(torch.equal(x, y) for x, y in zip(base, same))
    half = ones.clone()
    half[::2] = False
    masked = fgbg_gradients(m, o, d, tgt, 32, 32, 6000, occlusion_mask=half, bg_mode="BS", fmesh=fm)
    full = m.render_rays_fused(o, d, 32, 32, 6000, occlusion_mask=half, bg_mode="BS", fmesh=fm)
    assert not bool(full["fore_valid"][::2].any()) and not bool(full["bg_valid"][::2].any()) and bool(full["bg_valid"][1::2].all())
    assert bool((full["pred_color"][::2] == 0).all()) and float(masked[0]) != float(base[0])


# ---- 7. occlusion masks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trust_mesh", [False, True])
def test_mesh_occlusion_masks(terrain, trust_mesh):
    from scanerf_amd import occlusion
    V, F, _, fm = terrain
    H, W = 64, 96
    center, size = np.array([0.5, -0.5, 0.5], np.float32), np.array([6.0, 5.0, 3.0], np.float32)
    fm.set(T(center), T(size))
    cams = [FR.look_at(e, center, H, W, 70.0) for e in ([15.0, 3.0, 4.0], [-4.0, -16.0, 2.5], [1.0, 0.0, 12.0])]
    rays = [FR.camera_rays(c, k, H, W) for c, k in cams]
    masks = occlusion.mesh_occlusion_masks(fm, lambda i: (T(rays[i][0]), T(rays[i][1])), H, W, 3, trust_mesh=trust_mesh)
    assert masks.shape == (3, H, W, 1) and masks.dtype == torch.bool
    for i, (o, d) in enumerate(rays):
        if trust_mesh:
            depth, skip = FR.nearest_hit(o, d, V, F)
            cap = 0.01
        else:
            depth, skip = FR.first_enter(o, d, V, F, 6), np.zeros(len(o), bool)
            cap = 0.005
        b = FR.box_bounds(o, d, center, size)
        near = b[:, 0]
        inside = np.all(np.abs(o.astype(np.float64) - center) < size / 2.0, -1)
        want = ((depth > near) & (near != -1)) | (depth == 0) | inside
        got = masks[i].reshape(-1).cpu().numpy()
        differ = (got != want) & ~skip
        print(f"mesh_occlusion_masks(trust_mesh={trust_mesh}) camera {i}: {want.mean():.1%} visible, {int(skip.sum())} grazing pixels, "
              f"{int(differ.sum())} of {len(o)} other pixels differ")
        assert skip.mean() <= 0.01
        if trust_mesh:   # off grazing pixels only a depth within the parity bound of the box entry can fall the other way
            close = np.abs(depth - near) <= 2e-4 * np.maximum(depth, 1e-3)
            assert not (differ & ~close).any() and close.mean() <= 0.001
        else:
            assert differ.mean() <= cap
        assert 0.02 < want.mean() < 0.98 or i == 2


# ---- 8. launch-to-launch ---------------------------------------------------------------------------------------------------------
def test_two_launches_give_identical_bits_on_a_full_hd_frame(terrain):
    _, _, _, fm = terrain
    H, W = 1080, 1920
    c2w, K = FR.look_at([13.0, -9.0, 5.0], [0.0, 0.0, 0.0], H, W, 1400.0)
    o, d = FR.camera_rays(c2w, K, H, W)
    to, td = T(o), T(d)
    for fn in (fm.first_hit, fm.first_enter):
        a = fn(to, td).clone()
        b = fn(to, td)
        torch.cuda.synchronize()
        assert a.shape == (H * W,) and torch.equal(a, b)
        assert 0.2 < float((a > 0).float().mean()) <= 1.0
    fm.set(T(np.array([0.0, 0.0, 0.5], np.float32)), T(np.array([6.0, 6.0, 3.0], np.float32)))
    assert torch.equal(fm.render_mask(to, td), fm.render_mask(to, td))
