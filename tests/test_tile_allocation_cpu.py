"""Tile allocation without a GPU (scanerf_amd.allocation): the candidate grid, the tile / view selection rules on hand-built
matrices, the two files through formats' readers, ignore.log, the C entry point's validation before any launch, the absence of
a CPU path -- and the conditions tests/test_gpu_tile_allocation.py needs of its fixture, checked on the float64 yardstick alone
(tests/tile_allocation_reference.py) before anything runs on a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tile_allocation_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alloc():
    import scanerf_amd  # noqa
    from scanerf_amd import allocation
    return allocation


# ---- tile_grid --------------------------------------------------------------------------------------------------------------
def test_tile_grid_against_hand_computed_corners():
    A = _alloc()
    # extents (10, 5, 4), tiles (4, 4, 4), overlap 0.25 -> step 3; ceil(10 / 4) = 3, ceil(5 / 4) = 2, ceil(4 / 4) = 1
    corners, side = A.tile_grid([0, 0, 0, 10, 5, 4], [4, 4, 4], 0.25, [0, 0, 0], [100, 100, 100])
    assert side == [3, 2, 1] and corners.dtype == torch.float32
    want = [[0, 0, 0], [0, 3, 0], [3, 0, 0], [3, 3, 0], [6, 0, 0], [6, 3, 0]]           # x slowest, z fastest
    assert torch.equal(corners, torch.tensor(want, dtype=torch.float32))
    # a non-zero offset moves the grid's origin and shrinks the covered extent: (9, 5.5, 3) -> 3, 2, 1; the x axis clamped to 2
    corners, side = A.tile_grid([-1, -1, -1, 9, 4, 3], [4, 4, 4], 0.5, [1, -0.5, 1], [2, 100, 100])
    assert side == [2, 2, 1]
    assert torch.equal(corners, torch.tensor([[0, -1.5, 0], [0, 0.5, 0], [2, -1.5, 0], [2, 0.5, 0]], dtype=torch.float32))
    # z fastest
    corners, side = A.tile_grid([0, 0, 0, 2, 2, 4], [2, 2, 2], 0.0, [0, 0, 0], [100, 100, 100])
    assert side == [1, 1, 2] and torch.equal(corners, torch.tensor([[0, 0, 0], [0, 0, 2]], dtype=torch.float32))
    # an extent that is an exact multiple takes no extra tile; a clamp of 1 on every axis leaves one tile
    assert A.tile_grid([0, 0, 0, 8, 8, 8], [4, 4, 4], 0.0, [0, 0, 0], [100, 100, 100])[1] == [2, 2, 2]
    assert A.tile_grid([0, 0, 0, 8, 8, 8], [4, 4, 4], 0.0, [0, 0, 0], [1, 1, 1])[0].shape == (1, 3)


# ---- select_tiles -----------------------------------------------------------------------------------------------------------
# four tiles of side 10 in a row along x (no overlap); six cameras: 0, 1 in tile 0, 2 in tile 1, 3, 4, 5 in tile 3; none in tile 2
_CORNERS = [[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0]]
_CAMS = [[1, 5, 5], [9, 5, 5], [15, 5, 5], [31, 5, 5], [35, 5, 5], [39, 5, 5]]
_SIZE = [10, 10, 10]


def _related(rows):
    return torch.tensor(rows, dtype=torch.float32)


def _select(related, expect_num, min_num_image, scene_type="indoor", **kw):
    return _alloc().select_tiles(related, torch.tensor(_CAMS, dtype=torch.float32), torch.tensor(_CORNERS, dtype=torch.float32),
                                 _SIZE, expect_num, min_num_image, scene_type, **kw)


def test_select_tiles_fewer_than_expected_adds_the_nearest_set_aside_tile():
    rel = _related([[0.9, 0.8, 0.7, 0.0, 0.0, 0.0], [0.5, 0.6, 0.9, 0.3, 0.0, 0.0], [0.2, 0.3, 0.8, 0.7, 0.6, 0.0],
                    [0.0, 0.0, 0.2, 0.9, 0.8, 0.7]])
    r = _select(rel, 3, 1)                    # tiles 0, 1, 3 have cameras inside: exactly three, tile 2 stays out
    assert r["tiles"] == [0, 1, 3]
    r = _select(rel, 4, 1)                    # one short: tile 2, the only tile set aside, comes back
    assert r["tiles"] == [0, 1, 2, 3] and r["views"][2] == [2, 3, 4, 1, 0]
    assert torch.equal(r["corners"], torch.tensor(_CORNERS, dtype=torch.float32))
    # the inside test is half-open: a camera ON a tile's far face belongs to the next tile, one on the near face to this one
    A = _alloc()
    r = A.select_tiles(_related([[0.9, 0.9], [0.9, 0.9]]), torch.tensor([[10.0, 5, 5], [10.0, 0, 0]]),
                       torch.tensor([[0.0, 0, 0], [10.0, 0, 0]]), _SIZE, 1, 0, "indoor")
    assert r["tiles"] == [1]


def test_select_tiles_more_than_expected_keeps_the_nearest_and_renumbers():
    rel = _related([[0.9, 0.8, 0.7, 0.0, 0.0, 0.0], [0.5, 0.6, 0.9, 0.3, 0.0, 0.0], [0.2, 0.3, 0.8, 0.7, 0.6, 0.0],
                    [0.0, 0.0, 0.2, 0.9, 0.8, 0.7]])
    # mean camera-to-centre distance: tile 0 (centre x = 5): (4 + 4 + 10 + 26 + 30 + 34) / 6 = 18; tile 1 (15): (14 + 6 + 0 + 16 +
    # 20 + 24) / 6 = 13.33; tile 3 (35): (34 + 26 + 20 + 4 + 0 + 4) / 6 = 14.67 -> the nearest two are 1 and 3
    r = _select(rel, 2, 1)
    assert r["tiles"] == [1, 3]
    assert r["views"] == [[2, 1, 0, 3], [3, 4, 5, 2]]
    assert torch.equal(r["corners"], torch.tensor([[10, 0, 0], [30, 0, 0]], dtype=torch.float32))
    r = _select(rel, 1, 1)
    assert r["tiles"] == [1]
    # a kept tile with too few views drops out and the rest are renumbered by position: tile 1 has 4 views, tile 3 has 4, tile 0 has 3
    r = _select(rel, 3, 3)
    assert r["tiles"] == [1, 3] and len(r["views"]) == 2


def test_select_tiles_indoor_and_outdoor_scores():
    # camera 2 is inside tile 1 and sees little of it (0.05); camera 3 is outside and sees exactly the threshold
    rel = _related([[0.9, 0.8, 0.0, 0.0, 0.0, 0.0], [0.5, 0.6, 0.05, 0.1, 0.0, 0.0], [0, 0, 0, 0, 0, 0], [0.0, 0.0, 0.0, 0.9, 0.8, 0.7]])
    indoor = _select(rel, 3, 0, "indoor")
    assert indoor["tiles"] == [0, 1, 3] and indoor["views"][1] == [1, 0]            # 0.05 and 0.1 are not > 0.1
    outdoor = _select(rel, 3, 0, "outdoor")
    assert outdoor["views"][1] == [1, 0, 2]                                         # 0.1 * inside + 0.05 = 0.15 > 0.1; 0.1 is not
    assert outdoor["views"][0] == [0, 1] and outdoor["views"][2] == [3, 4, 5]       # 1.0, 0.9 | 1.0, 0.9, 0.8: the order stays
    # an inside camera that sees nothing of its tile scores exactly the threshold: not a view, indoor or outdoor
    rel0 = _related([[0.0, 0.8, 0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]])
    assert _select(rel0, 3, 0, "outdoor")["views"] == [[1]] and _select(rel0, 3, 0, "outdoor")["tiles"] == [0]
    # another threshold moves the cut and the outdoor bonus alike
    assert _select(rel, 3, 0, "indoor", thresh=0.04)["views"][1] == [1, 0, 3, 2]


def test_select_tiles_ignored_cameras_and_strict_bounds():
    rel = _related([[0.9, 0.8, 0.7, 0.0, 0.0, 0.0], [0.5, 0.6, 0.9, 0.3, 0.0, 0.0], [0.2, 0.3, 0.8, 0.7, 0.6, 0.0],
                    [0.0, 0.0, 0.2, 0.9, 0.8, 0.7]])
    r = _select(rel, 3, 1, ignore=[2, 3])
    assert r["tiles"] == [0, 1, 3] and r["views"] == [[0, 1], [1, 0], [4, 5]]
    r = _select(rel, 3, 1, "outdoor", ignore=[2, 3])          # the ignored columns are zeroed AFTER the inside bonus
    assert r["views"] == [[0, 1], [1, 0], [4, 5]]
    assert _select(rel, 3, 1, ignore=np.arange(2, 4))["views"] == r["views"]
    # strictly more than min_num_image views: tile 0 has 3, tiles 1 and 3 have 4
    assert _select(rel, 3, 3)["tiles"] == [1, 3]
    assert _select(rel, 3, 2)["tiles"] == [0, 1, 3]
    assert _select(rel, 3, 4)["tiles"] == [] and _select(rel, 3, 4)["corners"].shape == (0, 3)
    # the caller's matrix is left alone
    before = rel.clone()
    _select(rel, 3, 1, "outdoor", ignore=[0])
    assert torch.equal(rel, before)


def test_select_tiles_breaks_ties_by_the_lower_index():
    rel = _related([[0.5, 0.5, 0.5, 0.7, 0.5, 0.2], [0.3, 0.3, 0.3, 0.3, 0.3, 0.3], [0, 0, 0, 0, 0, 0], [0.2, 0.2, 0.2, 0.2, 0.2, 0.2]])
    r = _select(rel, 3, 0)
    assert r["views"] == [[3, 0, 1, 2, 4, 5], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]]
    # equal distances: two tiles mirror each other about the one camera; the lower tile id is the nearer
    A = _alloc()
    r = A.select_tiles(_related([[0.9], [0.9], [0.9]]), torch.tensor([[15.0, 5, 5]]), torch.tensor([[0.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0]]),
                       _SIZE, 2, 0, "indoor")
    assert r["tiles"] == [0, 1]                  # tile 1 holds the camera; of the set-aside tiles 0 and 2 (both 10 away), 0 comes first


# ---- files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_type,finest", [("outdoor", 8192), ("indoor", 4096)])
def test_written_files_read_back(tmp_path, scene_type, finest):
    A = _alloc()
    from scanerf_amd import formats
    result = {"tiles": [1, 3], "views": [[2, 1, 0, 3], [3, 4, 5]], "corners": torch.tensor([[10.0, -0.25, 0.125], [30.0, 0.0, 7.0]]),
              "tile_size": torch.tensor([10.0, 12.5, 8.0]), "scene_type": scene_type}
    tile_dir = tmp_path / "data" / "tiles"                    # created on the way
    A.write_allocation(str(tile_dir), result)
    tiles = formats.read_tile_info(str(tile_dir / "tile_info.txt"))
    assert [t["idx"] for t in tiles] == [0, 1]
    assert tiles[0]["corner"] == [10.0, -0.25, 0.12] or tiles[0]["corner"] == [10.0, -0.25, 0.13]      # %.2f
    assert tiles[1]["corner"] == [30.0, 0.0, 7.0] and tiles[0]["size"] == [10.0, 12.5, 8.0]
    assert all(t["resolution"] == [32, finest] and t["init_outside"] is False for t in tiles)
    assert formats.read_training_views(str(tile_dir / "training_views.txt")) == {0: [2, 1, 0, 3], 1: [3, 4, 5]}
    assert open(tile_dir / "tile_info.txt").readline() == formats.TILE_INFO_HEADER


def test_read_ignore_log(tmp_path):
    A = _alloc()
    assert A.read_ignore_log(str(tmp_path / "ignore.log")) == []            # no file: nothing ignored
    (tmp_path / "ignore.log").write_text("3\n10 14\n7\n1 2 3\n\n20 20\n")
    assert A.read_ignore_log(str(tmp_path / "ignore.log")) == [3, 10, 11, 12, 13, 7]   # `a b` is the half-open range


def test_coverage_ratio_keeps_the_full_resolution_denominator():
    A = _alloc()
    counts = torch.tensor([[825, 0], [400, 1]], dtype=torch.int32)
    got = A.coverage_ratio(counts, 102, 134, 4)
    assert got.dtype == torch.float32
    # 25 * 33 = 825 pixels of the truncated frame against 102 * 134 / 16 = 854.25: a fully covered view scores 0.9658, not 1
    assert abs(float(got[0, 0]) - 825 * 16 / (102 * 134)) < 1e-6 and float(got[0, 0]) < 0.97
    assert np.array_equal(got.numpy(), TR.ratio(counts.numpy(), 102, 134, 4))


# ---- the entry point --------------------------------------------------------------------------------------------------------
def test_view_coverage_validates_before_any_launch():
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    lib = _capi.lib()
    buf = (np.zeros(64, np.float32)).ctypes.data            # never read: every call below is refused or a no-op before a launch
    call = lambda C=2, H=100, W=100, scale=4, K=3, log2dim=6, p=buf, tris=buf, counts=buf: lib.scanerf_view_coverage(
        p, p, C, H, W, scale, p, p, K, p, p, tris, p, p, p, p, p, log2dim, counts, None)
    assert call(C=0) == 0 and call(K=0) == 0                 # nothing to count
    assert call(C=0, p=None, tris=None, counts=None) == 0
    assert call(scale=0) != 0 and b"scale=0" in lib.scanerf_last_error()
    assert call(scale=-4) != 0 and b"scale" in lib.scanerf_last_error()
    assert call(H=3) != 0 and b"no pixel" in lib.scanerf_last_error()          # 3 / 4 == 0 rows
    assert call(W=3) != 0 and b"no pixel" in lib.scanerf_last_error()
    for bad in (3, 8):
        assert call(log2dim=bad) != 0 and b"log2dim" in lib.scanerf_last_error()
    assert call(p=None) != 0 and b"null" in lib.scanerf_last_error()
    assert call(counts=None) != 0 and b"null" in lib.scanerf_last_error()
    assert call(C=-1) != 0 and call(K=-1) != 0 and call(C=70000) != 0
    # without pre-gathered triangles the indexed mesh must be there
    assert lib.scanerf_view_coverage(buf, buf, 2, 100, 100, 4, buf, buf, 3, None, None, None, buf, buf, buf, buf, buf, 6, buf, None) != 0
    assert b"null" in lib.scanerf_last_error()
    assert lib.scanerf_view_coverage_boxes_per_pass() >= 64


def test_view_coverage_has_no_cpu_path():
    A = _alloc()
    ks, c2ws = (torch.from_numpy(a) for a in TR.cameras(n=2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.view_coverage(None, ks, c2ws, TR.H, TR.W, torch.zeros(1, 3), torch.ones(1, 3))


def test_build_tiles_command_line_parses_the_allocation_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_tiles.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--tile-size", "--overlap-ratio", "--offset", "--expect-num", "--min-num-image", "--max-dim-tile", "--scene-type"):
        assert flag in out.stdout, flag


# ---- the fixture's own conditions -------------------------------------------------------------------------------------------
def test_the_fixture_is_fit_for_an_exact_comparison():
    """What tests/test_gpu_tile_allocation.py needs of its fixture, on the yardstick alone: few ambiguous pixels per (tile,
    camera), every bracket wholly on one side of the view threshold, and -- since the view lists are ordered by score -- no two
    views of a tile whose brackets overlap.  The end-to-end comparison is then exact and not a matter of luck."""
    f = TR.fixture(4)
    assert list(f["side"]) == [3, 3, 1] and f["pixels"] == 825 and f["pixels"] % 64 and f["pixels"] % 256
    lo, hi = f["lo"], f["hi"]
    share = (hi - lo) / f["pixels"]
    rlo, rhi = TR.ratio(lo, f["H"], f["W"], 4), TR.ratio(hi, f["H"], f["W"], 4)
    gap = float(np.minimum(np.abs(rlo - 0.1), np.abs(rhi - 0.1)).min())
    print(f"fixture: {int((hi - lo).sum())} ambiguous pixels, largest share {share.max():.3%}, smallest distance from the threshold "
          f"{gap:.4f}, views above it per tile {(rlo > 0.1).sum(1).tolist()}")
    assert share.max() <= 0.01
    assert ((rlo > 0.1) == (rhi > 0.1)).all() and gap > 0
    inside_bonus = np.float32(0.1)                           # outdoor: inside cameras score 0.1 + related; > 0.1 iff related > 0
    assert ((lo > 0) == (hi > 0)).all() and inside_bonus > 0
    for k in range(lo.shape[0]):
        order = np.argsort(-rlo[k], kind="stable")
        for a, b in zip(order[:-1], order[1:]):
            if rhi[k][a] > 0.1 or rhi[k][b] > 0.1:
                assert rhi[k][b] < rlo[k][a], (k, a, b)
    # the shape the end-to-end test leans on: only the central tile holds no camera, and 7 of the 9 tiles have more than 5 views
    cams = f["c2ws"][:, :, 3]
    loc = (cams[None] - f["corners"][:, None]) / f["tile_size"]
    inside = ((loc >= 0) & (loc < 1)).all(-1)
    assert np.flatnonzero(~inside.any(1)).tolist() == [4]
    assert (rlo > 0.1).sum(1).tolist() == [7, 8, 5, 8, 8, 8, 6, 7, 4]
    # the plain path's frame: the same rays (intrinsics / 4 are exact), the same bracket
    f1 = TR.fixture(1)
    assert (f1["H"], f1["W"]) == (25, 33) and np.array_equal(f1["ks"][:, :2] * 4, f["ks"][:, :2]) and np.array_equal(f1["lo"], lo)


def test_the_many_boxes_fixture_is_fit():
    m = TR.many_boxes_fixture()
    assert list(m["side"]) == [17, 17, 1] and len(m["corners"]) == 289
    share = (m["hi"] - m["lo"]) / m["pixels"]
    print(f"289 boxes: {int((m['hi'] - m['lo']).sum())} ambiguous pixels, largest share {share.max():.3%}, "
          f"{int((m['lo'] > 0).sum())} of {m['lo'].size} (box, camera) pairs covered")
    assert share.max() <= 0.01
    assert (m["lo"] > 0).sum() > 100 and (m["hi"] == 0).sum() > 100      # covered pairs and empty pairs in both passes
    assert (m["lo"][256:] > 0).any() and (m["lo"][:256] > 0).any()
