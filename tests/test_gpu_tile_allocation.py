"""Tile allocation on the GPU: the fused view-coverage kernel (scanerf_amd.allocation.view_coverage, csrc/coverage.hip) and the
path from a mesh and cameras to tiles/tile_info.txt and tiles/training_views.txt, against the float64 yardstick of
tests/tile_allocation_reference.py.

The counts are integers, so the bound is a bracket, not a tolerance: per (tile, camera) lo <= count <= hi, where lo counts the
pixels the yardstick covers unambiguously and hi adds the ambiguous ones (|near - depth| within the project's parity bound 1e-4
max(depth, 1e-3), or a grazing ray that meets the box).  tests/test_tile_allocation_cpu.py holds the fixture to at most 1 % of
ambiguous pixels per pair (measured: 11 pixels in all, 0.24 % at most; 1 pixel among the 289 boxes) and to brackets that lie wholly
on one side of the view threshold and apart from each other, so the end-to-end comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

import tile_allocation_reference as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def fmesh():
    import scanerf_amd  # noqa
    from scanerf_amd.fastmesh import FastMesh
    V, F = TR.mesh()
    return FastMesh.from_arrays(V, F, DEV)


def _counts(fm, f, centers=None, sizes=None, ks=None, c2ws=None):
    from scanerf_amd import allocation
    centers = f["corners"] + f["tile_size"] / 2 if centers is None else centers
    sizes = f["tile_size"][None] if sizes is None else sizes
    out = allocation.view_coverage(fm, T(f["ks"] if ks is None else ks), T(f["c2ws"] if c2ws is None else c2ws), f["H"], f["W"],
                                   T(np.asarray(centers, np.float32)), T(np.asarray(sizes, np.float32)), scale=f["scale"])
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(centers), len(f["ks"] if ks is None else ks))
    return out.cpu().numpy()


def _in_bracket(name, counts, f):
    lo, hi = f["lo"], f["hi"]
    print(f"{name}: {counts.size} (tile, camera) pairs, {int((hi > lo).sum())} with ambiguous pixels ({int((hi - lo).sum())} pixels), "
          f"{int((counts != lo).sum())} counts above lo, below lo {int((counts < lo).sum())}, above hi {int((counts > hi).sum())}")
    assert ((hi - lo) / f["pixels"]).max() <= 0.01
    assert (lo <= counts).all() and (counts <= hi).all()


# ---- 1. the bracket -----------------------------------------------------------------------------------------------------------
def test_counts_lie_in_the_yardsticks_bracket(fmesh):
    f4, f1 = TR.fixture(4), TR.fixture(1)
    c4 = _counts(fmesh, f4)
    _in_bracket("scale 4, 102 x 134", c4, f4)
    c1 = _counts(fmesh, f1)                      # the plain path: a 25 x 33 frame, 825 rays per camera
    _in_bracket("scale 1, 25 x 33", c1, f1)
    assert np.array_equal(c1, c4)                # intrinsics / 4 are exact in float32: the same rays through either path


# ---- 2. exact cases -----------------------------------------------------------------------------------------------------------
def test_exact_cases(fmesh):
    f = TR.fixture(4)
    eye = f["c2ws"][0][:, 3].astype(np.float64)
    fwd = f["c2ws"][0][:, 2].astype(np.float64)
    centers = np.stack([eye,                      # the camera inside the box: every pixel, sky included (near = 0 < depth)
                        eye - 6.0 * fwd,          # wholly behind the camera
                        eye + np.array([0.0, 0.0, 40.0]),   # far above: no ray of this downward-looking camera meets it
                        eye])                     # inside again, a huge box
    sizes = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.0], [500.0, 500.0, 500.0]])
    got = _counts(fmesh, f, centers, sizes, ks=f["ks"][:1], c2ws=f["c2ws"][:1])
    sky = int((TR._traced()[2][0][0] >= TR.SKY).sum())
    print(f"exact cases: counts {got[:, 0].tolist()} of {f['pixels']} pixels, {sky} of them sky")
    assert sky > 0 and got[:, 0].tolist() == [f["pixels"], 0, 0, f["pixels"]]
    # no boxes, no cameras: empty tables, nothing launched
    from scanerf_amd import allocation
    none = allocation.view_coverage(fmesh, T(f["ks"]), T(f["c2ws"]), f["H"], f["W"], torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV))
    assert tuple(none.shape) == (0, 8)
    with pytest.raises(RuntimeError, match="scale"):
        allocation.view_coverage(fmesh, T(f["ks"]), T(f["c2ws"]), f["H"], f["W"], T(np.float32(centers)), T(np.float32(sizes)), scale=0)
    with pytest.raises(RuntimeError, match="no pixel"):
        allocation.view_coverage(fmesh, T(f["ks"]), T(f["c2ws"]), 3, f["W"], T(np.float32(centers)), T(np.float32(sizes)), scale=4)


# ---- 3. more boxes than one pass holds ------------------------------------------------------------------------------------
def test_many_boxes_take_several_passes(fmesh):
    from scanerf_amd import allocation
    m = TR.many_boxes_fixture()
    K = len(m["corners"])
    assert K == 289 and K > allocation.boxes_per_pass() >= 64
    got = _counts(fmesh, m)
    _in_bracket(f"{K} boxes, 2 cameras", got, m)
    assert (got[allocation.boxes_per_pass():] > 0).any()        # the second pass counted something
    # a box count that fills the passes exactly, and one more
    for n in (allocation.boxes_per_pass(), allocation.boxes_per_pass() + 1, 1):
        part = _counts(fmesh, m, (m["corners"] + m["tile_size"] / 2)[:n])
        assert np.array_equal(part, got[:n]), n


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------
def test_counts_are_bit_reproducible(fmesh):
    from scanerf_amd.fastmesh import FastMesh
    V, F = TR.mesh()
    indexed = FastMesh.from_arrays(V, F, DEV, pregather=False)
    assert fmesh.tris is not None and indexed.tris is None
    for f in (TR.fixture(4), TR.many_boxes_fixture()):
        a, b = _counts(fmesh, f), _counts(fmesh, f)
        assert np.array_equal(a, b)
        assert np.array_equal(_counts(indexed, f), a)


# ---- 5. the same counts from the ops that were there before ---------------------------------------------------------------
def test_composed_path_lies_in_the_same_bracket(fmesh):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from bench_tile_alloc import composed_counts
    finally:
        sys.path.pop(0)
    for name, f in (("fixture", TR.fixture(4)), ("289 boxes", TR.many_boxes_fixture())):
        centers = T(np.float32(f["corners"] + f["tile_size"] / 2))
        sizes = T(np.float32(f["tile_size"]))[None].expand(centers.shape[0], 3).contiguous()
        composed = composed_counts(fmesh, T(f["ks"]), T(f["c2ws"]), f["H"], f["W"], centers, sizes, f["scale"]).cpu().numpy()
        _in_bracket("composed, " + name, composed, f)
        fused = _counts(fmesh, f)
        print(f"{name}: fused and composed counts differ in {int((fused != composed).sum())} of {fused.size} entries")


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expect_num,scene_type", [(9, "indoor"), (6, "outdoor")])
def test_allocation_end_to_end(fmesh, tmp_path, expect_num, scene_type):
    from scanerf_amd import allocation, formats
    f = TR.fixture(4)
    res = allocation.allocate_tiles(fmesh, f["ks"], f["c2ws"], f["H"], f["W"], tile_size=TR.TILE_SIZE, overlap_ratio=TR.OVERLAP,
                                    offset=TR.OFFSET, expect_num=expect_num, min_num_image=5, scene_type=scene_type)
    allocation.write_allocation(str(tmp_path / "tiles"), res)
    want = allocation.select_tiles(TR.ratio(f["lo"], f["H"], f["W"], 4), f["c2ws"][:, :, 3], np.float32(f["corners"]), f["tile_size"],
                                   expect_num, 5, scene_type)
    assert np.allclose(res["all_corners"].numpy(), f["corners"], atol=1e-5)
    if expect_num == 9:
        assert 4 in want["tiles"] and len(want["tiles"]) == 7     # the central tile, which no camera is inside, came back in
    else:
        assert 4 not in want["tiles"] and len(want["tiles"]) == 5  # the 6 nearest of 8 tiles, one of them short of views
    assert res["tiles"] == want["tiles"] and res["views"] == want["views"]
    tiles = formats.read_tile_info(str(tmp_path / "tiles" / "tile_info.txt"))
    views = formats.read_training_views(str(tmp_path / "tiles" / "training_views.txt"))
    assert [t["idx"] for t in tiles] == list(range(len(want["tiles"])))
    assert views == {i: v for i, v in enumerate(want["views"])}
    for t, k in zip(tiles, want["tiles"]):
        assert np.allclose(t["corner"], f["corners"][k], atol=0.005 + 1e-6) and t["size"] == [8.0, 8.0, 8.0]
        assert t["resolution"] == [32, 8192 if scene_type == "outdoor" else 4096] and t["init_outside"] is False


def test_build_tiles_command(fmesh, tmp_path):
    """tools/build_tiles.py on a directory holding the fixture's PLY and camera.log (+ an ignore.log)."""
    import subprocess
    from scanerf_amd import allocation, formats
    f = TR.fixture(4)
    data = tmp_path / "scene"
    (data / "mesh").mkdir(parents=True)
    formats.write_ply(str(data / "mesh" / "mesh.ply"), f["V"], f["F"])
    formats.write_campara(str(data / "camera.log"), f["ks"], f["c2ws"], f["H"], f["W"])
    (data / "ignore.log").write_text("2\n")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_tiles.py"), str(data), "--tile-size", "8", "8", "8",
                          "--overlap-ratio", "0.2", "--expect-num", "9", "--min-num-image", "5", "--scene-type", "outdoor"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    # camera.log keeps 8 digits of the poses: select on the counts of the cameras as the file holds them
    ks, c2ws, H, W = formats.read_campara(str(data / "camera.log"), True)
    res = allocation.allocate_tiles(fmesh, ks, c2ws, H, W, tile_size=TR.TILE_SIZE, expect_num=9, min_num_image=5, ignore=[2])
    views = formats.read_training_views(str(data / "tiles" / "training_views.txt"))
    assert views == {i: v for i, v in enumerate(res["views"])} and all(2 not in v for v in views.values()) and len(views) >= 5
    assert len(formats.read_tile_info(str(data / "tiles" / "tile_info.txt"))) == len(views)
