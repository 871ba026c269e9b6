"""The inputs of the many-tile render-time tests do what they claim: conditions on tests/render_scenes.py's scenes and rays,
checked with the oracle alone (no GPU, no kernel of the build) at B = 509 rays, S = 32 samples.

No list of exactly three occurs in a grid scene, and none can: a tile shares a sample (or a ray's exit distance) when its x
range AND its z range do, and the ranges of neighbouring columns / rows overlap pairwise only, so the count is a product of
two numbers out of {1, 2}.  That is asserted here; slot and exit lists of exactly three come from STACK3.

Observed, shuffled order (`>=2` / `==4`: share of the samples that list a tile, over every tracing pass with all rays kept
running; `exits`: rays per length 1 / 2 / 3 / 4 of update_outgoing_bidx's list; `run`: samples from sample 0 of the sorted
order whose first-pass lists hold tiles >= 32 only):
    scene   nb  max_tracing  listed samples   >=2     ==4    exits 1 / 2 / 3 / 4    first-slot tiles (passes 0-1)   run
    G8       8       8           31 008      0.642   0.196   189 / 165 / 0 / 128              8                       -
    G9       9       7           34 016      0.635   0.163   208 / 145 / 0 / 126              9                       -
    G36     36      14           68 064      0.450   0.064   321 / 103 / 0 /  59             36                     8 726
    G64     64      19           85 440      0.456   0.059   307 / 112 / 0 /  63             64                    11 078
    G65     65      26          106 144      0.435   0.056   285 / 139 / 0 /  60             65                    10 328
    STACK3 / STACK6: 14 720 / 14 656 listed samples, every list [0,1,2] / [0,1,2,3]; 485 hitting rays each, 24 misses.
"""
import functools

import numpy as np
import pytest

import render_scenes as RS
from oracle import oracle as O

S = 32
GRIDS = tuple(RS.GRIDS)
HIGH = ("G36", "G64", "G65")


@functools.lru_cache(maxsize=None)
def figures(name):
    sc, rays = RS.named(name)
    nb = sc["corners"].shape[0]
    o, d = rays["shuffled"]
    passes = RS.trace_samples(sc, o, d, S)
    bi = np.concatenate([p[2].reshape(-1, 4) for p in passes])
    bi = bi[bi[:, 0] != -1]
    n_slots = (bi != -1).sum(-1)
    inter = O.ray_block_intersection(o, d, sc["corners"], sc["sizes"])
    tb, max_tracing = RS.tracing_order(inter)
    ob, bw = O.update_outgoing_bidx(o, d, sc["corners"], sc["sizes"], tb, inter, 0.12, False)
    n_exit = (ob != -1).sum(-1)
    first0 = np.concatenate([p[2][..., 0] for p in passes[:2]])
    so, sd = rays["sorted"]
    b0 = RS.trace_samples(sc, so, sd, S, passes=1)[0][2].reshape(-1, 4)   # [B*S,4] in sample order (layout 0)
    high_only = ((b0 >= 32) | (b0 == -1)).all(-1)   # (a sample without a tile -- a ray that met no occupied cell -- lists none)
    run = int(np.argmin(high_only)) if not high_only.all() else high_only.size
    run_listed = float((b0[:4096, 0] != -1).mean())
    f = dict(nb=nb, listed=np.unique(bi[bi != -1]), first_pass0=np.unique(first0[first0 != -1]), n_listed=len(bi),
             ge2=float((n_slots >= 2).mean()), eq3=int((n_slots == 3).sum()), eq4=float((n_slots == 4).mean()),
             exits=[int((n_exit == k).sum()) for k in range(5)], max_tracing=max_tracing, run=run, run_listed=run_listed, bi=bi, ob=ob, tb=tb, inter=inter,
             hit=(inter[..., 0] != 1e7).any(-1))
    print(f"{name}: nb {nb} max_tracing {max_tracing} listed samples {len(bi)} >=2 {f['ge2']:.3f} ==4 {f['eq4']:.3f} "
          f"exits {f['exits'][1:]} tiles listed {len(f['listed'])} first-slot tiles in passes 0-1 {len(f['first_pass0'])} run {run} (listed {run_listed:.3f})")
    return f


@pytest.mark.parametrize("name", GRIDS)
def test_grid_scene_rays_meet_every_tile_and_every_overlap(name):
    f = figures(name)
    nb = f["nb"]
    assert np.array_equal(f["listed"], np.arange(nb)), "every tile index occurs in some sample's slot list"
    assert np.array_equal(f["first_pass0"], np.arange(nb)), "every tile is some sample's FIRST slot within the first two passes"
    assert f["ge2"] >= 0.10 and f["eq4"] >= 0.01
    assert f["eq3"] == 0, "three tiles cannot share a sample in a grid (module docstring)"
    assert f["exits"][2] >= 5 and f["exits"][4] >= 5
    assert f["exits"][3] == 0, "three tiles cannot share an exit distance in a grid (module docstring)"
    assert f["max_tracing"] >= 4
    assert f["hit"].sum() > 400 and (~f["hit"]).sum() >= 20
    if name in HIGH:
        assert f["listed"].max() == nb - 1 and (f["listed"] >= 32).sum() == nb - 32
        assert f["run_listed"] >= 0.9
        assert f["run"] >= 8192, "sorted order: the batch opens with a run of 8192 samples (a chunk of either kernel) on tiles >= 32 only"
    if name == "G64":
        assert 63 in f["listed"]


def test_the_two_orders_hold_the_same_rays():
    for name in GRIDS + tuple(RS.STACKS):
        _, rays = RS.named(name)
        a, b = (np.concatenate(rays[k], 1) for k in ("shuffled", "sorted"))
        assert a.shape == (RS.B_RAYS, 6) and RS.B_RAYS % 32
        assert np.array_equal(a[np.lexsort(a.T)], b[np.lexsort(b.T)])
        assert not np.array_equal(a, b)


@pytest.mark.parametrize("name,n", list(RS.STACKS.items()))
def test_stacked_scene_lists_are_the_first_four_tiles(name, n):
    f = figures(name)
    k = min(n, 4)
    want = np.int16(list(range(k)) + [-1] * (4 - k))
    assert f["n_listed"] > 5000 and (f["bi"] == want).all()
    assert f["hit"].sum() > 400 and (~f["hit"]).sum() >= 20
    assert f["max_tracing"] == n
    first4 = np.full((RS.B_RAYS, 4), -1, np.int16)
    first4[:, :k] = f["tb"][:, :k]
    assert np.array_equal(f["ob"][f["hit"]], first4[f["hit"]]) and (f["ob"][~f["hit"]] == -1).all()
    assert np.array_equal(first4[f["hit"]], np.broadcast_to(want, (int(f["hit"].sum()), 4)))
