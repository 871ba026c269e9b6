"""The closest-point query on the GPU (csrc/mesh_distance.hip; FastMesh.closest_point, evaluation.compare_meshes,
TileSetRenderer.evaluate_mesh, tools/compare_meshes.py and the extraction commands' --compare): the grid route against
the brute-force route bit for bit at every log2dim and for both triangle forms (the test of the stopping bound), both against float64
within K x the float32 yardstick's own error (profiles/mesh_distance_error.md holds the figures), the max_dist cut, the engineered
cases of tests/mesh_distance_reference.py, the C entries on guarded buffers, and the evaluation on top."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import mesh_distance_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8                    # the project's margin over a float32 yardstick's maximum; not fitted to this kernel
LOG2DIMS = (4, 5, 6, 7)
CASES = sorted(R.cases())

_meshes = {}


def mesh_of(name, L=6, pre=True):
    import scanerf_amd  # noqa
    from scanerf_amd.fastmesh import FastMesh
    V, F, _ = R.cases()[name]
    key = (id(V), id(F), L, pre)          # (the cases that share the terrain's arrays share its structures)
    if key not in _meshes:
        _meshes[key] = FastMesh.from_arrays(V, F, DEV, log2dim=L, pregather=pre)
        assert (_meshes[key].tris is not None) == pre
    return _meshes[key]


def points_of(name):
    return torch.from_numpy(R.cases()[name][2]).to(DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def bound_of(name):
    """K x the yardstick's largest |d32 - d64| on the case, the yardstick floored at one rounding of the largest coordinate."""
    V, _, P = R.cases()[name]
    M = float(max(np.abs(V).max(), np.abs(P[np.isfinite(P).all(1)]).max()))
    return K * max(R.yardstick_error(name), 2.0 ** -24 * M), M


@pytest.mark.parametrize("name", CASES)
def test_grid_equals_brute_force_bit_for_bit(name):
    """dist, face and closest of the grid route equal the brute-force route's bits at log2dim 4..7, pre-gathered and indexed: all
    eight grid results are one result.  A face missed by the stopping bound or by the cell_box pruning shows here."""
    P = points_of(name)
    want = mesh_of(name).closest_point(P, route="brute")
    assert want[0].shape == (len(P),) and want[1].dtype == torch.int32 and want[2].shape == (len(P), 3)
    for L in LOG2DIMS:
        for pre in (True, False):
            m = mesh_of(name, L, pre)
            got = m.closest_point(P)
            bad = (bits(got[0]) != bits(want[0])) | (got[1] != want[1]) | (bits(got[2]) != bits(want[2])).any(1)
            assert not bool(bad.any()), (name, L, pre, int(bad.sum()), bad.nonzero()[:4, 0].tolist())
            assert same(m.closest_point(P), got)                              # a second launch: equal bits
            if L != 6:
                assert same(m.closest_point(P, route="brute"), want)          # (the brute route does not depend on the grid)


@pytest.mark.parametrize("name", CASES)
def test_against_float64(name):
    """|d - d64| <= K x the yardstick's error (absolute), for EVERY point; the reported face is as near as the nearest in float64
    within the same bound; closest is that face's point; found / not found as float64 says."""
    V, F, P = R.cases()[name]
    ref = R.reference(name)
    bound, M = bound_of(name)
    d, face, q = (t.cpu().numpy() for t in mesh_of(name).closest_point(points_of(name)))
    found = np.isfinite(ref["d64"])
    assert np.array_equal(np.isfinite(d), found) and np.array_equal(face >= 0, found)
    assert np.array_equal(q[~found], P[~found], equal_nan=True) and (face[~found] == -1).all()
    if not found.any():
        return
    err = np.abs(d[found].astype(np.float64) - ref["d64"][found]).max()
    excess = (R.dist_to_face64(P[found], V, F, face[found]) - ref["d64"][found]).max()
    qerr = np.abs(np.linalg.norm(P[found].astype(np.float64) - q[found], axis=1) - ref["d64"][found]).max()
    equal32 = float((d[found] == np.sqrt(ref["d2_32"][found])).mean())
    print(f"mesh_distance_error | {name} | {M:.3g} | {R.yardstick_error(name):.3e} | {err:.3e} | "
          f"{err / max(R.yardstick_error(name), 2.0 ** -24 * M):.2f} | {excess:.3e} | {equal32:.4f}")
    assert err <= bound, (name, err, bound)
    assert excess <= bound, (name, excess, bound)
    assert qerr <= bound, (name, qerr, bound)
    assert (0 <= face[found]).all() and (face[found] < len(F)).all() and R.live32(V, F)[face[found]].all()


@pytest.mark.parametrize("max_dist", R.MAX_DISTS)
def test_the_max_dist_cut(max_dist):
    """Outside a band of 1e-4 max_dist around the cut, found / not found is float64's decision; what is found has the uncut run's bits;
    what is not has dist = +inf, face = -1, closest = the point."""
    name = "terrain"
    P = points_of(name)
    d64 = R.reference(name)["d64"]
    band = np.abs(d64 - max_dist) <= R.BAND * max_dist
    assert band.mean() <= 0.01
    for L, pre in ((6, True), (7, False), (4, True)):
        m = mesh_of(name, L, pre)
        full = m.closest_point(P)
        cut = m.closest_point(P, max_dist=max_dist)
        assert same(cut, m.closest_point(P, max_dist=max_dist, route="brute"))
        found = torch.isfinite(cut[0])
        assert np.array_equal(found.cpu().numpy()[~band], (d64 <= max_dist)[~band])
        assert 0.2 < float(found.float().mean()) < 0.8
        assert same([t[found] for t in cut], [t[found] for t in full])
        assert bool((cut[1][~found] == -1).all()) and torch.equal(bits(cut[2][~found]), bits(P[~found]))
        assert bool((cut[0][found] <= max_dist * (1 + 1e-6)).all())
    d0 = mesh_of(name).closest_point(P, max_dist=0.0)            # a cut at zero: only points ON the surface
    assert not bool(torch.isfinite(d0[0]).any())
    V0 = torch.from_numpy(R.cases()[name][0][:40]).to(DEV)   # each the first corner of one of its faces
    assert bool((mesh_of(name).closest_point(V0, max_dist=0.0)[0] == 0).all())


def test_engineered_cases_say_what_they_are_for():
    # vertices and exact edge midpoints on cell planes: d = 0 exactly, at every log2dim
    n0 = 578 + 192
    for L in LOG2DIMS:
        d, face, q = mesh_of("cell_planes", L).closest_point(points_of("cell_planes"))
        assert bool((d[:n0] == 0).all()) and torch.equal(bits(q[:n0]), bits(points_of("cell_planes")[:n0])) and bool((face >= 0).all())
    # only dead faces: nothing answers, through the grid and through every face
    P = points_of("dead_only")
    for route in ("grid", "brute"):
        d, face, q = mesh_of("dead_only").closest_point(P, route=route)
        assert bool(torch.isinf(d).all()) and bool((face == -1).all()) and torch.equal(bits(q), bits(P))
    # dead faces in front of the terrain's: the answers are the terrain's, the indices shifted by the two dead faces
    Pm = points_of("dead_mixed")
    d, face, q = mesh_of("dead_mixed").closest_point(Pm)
    d0, face0, q0 = mesh_of("terrain").closest_point(Pm)
    assert same((d, q), (d0, q0)) and torch.equal(face, face0 + 2)
    # non-finite points among finite ones: their rows say "nothing", the others are the terrain's
    Pn = points_of("non_finite")
    d, face, q = mesh_of("non_finite").closest_point(Pn)
    bad = ~torch.isfinite(Pn).all(1)
    assert int(bad.sum()) == 4 and bool(torch.isinf(d[bad]).all()) and bool((face[bad] == -1).all())
    assert torch.equal(bits(q[bad]), bits(Pn[bad])) and bool(torch.isfinite(d[~bad]).all())
    # an empty mesh is refused by the structure; the brute entry takes F = 0 and finds nothing
    from scanerf_amd import _capi
    from scanerf_amd.fastmesh import FastMesh
    with pytest.raises(ValueError, match="vertices and faces"):
        FastMesh.from_arrays(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32), DEV)
    dist2 = torch.full((65,), -7.0, device=DEV)
    fc = torch.full((65,), -7, dtype=torch.int32, device=DEV)
    P65 = points_of("n65")
    _capi.check(_capi.lib().scanerf_mesh_closest_point_brute(P65.data_ptr(), 65, None, None, 0, 0, None, 6, float("inf"),
                                                             dist2.data_ptr(), fc.data_ptr(), None, _capi.stream()), "brute F=0")
    assert bool(torch.isinf(dist2).all()) and bool((fc == -1).all())
    # wrong dtype, shape and max_dist are refused with GPU tensors too; want_closest=False returns None
    m = mesh_of("terrain")
    with pytest.raises(RuntimeError, match="float32"):
        m.closest_point(P65.double())
    with pytest.raises(ValueError, match="max_dist"):
        m.closest_point(P65, max_dist=-1.0)
    d1, f1, q1 = m.closest_point(P65, want_closest=False)
    assert q1 is None and same((d1, f1), m.closest_point(P65)[:2])
    assert m.closest_point(P65[:0])[0].shape == (0,)


def test_c_entries_write_exactly_their_rows():
    """Sentinel-filled buffers with guard regions: exactly N rows of each output are written and nothing outside them; closest = NULL
    is accepted; bad arguments return the error status and write nothing."""
    from scanerf_amd import _capi
    lib = _capi.lib()
    m = mesh_of("terrain", 6, True)
    mi = mesh_of("terrain", 6, False)
    G = 256
    for N in (1, 65, 1792):
        P = points_of("terrain")[:N].contiguous()

        def buffers():
            return (torch.full((N + 2 * G,), -7.0, device=DEV), torch.full((N + 2 * G,), -7, dtype=torch.int32, device=DEV),
                    torch.full((3 * N + 2 * G,), -7.0, device=DEV))

        def grid(mesh, bufs, closest=True, L=6, md=float("inf"), N_=N):
            d2, fc, cl = bufs
            return lib.scanerf_mesh_closest_point(
                P.data_ptr(), N_, mesh.vertices.data_ptr(), mesh.faces.data_ptr(), mesh.tris.data_ptr() if mesh.tris is not None else None,
                mesh.bitmask.data_ptr(), mesh.rank.data_ptr(), mesh.start_num.data_ptr(), mesh.cell_faces.data_ptr(),
                mesh.cell_box.data_ptr(), mesh.scene_info.data_ptr(), L, md, d2.data_ptr() + 4 * G, fc.data_ptr() + 4 * G,
                cl.data_ptr() + 4 * G if closest else None, _capi.stream())

        def brute(bufs, closest=True, md=float("inf"), N_=N):
            d2, fc, cl = bufs
            return lib.scanerf_mesh_closest_point_brute(
                P.data_ptr(), N_, m.vertices.data_ptr(), m.faces.data_ptr(), m.vertices.shape[0], m.faces.shape[0],
                m.scene_info.data_ptr(), 6, md, d2.data_ptr() + 4 * G, fc.data_ptr() + 4 * G, cl.data_ptr() + 4 * G if closest else None,
                _capi.stream())

        def untouched(b):
            return bool((b == -7).all())

        want = m.closest_point(P)
        for call in (lambda b, **k: grid(m, b, **k), lambda b, **k: grid(mi, b, **k), brute):
            bufs = buffers()
            assert call(bufs) == 0
            torch.cuda.synchronize()
            for b in bufs:
                assert untouched(b[:G]) and untouched(b[-G:]) and not bool((b[G:-G] == -7).any())
            assert same((torch.sqrt(bufs[0][G:-G]), bufs[1][G:-G], bufs[2][G:-G].view(N, 3)), want)
            part = buffers()
            assert call(part, closest=False) == 0                       # closest = NULL: the other two as before, closest untouched
            torch.cuda.synchronize()
            assert same(part[:2], bufs[:2]) and untouched(part[2])
            bad = buffers()
            assert call(bad, md=-1.0) != 0 and b"max_dist" in lib.scanerf_last_error()
            assert call(bad, md=float("nan")) != 0 and call(bad, N_=-3) != 0
            torch.cuda.synchronize()
            assert all(untouched(b) for b in bad)
        bad = buffers()
        assert grid(m, bad, L=8) != 0 and b"log2dim" in lib.scanerf_last_error()
        torch.cuda.synchronize()
        assert all(untouched(b) for b in bad)


# ---- the evaluation on top ----------------------------------------------------------------------------------------------------------
def test_compare_meshes_against_itself_and_against_float64():
    import scanerf_amd  # noqa
    from scanerf_amd import evaluation
    V, F, _ = R.cases()["terrain"]
    bound, _ = bound_of("terrain")
    res = evaluation.compare_meshes((V, F), (torch.from_numpy(V).to(DEV), torch.from_numpy(F).to(DEV)), 4096, [bound, 0.1],
                                    return_distances=True)
    for direction in ("pred_to_gt", "gt_to_pred"):
        assert float(res["distances"][direction]["dist"].max()) <= bound
        assert res[direction]["not_found"] == 0.0 and res[direction]["n"] == 4096
    assert res["precision"] == {bound: 1.0, 0.1: 1.0} and res["recall"] == res["precision"] and res["fscore"] == res["precision"]
    assert res["chamfer"] <= bound and res["max_dist"] is None and res["n_samples"] == 4096
    # the terrain against a copy shifted by (0, 0, 0.25): every sample's distance against the float64 brute force of the same samples
    Vs = (V + np.array([0, 0, 0.25], np.float32)).astype(np.float32)
    n, ts = 1024, [0.1, 0.2, 0.26]
    res = evaluation.compare_meshes((V, F), (Vs, F), n, ts, max_dist=0.24, seed=3, return_distances=True, device=DEV)
    scores = {}
    for direction, (Vo, seed) in (("pred_to_gt", (Vs, 3)), ("gt_to_pred", (V, 4))):
        dd = res["distances"][direction]
        pts = dd["points"].cpu().numpy()
        want_pts, want_face = evaluation.sample_surface(torch.from_numpy(Vs if direction == "gt_to_pred" else V), torch.from_numpy(F), n, seed)
        assert np.array_equal(pts, want_pts.numpy()) and np.array_equal(dd["sample_face"].cpu().numpy(), want_face.numpy())
        d64 = np.sqrt(R.closest(pts, Vo, F)[0])
        d = dd["dist"].cpu().numpy().astype(np.float64)
        band = np.abs(d64 - 0.24) <= R.BAND * 0.24
        assert band.mean() <= 0.01
        assert np.array_equal(np.isfinite(d)[~band], (d64 <= 0.24)[~band])
        ok = np.isfinite(d)
        assert np.abs(d[ok] - d64[ok]).max() <= bound
        assert 0.05 < res[direction]["not_found"] < 0.95                     # the cut splits the samples
        scores[direction] = d
    want = evaluation.summarize(torch.from_numpy(scores["pred_to_gt"]), torch.from_numpy(scores["gt_to_pred"]), ts)
    for k in ("precision", "recall", "fscore"):
        assert res[k] == pytest.approx(want[k])
    assert res["chamfer"] == pytest.approx(want["chamfer"]) and res["max_dist"] == 0.24
    assert res["pred_to_gt"]["median"] == pytest.approx(want["pred_to_gt"]["median"])
    assert res["precision"][0.26] == pytest.approx(1.0 - res["pred_to_gt"]["not_found"])
    again = evaluation.compare_meshes((V, F), (Vs, F), n, ts, max_dist=0.24, seed=3, device=DEV)
    assert json.loads(evaluation.json_line(again)) == json.loads(evaluation.json_line(res))


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _last_json(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def test_the_renderers_method_and_the_commands(tmp_path, capsys):
    """TileSetRenderer.evaluate_mesh is compare_meshes of its extracted mesh; tools/compare_meshes.py prints that dict as one JSON line
    and stores the distances; both extraction commands print the same line with --compare and nothing new without it."""
    import render_scenes as RS
    import scene_mesh_reference as M
    import scanerf_amd  # noqa
    from scanerf_amd import evaluation, formats, renderer
    sc = M.scene("G9")
    tiles = RS.renderer_tiles(sc)
    rnd = renderer.TileSetRenderer(DEV, tiles)
    level = M.reference(M.CASES[0])[6]
    mesh = rnd.extract_mesh(level, cells_per_axis=20, min_faces=1)
    assert mesh.faces.shape[0] > 0
    gt_v = (mesh.vertices + torch.tensor([0.0, 0.05, 0.0], device=DEV)).cpu().numpy()
    gt_f = mesh.faces.cpu().numpy()[::-1].copy()
    kw = dict(n_samples=2000, thresholds=[0.02, 0.06], max_dist=1.0, seed=2, log2dim=5)
    want = evaluation.compare_meshes((mesh.vertices, mesh.faces), (gt_v, gt_f), kw["n_samples"], kw["thresholds"], max_dist=1.0, seed=2,
                                     log2dim=5)
    got = rnd.evaluate_mesh((gt_v, gt_f), level, cells_per_axis=20, min_faces=1, **kw)
    assert json.loads(evaluation.json_line(got)) == json.loads(evaluation.json_line(want))
    assert want["recall"][0.06] == 1.0 and 0.0 < want["chamfer"] <= 0.05 + 1e-5
    # the command on two PLY files
    pred_ply, gt_ply = str(tmp_path / "pred.ply"), str(tmp_path / "gt.ply")
    formats.write_ply(pred_ply, mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy())
    formats.write_ply(gt_ply, gt_v, gt_f)
    capsys.readouterr()
    npz, js = str(tmp_path / "d.npz"), str(tmp_path / "score.json")
    score = ["--samples", "2000", "--threshold", "0.02", "0.06", "--max-dist", "1.0", "--seed", "2", "--log2dim", "5"]
    assert _load_tool("compare_meshes").main([pred_ply, gt_ply, *score, "--json", js, "--distances", npz]) == 0
    out = capsys.readouterr().out
    assert len(out.strip().splitlines()) == 1
    line = _last_json(out)
    assert line == json.loads(evaluation.json_line(want)) and json.load(open(js)) == line
    z = np.load(npz)
    assert sorted(z.files) == sorted(f"{d}_{k}" for d in ("pred_to_gt", "gt_to_pred") for k in ("points", "sample_face", "dist", "face"))
    assert z["pred_to_gt_points"].shape == (2000, 3) and z["gt_to_pred_dist"].shape == (2000,) and z["gt_to_pred_face"].dtype == np.int32
    assert float(np.mean(z["pred_to_gt_dist"])) == pytest.approx(line["pred_to_gt"]["mean"], rel=1e-6)
    # the extraction commands: tiles as renderer.export_tile writes them
    dirs = []
    for b, tile in enumerate(tiles):
        path = str(tmp_path / f"tile-{b}")
        os.makedirs(path)
        t = torch.as_tensor
        renderer.write_feature_npz(path, t(tile["features"]), t(tile["occupied_grid"]), t(tile["block_corner"]), t(tile["block_size"]),
                                   t(tile["grid_log2dim"]), t(tile["resolution"]))
        torch.save(dict(M.O.unpack_blob(torch.from_numpy(tile["blob"]))), os.path.join(path, "decoder.pth"))
        dirs.append(path)
    scene_tool = _load_tool("extract_scene_mesh")
    base = [*dirs, "--level", repr(level), "--cells-per-axis", "20", "--min-faces", "1", "--out", str(tmp_path / "scene.ply")]
    assert scene_tool.main(base) == 0
    plain = capsys.readouterr().out
    assert "{" not in plain and len(plain.strip().splitlines()) == 2           # without --compare: the two lines it always printed
    assert scene_tool.main([*base, "--compare", gt_ply, *score]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and _last_json(out) == line
    with pytest.raises(SystemExit):
        scene_tool.main([*base, "--compare", gt_ply])                          # --compare needs --threshold
    capsys.readouterr()
    tile_tool = _load_tool("extract_mesh")
    tail = ["--level", repr(level), "--cells-per-axis", "16", "--out", str(tmp_path / "tiles")]
    assert tile_tool.main([*dirs, *tail]) == 0
    assert "{" not in capsys.readouterr().out
    with_faces = [b for b in range(len(dirs)) if len(formats.read_ply(str(tmp_path / "tiles" / f"tile-{b}.ply"))[1])]
    assert with_faces
    b = with_faces[0]
    assert tile_tool.main([dirs[b], *tail]) == 0
    plain = capsys.readouterr().out
    assert tile_tool.main([dirs[b], *tail, "--compare", gt_ply, *score]) == 0
    out = capsys.readouterr().out
    tv, tf = formats.read_ply(str(tmp_path / "tiles" / f"tile-{b}.ply"))[:2]
    tile_want = evaluation.compare_meshes((tv, tf), gt_ply, 2000, [0.02, 0.06], max_dist=1.0, seed=2, log2dim=5, device=DEV)
    assert out.startswith(plain) and _last_json(out) == json.loads(evaluation.json_line(tile_want))
