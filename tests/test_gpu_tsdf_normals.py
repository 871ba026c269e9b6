"""The fused mesh's normals on the GPU (csrc/tsdf.hip, scanerf_tsdf_vertex_normals; scanerf_amd/fusion.py, evaluation.py; DESIGN.md
4.22): the fused kernel against the composed torch route against the numpy float32 restatement bit for bit at every vertex, against
float64 within the derived bound on the judged vertices; vertex counts around a wavefront, guard regions, prefilled outputs, a second
run, refusals, a side stream; extract / fuse_depth_maps / fuse_mesh / the command with normals; and normal consistency in
compare_meshes."""
import ctypes
import math

import numpy as np
import pytest
import torch

import tsdf_normals_reference as NR
import tsdf_reference as TR
from test_gpu_tsdf import DEV, SENTINEL, _bits, _guarded, _guards_intact, _icosphere, _np, _trace_depth, tile_scene  # noqa: F401

pytestmark = pytest.mark.gpu
ENTRY = "scanerf_tsdf_vertex_normals"


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _mesh(cells, lattice):
    from scanerf_amd import meshing
    V = len(cells)
    return meshing.Mesh(torch.zeros((V, 3), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV),
                        _dev(np.reshape(cells, (V, 3)), np.int32), _dev(np.reshape(lattice, (V, 3)), np.float32), None)


def _volume(n, spacing):
    from scanerf_amd import fusion
    return fusion.TSDFVolume([0.0, 0.0, 0.0], list(spacing), list(n), 1.0, DEV)


def _three_routes(f, cells, lattice, what):
    """fused, composed and numpy float32 on the field f = {n, spacing, values, observed}: equal bits; then float64 within the bound."""
    n, spacing = f["n"], f["spacing"]
    vol, mesh = _volume(n, spacing), _mesh(cells, lattice)
    shape = [m + 1 for m in n]
    values, observed = _dev(f["values"].reshape(shape), np.float32), _dev(f["observed"].reshape(shape), np.bool_)
    got = vol.vertex_normals(mesh, values=values, observed=observed)
    wit = vol.vertex_normals(mesh, values=values, observed=observed, route="composed")
    r32 = NR.vertex_normals(f["values"], f["observed"], n, spacing, cells, lattice, np.float32)
    r64 = NR.vertex_normals(f["values"], f["observed"], n, spacing, cells, lattice, np.float64)
    V = len(cells)
    out = {}
    for i, key in enumerate(("normal", "grad")):
        g, w = _np(got[i]), _np(wit[i])
        assert g.dtype == np.float32 and g.shape == (V, 3) and w.dtype == np.float32 and w.shape == (V, 3)
        d_np, d_w = (_bits(g) != _bits(r32[key])).any(1), (_bits(g) != _bits(w)).any(1)
        print(f"tsdf normals {what}: {key}: V {V}, evaluated {int(r32['evaluated'].sum())}; fused != numpy f32 in {int(d_np.sum())} vertices, "
              f"fused != composed in {int(d_w.sum())} vertices")
        if d_np.any():      # name the first differing vertex and component: which operation, not how much
            v = int(np.nonzero(d_np)[0][0])
            print(f"tsdf normals {what}: first difference at vertex {v}: cell {cells[v]}, lattice {lattice[v]}, fused {g[v]}, numpy {r32[key][v]}, "
                  f"composed {w[v]}, branches {r32['branches'][v].tolist()}")
        assert not d_w.any(), f"{key}: the fused kernel and the composed route differ"
        assert not d_np.any(), f"{key}: the fused kernel and the numpy float32 restatement differ"
        out[key] = g
    j = r64["judged"]
    gerr = np.abs(out["grad"].astype(np.float64) - r64["grad"])
    nerr = np.abs(out["normal"].astype(np.float64) - r64["normal"]).max(1)
    ev = r64["evaluated"]
    print(f"tsdf normals {what}: judged {int(j.sum())} of {V}; max grad error / bound "
          f"{(gerr[j & ev] / np.maximum(r64['grad_bound'][j & ev], 1e-300)).max() if (j & ev).any() else 0.0:.3f}, max normal error / bound "
          f"{(nerr[j & ev] / r64['normal_bound'][j & ev]).max() if (j & ev).any() else 0.0:.3f}")
    assert (gerr[j] <= r64["grad_bound"][j]).all() and (nerr[j] <= r64["normal_bound"][j]).all()
    assert not out["grad"][~ev].any() and not out["normal"][~ev].any()
    return out, r64


# ---- bit equality and float64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TR.CASES)
def test_fused_composed_and_numpy_float32_agree_in_every_bit_on_the_reference_meshes(name):
    f = NR.field(name)
    for what, m in (("culled", f["mesh"]), ("raw", f["raw"])):
        out, r64 = _three_routes(f, np.asarray(m.cells, np.int32), np.asarray(m.lattice, np.float32), f"{name} {what}")
        if what == "culled" and name in NR.SPHERES:
            assert r64["evaluated"].all() and r64["judged"].mean() >= NR.JUDGED_SHARE
            ang = NR.angles_deg(out["normal"], np.asarray(m.vertices, np.float64))
            print(f"tsdf normals {name}: mean angle to the radial direction {ang.mean():.2f} deg (reference {NR.RADIAL_MEAN_DEG[name]})")
            assert ang.mean() <= NR.RADIAL_MARGIN * NR.RADIAL_MEAN_DEG[name]
            assert np.abs(np.linalg.norm(out["normal"].astype(np.float64), axis=1) - 1.0).max() <= 1e-6


def test_hand_lattices_every_branch_the_zeros_and_the_unit_lattice():
    h = NR.hand()
    out, r64 = _three_routes(h, h["cells"], h["lattice"], "hand (n_z = 65)")
    assert r64["evaluated"].any() and not r64["evaluated"].all()
    n, spacing, val, obs = NR.unit_lattice()
    f = {"n": list(n), "spacing": list(spacing), "values": val, "observed": obs}
    cells = np.zeros((5, 3), np.int32)
    cells[4] = (0, 1, 0)
    lattice = np.array([[0.5, 0.5, 0.5], [0, 0, 0], [1, 1, 1], [0.25, 0.75, 0.5], [0.5, 1.5, 0.5]], np.float32)
    out, _ = _three_routes(f, cells, lattice, "unit lattice")
    assert out["grad"][:3].tolist() == [[1.5, 2.0, 1.125], [1.0, 1.0, 1.0], [3.0, 5.0, 1.5]] and not out["grad"][4].any()
    # a linear field on a lattice with holes: exact, whatever is unobserved
    n, spacing, coeffs = (5, 4, 6), (0.5, 0.25, 2.0), (0.25, -0.5, 1.0)
    val = NR.linear_field(n, coeffs, 0.375)
    rng = np.random.default_rng(15)
    f = {"n": list(n), "spacing": list(spacing), "values": val, "observed": rng.uniform(size=len(val)) >= 0.1}
    cells = np.stack([rng.integers(0, m, 300) for m in n], 1).astype(np.int32)
    lattice = (cells + rng.integers(0, 9, cells.shape) / 8.0).astype(np.float32)
    out, r64 = _three_routes(f, cells, lattice, "linear field with holes")
    ev = r64["evaluated"]
    assert ev.any() and (~ev).any() and (out["grad"][ev] == np.asarray([0.5, -2.0, 0.5], np.float32)).all()
    # a constant field: a zero gradient gives a zero normal
    f["values"] = np.full(len(val), 0.5, np.float32)
    out, _ = _three_routes(f, cells, lattice, "constant field")
    assert not out["grad"].any() and not out["normal"].any()


# ---- sizes, guards, prefilled outputs, a second run ------------------------------------------------------------------------------------
def _guarded_copy(a, fill):
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf, view = _guarded(tuple(t.shape), t.dtype, fill)
    view.copy_(t.to(DEV))
    return buf, view


@pytest.mark.parametrize("V", [0, 1, 63, 64, 65, 257])
def test_vertex_counts_guard_regions_prefilled_outputs_and_a_second_run(V):
    from scanerf_amd import _capi
    h = NR.hand()
    assert h["n"][2] == 65
    order = np.argsort(~h["ref32"]["evaluated"], kind="stable")      # evaluated vertices first: a count of 1 computes something
    cells, lattice = h["cells"][order][:V], h["lattice"][order][:V]
    want = NR.vertex_normals(h["values"], h["observed"], h["n"], h["spacing"], cells, lattice, np.float32)
    # through the library
    got = _volume(h["n"], h["spacing"]).vertex_normals(_mesh(cells, lattice), values=_dev(h["values"].reshape([m + 1 for m in h["n"]])),
                                                       observed=_dev(h["observed"].reshape([m + 1 for m in h["n"]])))
    assert got[0].shape == (V, 3) and got[1].shape == (V, 3) and got[0].dtype == torch.float32
    assert np.array_equal(_bits(_np(got[0])), _bits(want["normal"])) and np.array_equal(_bits(_np(got[1])), _bits(want["grad"]))
    if V == 0:
        return
    # through the C entry on guarded buffers
    vbuf, values = _guarded_copy(h["values"], SENTINEL)
    obuf, observed = _guarded_copy(h["observed"].astype(np.uint8), 1)      # a read outside would count as observed
    cbuf, cd = _guarded_copy(cells, 1)                                      # a read outside would be a valid cell
    lbuf, ld = _guarded_copy(lattice, SENTINEL)
    nbuf, normal = _guarded((V, 3), torch.float32, SENTINEL)
    gbuf, grad = _guarded((V, 3), torch.float32, SENTINEL)
    spacing = (ctypes.c_float * 3)(*h["spacing"])
    st = torch.cuda.current_stream().cuda_stream
    fn = _capi.tool(ENTRY)
    runs = []
    for fill in (math.nan, SENTINEL):
        normal.fill_(fill), grad.fill_(fill)
        assert fn(values.data_ptr(), observed.data_ptr(), *h["n"], spacing, cd.data_ptr(), ld.data_ptr(), V, normal.data_ptr(), grad.data_ptr(), st) == 0
        runs.append((_np(normal).copy(), _np(grad).copy()))
        assert np.isfinite(runs[-1][0]).all() and np.isfinite(runs[-1][1]).all(), "an element of the outputs was not written"
        assert np.array_equal(_bits(runs[-1][0]), _bits(want["normal"])) and np.array_equal(_bits(runs[-1][1]), _bits(want["grad"]))
        for buf, fill_ in ((vbuf, SENTINEL), (obuf, 1), (cbuf, 1), (lbuf, SENTINEL)):
            assert _guards_intact(buf, fill_)
        assert _guards_intact(nbuf, SENTINEL) and _guards_intact(gbuf, SENTINEL), "an output's guard region was written"
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])), "a second run differs"
    # the inputs hold what they held
    assert np.array_equal(_bits(_np(values)), _bits(h["values"])) and np.array_equal(_np(observed), h["observed"].astype(np.uint8))
    assert np.array_equal(_np(cd), cells) and np.array_equal(_bits(_np(ld)), _bits(lattice))


def test_refusals_through_the_c_entry_leave_the_outputs_untouched():
    from scanerf_amd import _capi
    h = NR.hand()
    V = 8
    values, observed = _dev(h["values"]), _dev(h["observed"].astype(np.uint8))
    cells, lattice = _dev(h["cells"][:V]), _dev(h["lattice"][:V])
    nbuf, normal = _guarded((V, 3), torch.float32, SENTINEL)
    gbuf, grad = _guarded((V, 3), torch.float32, SENTINEL)
    s3 = lambda *v: (ctypes.c_float * 3)(*v)
    ok = dict(values=values.data_ptr(), observed=observed.data_ptr(), nx=h["n"][0], ny=h["n"][1], nz=h["n"][2], spacing=s3(*h["spacing"]),
              cells=cells.data_ptr(), lattice=lattice.data_ptr(), V=V, normal=normal.data_ptr(), grad=grad.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    fn = _capi.tool(ENTRY)
    overs = [{k: None} for k in ("values", "observed", "spacing", "cells", "lattice", "normal", "grad")]
    overs += [{"V": -1}, {"nx": 0}, {"ny": -3}, {"nz": 0}, {"nx": 2047, "ny": 2047, "nz": 2047}, {"spacing": s3(0.5, 0.0, 0.125)},
              {"spacing": s3(0.5, 0.25, -0.125)}, {"spacing": s3(math.inf, 0.25, 0.125)}, {"spacing": s3(0.5, math.nan, 0.125)}]
    for over in overs:
        assert fn(*{**ok, **over}.values(), st) != 0, over
    assert fn(*{**ok, "V": 0}.values(), st) == 0      # V == 0 launches nothing
    torch.cuda.synchronize()
    for b in (nbuf, gbuf):
        assert bool((b == SENTINEL).all()), "a refused or empty call wrote something"
    assert fn(*ok.values(), st) == 0
    want = NR.vertex_normals(h["values"], h["observed"], h["n"], h["spacing"], h["cells"][:V], h["lattice"][:V], np.float32)
    assert np.array_equal(_bits(_np(normal)), _bits(want["normal"])) and np.array_equal(_bits(_np(grad)), _bits(want["grad"]))
    # the Python level: a mesh on another lattice's volume, mismatched shapes
    vol = _volume(h["n"], h["spacing"])
    with pytest.raises(RuntimeError, match=r"values and observed must be \[4, 5, 66\]"):
        vol.vertex_normals(_mesh(h["cells"][:V], h["lattice"][:V]), values=values, observed=observed)
    with pytest.raises(RuntimeError, match="dtype"):
        vol.vertex_normals(_mesh(h["cells"][:V], h["lattice"][:V]), values=values.reshape(4, 5, 66).double(), observed=observed.reshape(4, 5, 66))


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
def test_stream_the_op_runs_on_the_callers_stream(monkeypatch):
    import stream_cases as SC
    from scanerf_amd import _capi
    from test_gpu_stream_contract import Delay, same_bits
    n, spacing = (40, 36, 44), (0.05, 0.06, 0.04)
    shape = [m + 1 for m in n]

    def build(seed):
        rng = np.random.default_rng(700 + seed)
        return {"values": torch.from_numpy(rng.uniform(0.0, 1.0, shape).astype(np.float32)),
                "observed": torch.from_numpy((rng.uniform(size=shape) > 0.01).astype(np.uint8))}

    def setup(state):
        cells, lattice = NR.random_vertices(n, 20000, 9)
        state["mesh"] = _mesh(cells, lattice)
        state["vol"] = _volume(n, spacing)

    def run_(state):
        i = state["in"]
        return state["vol"].vertex_normals(state["mesh"], values=i["values"], observed=i["observed"])

    c = SC.Case("tsdf_normals", [ENTRY], build, run_, setup=setup)
    X, Y = c.build(1), c.build(2)
    assert all(not torch.equal(X[k], Y[k]) and X[k].shape == Y[k].shape for k in X)
    state = c.to_device(X)
    Xd, Yd = SC.stage(X), SC.stage(Y)
    handles = []
    real = _capi.tool(ENTRY)

    def recorded(*a):
        handles.append(int(a[-1] or 0))
        return real(*a)
    monkeypatch.setitem(_capi._tools, ENTRY, recorded)
    torch.cuda.synchronize()
    R_X = c.run(state)
    c.refill(state, Yd)
    R_Y = c.run(state)
    torch.cuda.synchronize()
    assert not same_bits(R_X[:1], R_Y[:1]) and not same_bits(R_X[1:], R_Y[1:]), "the two seeds give the same answer: a stale read would not show"
    assert handles == [torch.cuda.current_stream().cuda_stream] * 2
    delay = Delay()
    s = torch.cuda.Stream()
    del handles[:]
    with torch.cuda.stream(s):
        pending = delay(20.0)
        c.refill(state, Xd)           # queued behind the delay: a launch on any other stream reads Y
        R = c.run(state)
        still = not pending.query()
    s.synchronize()
    torch.cuda.synchronize()
    assert handles == [s.cuda_stream] and s.cuda_stream != 0, "the call did not carry the caller's stream"
    assert still, "the call waited for its stream (the delay ran out before it returned)"
    assert same_bits(R, R_X), "under a side stream the op read stale inputs: the launch went to another stream"


# ---- through the public routes -----------------------------------------------------------------------------------------------------------
def _same_geometry(got, plain, what):
    for k in ("vertices", "faces", "cells", "lattice"):
        a, b = getattr(got, k), getattr(plain, k)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, k)


@pytest.mark.parametrize("name", NR.SPHERES)
def test_extract_with_normals_is_extract_plus_vertex_normals(name):
    from scanerf_amd import meshing
    from test_gpu_tsdf_color import fused
    vol = fused(name)
    plain = vol.extract()
    assert plain.normals is None
    report = {}
    got = vol.extract(report=report, normals=True)
    assert isinstance(got, meshing.Mesh) and got.normals is not None and got.normals.shape == got.vertices.shape
    _same_geometry(got, plain, f"{name}: extract(normals=True) against extract()")
    for route in ("fused", "composed"):
        normal, grad = vol.vertex_normals(plain, route=route)      # values / observed computed by the call itself
        assert torch.equal(normal.view(torch.int32), got.normals.view(torch.int32)), route
    values, observed = vol.values(1)
    handed = vol.vertex_normals(plain, values=values, observed=observed)
    assert torch.equal(handed[0].view(torch.int32), got.normals.view(torch.int32)) and torch.equal(handed[1].view(torch.int32), grad.view(torch.int32))
    f = NR.field(name)
    want = NR.vertex_normals(f["values"], f["observed"], f["n"], f["spacing"], _np(plain.cells), _np(plain.lattice), np.float32)
    assert np.array_equal(_bits(_np(got.normals)), _bits(want["normal"])) and report["normals"] == 0
    # with colours the return stays (mesh, rgb), the mesh the same, the colours the same
    report2 = {}
    both, rgb = vol.extract(report=report2, colors=True, normals=True)
    only, rgb0 = vol.extract(colors=True)
    _same_geometry(both, plain, f"{name}: extract(colors=True, normals=True) against extract()")
    assert only.normals is None and torch.equal(both.normals.view(torch.int32), got.normals.view(torch.int32))
    assert torch.equal(rgb.view(torch.int32), rgb0.view(torch.int32)) and report2["normals"] == 0 and report2["color"] == 0
    # min_weight reaches the normals: observed is a different set
    heavy = vol.extract(min_weight=3, normals=True)
    if heavy.vertices.shape[0]:
        again = vol.vertex_normals(vol.extract(min_weight=3), min_weight=3)[0]
        assert torch.equal(heavy.normals.view(torch.int32), again.view(torch.int32))


def test_end_to_end_on_a_traced_icosphere_the_normals_point_outwards():
    from scanerf_amd import fusion
    from scanerf_amd.fastmesh import FastMesh
    c = TR.case("sphere40")
    V, F = _icosphere(TR.RADIUS, 3)
    fm = FastMesh.from_arrays(V, F, DEV)
    H, W = c["depths"].shape[1:]
    depths = _trace_depth(fm, c["ks"], c["c2ws"], H, W)
    kw = dict(trunc=TR.TRUNC, views_per_batch=7, near=TR.NEAR, far=TR.FAR)
    report = {}
    mesh = fusion.fuse_depth_maps(depths, c["ks"], c["c2ws"], c["origin"], [TR.BOX[1]] * 3, c["n"], report=report, normals=True, **kw)
    plain = fusion.fuse_depth_maps(depths, c["ks"], c["c2ws"], c["origin"], [TR.BOX[1]] * 3, c["n"], **kw)
    _same_geometry(mesh, plain, "fuse_depth_maps with normals against the call without")
    assert plain.normals is None and mesh.vertices.shape[0] > 100 and report["normals"] == 0
    v, nrm = _np(mesh.vertices).astype(np.float64), _np(mesh.normals)
    ang = NR.angles_deg(nrm, v)
    face = NR.angles_deg(NR.face_average_normals(v, _np(mesh.faces)), v)
    print(f"tsdf normals end to end: V {len(v)}, mean angle to the radial direction {ang.mean():.2f} deg, max {ang.max():.1f} (the reference mesh: "
          f"{NR.RADIAL_MEAN_DEG['sphere40']}); the face-normal average of the same mesh: {face.mean():.2f} deg")
    assert ang.mean() <= NR.RADIAL_MARGIN * NR.RADIAL_MEAN_DEG["sphere40"]
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() <= 1e-6


def _masked_renders(rnd, cams, scale, max_transparency):
    from scanerf_amd import fusion
    ks, c2ws, H, W = cams
    k2 = fusion.scale_cameras(ks, scale)
    maps, images = [], []
    for K, c2w in zip(k2, torch.as_tensor(c2ws)):
        diffuse, specular, depth, transp = rnd.render(H // scale, W // scale, K, c2w)
        maps.append(fusion.mask_depth(depth[..., 0], transp[..., 0], max_transparency))
        images.append(fusion.clamped_image(diffuse))
    return k2, torch.stack(maps).contiguous(), torch.stack(images).contiguous()


def test_fuse_mesh_with_normals_equals_fuse_depth_maps_on_its_renders(tile_scene):  # noqa: F811
    from scanerf_amd import fusion, meshing
    rnd, cams = tile_scene["rnd"], tile_scene["cameras"]
    kw = dict(cells_per_axis=20, max_transparency=0.9, scale=2, views_per_batch=2)
    report = {}
    mesh = rnd.fuse_mesh(cams, report=report, normals=True, **kw)
    plain = rnd.fuse_mesh(cams, **kw)
    assert isinstance(mesh, meshing.Mesh) and plain.normals is None and mesh.normals is not None
    _same_geometry(mesh, plain, "fuse_mesh with normals against fuse_mesh without")
    k2, maps, images = _masked_renders(rnd, cams, 2, 0.9)
    corner, size = rnd.scene_box()
    n = meshing.cells_per_axis(size, 20)
    want = fusion.fuse_depth_maps(maps, k2, cams[1], corner, size, n, views_per_batch=5, normals=True)
    _same_geometry(mesh, want, "fuse_mesh against fuse_depth_maps on the same masked renders")
    assert torch.equal(mesh.normals.view(torch.int32), want.normals.view(torch.int32))
    both, rgb = rnd.fuse_mesh(cams, colors="diffuse", normals=True, **kw)
    want2, rgb2 = fusion.fuse_depth_maps(maps, k2, cams[1], corner, size, n, views_per_batch=5, colors=images, normals=True)
    assert torch.equal(both.normals.view(torch.int32), mesh.normals.view(torch.int32)) and torch.equal(rgb.view(torch.int32), rgb2.view(torch.int32))
    assert torch.equal(want2.normals.view(torch.int32), mesh.normals.view(torch.int32))
    length = mesh.normals.double().norm(dim=1)
    print(f"tsdf normals tile fixture: V {mesh.vertices.shape[0]}, zero normals {report['normals']}, | |n| - 1 | max {float((length - 1).abs().max()):.2e}")
    assert mesh.vertices.shape[0] > 100 and report["normals"] == int((length == 0).sum()) and bool(torch.isfinite(mesh.normals).all())
    assert bool((length <= 1.0 + 1e-6).all())      # |n| = len / (len + 1e-8) <= 1 but for the roundings; how far below depends on len


def test_the_command_writes_normals_and_colours_into_one_ply(tile_scene, tmp_path, capsys):  # noqa: F811
    from scanerf_amd import formats
    from test_gpu_mesh_components import _tool
    out = str(tmp_path / "fused_normals.ply")
    head = [tile_scene["path"], "--cameras", tile_scene["log"], "--out", out, "--cells-per-axis", "20", "--scale", "2", "--max-transparency", "0.9",
            "--views-per-batch", "2"]
    assert _tool("fuse_mesh").main(head + ["--normals", "--colors", "diffuse"]) == 0
    want, rgb = tile_scene["rnd"].fuse_mesh(tile_scene["cameras"], cells_per_axis=20, max_transparency=0.9, scale=2, views_per_batch=2,
                                            colors="diffuse", normals=True)
    v, f, nrm, col = formats.read_ply(out, normals=True, colors=True)
    assert np.array_equal(np.asarray(v, np.float32).reshape(-1, 3), _np(want.vertices)) and np.array_equal(np.asarray(f, np.int32).reshape(-1, 3), _np(want.faces))
    assert np.array_equal(_bits(nrm), _bits(_np(want.normals))) and np.array_equal(col, formats.quantize_colors(_np(rgb)))
    printed = capsys.readouterr().out
    assert "normals:" in printed and "colours (diffuse)" in printed
    assert _tool("fuse_mesh").main(head + ["--normals"]) == 0
    v2, f2, nrm2 = formats.read_ply(out, normals=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(_bits(nrm2), _bits(nrm))
    with pytest.raises(ValueError, match="lacks one of"):
        formats.read_ply(out, colors=True)


# ---- normal consistency --------------------------------------------------------------------------------------------------------------------
def test_compare_meshes_normal_consistency_on_concentric_and_flipped_icospheres():
    from scanerf_amd import evaluation
    V, F = _icosphere(1.0, 3)
    a = (_dev(V), _dev(F))
    b = (_dev(_icosphere(1.05, 3)[0]), _dev(F))      # a concentric copy of another radius
    flipped = (a[0], a[1][:, [0, 2, 1]].contiguous())
    kw = dict(max_dist=0.5, seed=3, device=DEV)
    plain = evaluation.compare_meshes(a, b, 20000, (0.02, 0.1), **kw)
    got = evaluation.compare_meshes(a, b, 20000, (0.02, 0.1), normals=True, **kw)
    assert "normal_consistency" not in plain and set(got) == set(plain) | {"normal_consistency"}
    assert all(got[k] == plain[k] or (isinstance(plain[k], float) and math.isnan(plain[k])) for k in plain), "an existing key changed"
    nc = got["normal_consistency"]
    print(f"normal consistency concentric: {nc}")
    assert nc["pred_to_gt"]["mean"] > 0.99 and nc["gt_to_pred"]["mean"] > 0.99 and nc["mean"] == 0.5 * (nc["pred_to_gt"]["mean"] + nc["gt_to_pred"]["mean"])
    assert nc["pred_to_gt"]["skipped"] == 0.0 and nc["gt_to_pred"]["skipped"] == 0.0
    assert nc["pred_to_gt"]["mean_abs"] >= nc["pred_to_gt"]["mean"]
    inside_out = evaluation.compare_meshes(a, flipped, 20000, (0.02,), normals=True, **kw)["normal_consistency"]
    print(f"normal consistency against the flipped winding: {inside_out}")
    assert inside_out["pred_to_gt"]["mean"] < -0.99 and inside_out["gt_to_pred"]["mean"] < -0.99 and inside_out["mean"] < -0.99
    assert inside_out["pred_to_gt"]["mean_abs"] > 0.99
    # a cut that leaves nothing found: every sample skipped, the means NaN, the distances' keys as without the argument
    far = evaluation.compare_meshes(a, (_dev(_icosphere(3.0, 1)[0]), _dev(_icosphere(3.0, 1)[1])), 2000, (0.02,), max_dist=0.1, seed=3, device=DEV, normals=True)
    assert far["normal_consistency"]["pred_to_gt"]["skipped"] == 1.0 and math.isnan(far["normal_consistency"]["mean"])
    # with the distances returned: the same figures from the arrays by hand
    full = evaluation.compare_meshes(a, b, 20000, (0.02, 0.1), normals=True, return_distances=True, **kw)
    d = full["distances"]["pred_to_gt"]
    pn, pa = evaluation.face_normals(*a)
    gn, ga = evaluation.face_normals(*b)
    again = evaluation._consistency(d["dist"], d["sample_face"], d["face"], pn, pa, gn, ga)
    assert again == nc["pred_to_gt"] and full["normal_consistency"] == nc
