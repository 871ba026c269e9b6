"""The blended density's gradient without a GPU: the yardstick (tests/scene_normals_reference.py) checked on its own -- against a finite
difference of its float64 field, against the one-tile gradient, the conditions its EDGES claim, its float32 figures, its zeros -- and the
new surface: prototype, refusals, the mesh ops' arguments, normals in the PLY files."""
import inspect

import numpy as np
import pytest
import torch

import normals_reference as NR
import scene_mesh_reference as SM
import scene_normals_reference as R

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------- 1. finite difference
@pytest.mark.parametrize("name", ["G9", "STACK6"])
def test_gradient_matches_a_central_difference_of_the_float64_blended_field(name):
    """g against (v(p + h e_k) - v(p - h e_k)) / 2h of the float64 field with every selection pinned (membership, weight branch, sides,
    occupancy and hash cells; pt and the cell offsets move in float64), h = 1e-6 world units, at the random points whose cell offsets
    lie in (0.01, 0.99) at every level of every contributing tile and whose pt stays away from 0, 0.5 and 1 in every listed tile; the
    bound of test_normals_reference_cpu.py: 1e-6 of the conditioning scale.  And the field decreases along n there."""
    sc = SM.scene(name)
    p, r64, _ = R.random_reference(name)
    pin = R.pinned(sc, p)
    h, margin = 1e-6, 1e-4
    keep = r64["run"] > 0
    for t in pin["tiles"]:
        pt = t["pt"].astype(np.float64)
        away = np.all([np.abs(pt - q).min(1) > margin for q in (0.0, 0.5, 1.0)], axis=0)
        keep &= ~t["listed"] | away
        inside = np.ones(len(p), bool)
        inside[t["run"]] = np.all((t["t"] > 0.01) & (t["t"] < 0.99), axis=(1, 2))
        keep &= inside
    assert keep.sum() >= 64, keep.sum()
    sub = R.pinned(sc, p[keep])
    base = R.evaluate(sc, sub, np.float64)
    assert np.allclose(base["g"], r64["g"][keep], rtol=1e-9, atol=0)   # (the same points, evaluated in a batch of their own)
    fd = np.zeros_like(base["g"])
    for k in range(3):
        s = np.zeros_like(base["g"])
        s[:, k] = h
        fd[:, k] = (R.evaluate(sc, sub, np.float64, shift=s)["v"] - R.evaluate(sc, sub, np.float64, shift=-s)["v"]) / (2 * h)
    err = np.linalg.norm(base["g"] - fd, axis=1) / np.linalg.norm(base["cond"], axis=1)
    print(f"{name}: finite difference on {int(keep.sum())} points: max error over the conditioning scale {err.max():.2e}; "
          f"{int((base['listed'] > 1).sum())} of them in more than one tile")
    assert (base["listed"] > 1).sum() >= 16                  # the weight terms take part
    assert np.linalg.norm(base["g"], axis=1).min() > 0
    assert err.max() < 1e-6
    along = h * base["n"]
    dv = R.evaluate(sc, sub, np.float64, shift=along)["v"] - R.evaluate(sc, sub, np.float64, shift=-along)["v"]
    assert (dv < 0).all()


# ------------------------------------------------------------------------------------------------------------- 2. single-tile limit
def test_one_tile_gives_the_tile_densitys_own_gradient():
    """With one tile v = sigma and the weight terms cancel: g equals normals_reference.sigma_normals' g with A = 2 / size wherever
    w > 0, to 1e-12 of the scale."""
    sc = SM.scene("single")
    checked = 0
    for p, r64 in ((R.random_reference("single")[0], R.random_reference("single")[1]),
                   (R.lattice_reference(R.LATTICE_CASES[[c.scene for c in R.LATTICE_CASES].index("single")])[:2])):
        t = R.pinned(sc, p)["tiles"][0]
        A = (f32(2.0) / np.asarray(sc["sizes"], f32)[0]).astype(f32)
        sd = SM.O.unpack_blob(torch.from_numpy(np.asarray(sc["params"], f32)[0]))
        one = NR.sigma_normals(t["x"], A, torch.from_numpy(sc["tables"][0]), np.asarray(sc["res"], np.int32)[0], sd,
                               torch.ones(32), NR.F64)
        run = t["run"]
        pos = r64["W"][run] > 0
        assert pos.sum() >= 64
        err = np.linalg.norm(r64["g"][run] - one["g"].numpy(), axis=1)[pos] / np.linalg.norm(r64["cond"][run], axis=1)[pos]
        print(f"single: {int(pos.sum())} points, max |g - g_tile| over the scale {err.max():.2e}")
        assert err.max() < 1e-12
        assert np.abs(r64["v"][run][pos] - one["sigma"].numpy()[pos]).max() <= 1e-12 * one["sigma"].numpy()[pos].max()
        checked += int(pos.sum())
    assert checked >= 128


# ------------------------------------------------------------------------------------------------------------- 3. the EDGES
def test_every_edge_point_holds_the_condition_it_is_named_for():
    E = R.edges()
    assert len(E) == 10

    def at(name):
        scene, p = E[name]
        assert np.array_equal(p.astype(np.float64) * 8, np.round(p.astype(np.float64) * 8))   # dyadic: exact in float32
        pin = R.pinned(SM.scene(scene), p[None])
        listed = [b for b, t in enumerate(pin["tiles"]) if t["listed"][0]]
        run = [b for b, t in enumerate(pin["tiles"]) if t["run"][0]]
        return pin["tiles"], listed, run, R.evaluate(SM.scene(scene), pin, np.float64)

    t, listed, run, r = at("pt_x == 0.5 in a single tile")
    assert listed == [0] and run == [0] and t[0]["pt"][0, 0] == 0.5 and t[0]["side"][0, 0] == 0 and t[0]["branch"][0] == R.BOTH
    t, listed, run, r = at("interior face x == 3")
    assert listed == [0, 3] and 3 in run and t[3]["pt"][0, 0] == 0 and t[3]["branch"][0] == R.ONLY_Z and t[0]["branch"][0] == R.BOTH
    t, listed, run, r = at("two faces x == 3, z == 3")
    assert listed == [0, 1, 3, 4] and len(run) >= 1
    assert [int(t[b]["branch"][0]) for b in listed] == [R.BOTH, R.ONLY_X, R.ONLY_Z, R.NEITHER]
    t, listed, run, r = at("four-tile corner")
    assert listed == [0, 1, 3, 4] and all(t[b]["branch"][0] == R.BOTH for b in listed) and np.array_equal(E["four-tile corner"][1], [3.5, 0, 3.5])
    t, listed, run, r = at("outer edge x == 0, z == 0")
    assert listed == [0] and run == [0] and t[0]["branch"][0] == R.NEITHER and r["W"][0] == 0 and r["listed"][0] == 1
    assert np.all(r["g"] == 0) and r["v"][0] == 0
    t, listed, run, r = at("outside every tile")
    assert listed == [] and run == []
    t, listed, run, r = at("y outside [-2, 2]")
    assert listed == [] and abs(E["y outside [-2, 2]"][1][1]) > 2
    inside_xz = [b for b, tl in enumerate(t) if np.all((tl["pt"][0, [0, 2]] >= 0) & (tl["pt"][0, [0, 2]] <= 1))]
    assert inside_xz == [SM.CENTRE]                      # only y keeps it out
    for name, neighbour in (("hole: the centre lists, a neighbour contributes", 1), ("hole: a second one", 3)):
        t, listed, run, r = at(name)
        assert listed == sorted([neighbour, SM.CENTRE]) and run == [neighbour] and r["v"][0] > 0 and np.linalg.norm(r["g"]) > 0
        assert r["W"][0] > 0
    t, listed, run, r = at("listed, none contributes")
    assert len(listed) == 4 and run == [] and r["W"][0] > 0
    assert r["v"][0] == 0 and np.all(r["g"] == 0) and np.all(r["n"] == 0)


# ------------------------------------------------------------------------------------------------------------- 4. the yardstick
def test_float32_yardstick_is_at_float32_rounding():
    """The yardstick's own figures (over the conditioning scale) at the contributing points of every list, and the share of points
    whose unit normal is left unjudged: capped on the reference alone."""
    lists = [(SM.case_id(c),) + R.lattice_reference(c)[1:] for c in R.LATTICE_CASES]
    lists += [(f"{s}-random",) + R.random_reference(s)[1:] for s in R.SCENES]
    for name, r64, r32 in lists:
        m = r64["run"] > 0
        assert m.sum() >= 64, (name, m.sum())
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a[m].astype(np.float64)))
        g = NR.figures(T(r32["g"]), T(r64["g"]), T(r64["cond"]).norm(dim=1))
        share = R.left_out_share(r64, r32)
        j = R.normal_judged(r64, r32)
        Tj = lambda a: torch.from_numpy(np.ascontiguousarray(a[j].astype(np.float64)))
        n = NR.figures(Tj(r32["n"]), Tj(r64["n"]))
        print(f"{name}: {int(m.sum())} contributing of {len(m)}; f32 g median / p99 / max {g['median']:.2e} / {g['p99']:.2e} / {g['max']:.2e}; "
              f"n {n['median']:.2e} / {n['p99']:.2e} / {n['max']:.2e}; share without a judged normal {share:.4f}")
        assert 1e-9 < g["median"] < 1e-6 and g["max"] < 1e-5, (name, g)
        assert share <= R.N_CAP, (name, share)
        assert np.array_equal(r32["run"], r64["run"]) and np.array_equal(r32["listed"], r64["listed"])
    for s in ("G9", "G9-hole"):                # the EDGES, pooled with their scene's random points
        (_, _, e64, e32), (_, r64, r32) = R.edge_reference(s), R.random_reference(s)
        pool = lambda a, b, k: np.concatenate([a[k], b[k]])
        p64, p32 = ({k: pool(e, r, k) for k in ("g", "cond", "run")} for e, r in ((e64, r64), (e32, r32)))
        share = R.left_out_share(p64, p32)
        print(f"{s}: edges + random: share without a judged normal {share:.4f} (edges alone {R.left_out_share(e64, e32):.4f})")
        assert share <= R.N_CAP, (s, share)
    assert {c.scene for c in R.LATTICE_CASES} == set(R.SCENES)
    g65 = [c for c in R.LATTICE_CASES if c.scene == "G65"][0]
    assert g65.n == (19, 5, 45) and SM.scene("G65")["corners"].shape[0] == 65 and SM.scene("single")["corners"].shape[0] == 1
    assert R.lattice_reference(g65)[1]["listed"].max() == 4 and R.random_reference("STACK6")[1]["listed"].max() == 6


# ------------------------------------------------------------------------------------------------------------- 5. zeros
def test_points_without_a_contributing_tile_give_exact_zeros():
    seen = 0
    for s in R.SCENES:
        _, r64, r32 = R.random_reference(s)
        idle = r64["run"] == 0
        seen += int(idle.sum())
        for r in (r64, r32):
            for k in ("v", "g", "n", "cond"):
                assert not np.any(r[k][idle]), (s, k)
                assert not np.signbit(r[k][idle]).any(), (s, k)      # +0.0
        assert (r64["listed"][idle] > 0).any()                         # listed, W > 0, nothing contributes
        assert (r64["listed"][idle] == 0).any()                        # outside every tile
    assert seen >= 600


# ------------------------------------------------------------------------------------------------------------- 6. surface
NAME = "scanerf_scene_sigma_normals_points"


def test_the_prototype_agrees_with_the_header_and_the_library_exports_it():
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    from test_capi_cpu import _header_prototypes
    assert _header_prototypes()[NAME] == _capi.PROTOTYPES[NAME][:2] == ("I", "PPPPPPPPPIIPPPIP")
    assert _capi.PROTOTYPES[NAME][2] is _capi.REQ and hasattr(_capi.lib(), NAME)
    assert _capi.lib().scanerf_abi_version() == 10


def _call(ptrs=None, T=16, nb=2, N=5, **null):
    """Dummy non-null pointers that nothing dereferences: every case here is refused, or returns, before any launch."""
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    names = ["points", "tables", "blobs", "resolution", "occ", "grid_starts", "log2dim", "corners", "sizes", "sigma", "grad", "normal"]
    p = {k: (None if null.get(k) else 64) for k in names}
    lib = _capi.lib()
    rc = getattr(lib, NAME)(*[p[k] for k in names[:9]], T, nb, p["sigma"], p["grad"], p["normal"], N, None)
    return rc, lib.scanerf_last_error().decode()


def test_refusals_before_any_launch():
    for name in ("points", "tables", "blobs", "resolution", "occ", "grid_starts", "log2dim", "corners", "sizes", "sigma", "normal"):
        rc, msg = _call(**{name: True})
        assert rc != 0 and "scene_sigma_normals_points" in msg and "null pointer" in msg, (name, rc, msg)
    for kw, word in ((dict(N=-1), "N=-1"), (dict(nb=0), "nb=0"), (dict(nb=-3), "nb=-3"), (dict(T=0), "T=0"), (dict(T=1), "T=1"),
                     (dict(T=24), "T=24"), (dict(T=-16), "T=-16")):
        rc, msg = _call(**kw)
        assert rc != 0 and "scene_sigma_normals_points" in msg and word in msg, (kw, rc, msg)
    assert _call(N=0)[0] == 0                   # nothing to do: no launch
    assert _call(N=0, grad=True)[0] == 0        # grad may be null
    assert _call(N=0, nb=0)[0] != 0             # (an empty call is still checked)


def test_the_mesh_ops_take_normals():
    import scanerf_amd  # noqa
    from scanerf_amd import meshing, renderer
    for fn in (meshing.extract_scene_mesh, renderer.TileSetRenderer.extract_mesh):
        par = inspect.signature(fn).parameters
        assert par["normals"].default is False and par["route"].default == "fused"
    par = inspect.signature(meshing.scene_sigma_normals_points).parameters
    assert list(par)[:9] == ["points", "feature_tables", "resolutions", "blobs", "corners", "sizes", "occupied_grid", "grid_starts", "log2dim"]
    assert par["want_grad"].default is False and par["route"].default == "fused"
    with pytest.raises(RuntimeError, match="route"):
        meshing.scene_sigma_normals_points(torch.zeros(1, 3), *[None] * 8, route="eager")
    with pytest.raises(RuntimeError, match=r"\[N,3\]"):
        meshing.scene_sigma_normals_points(torch.zeros(3), *[None] * 8)
    with pytest.raises(RuntimeError, match="GPU"):                      # the shared checks: no CPU path
        meshing.scene_sigma_normals_points(torch.zeros(1, 3), torch.zeros(1, 16, 8, 2, dtype=torch.float16), *[None] * 7)


# ------------------------------------------------------------------------------------------------------------- 7. PLY
def _mesh():
    rng = np.random.default_rng(5)
    v = rng.normal(size=(7, 3)).astype(f32)
    n = rng.normal(size=(7, 3)).astype(f32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    fc = np.int32([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]])
    return v, n.astype(f32), fc


@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trips_normals(tmp_path, binary):
    import scanerf_amd  # noqa
    from scanerf_amd import formats
    v, n, fc = _mesh()
    path = str(tmp_path / "m.ply")
    formats.write_ply(path, v, fc, binary=binary, normals=n)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode()
    assert head.index("property float z") < head.index("property float nx") < head.index("property float ny") < head.index("property float nz") < head.index("element face")
    rv, rf, rn = formats.read_ply(path, normals=True)
    assert np.array_equal(rv, v) and np.array_equal(rf, fc) and np.array_equal(rn, n) and rn.dtype == np.float32
    two = formats.read_ply(path)
    assert len(two) == 2 and np.array_equal(two[0], v) and np.array_equal(two[1], fc)      # the default return is unchanged
    formats.write_ply(path, v[:0], fc[:0], binary=binary, normals=n[:0])                    # an empty mesh
    rv, rf, rn = formats.read_ply(path, normals=True)
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and rn.shape == (0, 3)
    formats.write_ply(path, v, fc, binary=binary)
    with pytest.raises(ValueError, match="nx"):
        formats.read_ply(path, normals=True)
    with pytest.raises(ValueError, match="normals"):
        formats.write_ply(path, v, fc, binary=binary, normals=n[:3])


def test_ply_without_normals_is_byte_identical_to_the_format(tmp_path):
    import scanerf_amd  # noqa
    from scanerf_amd import formats
    v, _, fc = _mesh()
    hdr = ("ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
           "element face %d\nproperty list uchar int vertex_indices\nend_header\n")
    path = str(tmp_path / "m.ply")
    formats.write_ply(path, v, fc)
    want = (hdr % ("binary_little_endian", 7, 4)).encode("ascii") + v.astype("<f4").tobytes()
    want += b"".join(b"\x03" + t.astype("<i4").tobytes() for t in fc)
    assert open(path, "rb").read() == want
    formats.write_ply(path, v, fc, binary=False)
    want = (hdr % ("ascii", 7, 4)).encode("ascii")
    want += "".join("%r %r %r\n" % tuple(float(x) for x in r) for r in v).encode("ascii")
    want += "".join("3 %d %d %d\n" % tuple(t) for t in fc).encode("ascii")
    assert open(path, "rb").read() == want
