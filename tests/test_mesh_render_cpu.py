"""The hit record and the rendered mesh, without a GPU: the numpy reference (tests/mesh_render_reference.py) against
known answers and hand-made tie rows, in float64 and in its float32 restatement; evaluation.compare_renders on hand arrays; the
refusals of the three entries and of the Python layer; the header, the prototypes and the commands' options; and the condition on
the inputs of tests/test_gpu_mesh_render.py (at most 1 % grazing rays in every camera grid it uses)."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import mesh_render_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("scanerf_mesh_trace", "scanerf_mesh_trace_brute", "scanerf_mesh_render_views")
f32, f64 = np.float32, np.float64
DTYPES = [f64, f32]
EPS = 2.0 ** -24          # float32 unit roundoff


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- known answers ------------------------------------------------------------------------------------------------------------------
HALF, N = 12.0, 8
SHELL_EYE = (1.3, -2.1, 0.7)


def _shell_view(H=20, W=28):
    """The shell seen from inside, and per pixel the closed-form answer in float64: depth along the float64 ray, the side, the
    quad and the triangle of the hit, and `clear`: the hit lies at least 1e-3 quads from every quad edge and diagonal."""
    V, F = R.shell_fixture(HALF, N)
    c2w, K = R.look_at(SHELL_EYE, (9.0, 4.0, 3.0), H, W, 0.6 * W)
    o, d = R.pixel_rays(K, c2w, H, W, f64)
    with np.errstate(divide="ignore"):
        t_axis = np.where(d > 0, (HALF - o) / d, np.where(d < 0, (-HALF - o) / d, np.inf))
    axis = t_axis.argmin(1)
    t = t_axis[np.arange(len(t_axis)), axis]
    p = o + t[:, None] * d
    side = (d[np.arange(len(d)), axis] > 0).astype(int)
    r = np.arange(len(p))
    a = (p[r, (axis + 1) % 3] + HALF) / (2 * HALF / N)
    b = (p[r, (axis + 2) % 3] + HALF) / (2 * HALF / N)
    i, j = np.floor(a).astype(int), np.floor(b).astype(int)
    s, q = a - i, b - j
    tri = (q > s).astype(int)            # triangle 0 = (0,0) (1,0) (1,1): s >= q
    face = (((axis * 2 + side) * N + i) * N + j) * 2 + tri
    clear = np.minimum.reduce([s, 1 - s, q, 1 - q, np.abs(s - q)]) > 1e-3
    return V, F, K, c2w, H, W, t, face.astype(np.int32), axis, clear


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_shell_seen_from_inside_has_closed_form_depth_and_known_faces(dtype):
    V, F, K, c2w, H, W, t, face, axis, clear = _shell_view()
    got = R.render(K[None], c2w[None], H, W, V, F, face_normals=True, dtype=dtype)
    assert got["depth"].dtype == dtype and got["face"].dtype == np.int32 and got["depth"].shape == (1, H, W)
    assert clear.mean() > 0.95 and len(set(axis.tolist())) >= 2                       # the view shows more than one side
    depth, fa = got["depth"].reshape(-1), got["face"].reshape(-1)
    assert (fa >= 0).all()                                                            # a closed shell: no miss
    assert np.array_equal(fa[clear], face[clear])
    # the float32 bound is test_gpu_fastmesh's parity bound; float64 has nothing to lose here
    assert np.all(np.abs(depth - t) <= (1e-4 if dtype is f32 else 1e-12) * t)
    # every side's two triangle normals are +axis as wound ((a, b) -> axis is cyclic), for the near and the far side alike
    want = np.zeros((len(fa), 3))
    want[np.arange(len(fa)), axis] = 1.0
    assert np.abs(got["normal"].reshape(-1, 3) - want)[clear].max() <= 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_nearest_hit_over_the_sloping_plane_is_the_boxes_top(dtype):
    V, F, (o, d), top = R.sloping_plane_fixture()
    t, face, u, v = R.nearest(o, d, V, F, dtype)
    assert set(face.tolist()) <= {4, 5} and len(set(face.tolist())) == 2             # 2 plane faces, then the cube's: 2, 3 = bottom; 4, 5 = top
    z = o[:, 2].astype(f64) + t.astype(f64) * d[:, 2].astype(f64)
    assert np.abs(z - top).max() <= 1e-4 * 4.0
    # the point A + u e1 + v e2 is the point o + t d
    A, E1, E2 = R.triangles(V, F, f64)
    P = A[face] + u[:, None].astype(f64) * E1[face] + v[:, None].astype(f64) * E2[face]
    assert np.abs(P - (o.astype(f64) + t[:, None].astype(f64) * d.astype(f64))).max() <= (1e-4 if dtype is f32 else 1e-12) * 4.0


def test_a_linear_attribute_comes_back_at_the_hit_point():
    """Barycentric interpolation reproduces linear functions: with a(p) = c . p + b on the vertices, the interpolated value at
    (u, v) is a(A + u e1 + v e2) exactly in real arithmetic.  float64: against c . (o + t d) + b, where the two points agree to
    float64 rounding (1e-9 M is generous).  float32: against a at the float64 point A + u e1 + v e2 of the SAME float32 (u, v), so that
    only the interpolation's own roundings count: w0 = (1 - u) - v is two roundings of values <= 1 (absolute 2 eps, times |a_A| <= M);
    three products with factors of magnitude <= 1 (3 eps M); two sums of partial results of magnitude <= M (2 eps M): 7 eps M, and
    the vertex attribute itself is rounded to float32 once (1 eps M): 8 eps M, eps = 2^-24, M = max |a| over the vertices."""
    V, F, sets = R.terrain_fixture()
    o, d = (x[:512] for x in sets["inside"])
    c, b = np.array([[0.3, -1.1, 0.7], [2.0, 0.25, -0.5], [0.0, 0.9, 1.3]]), np.array([0.5, -2.0, 4.0])
    attr = V.astype(f64) @ c.T + b                                                    # [V,3]: three linear functions
    M = np.abs(attr).max()
    A, E1, E2 = R.triangles(V, F, f64)
    for dtype in DTYPES:
        t, face, u, v = R.nearest(o, d, V, F, dtype)
        hit = face >= 0
        assert hit.sum() > 200 and (~hit).sum() > 50                                      # hits to judge, and misses to see zeroed
        got = R.interpolate(attr.astype(f32) if dtype is f32 else attr, F, face, u, v, dtype)
        if dtype is f64:
            P = o.astype(f64) + t[:, None] * d.astype(f64)
            bound = 1e-9 * M
        else:
            P = A[face] + u[:, None].astype(f64) * E1[face] + v[:, None].astype(f64) * E2[face]
            bound = 8 * EPS * M
        err = np.abs(got.astype(f64) - (P @ c.T + b))[hit]
        print(f"linear attribute ({dtype.__name__}): max error {err.max():.3e}, bound {bound:.3e}")
        assert err.max() <= bound
        assert not got[~hit].any()                                                    # a miss interpolates to 0


# ---- ties, by hand ------------------------------------------------------------------------------------------------------------------
SQUARE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], f32)
DOWN = (np.array([[0.5, 0.5, 1.0]], f32), np.array([[0.0, 0.0, -1.0]], f32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_ray_through_a_shared_edge_returns_the_lowest_index(dtype):
    for F in (np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([[0, 2, 3], [0, 1, 2]], np.int32)):
        t, face, u, v = R.nearest(*DOWN, SQUARE, F, dtype)                         # (0.5, 0.5) lies on the diagonal of both
        each = R.on_face(np.repeat(DOWN[0], 2, 0), np.repeat(DOWN[1], 2, 0), SQUARE, F, np.array([0, 1]), dtype)
        assert each[3].all() and each[0][0] == each[0][1] == 1.0                      # both faces are hit, at the same t
        assert (t[0], face[0]) == (1.0, 0)
        assert (u[0], v[0]) == (each[1][0], each[2][0])                               # the barycentrics are face 0's


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_ray_through_a_shared_vertex_returns_the_lowest_index(dtype):
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], f32)
    F = np.array([[0, 3, 4], [0, 1, 2], [0, 2, 3], [0, 4, 1]], np.int32)             # a fan around vertex 0
    o, d = np.array([[0.0, 0.0, 2.0]], f32), np.array([[0.0, 0.0, -1.0]], f32)
    t, face, u, v = R.nearest(o, d, V, F, dtype)
    assert (t[0], face[0], u[0], v[0]) == (2.0, 0, 0.0, 0.0)
    assert all(R.on_face(o, d, V, F, np.array([k]), dtype)[3][0] for k in range(4))    # every face of the fan is hit there


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_duplicated_face_returns_the_lower_index(dtype):
    F = np.array([[0, 1, 3], [0, 1, 2], [0, 1, 2]], np.int32)
    o, d = np.array([[0.75, 0.5, 3.0]], f32), np.array([[0.0, 0.0, -1.0]], f32)      # inside (0, 1, 2) only
    t, face, _, _ = R.nearest(o, d, SQUARE, F, dtype)
    assert (t[0], face[0]) == (3.0, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_back_facing_hit_is_accepted_with_the_normal_as_wound(dtype):
    F = np.array([[0, 1, 2]], np.int32)                                               # wound counter-clockwise seen from +z: n = +z
    o, d = np.array([[0.75, 0.25, -2.0]], f32), np.array([[0.0, 0.0, 1.0]], f32)     # from below
    t, face, _, _ = R.nearest(o, d, SQUARE, F, dtype)
    assert (t[0], face[0]) == (2.0, 0)
    n = R.unit(R.face_normal(SQUARE, F, face, dtype), dtype)
    assert n[0, 2] > 0.999 and float(n[0] @ d[0]) > 0                                 # the normal points along the ray: not flipped


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_dead_face_is_never_returned(dtype):
    V = np.concatenate([SQUARE, SQUARE - np.array([0, 0, 1], f32)])
    F = np.array([[0, 2, 2], [1, 1, 1], [4, 5, 6]], np.int32)                         # two faces without area in front of a live one
    o, d = np.array([[0.75, 0.25, 1.0]], f32), np.array([[0.0, 0.0, -1.0]], f32)
    t, face, _, _ = R.nearest(o, d, V, F, dtype)
    assert (t[0], face[0]) == (2.0, 2)
    t, face, u, v = R.nearest(o, d, V, F[:2], dtype)
    assert (t[0], face[0], u[0], v[0]) == (0.0, -1, 0.0, 0.0)                         # only dead faces: a miss, with the sentinels


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_ray_starting_on_a_face_answers_with_t_above_zero_only(dtype):
    V = np.concatenate([SQUARE, SQUARE - np.array([0, 0, 1], f32)])
    F = np.array([[0, 1, 2], [4, 5, 6]], np.int32)
    o, d = np.array([[0.75, 0.25, 0.0]], f32), np.array([[0.0, 0.0, -1.0]], f32)     # on face 0
    t, face, _, _ = R.nearest(o, d, V, F, dtype)
    assert (t[0], face[0]) == (1.0, 1)                                                # t = 0 is no hit: the face behind answers
    t, face, _, _ = R.nearest(o, -d, V, F, dtype)
    assert (t[0], face[0]) == (0.0, -1)


def test_the_pixel_ray_is_the_header_formula_and_the_two_precisions_agree():
    V, F, _ = R.terrain_fixture()
    Ks, Ms = R.terrain_cameras()
    for K, M in zip(Ks, Ms):
        o64, d64 = R.pixel_rays(K, M, 24, 32, f64)
        o32, d32 = R.pixel_rays(K, M, 24, 32, f32)
        assert o32.dtype == d32.dtype == f32 and np.array_equal(o32, o64.astype(f32))
        assert np.abs(d32 - d64).max() <= 8 * EPS * np.abs(d64).max()
        fo, fd = R.camera_rays(M, K, 24, 32)                                          # fastmesh_reference's rays: the same pixels
        assert np.abs(fd - d64).max() <= 8 * EPS * np.abs(d64).max() and np.array_equal(fo, o32)
        fwd = M[:, 2].astype(f64)
        assert np.abs(d64 @ fwd - 1.0).max() <= 1e-6                                  # camera-z component 1: t is z-depth


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
def test_at_most_one_percent_of_the_gpu_tests_rays_are_grazing():
    """A condition on the inputs, checked on the reference alone (DESIGN.md 4.10 measured 1 of 4 096 and 4 of 2 048 on the fixture's ray
    sets; test_fastmesh_cpu.py asserts the `inside` set): the camera grids test_gpu_mesh_render.py adds."""
    V, F, sets = R.terrain_fixture()
    Ks, Ms = R.terrain_cameras()
    for c, (K, M) in enumerate(zip(Ks, Ms)):
        o, d = R.pixel_rays(K, M, 24, 32, f32)
        share = R.grazing_rays(o, d, V, F).mean()
        print(f"terrain camera {c}: grazing share {share:.4f}")
        assert share <= 0.01, c
    for name in ("outside", "axial"):
        o, d = sets[name]
        assert R.grazing_rays(o, d, V, F).mean() <= 0.01, name


# ---- compare_renders ----------------------------------------------------------------------------------------------------------------
def _hand():
    nan, inf = float("nan"), float("inf")
    pred = {"depth": torch.tensor([[[1.0, 2.0, 0.0], [4.0, nan, 3.0]], [[0.0, 0.0, 0.0], [0.0, 5.0, 0.0]]])}
    targ = {"depth": torch.tensor([[[1.5, 0.0, 0.0], [2.0, 1.0, inf]], [[0.0, 0.0, 0.0], [0.0, 0.0, -1.0]]])}
    # view 0: P = {00, 01, 10, 12}, T = {00, 10, 11}; J = {00, 10}; E = 5.  view 1: P = {11}, T = {} (-1 covers nothing); J = {}
    pred["color"] = torch.zeros(2, 2, 3, 3)
    targ["color"] = torch.zeros(2, 2, 3, 3)
    pred["color"][0, 0, 0] = torch.tensor([0.2, 0.4, 0.6])
    targ["color"][0, 0, 0] = torch.tensor([0.4, 0.4, 0.2])
    pred["color"][0, 1, 0] = torch.tensor([1.0, 1.0, 1.0])
    targ["color"][0, 1, 0] = torch.tensor([1.0, 0.0, 1.0])
    pred["normal"] = torch.zeros(2, 2, 3, 3)
    targ["normal"] = torch.zeros(2, 2, 3, 3)
    pred["normal"][0, 0, 0] = torch.tensor([0.0, 0.0, 2.0])
    targ["normal"][0, 0, 0] = torch.tensor([0.0, 3.0, 0.0])                           # 90 degrees, any lengths
    pred["normal"][0, 1, 0] = torch.tensor([1.0, 0.0, 0.0])                           # target normal 0 there: not counted
    return pred, targ


def test_compare_renders_on_hand_arrays():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation, metrics
    pred, targ = _hand()
    r = evaluation.compare_renders(pred, targ)
    assert r["n_views"] == 2 and r["max_depth_diff"] is None and len(r["per_view"]) == 2
    v0, v1, pooled = r["per_view"][0], r["per_view"][1], r["pooled"]
    assert set(v0) == set(pooled) == {"coverage", "pred_only", "target_only", "depth_abs_mean", "depth_rmse", "psnr", "normal_deg_mean"}
    assert (v0["coverage"], v0["pred_only"], v0["target_only"]) == (2 / 5, 2 / 5, 1 / 5)
    assert v0["depth_abs_mean"] == pytest.approx((0.5 + 2.0) / 2) and v0["depth_rmse"] == pytest.approx(math.sqrt((0.25 + 4.0) / 2))
    sq = np.array([0.2, 0.0, 0.4, 0.0, 1.0, 0.0]) * 255.0
    assert v0["psnr"] == pytest.approx(10 * math.log10(255.0 ** 2 / ((sq ** 2).mean() + 1e-8)), rel=1e-6)
    assert v0["psnr"] == metrics.psnr(255.0 * torch.stack([pred["color"][0, 0, 0], pred["color"][0, 1, 0]]),
                                      255.0 * torch.stack([targ["color"][0, 0, 0], targ["color"][0, 1, 0]]))
    assert v0["normal_deg_mean"] == pytest.approx(90.0)
    # view 1: one render covers a pixel, nothing is jointly covered
    assert (v1["coverage"], v1["pred_only"], v1["target_only"]) == (0.0, 1.0, 0.0)
    assert all(math.isnan(v1[k]) for k in ("depth_abs_mean", "depth_rmse", "psnr", "normal_deg_mean"))
    # pooled: the pixels of both views together
    assert (pooled["coverage"], pooled["pred_only"], pooled["target_only"]) == (2 / 6, 3 / 6, 1 / 6)
    assert pooled["depth_abs_mean"] == pytest.approx(v0["depth_abs_mean"]) and pooled["psnr"] == pytest.approx(v0["psnr"], rel=1e-6)
    # max_depth_diff leaves the pixel whose depths differ by 2 out of the colours and normals, not out of the depth figures
    cut = evaluation.compare_renders(pred, targ, max_depth_diff=1.0)["per_view"][0]
    assert cut["depth_abs_mean"] == v0["depth_abs_mean"] and cut["coverage"] == v0["coverage"]
    assert cut["psnr"] == pytest.approx(10 * math.log10(255.0 ** 2 / ((sq[:3] ** 2).mean() + 1e-8)), rel=1e-6)
    # batch by batch gives the one-call figures
    acc = evaluation.RenderScore()
    for c in range(2):
        acc.add({k: v[c:c + 1] for k, v in pred.items()}, {k: v[c:c + 1] for k, v in targ.items()})
    assert evaluation.render_score_line(acc.result()) == evaluation.render_score_line(r)


def test_compare_renders_on_empty_sets_and_missing_maps():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import evaluation
    z = {"depth": torch.zeros(1, 2, 2)}
    r = evaluation.compare_renders(z, z)
    assert set(r["pooled"]) == {"coverage", "pred_only", "target_only", "depth_abs_mean", "depth_rmse"}      # no colour, no normals: no key
    assert all(math.isnan(v) for v in r["pooled"].values()) and all(math.isnan(v) for v in r["per_view"][0].values())
    none = evaluation.compare_renders({"depth": torch.zeros(0, 2, 2)}, {"depth": torch.zeros(0, 2, 2)})
    assert none["n_views"] == 0 and none["per_view"] == [] and math.isnan(none["pooled"]["coverage"])
    one = {"depth": torch.ones(1, 2, 2), "color": torch.zeros(1, 2, 2, 3)}
    assert "psnr" not in evaluation.compare_renders(one, {"depth": torch.ones(1, 2, 2)})["pooled"]           # colour on one side only
    same = evaluation.compare_renders(one, one)["pooled"]
    assert same["coverage"] == 1.0 and same["depth_rmse"] == 0.0 and same["psnr"] == pytest.approx(10 * math.log10(255.0 ** 2 / 1e-8))
    with pytest.raises(RuntimeError, match="depth"):
        evaluation.compare_renders({"depth": torch.zeros(1, 2, 2)}, {"depth": torch.zeros(1, 2, 3)})
    with pytest.raises(RuntimeError, match="color"):
        evaluation.compare_renders({"depth": torch.zeros(1, 2, 2), "color": torch.zeros(1, 2, 2)}, one)
    with pytest.raises(ValueError, match="max_depth_diff"):
        evaluation.compare_renders(z, z, max_depth_diff=-1.0)


# ---- the header, the prototypes, the entries' refusals ---------------------------------------------------------------------------------
def test_new_entries_match_the_second_header():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    from test_mesh_visibility_cpu import TOOLS_HEADER, _prototypes
    hdr = _prototypes(TOOLS_HEADER)
    for name in ENTRIES:
        assert name in hdr and name in _capi.TOOL_PROTOTYPES and tuple(_capi.TOOL_PROTOTYPES[name]) == hdr[name], name
        assert hdr[name][0] == "I" and hdr[name][1].endswith("P")
    trace, views = _capi.TOOL_PROTOTYPES[ENTRIES[0]][1], _capi.TOOL_PROTOTYPES[ENTRIES[2]][1]
    first_hit = _capi.PROTOTYPES["scanerf_mesh_first_hit"][1]
    assert trace[:12] == first_hit[:12] and trace[12:] == "PPPP"                      # first_hit's arguments up to log2dim, then t, face, bary
    assert views == "PPIII" + trace[3:12] + "PPPPPPP"                                 # cameras and size, the tracer's arrays, attributes, outputs
    text = open(TOOLS_HEADER).read()
    for words in ("AMONG THE FACES THE WALK TESTED", "w0 = (1 - u) - v", "A MISS gives t = 0, face = -1", "1e-8f", "8 x 8 pixel block",
                  "C H W >= 2^31"):
        assert words in text, words


def _refused(name, args, text):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    status = _capi.tool(name)(*args.values(), None)
    msg = _capi.lib().scanerf_last_error()
    assert status != 0 and text in msg, (name, text, msg)


def test_trace_entries_refuse_before_any_launch():
    """Placeholder pointers (never dereferenced on the host): every case here must be refused before any launch."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    grid = dict(rays_o=16, rays_d=16, B=4, vertices=16, faces=16, tris=None, bitmask=16, rank=16, start_num=16, cell_faces=16,
                scene_info=16, log2dim=6, t=16, face=16, bary=16)
    for over, text in (({"B": -1}, b"B=-1"), ({"B": 2 ** 29 + 1}, b"B="), ({"log2dim": 3}, b"log2dim=3"), ({"log2dim": 8}, b"log2dim=8"),
                       ({"rays_o": None}, b"null pointer"), ({"rays_d": None}, b"null pointer"), ({"scene_info": None}, b"null pointer"),
                       ({"t": None}, b"null pointer"), ({"face": None}, b"null pointer"), ({"bary": None}, b"null pointer"),
                       ({"bitmask": None}, b"null pointer"), ({"rank": None}, b"null pointer"), ({"start_num": None}, b"null pointer"),
                       ({"cell_faces": None}, b"null pointer"), ({"cell_faces": None, "tris": 16}, b"null pointer"),
                       ({"vertices": None}, b"neither triangles"), ({"faces": None}, b"neither triangles")):
        _refused(ENTRIES[0], dict(grid, **over), text)
    brute = dict(rays_o=16, rays_d=16, B=4, vertices=16, faces=16, V=4, F=2, scene_info=16, log2dim=6, t=16, face=16, bary=16)
    for over, text in (({"B": -1}, b"B=-1"), ({"log2dim": 9}, b"log2dim=9"), ({"V": -1}, b"V=-1"), ({"F": -1}, b"F=-1"),
                       ({"rays_o": None}, b"null pointer"), ({"rays_d": None}, b"null pointer"), ({"scene_info": None}, b"null pointer"),
                       ({"t": None}, b"null pointer"), ({"face": None}, b"null pointer"), ({"bary": None}, b"null pointer"),
                       ({"vertices": None}, b"null pointer"), ({"faces": None}, b"null pointer")):
        _refused(ENTRIES[1], dict(brute, **over), text)
    # B == 0 launches nothing, whatever else is passed
    assert _capi.tool(ENTRIES[0])(*dict(grid, B=0, rays_o=None).values(), None) == 0
    assert _capi.tool(ENTRIES[1])(*dict(brute, B=0, t=None).values(), None) == 0


def test_render_views_entry_refuses_before_any_launch():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    a = dict(Ks=16, C2Ws=16, C=2, H=4, W=4, vertices=16, faces=16, tris=None, bitmask=16, rank=16, start_num=16, cell_faces=16,
             scene_info=16, log2dim=6, vertex_normals=None, vertex_colors=None, depth=16, face=16, normal=None, color=None)
    for over, text in (({"C": -1}, b"C=-1"), ({"H": 0}, b"H=0"), ({"W": 0}, b"W=0"), ({"W": -3}, b"W=-3"),
                       ({"C": 2 ** 11, "H": 2 ** 10, "W": 2 ** 10}, b"does not fit 31 bits"),
                       ({"C": 1, "H": 2 ** 16, "W": 2 ** 15}, b"does not fit 31 bits"),
                       ({"log2dim": 3}, b"log2dim=3"), ({"log2dim": 8}, b"log2dim=8"),
                       ({"color": 16}, b"needs vertex_colors"), ({"color": 16, "vertex_normals": 16, "normal": 16}, b"needs vertex_colors"),
                       *(({k: None}, b"null pointer") for k in ("Ks", "C2Ws", "vertices", "faces", "bitmask", "rank", "start_num", "cell_faces",
                                                                "scene_info", "depth", "face")),
                       ({"C": 0, "depth": None}, b"null pointer"), ({"C": 0, "H": 0}, b"H=0")):      # C == 0 is still checked
        _refused(ENTRIES[2], dict(a, **over), text)
    assert _capi.tool(ENTRIES[2])(*dict(a, C=0).values(), None) == 0                  # C == 0 launches nothing
    assert _capi.tool(ENTRIES[2])(*dict(a, C=0, tris=16, vertex_normals=16, normal=16).values(), None) == 0


# ---- the Python refusals -----------------------------------------------------------------------------------------------------------
def _cpu_tracer():
    """A FastMesh whose arrays live on the CPU: enough for every check that comes before a library call."""
    from scanerf_amd.fastmesh import FastMesh
    fm = FastMesh.__new__(FastMesh)
    fm.vertices, fm.faces = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    fm.log2dim, fm.tris = 6, None
    return fm


def test_python_refusals_happen_before_any_library_call(monkeypatch):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi, evaluation

    def no_call(name):
        raise AssertionError(f"{name} was reached")
    monkeypatch.setattr(_capi, "tool", no_call)
    fm = _cpu_tracer()
    o = torch.zeros((5, 3))
    with pytest.raises(ValueError, match="route must be"):
        fm.trace(o, o, route="dense")
    for bad, text in ((np.zeros((5, 3), f32), "must be a torch.Tensor"), (o.double(), r"must be \[N,3\]"), (torch.zeros((5, 4)), r"must be \[N,3\]"),
                      (torch.zeros(15), r"must be \[N,3\]"), (torch.zeros((3, 5)).t(), "must be contiguous"), (o, "must live on the GPU")):
        with pytest.raises(RuntimeError, match=text):
            fm.trace(bad, o)
    with pytest.raises(RuntimeError, match=r"rays_d must be \[5,3\]"):
        fm.trace(o, torch.zeros((6, 3)))
    ks, c2ws = torch.eye(3)[None], torch.eye(4)[None, :3]
    with pytest.raises(ValueError, match="route must be"):
        fm.render_views(ks, c2ws, 4, 4, route="grid")
    with pytest.raises(ValueError, match="want_normals"):
        fm.render_views(ks, c2ws, 4, 4, want_normals=1)
    for H, W in ((0, 4), (4, -1), (2.5, 4), (True, 4)):
        with pytest.raises(ValueError, match="positive integer"):
            fm.render_views(ks, c2ws, H, W)
    for name in ("normals", "colors"):
        for bad, text in ((torch.zeros((5, 3)), rf"{name} must be \[4,3\]"), (torch.zeros((4, 3)).double(), rf"{name} must be \[4,3\]"),
                          (torch.zeros((3, 4)).t(), "must be contiguous"), (np.zeros((4, 3), f32), "must be a torch.Tensor"),
                          (torch.zeros((4, 3)), "must live on the GPU")):
            with pytest.raises(RuntimeError, match=text):
                fm.render_views(ks, c2ws, 4, 4, **{name: bad})
    with pytest.raises(RuntimeError, match="ks must be"):
        fm.render_views(torch.eye(3), c2ws, 4, 4)
    with pytest.raises(RuntimeError, match="c2ws must be"):
        fm.render_views(ks, torch.eye(4)[None, :2], 4, 4)
    with pytest.raises(ValueError, match="do not fit 31 bits"):
        fm.render_views(ks.expand(2 ** 11, 3, 3), c2ws.expand(2 ** 11, 3, 4), 2 ** 10, 2 ** 10)
    # the public routes check their own arguments first
    mesh = (torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="views_per_batch"):
        evaluation.render_mesh(mesh, (ks, c2ws, 4, 4), views_per_batch=0)
    with pytest.raises(RuntimeError, match="cameras="):
        evaluation.render_mesh(mesh, (ks, c2ws))
    with pytest.raises(RuntimeError, match=r"colors must be \[V,3\]"):
        evaluation.render_mesh(mesh, (ks, c2ws, 4, 4), colors=torch.zeros((5, 3)), device="cpu")
    with pytest.raises(RuntimeError, match=r"normals must be \[V,3\]"):
        evaluation.render_mesh(mesh, (ks, c2ws, 4, 4), normals=torch.zeros((4, 2)), device="cpu")


def test_fuse_mesh_and_score_mesh_check_their_new_arguments_first():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import renderer
    rnd = renderer.TileSetRenderer.__new__(renderer.TileSetRenderer)                  # no tiles: only the argument checks run
    with pytest.raises(RuntimeError, match="score must be True or False"):
        rnd.fuse_mesh(None, score=1)
    with pytest.raises(RuntimeError, match="pass report"):
        rnd.fuse_mesh(None, score=True)
    with pytest.raises(RuntimeError, match="which must be"):
        rnd.score_mesh(None, None, which="specular")
    with pytest.raises(RuntimeError, match="normals must be True or False"):
        rnd.score_mesh(None, None, normals=1)
    with pytest.raises(RuntimeError, match="cameras="):
        rnd.score_mesh(None, None)
    with pytest.raises(RuntimeError, match="leave no pixel"):
        rnd.score_mesh(None, (torch.eye(3)[None], torch.eye(4)[None, :3], 3, 8), scale=4)


# ---- the commands ------------------------------------------------------------------------------------------------------------------
def test_commands_take_the_new_options():
    args = _tool("render_mesh").parser().parse_args(["m.ply", "--cameras", "c.log", "--out", "dir"])
    assert (args.mesh, args.cameras, args.out, args.scale, args.log2dim, args.views_per_batch, args.gpu) == ("m.ply", "c.log", "dir", 1, 6, 8, 0)
    args = _tool("render_mesh").parser().parse_args(["m.ply", "--cameras", "c.log", "--out", "dir", "--scale", "4", "--log2dim", "7",
                                                     "--views-per-batch", "3"])
    assert (args.scale, args.log2dim, args.views_per_batch) == (4, 7, 3)
    for missing in (["m.ply", "--out", "dir"], ["m.ply", "--cameras", "c.log"], ["--cameras", "c.log", "--out", "dir"]):
        with pytest.raises(SystemExit):
            _tool("render_mesh").parser().parse_args(missing)
    fuse = _tool("fuse_mesh").parser()
    assert fuse.parse_args(["t", "--cameras", "c.log", "--out", "o.ply"]).render_score is False
    assert fuse.parse_args(["t", "--cameras", "c.log", "--out", "o.ply", "--render-score"]).render_score is True
