"""The product's HIP ops against the reference's own kernels, built for gfx950 from its CUDA sources by
oracle/build_ref.py into oracle/_ref/ (test infrastructure; loaded by path, the reference tree is never read here).

Each test builds one input set, clones it for each side, calls the reference op (`R`) and the product op under the same
binding name, and compares; it also compares the CPU oracle (oracle/scanerf_oracle.c) with the reference's output, which is
what pins the oracle's restatement of the `.cu` half.  Both sides and the oracle are built without mul+add contraction, so
ops the product claims bit-exact are asserted bit-exact against the reference too; ops whose reference kernel adds with float
atomics are held to the bound the op's existing parity test uses.  Needs an MI355X: `pytest -m gpu`.
"""
import numpy as np
import pytest
import torch

from oracle import build_ref
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ref(name):
    mod = build_ref.load(name)
    if mod is None:
        pytest.skip(f"oracle/_ref/{name}.so not built (oracle/build_ref.py needs the reference checkout)")
    return mod


@pytest.fixture(scope="module")
def RC():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    _capi.lib()
    return _ref("CUDA_EXT")


@pytest.fixture(scope="module")
def RH():
    import scanerf_amd  # noqa: F401
    return _ref("HASHGRID")


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def both(*ts):
    """(reference copy, product copy) of each device tensor."""
    return [t.clone() for t in ts], [t.clone() for t in ts]


def bits(t):
    a = t.detach().cpu().numpy()
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b, what):
    x, y = bits(a) if torch.is_tensor(a) else a, bits(b) if torch.is_tensor(b) else b
    if x.dtype.kind == "f":
        x = x.view({2: np.uint16, 4: np.uint32}[x.itemsize])
    if y.dtype.kind == "f":
        y = y.view({2: np.uint16, 4: np.uint32}[y.itemsize])
    n = int((x != y).sum())
    assert n == 0, f"{what}: {n} of {x.size} entries differ"


def worst(family, what, got, want):
    """Print the worst error of `got` against `want`: max |got - want| / max |want| (normwise, so small entries do not blow it
    up) and the largest elementwise relative error among entries with |want| >= 1e-3 * max |want|."""
    a = (got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).astype(np.float64)
    b = (want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)).astype(np.float64)
    top = np.abs(b).max() if b.size else 0.0
    e = np.abs(a - b)
    big = np.abs(b) >= 1e-3 * top
    elem = float((e[big] / np.abs(b[big])).max()) if big.any() else 0.0
    print(f"WORST {family} {what}: normwise {float(e.max()) / max(top, 1e-30) if b.size else 0.0:.2e} elementwise {elem:.2e}")


# ------------------------------------------------------------------ rays
def test_compute_ray_forward_backward_vs_reference(RC):
    """Forward bit-exact.  Backward: the reference's kernel reads the incoming gradients by VIEW index
    (compute_ray_kernel.cu:71-72), which the oracle reproduces with ref_bug=True; the product keeps the per-ray adjoint and is
    compared with ref_bug=False (deliberate)."""
    from scanerf_amd.cuda import compute_ray_backward, compute_ray_forward
    rng = np.random.default_rng(100)
    C, B, W, H = 5, 6000, 640, 480
    Ks = np.stack([np.float32([500 + 10 * c, 0, 320.3, 0, 510 - 5 * c, 239.6, 0, 0, 1]) for c in range(C)])
    M = rng.normal(size=(C, 12)).astype(np.float32)
    locs = np.stack([rng.integers(0, C, B), rng.integers(0, W, B), rng.integers(0, H, B)], 1).astype(np.int32)
    corners = np.int32([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]])
    for c in range(C):   # every view's four image corners
        locs[4 * c:4 * c + 4, 0], locs[4 * c:4 * c + 4, 1:] = c, corners
    o_ref, d_ref = O.compute_ray_forward(locs, Ks, M)
    (ro, rd), (po, pd) = both(torch.zeros(B, 3, device=DEV), torch.zeros(B, 3, device=DEV))
    RC.compute_ray_forward(ro, rd, g(Ks), g(M), g(locs))
    compute_ray_forward(po, pd, g(Ks), g(M), g(locs))
    same_bits(ro, po, "rays_o ref/product")
    same_bits(rd, pd, "rays_d ref/product")
    same_bits(ro, o_ref, "rays_o ref/oracle")
    same_bits(rd, d_ref, "rays_d ref/oracle")

    go, gd = rng.normal(size=(B, 3)).astype(np.float32), rng.normal(size=(B, 3)).astype(np.float32)
    (rg,), (pg,) = both(torch.zeros(C, 12, device=DEV))
    RC.compute_ray_backward(g(go), g(gd), g(Ks), rg, g(locs))
    compute_ray_backward(g(go), g(gd), g(Ks), pg, g(locs))
    want_ref, want_prod = (O.compute_ray_backward(go, gd, Ks, locs, C, ref_bug=True),
                           O.compute_ray_backward(go, gd, Ks, locs, C, ref_bug=False))
    np.testing.assert_allclose(rg.cpu().numpy(), want_ref, rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(pg.cpu().numpy(), want_prod, rtol=2e-4, atol=2e-3)
    worst("rays", "backward ref/oracle(ref_bug)", rg, want_ref)
    worst("rays", "backward product/oracle", pg, want_prod)
    assert not np.allclose(rg.cpu().numpy(), pg.cpu().numpy(), rtol=1e-2), "the two adjoints must differ on these inputs"


# ------------------------------------------------------------------ box / samplers
def _edge_rays(rng, corner, size, B):
    """rays with the edges of a slab test: axis-parallel (zero direction components), origins on faces and corners,
    grazing a face, missing the box, plus random rays from around the box"""
    corner, size = np.float32(corner), np.float32(size)
    hi = corner + size
    o = (corner + rng.uniform(-0.5, 1.5, (B, 3)) * size).astype(np.float32)
    d = rng.normal(size=(B, 3)).astype(np.float32)
    n = B // 10
    d[0:n, 1:] = 0.0                                   # x-parallel
    d[n:2 * n, 0] = 0.0                                # one zero component
    d[2 * n:3 * n, :2] = 0.0                           # z-parallel
    o[3 * n:4 * n, 0] = corner[0]                      # origin on the -x face
    o[4 * n:5 * n] = np.where(rng.random((n, 3)) < 0.5, corner, hi)   # origin on a box corner
    o[5 * n:6 * n, 1] = hi[1]                          # grazing the +y face: in the face plane, moving within it
    d[5 * n:6 * n, 1] = 0.0
    o[6 * n:7 * n] = hi + 5.0                          # misses: outside, moving away
    d[6 * n:7 * n] = np.abs(d[6 * n:7 * n])
    return o, d.astype(np.float32)


@pytest.mark.parametrize("center,size", [((0.5, -1, 2), (8, 6, 10)), ((0, 0, 0), (4, 4, 4))])
def test_ray_aabb_intersection_vs_reference(RC, center, size):
    from scanerf_amd.cuda import ray_aabb_intersection, ray_aabb_intersection_v2
    rng = np.random.default_rng(101)
    c, s = np.float32(center), np.float32(size)
    o, d = _edge_rays(rng, c - s / 2, s, 5003)
    (rb,), (pb,) = both(torch.full((o.shape[0], 2), -1.0, device=DEV))
    RC.ray_aabb_intersection(g(o), g(d), g(c), g(s), rb)
    ray_aabb_intersection(g(o), g(d), g(c), g(s), pb)
    same_bits(rb, pb, "bounds ref/product")
    same_bits(rb, O.ray_aabb_intersection(o, d, c, s), "bounds ref/oracle")
    r = rb.cpu().numpy()
    assert (r[:, 0] == -1).sum() > 100 and (r[:, 0] != -1).sum() > 1000
    cs = np.concatenate([c[None], rng.uniform(-5, 5, (5, 3))]).astype(np.float32)
    ss = np.concatenate([s[None], rng.uniform(2, 9, (5, 3))]).astype(np.float32)
    (rb2,), (pb2,) = both(torch.full((o.shape[0], 6, 2), -1.0, device=DEV))
    RC.ray_aabb_intersection_v2(g(o), g(d), g(cs), g(ss), rb2)
    ray_aabb_intersection_v2(g(o), g(d), g(cs), g(ss), pb2)
    same_bits(rb2, pb2, "bounds_v2 ref/product")
    same_bits(rb2, O.ray_aabb_intersection(o, d, cs, ss), "bounds_v2 ref/oracle")


@pytest.mark.parametrize("l2d,S_,fill", [((4, 4, 4), 64, 1.0), ((5, 4, 6), 100, 0.3), ((7, 7, 7), 128, 0.05),
                                         ((3, 3, 3), 7, 0.5), ((4, 4, 4), 32, 0.0), ((2, 6, 3), 48, 0.2)])
def test_sample_points_grid_vs_reference(RC, l2d, S_, fill):
    from scanerf_amd.cuda import sample_points_grid
    rng = np.random.default_rng(102)
    B = 4000
    corner, size = np.float32([-4, -3, -5]), np.float32([8, 6, 10])   # non-cubic box
    o, d = _edge_rays(rng, corner, size, B)
    occ = rng.random(tuple(2 ** k for k in l2d)) < fill
    (rz, rd), (pz, pd) = both(torch.full((B, S_), -1.0, device=DEV), torch.full((B, S_), -1.0, device=DEV))
    args = (g(corner), g(size), g(occ), g(np.int32(l2d)))
    RC.sample_points_grid(g(o), g(d), rz, rd, *args)
    sample_points_grid(g(o), g(d), pz, pd, *args)
    same_bits(rz, pz, "z_vals ref/product")
    same_bits(rd, pd, "dists ref/product")
    z_ref, d_ref = O.sample_points_grid(o, d, corner, size, occ, np.int32(l2d), S_)
    same_bits(rz, z_ref, "z_vals ref/oracle")
    same_bits(rd, d_ref, "dists ref/oracle")
    hits = (z_ref != -1).sum(1)
    if fill == 0.0:
        assert hits.max() == 0
    else:   # a ray that meets an occupied cell gets all S samples, split over its cells
        assert (hits > 0).sum() > B // 10 and set(np.unique(hits)) <= {0, S_}


def test_sample_insideout_block_and_background_sampling_vs_reference(RC):
    from scanerf_amd.cuda import background_sampling_cuda, sample_insideout_block
    rng = np.random.default_rng(103)
    B = 3001
    c, s = np.float32([0.5, -0.5, 1]), np.float32([4, 6, 3])   # non-cubic
    o = (c + rng.uniform(-0.5, 0.5, (B, 3)) * s).astype(np.float32)   # inside (the only use of the op)
    o[:50, 0] = c[0] + s[0] / 2                                        # on a face
    d = rng.normal(size=(B, 3)).astype(np.float32)
    d[50:100, 1:] = 0.0
    d[100:150, 0] = 0.0
    for S_, Sb in ((64, 32), (33, 7)):
        (rz, rzb), (pz, pzb) = both(torch.zeros(B, S_, device=DEV), torch.zeros(B, Sb, device=DEV))
        RC.sample_insideout_block(g(o), g(d), S_, Sb, g(c), g(s), 200.0, rz, rzb)
        sample_insideout_block(g(o), g(d), S_, Sb, g(c), g(s), 200.0, pz, pzb)
        same_bits(rz, pz, "z ref/product")
        same_bits(rzb, pzb, "z_bg ref/product")
        z_ref, zb_ref, missed = O.sample_insideout_block(o, d, S_, Sb, c, s, 200.0)
        assert missed == 0
        same_bits(rz, z_ref, "z ref/oracle")
        same_bits(rzb, zb_ref, "z_bg ref/oracle")
    st, bd = rng.uniform(0, 3, B).astype(np.float32), rng.uniform(1, 20, B).astype(np.float32)
    st[:10], bd[:10] = 0.0, st[:10]
    for S_, rng_ in ((48, 1.6), (5, 0.25)):
        (rz,), (pz,) = both(torch.zeros(B, S_, device=DEV))
        RC.background_sampling_cuda(g(o), g(d), g(st), g(bd), rz, S_, rng_)
        background_sampling_cuda(g(o), g(d), g(st), g(bd), pz, S_, rng_)
        same_bits(rz, pz, "bg z ref/product")
        same_bits(rz, O.background_sampling(st, bd, S_, rng_), "bg z ref/oracle")


# ------------------------------------------------------------------ encoder
def _lattice_points(rng, N, res, lo, hi, outside=True):
    """random points in [lo, hi] (per axis), a share of them moved onto lattice vertices of random levels, onto the box faces,
    and (outside=True) outside the box.  Both reference kernels map the domain onto res - 1 cells per axis
    (hashgrid_bg_kernel.cu:128, hashgrid_kernel.cu:132), so vertex i of a level sits at lo + i / (res - 1) * (hi - lo)."""
    lo, hi = np.float32(lo), np.float32(hi)
    p = (lo + rng.random((N, 3)) * (hi - lo)).astype(np.float32)
    n = N // 8
    lv = rng.integers(0, res.shape[0], n)
    cells = rng.integers(0, 1 << 20, (n, 3)) % res[lv]
    p[:n] = (lo + cells / (res[lv] - 1).astype(np.float32) * (hi - lo)).astype(np.float32)   # on level lattice vertices
    p[n:2 * n] = np.where(rng.random((n, 3)) < 0.5, lo, hi)                               # box faces / corners
    if outside:
        p[2 * n:3 * n] = (lo + rng.uniform(-0.2, 1.2, (n, 3)) * (hi - lo)).astype(np.float32)  # partly outside
    return p


ENC_CASES = [  # (L, log2 T, base res, finest res): non-cubic per-axis resolutions as G13 (PyHashGridBG) produces them
    (16, 10, (16, 16, 16), (256, 256, 256)),
    (8, 19, (32, 48, 24), (2048, 3072, 1536)),
    (16, 19, (32, 32, 32), (2048, 2048, 2048)),
    (2, 24, (512, 384, 640), (4096, 3072, 5120)),   # the 2^24 hash mask, two levels only (the table is 256 MB)
]


@pytest.mark.parametrize("in_domain", [True, False])
@pytest.mark.parametrize("L,log2_T,base,finest", ENC_CASES)
def test_embedding_bg_vs_reference(RH, L, log2_T, base, finest, in_domain):
    """Forward at 1e-5 relative; gradients at test_embedding_bg_backward's bounds against the oracle, on both sides.
    Regression (in_domain=False): points outside [-2, 2]^3, which the reference's kernel extrapolates, once got wrong table
    gradients from the binding's binned route (its records are defined for in-domain points only); they now take the atomic
    kernel."""
    from scanerf_amd.hashgrid import embedding_bg_backward_cuda, embedding_bg_forward_cuda
    rng = np.random.default_rng(104 + log2_T)
    T, N = 2 ** log2_T, 20011
    res = O.level_resolutions(torch.tensor(base), torch.tensor(finest), L).numpy()
    pts = _lattice_points(rng, N, res, (-2, -2, -2), (2, 2, 2), outside=not in_domain)
    feat = rng.standard_normal((L, T, 2), dtype=np.float32)
    feat *= 0.5
    F, P, RES = g(feat), g(pts), g(res)
    (ro,), (po,) = both(torch.zeros(N, L, 2, device=DEV))
    RH.embedding_bg_forward_cuda(P, ro, F, RES)
    embedding_bg_forward_cuda(P, po, F, RES)
    np.testing.assert_allclose(po.cpu().numpy(), ro.cpu().numpy(), rtol=1e-5, atol=2e-6, err_msg="forward product/ref")
    want = O.embedding_forward(pts, feat, res)
    np.testing.assert_allclose(ro.cpu().numpy(), want, rtol=1e-5, atol=2e-6, err_msg="forward ref/oracle")
    tag = f"encoder bg L{L} T2^{log2_T} {'in' if in_domain else 'out'}"
    worst(tag, "forward product/ref", po, ro)
    worst(tag, "forward ref/oracle", ro, want)
    if log2_T == 24:
        return   # the table gradient at 2^24 would need two more 256 MB tables per side; the mask is what this case pins
    gin = rng.normal(size=(N, L, 2)).astype(np.float32)
    (rgp, rgf), (pgp, pgf) = both(torch.zeros(N, 3, device=DEV), torch.zeros(L, T, 2, device=DEV))
    RH.embedding_bg_backward_cuda(P, g(gin), rgp, rgf, F, RES)
    gp_ref, gf_ref = O.embedding_backward(pts, gin, feat, res)
    embedding_bg_backward_cuda(P, g(gin), pgp, pgf, F, RES)
    # table gradients: float atomics on the reference, another order on the product -> the existing test's bound vs the oracle
    for name, got in (("ref", rgf), ("product", pgf)):
        np.testing.assert_allclose(got.cpu().numpy(), gf_ref, rtol=1e-3, atol=2e-4, err_msg=f"grad_features {name}/oracle")
    sc = np.abs(gp_ref).max()
    for name, got in (("ref", rgp), ("product", pgp)):
        np.testing.assert_allclose(got.cpu().numpy() / sc, gp_ref / sc, rtol=1e-4, atol=2e-6, err_msg=f"grad_points {name}/oracle")
    for name, a, b in (("grad_features", rgf, gf_ref), ("grad_points", rgp, gp_ref)):
        worst(tag, f"{name} ref/oracle", a, b)
    for name, a, b in (("grad_features", pgf, gf_ref), ("grad_points", pgp, gp_ref)):
        worst(tag, f"{name} product/oracle", a, b)


@pytest.mark.parametrize("L,log2_T", [(8, 10), (16, 19)])
def test_embedding_box_variant_vs_reference(RH, L, log2_T):
    from scanerf_amd.hashgrid import embedding_backward_cuda, embedding_forward_cuda
    rng = np.random.default_rng(105)
    T, N = 2 ** log2_T, 15013
    res = O.level_resolutions(torch.tensor([16, 24, 20]), torch.tensor([512, 768, 640]), L).numpy()
    corner, size = np.float32([-1, 0, 2]), np.float32([4, 6, 5])
    pts = _lattice_points(rng, N, res, corner, corner + size)   # partly outside: the box variant clamps
    feat = (rng.normal(size=(L, T, 2)) * 0.5).astype(np.float32)
    F, P, RES, Cn, Sz = g(feat), g(pts), g(res), g(corner), g(size)
    (ro,), (po,) = both(torch.zeros(N, L, 2, device=DEV))
    RH.embedding_forward_cuda(P, ro, F, Cn, Sz, RES)
    embedding_forward_cuda(P, po, F, Cn, Sz, RES)
    np.testing.assert_allclose(po.cpu().numpy(), ro.cpu().numpy(), rtol=1e-5, atol=2e-6, err_msg="forward product/ref")
    np.testing.assert_allclose(ro.cpu().numpy(), O.embedding_forward(pts, feat, res, corner, size), rtol=1e-5, atol=2e-6,
                               err_msg="forward ref/oracle")
    gin = rng.normal(size=(N, L, 2)).astype(np.float32)
    (rgp, rgf), (pgp, pgf) = both(torch.zeros(N, 3, device=DEV), torch.zeros(L, T, 2, device=DEV))
    RH.embedding_backward_cuda(P, g(gin), rgp, rgf, F, Cn, Sz, RES)
    embedding_backward_cuda(P, g(gin), pgp, pgf, F, Cn, Sz, RES)
    gp_ref, gf_ref = O.embedding_backward(pts, gin, feat, res, corner, size)
    for name, got in (("ref", rgf), ("product", pgf)):
        np.testing.assert_allclose(got.cpu().numpy(), gf_ref, rtol=1e-3, atol=2e-4, err_msg=f"grad_features {name}/oracle")
    sc = np.abs(gp_ref).max()
    for name, got in (("ref", rgp), ("product", pgp)):
        np.testing.assert_allclose(got.cpu().numpy() / sc, gp_ref / sc, rtol=1e-4, atol=2e-6, err_msg=f"grad_points {name}/oracle")


# ------------------------------------------------------------------ Adam
@pytest.mark.parametrize("K", [1, 255, 4099])
@pytest.mark.parametrize("fp16", [False, True])
def test_sparse_adam_vs_reference(RC, K, fp16):
    """Bit-exact.  Zero-gradient entries keep params and moments; `step` is the previous count on both sides (the reference's
    `int &step` increment is invisible to the caller); fp16 moments near overflow and in the subnormal range."""
    from scanerf_amd.cuda import adam_step_cuda, adam_step_cuda_fp16
    rng = np.random.default_rng(106)
    p = rng.normal(size=(K, 8)).astype(np.float32)
    gr = (rng.normal(size=(K, 8)) * 1e-3).astype(np.float32)
    gr[rng.random((K, 8)) < 0.6] = 0.0
    mdt = np.float16 if fp16 else np.float32
    m = (rng.normal(size=(K, 8)) * 1e-2).astype(mdt)
    v = (np.abs(rng.normal(size=(K, 8))) * 1e-3).astype(mdt)
    if fp16:
        hot = rng.random((K, 8)) < 0.1
        gr[hot] = np.float32(rng.choice([-1.0, 1.0], hot.sum()) * 3.5)       # 128 * g near the f16 range, g^2 * 128 past it
        m[hot] = np.float16(6.0e4)
        tiny = (rng.random((K, 8)) < 0.1) & ~hot
        gr[tiny] = np.float32(1e-7)                                          # moments land in the f16 subnormal range
        v[tiny] = np.float16(3e-7)
    (rP, rM, rV), (pP, pM, pV) = both(g(p), g(m), g(v))
    pr, mr, vr = p.copy(), m.copy(), v.copy()
    G = g(gr)
    for step in (0, 1, 7, 1000):
        (RC.adam_step_cuda_fp16 if fp16 else RC.adam_step_cuda)(rP, G, rM, rV, 1e-3, 0.9, 0.99, 1e-15, step)
        (adam_step_cuda_fp16 if fp16 else adam_step_cuda)(pP, G, pM, pV, 1e-3, 0.9, 0.99, 1e-15, step)
        O.adam_step(pr, gr, mr.view(np.uint16) if fp16 else mr, vr.view(np.uint16) if fp16 else vr, 1e-3, 0.9, 0.99,
                    1e-15, step, fp16=fp16)
        for name, a, b, c in (("params", rP, pP, pr), ("exp_avg", rM, pM, mr), ("exp_avg_sq", rV, pV, vr)):
            same_bits(a, b, f"{name} ref/product step {step}")
            same_bits(a, c, f"{name} ref/oracle step {step}")
    untouched = gr == 0
    assert np.array_equal(rP.cpu().numpy()[untouched], p[untouched])


# ------------------------------------------------------------------ render-time
def _scene(rng, T=2 ** 10):
    corners = np.float32([[-4, -2, -2], [-1, -2, -2], [2, -2, -2]])
    sizes = np.float32([[4, 4, 4], [4, 4, 4], [4, 4, 4]])
    l2d = np.int32([[3, 3, 3], [4, 3, 3], [3, 3, 3]])
    grids = [rng.random(tuple(2 ** k for k in l)) < 0.35 for l in l2d]
    starts = np.cumsum([0] + [gr.size for gr in grids[:-1]]).astype(np.int64)
    occ = np.concatenate([gr.reshape(-1) for gr in grids])
    tables = (rng.normal(size=(3, 16, T, 2)) * 0.6).astype(np.float16)
    params = []
    for b in range(3):
        sd = O.init_mlp(seed=20 + b, bias_scale=0.05)
        sd["sigma_layer.mlp.0.bias"] = sd["sigma_layer.mlp.0.bias"] + 4.0
        params.append(O.pack_blob(sd).numpy())
    res1 = O.level_resolutions(torch.tensor([32, 32, 32]), torch.tensor([2048, 2048, 2048])).numpy()
    return dict(corners=corners, sizes=sizes, l2d=l2d, starts=starts, occ=occ, tables=tables, params=np.stack(params),
                res=np.stack([res1] * 3).astype(np.int32))


def _rays(rng, B):
    o = np.stack([rng.uniform(-9, -5, B), rng.uniform(-1.5, 1.5, B), rng.uniform(-1.5, 1.5, B)], 1).astype(np.float32)
    d = np.stack([np.ones(B), rng.normal(0, 0.12, B), rng.normal(0, 0.12, B)], 1).astype(np.float32)
    d *= rng.uniform(0.7, 1.3, (B, 1)).astype(np.float32)
    o[: B // 8] = [0.5, 0.2, -0.3]       # cameras inside tile 1
    o[B // 8: B // 6] = [-20, 30, 0]     # rays that miss everything
    d[B // 6: B // 5, 1:] = 0.0          # axis-parallel rays
    return o, d.astype(np.float32)


# per INFER_ARITH, against the reference's scalar f32 decoder (another summation order, other exp / log), with atol 2e-6:
# measured worst normwise error 3.1e-6 for each of t16 / h3 / f32 (the f32 kernel's products are exact, its sums and
# activations are not the reference's), and no entry needs more than rtol 2e-5 + atol 2e-6
INFER_BOUNDS = {"t16": 2e-5, "h3": 2e-5, "f32": 2e-5}


def _np(t):
    return t.detach().cpu().numpy()


# (the three-tile cases keep the ids they had: [t16], [h3], [f32])
@pytest.mark.parametrize("arith,scene", [pytest.param(a, s, id=a if s == "row3" else f"{a}-{s}")
                                         for s in ("row3", "G36") for a in ("t16", "h3", "f32")])
def test_render_loop_stage_by_stage_vs_reference(RH, arith, scene, monkeypatch):
    """rendering.py's novel-view loop driven through both HASHGRID modules stage by stage on the same inputs, and the oracle's
    restatement of each stage on the reference's inputs: integer and sampler outputs bit-exact (all three), inference at the
    bound of the product's INFER_ARITH against the reference's own decoder, the oracle's decoder at 1e-4 (its parity bound).
    On three tiles in a row, and on G36 (tests/render_scenes.py): a 6 x 6 grid whose samples list up to four tiles, tiles
    from 32 on among them, and whose rays leave up to four tiles at one distance -- never more, so the reference's unchecked
    fifth entry is not written (the stacked scenes are NOT for the reference's kernels)."""
    from scanerf_amd import hashgrid as H
    from scanerf_amd.hashgrid.lib import HASHGRID as HL
    monkeypatch.setattr(HL, "INFER_ARITH", arith)
    tol = INFER_BOUNDS[arith]
    if scene == "row3":
        rng = np.random.default_rng(107)
        sc = _scene(rng)
        B, S, nb, n_bg = 700, 64, 3, 2
        o, d = _rays(rng, B)
    else:
        import render_scenes as RS
        sc, rays = RS.named(scene)
        o, d = rays["shuffled"]
        B, S, nb, n_bg = o.shape[0], 32, sc["corners"].shape[0], 4
    cn, sz, occ, st, l2 = sc["corners"], sc["sizes"], sc["occ"], sc["starts"], sc["l2d"]
    tabs, par, res = sc["tables"], sc["params"], sc["res"]
    C, Z, OCC, ST, L2 = g(cn), g(sz), g(occ), g(st), g(l2)
    RO, RD, TAB, PAR, RES = g(o), g(d), g(tabs), g(par), g(res)

    def infer(name, prod, ref, orc):
        np.testing.assert_allclose(_np(prod), _np(ref), rtol=tol, atol=2e-6, err_msg=f"{name} product/ref ({arith})")
        np.testing.assert_allclose(_np(ref), orc, rtol=1e-4, atol=2e-6, err_msg=f"{name} ref/oracle")
        worst(f"render-time {arith}", f"{name} product/ref", prod, ref)
        worst("render-time", f"{name} ref/oracle", ref, orc)

    (ri,), (pi,) = both(torch.full((B, nb, 2), 1e7, device=DEV))
    RH.ray_block_intersection(RO, RD, C, Z, ri)
    H.ray_block_intersection(RO, RD, C, Z, pi)
    same_bits(ri, pi, "intersections")
    inter = O.ray_block_intersection(o, d, cn, sz)
    same_bits(ri, inter, "intersections ref/oracle")
    TB = torch.argsort(ri[..., 0], dim=-1, stable=True).int().contiguous()
    tb = _np(TB)
    max_tracing = int((inter != 1e7).astype(np.float32).mean(-1).sum(-1).max())
    assert max_tracing == 3 if scene == "row3" else max_tracing >= 4

    (rl,), (pl,) = both(torch.full((B,), -1, dtype=torch.int32, device=DEV))
    RH.get_last_block(TB, rl, ri)
    H.get_last_block(TB, pl, pi)
    same_bits(rl, pl, "get_last_block")
    same_bits(rl, O.get_last_block(tb, inter), "get_last_block ref/oracle")
    (rh,), (ph,) = both(torch.full((B,), -1, dtype=torch.int16, device=DEV))
    RH.ray_firsthit_block(RO, RD, C, Z, OCC, ST, L2, TB, ri, rh)
    H.ray_firsthit_block(RO, RD, C, Z, OCC, ST, L2, TB, pi, ph)
    same_bits(rh, ph, "ray_firsthit_block")
    same_bits(rh, O.ray_firsthit_block(o, d, cn, sz, occ, st, l2, tb, inter), "ray_firsthit_block ref/oracle")

    (rTI, rZS, rTR, rDI, rSP, rDE), (pTI, pZS, pTR, pDI, pSP, pDE) = both(
        torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, device=DEV), torch.ones(B, 1, device=DEV),
        torch.zeros(B, 3, device=DEV), torch.zeros(B, 3, device=DEV), torch.zeros(B, 1, device=DEV))
    n_overlap = 0
    for step in range(max_tracing):
        running = ((rTI < max_tracing) & (rTR[:, 0] > 1e-5)).contiguous()
        ti, zs = _np(rTI).copy(), _np(rZS).copy()   # the oracle advances its own copy of the ray state
        (rz, rdd), (pz, pdd) = both(torch.full((B, S), -1.0, device=DEV), torch.full((B, S), -1.0, device=DEV))
        RH.sample_points(RO, RD, C, Z, OCC, ST, L2, TB, ri, rTI, rZS, rz, rdd)
        H.sample_points(RO, RD, C, Z, OCC, ST, L2, TB, pi, pTI, pZS, pz, pdd)
        z_o, d_o = O.render_sample_points(o, d, cn, sz, occ, st, l2, S, tb, inter, ti, zs)
        for name, a, b, c in (("z_vals", rz, pz, z_o), ("dists", rdd, pdd, d_o), ("tracing_idx", rTI, pTI, ti),
                              ("z_start", rZS, pZS, zs)):
            same_bits(a, b, f"sample_points {name} step {step}")
            same_bits(a, c, f"sample_points {name} ref/oracle step {step}")
        (rbi,), (pbi,) = both(torch.full((B, S, 4), -1, dtype=torch.int16, device=DEV))
        RH.prepare_points(rz, running, ri, rbi)
        H.prepare_points(pz, running, pi, pbi)
        same_bits(rbi, pbi, f"prepare_points step {step}")
        bi = O.prepare_points(_np(rz), _np(running), inter)
        same_bits(rbi, bi, f"prepare_points ref/oracle step {step}")
        n_overlap += int((bi[..., 1] != -1).sum())
        (rd_, rs_, ra_), (pd_, ps_, pa_) = both(torch.zeros(B, S, 3, device=DEV), torch.zeros(B, S, 3, device=DEV),
                                                torch.zeros(B, S, 1, device=DEV))
        RH.pts_inference(RO, RD, rz, rdd, rbi, TAB, PAR, RES, OCC, ST, L2, C, Z, rd_, rs_, ra_)
        H.pts_inference(RO, RD, pz, pdd, pbi, TAB, PAR, RES, OCC, ST, L2, C, Z, pd_, ps_, pa_)
        od, os_, oa = O.pts_inference(o, d, _np(rz), _np(rdd), bi, tabs, par, res, occ, st, l2, cn, sz)
        infer("alpha", pa_, ra_, oa)
        infer("diffuse", pd_, rd_, od)
        infer("specular", ps_, rs_, os_)
        # both sides accumulate the reference's per-sample values, so the compositing op is compared on its own
        acc = [_np(t).copy() for t in (rTR, rDI, rSP, rDE)]
        RH.accumulate_color(rd_, rs_, ra_, rTR, rz, rDI, rSP, rDE)
        H.accumulate_color(rd_, rs_, ra_, pTR, pz, pDI, pSP, pDE)
        O.accumulate_color(_np(rd_), _np(rs_), _np(ra_), acc[0], _np(rz), acc[1], acc[2], acc[3])
        for name, a, b, c in zip(("transparency", "diffuse", "specular", "depth"), (rTR, rDI, rSP, rDE), (pTR, pDI, pSP, pDE), acc):
            np.testing.assert_allclose(_np(b), _np(a), rtol=1e-5, atol=1e-7, err_msg=f"accumulate {name}")
            np.testing.assert_allclose(_np(a), c, rtol=1e-5, atol=1e-7, err_msg=f"accumulate {name} ref/oracle")
    assert n_overlap > 100, "the scene must exercise multi-tile blending"
    assert float(rTR.min()) < 0.5

    (rob, rbw), (pob, pbw) = both(torch.full((B, 4), -1, dtype=torch.int16, device=DEV), torch.zeros(B, 4, device=DEV))
    RH.update_outgoing_bidx(RO, RD, C, Z, TB, ri, rob, rbw, 0.12, False)
    H.update_outgoing_bidx(RO, RD, C, Z, TB, pi, pob, pbw, 0.12, False)
    ob, bw = O.update_outgoing_bidx(o, d, cn, sz, tb, inter, 0.12, False)
    for name, a, b, c in (("bidx", rob, pob, ob), ("weights", rbw, pbw, bw)):
        same_bits(a, b, f"update_outgoing_bidx {name}")
        same_bits(a, c, f"update_outgoing_bidx {name} ref/oracle")
    (rob2, rbw2), (pob2, pbw2) = both(torch.full((B, 4), -1, dtype=torch.int16, device=DEV), torch.zeros(B, 4, device=DEV))
    RH.update_outgoing_bidx_v2(RO, RD, C, Z, TB, ri, rob2, rbw2)
    H.update_outgoing_bidx_v2(RO, RD, C, Z, TB, pi, pob2, pbw2)
    ob2, bw2 = O.update_outgoing_bidx_v2(o, cn, sz)
    for name, a, b, c in (("bidx", rob2, pob2, ob2), ("weights", rbw2, pbw2, bw2)):
        same_bits(a, b, f"update_outgoing_bidx_v2 {name}")
        same_bits(a, c, f"update_outgoing_bidx_v2 {name} ref/oracle")
    assert scene == "row3" or ((ob[:, 3] != -1).sum() >= 5 and ob.max() >= 32)
    Sb = 48 if scene == "row3" else 16
    for i in range(n_bg):
        (rzb,), (pzb,) = both(torch.full((B, Sb), -1.0, device=DEV))
        RH.inverse_z_sampling(ri, rob[:, i].contiguous(), rzb, 1e6)
        H.inverse_z_sampling(pi, pob[:, i].contiguous(), pzb, 1e6)
        same_bits(rzb, pzb, f"inverse_z_sampling slot {i}")
        same_bits(rzb, O.render_inverse_z_sampling(inter, ob[:, i], Sb, 1e6), f"inverse_z_sampling slot {i} ref/oracle")
        (rd_, rs_, ra_), (pd_, ps_, pa_) = both(torch.zeros(B, Sb, 3, device=DEV), torch.zeros(B, Sb, 3, device=DEV),
                                                torch.zeros(B, Sb, 1, device=DEV))
        RH.bg_pts_inference_v2(RO, RD, rzb, rob, i, C, Z, RES, TAB, PAR, rd_, rs_, ra_)
        H.bg_pts_inference_v2(RO, RD, pzb, pob, i, C, Z, RES, TAB, PAR, pd_, ps_, pa_)
        od, os_, oa = O.bg_pts_inference_v2(o, d, _np(rzb), ob, i, cn, sz, res, tabs, par)
        infer("bg alpha", pa_, ra_, oa)
        infer("bg diffuse", pd_, rd_, od)
        infer("bg specular", ps_, rs_, os_)
    zb = torch.full((B, Sb), -1.0, device=DEV)
    RH.inverse_z_sampling(ri, rob[:, 0].contiguous(), zb, 1e6)
    bw1 = (rbw.abs() + 0.1).contiguous()
    (rd_, rs_, ra_), (pd_, ps_, pa_) = both(torch.zeros(B, Sb, 3, device=DEV), torch.zeros(B, Sb, 3, device=DEV),
                                            torch.zeros(B, Sb, 1, device=DEV))
    RH.bg_pts_inference(RO, RD, zb, rob, bw1, C, Z, RES, TAB, PAR, rd_, rs_, ra_)
    H.bg_pts_inference(RO, RD, zb, rob, bw1, C, Z, RES, TAB, PAR, pd_, ps_, pa_)
    od, os_, oa = O.bg_pts_inference(o, d, _np(zb), ob, _np(bw1), cn, sz, res, tabs, par)
    infer("bg_v1 alpha", pa_, ra_, oa)
    infer("bg_v1 diffuse", pd_, rd_, od)
    infer("bg_v1 specular", ps_, rs_, os_)


def test_process_occupied_grid_vs_reference(RH):
    from scanerf_amd import hashgrid as H
    rng = np.random.default_rng(108)
    sc = _scene(rng)
    C, Z, OCC, ST, L2 = g(sc["corners"]), g(sc["sizes"]), g(sc["occ"]), g(sc["starts"]), g(sc["l2d"])
    (rt,), (pt,) = both(OCC.clone())
    ot = sc["occ"].astype(np.uint8).copy()
    for b in range(3):
        total = int(np.prod(2 ** sc["l2d"][b]))
        RH.process_occupied_grid(b, total, C, Z, OCC, ST, L2, rt)
        H.process_occupied_grid(b, total, C, Z, OCC, ST, L2, pt)
        O.process_occupied_grid(b, total, sc["corners"], sc["sizes"], sc["occ"], sc["starts"], sc["l2d"], ot)
    same_bits(rt, pt, "process_occupied_grid")
    same_bits(_np(rt).astype(np.uint8), ot, "process_occupied_grid ref/oracle")
    assert int(rt.sum()) > int(OCC.sum())


def test_sort_by_key_vs_reference(RH):
    """thrust sort_by_key + unique_by_key: the reference's sort is not stable, so values are compared as sets per key; unique
    keys and run starts against numpy (the oracle has no restatement of this host-side op)."""
    from scanerf_amd import hashgrid as H
    rng = np.random.default_rng(109)
    n = 5000
    keys = torch.as_tensor(rng.integers(0, 37, n).astype(np.int16)).to(DEV)
    vals = torch.arange(n, dtype=torch.int32, device=DEV)
    (rk, rv, rs), (pk, pv, ps) = both(keys, vals, torch.arange(n, dtype=torch.int32, device=DEV))
    nr = RH.sort_by_key(rk, rv, rs)
    npd = H.sort_by_key(pk, pv, ps)
    uk, first = np.unique(np.sort(_np(keys), kind="stable"), return_index=True)
    assert nr == npd == len(uk)
    same_bits(rk[:nr], pk[:npd], "unique keys")
    same_bits(rk[:nr], uk, "unique keys ref/numpy")
    same_bits(rs[:nr], ps[:npd], "segment starts")
    same_bits(rs[:nr], first.astype(np.int32), "segment starts ref/numpy")
    rv_, pv_, kk, stt = _np(rv), _np(pv), _np(keys), list(_np(rs[:nr])) + [n]
    for j in range(nr):
        want = set(np.nonzero(kk == uk[j])[0])
        assert set(rv_[stt[j]:stt[j + 1]]) == want and set(pv_[stt[j]:stt[j + 1]]) == want


# ------------------------------------------------------------------ warp (view_selection_kernel.cu, helper_kernel.cu:18-100)
def _warp_scene(N, B, H=48, W=64, seed=0):
    """N cameras on a ring looking at the origin; rays from near a camera to points near the origin, a share of the points
    outside the ring (behind the cameras on that side) and a share back-projected from the border pixels of camera 0."""
    from scanerf_amd import cameras as CM
    gen = torch.Generator().manual_seed(seed)
    c2w, ks = [], []
    for i in range(N):
        a = 2 * np.pi * i / N
        c = torch.tensor([3.0 * np.cos(a), 0.4 * float(torch.rand(1, generator=gen)) - 0.2, 3.0 * np.sin(a)], dtype=torch.float32)
        z = -c / c.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), z)
        x = x / x.norm()
        c2w.append(torch.cat([torch.stack([x, torch.linalg.cross(z, x), z], 1), c[:, None]], 1))
        ks.append(torch.tensor([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]]))
    ks, c2w = torch.stack(ks), torch.stack(c2w)
    owner = torch.randint(0, N, (B,), generator=gen)
    o = c2w[owner, :, 3] + 0.05 * torch.randn(B, 3, generator=gen)
    p = (torch.rand(B, 3, generator=gen) - 0.5) * 1.0
    n = B // 8
    p[:n] = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=1) * 4.5          # outside the ring
    u = torch.where(torch.rand(n, generator=gen) < 0.5, 0.0, float(W - 1))                        # camera 0's border columns
    v = torch.rand(n, generator=gen) * (H - 1)
    cam = torch.stack([(u - W / 2) / 40.0, (v - H / 2) / 40.0, torch.ones(n)], 1) * 2.5
    p[n:2 * n] = cam @ c2w[0, :, :3].T + c2w[0, :, 3]
    depth = 0.5 + torch.rand(B, generator=gen)
    d = (p - o) / depth[:, None]
    q = torch.cat([depth[:, None], 0.6 * torch.rand(B, 6, generator=gen)], 1)
    images = torch.rand(N, H, W, 3, generator=gen)
    return CM.CameraSet(ks, c2w, DEV), c2w, images, o.to(DEV), d.to(DEV), q.to(DEV), H, W


def test_warp_view_costs_selection_and_projection_vs_reference(RC):
    """computeViewcost against warp_reference.view_costs (float64) and the product's selected views; proj2neighbor_forward against
    warp_reference.project and the product's projection; proj2neighbor_backward against the float64 Jacobian of
    pixel = K (R p + t).  Entries float32 cannot decide (a projection within 1e-3 px of the image border, a depth at the 0.001
    cut, a cost within 1e-5 of the 0.176 threshold or of the K-th / (K+1)-th boundary) are excluded and counted; ties between
    equal costs go to the lower camera index on both sides (a stable sort)."""
    import warp_reference as WR
    from scanerf_amd.warp import WarpLoss
    N, B = 12, 4000
    cams, c2w, images, o, d, q, H, W = _warp_scene(N, B, seed=7)
    w = WarpLoss(cams, images.to(DEV), None, voxel_size=0.05)
    K = w.K
    ks, rts = cams.ks.detach().contiguous(), cams.get_rts().detach().contiguous()
    pts = (o + q[:, :1] * d).contiguous()
    costs = torch.zeros(N, B, device=DEV)
    RC.computeViewcost(o.contiguous(), d.contiguous(), pts, ks, rts, costs, H, W)
    ref = costs.t().double().cpu()
    o64, d64, p64, ks64, rts64 = [t.double().cpu() for t in (o, d, pts, ks, rts)]
    full = WR.view_costs(o64, d64, p64, ks64, rts64, H, W)
    R, t = rts64[:, :, :3], rts64[:, :, 3]
    uv = torch.einsum("nij,bnj->bni", ks64, torch.einsum("nij,bj->bni", R, p64) + t[None])
    x, y, zc = uv[..., 0] / uv[..., 2], uv[..., 1] / uv[..., 2], uv[..., 2]
    amb = (torch.minimum(torch.minimum(x.abs(), (x - (W - 1)).abs()), torch.minimum(y.abs(), (y - (H - 1)).abs())) < 1e-3) | \
          ((zc - 0.001).abs() < 1e-6)
    assert int(amb.sum()) < 0.03 * amb.numel()   # mostly the border points of camera 0
    assert int(((zc <= 0) & ~amb).sum()) > 100 and int(((full == 1) & ~amb).sum()) > 100   # behind a camera / off the image
    np.testing.assert_allclose(ref[~amb].numpy(), full[~amb].numpy(), rtol=0, atol=1e-5)
    worst("warp", "view cost ref/float64", ref[~amb], full[~amb])
    # the K views: the reference's costs selected as warp_loss.py:390-413 does vs the product's scanerf_warp_select_views
    views, _, valid = w.select(o, d, q)
    rv, rc, rvalid = WR.select(ref, K)
    srt = torch.sort(ref, dim=1, stable=True)[0]
    undecided = amb.any(1) | ((ref - WR.VALID_COST).abs() < 1e-5).any(1)
    if N > K:
        undecided |= ((srt[:, K] - srt[:, K - 1]).abs() < 1e-5) & (srt[:, K - 1] <= WR.VALID_COST + 1e-5)
    views, valid = views.cpu(), valid.cpu()
    n_sel = 0
    for b in range(B):
        if undecided[b]:
            continue
        got = {int(v) for v, ok in zip(views[b], valid[b]) if ok}
        want = {int(v) for v, ok in zip(rv[b], rvalid[b]) if ok}
        assert got == want, (b, got, want)
        n_sel += len(got)
    assert n_sel > B // 2 and int(undecided.sum()) < 0.25 * B

    # projection of the selected views (reference int32 views, bool valid)
    nv, nvalid = views.to(DEV).int().contiguous(), valid.to(DEV).contiguous()
    org, dirn, grid = (torch.zeros(B, K, 3, device=DEV) for _ in range(3))
    RC.proj2neighbor_forward(pts, ks, rts, nv, nvalid, org, dirn, grid)
    g64, dep64, org64, dir64 = WR.project(p64, ks64, rts64, views.long())
    pr = w.project(o, d, q, views.to(DEV), valid.to(DEV))
    m = valid
    rgrid = grid[..., :2] / (grid[..., 2:3] + 1e-8) - 0.5
    for name, a, b, tol in (("grid", rgrid, g64, (1e-5, 1e-4)), ("depth", grid[..., 2], dep64, (1e-5, 1e-6)),
                            ("origin", org, org64, (1e-5, 1e-5)), ("direction", dirn, dir64, (1e-5, 1e-5))):
        np.testing.assert_allclose(_np(a)[m], b[m].numpy(), rtol=tol[0], atol=tol[1], err_msg=f"proj2neighbor {name} ref/float64")
        worst("warp", f"proj2neighbor {name} ref/float64", _np(a)[m], b[m].numpy())
    for name, a, b in (("grid", rgrid, pr["grid"]), ("depth", grid[..., 2], pr["proj_depth"]), ("origin", org, pr["nei_origin"]),
                       ("direction", dirn, pr["nei_direction"])):
        np.testing.assert_allclose(_np(b)[m], _np(a)[m], rtol=1e-5, atol=1e-4, err_msg=f"projection {name} product/ref")

    # backward: the reference's adjoint (float atomics) vs the float64 Jacobian of pixel = K (R p + t) on the valid slots
    gin = torch.randn(B, K, 3, device=DEV)
    gp, grt = torch.zeros(B, 3, device=DEV), torch.zeros(N, 3, 4, device=DEV)
    RC.proj2neighbor_backward(pts, ks, rts, nv, nvalid, gin.contiguous(), gp, grt)
    P = p64.clone().requires_grad_(True)
    Rt = rts64.clone().requires_grad_(True)
    vl = views.long()
    cam = (Rt[vl][..., :3] @ P[:, None, :, None])[..., 0] + Rt[vl][..., 3]
    pix = (ks64[vl] @ cam[..., None])[..., 0]
    (pix * gin.double().cpu() * m[..., None]).sum().backward()
    for name, a, b in (("grad_pts", gp, P.grad), ("grad_rts", grt, Rt.grad)):
        b = b.numpy()
        np.testing.assert_allclose(_np(a), b, rtol=1e-4, atol=1e-5 * np.abs(b).max(), err_msg=f"proj2neighbor_backward {name}")
        worst("warp", f"proj2neighbor_backward {name} ref/float64", a, b)


def test_proj2pixel_and_fetch_color_vs_reference(RC):
    """Every point into every camera: pixel (x, y, camera depth) and its bilinear colour inside the image, (-1,-1,-1) and black
    behind a camera or off the image, black within a pixel of the border (interpolation.h:47); against a float64 restatement,
    entries within 1e-3 px of a cut excluded."""
    N, B = 6, 3000
    _, c2w, images, o, d, q, H, W = _warp_scene(N, B, seed=9)
    pts = (o + q[:, :1] * d).contiguous()
    ks = torch.tensor([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]]).expand(N, 3, 3).contiguous()
    loc, col = torch.zeros(B, N, 3, device=DEV), torch.zeros(B, N, 3, device=DEV)
    RC.proj2pixel_and_fetch_color(pts, ks.to(DEV), c2w.contiguous().to(DEV), images.contiguous().to(DEV), loc, col)
    p = pts.double().cpu()
    R, t = c2w[:, :, :3].double(), c2w[:, :, 3].double()
    cam = torch.einsum("nji,bnj->bni", R, p[:, None, :] - t[None])
    pix = torch.einsum("nij,bnj->bni", ks.double(), cam)
    front = pix[..., 2] > 0
    x, y = pix[..., 0] / pix[..., 2], pix[..., 1] / pix[..., 2]
    inside = front & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    interp = inside & (x >= 1) & (x < W - 1) & (y >= 1) & (y < H - 1)
    cuts = torch.stack([x, x - 1, x - (W - 1), y, y - 1, y - (H - 1)]).abs().min(0)[0]
    decided = (pix[..., 2].abs() > 1e-6) & ((cuts > 1e-3) | ~front)
    want_loc = torch.where(inside[..., None], torch.stack([x, y, cam[..., 2]], -1), torch.full_like(cam, -1.0))
    img = images.double()
    x0, y0 = x.clamp(0, W - 2).long(), y.clamp(0, H - 2).long()
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    n = torch.arange(N)[None].expand(B, N)
    want_col = (img[n, y0, x0] * (1 - fx) * (1 - fy) + img[n, y0 + 1, x0] * (1 - fx) * fy + img[n, y0, x0 + 1] * fx * (1 - fy)
                + img[n, y0 + 1, x0 + 1] * fx * fy)
    want_col = torch.where(interp[..., None], want_col, torch.zeros_like(want_col))
    assert int(decided.sum()) > 0.95 * decided.numel()   # mostly camera 0's border points are undecided
    assert int((~front).sum()) > 100 and int((front & ~inside).sum()) > 100 and int(interp.sum()) > 1000
    assert int((inside & ~interp & decided).sum()) > 0   # on the border: located, not interpolated
    m = decided
    np.testing.assert_allclose(_np(loc)[m], want_loc[m].numpy(), rtol=1e-5, atol=1e-4, err_msg="fetched_pixels")
    np.testing.assert_allclose(_np(col)[m], want_col[m].numpy(), rtol=0, atol=2e-5, err_msg="fetched_colors")
    worst("warp", "fetched_pixels ref/float64", _np(loc)[m], want_loc[m].numpy())
    worst("warp", "fetched_colors ref/float64", _np(col)[m], want_col[m].numpy())


# ------------------------------------------------------------------ voxelize (cuda/include/voxelize.h, host code)
@pytest.mark.parametrize("l2d,init_out", [((4, 4, 4), False), ((6, 5, 7), True)])
def test_voxelize_mesh_vs_reference(RC, tmp_path, l2d, init_out):
    """The mesh of test_voxelize_mesh_bit_exact plus a triangle lying in a voxel plane: the reference's host voxelizer, the
    product's HIP one and the oracle give the same occupancy and outside grids."""
    from scanerf_amd import formats
    from scanerf_amd.cuda import voxelize_mesh
    rng = np.random.default_rng(sum(l2d))
    corner, size = np.array([-4, -3, -5], np.float32), np.array([8, 4, 16], np.float32)

    def mesh(n_faces, lo, hi, edge):
        c = rng.uniform(lo, hi, (n_faces, 1, 3))
        v = (c + rng.normal(scale=edge, size=(n_faces, 3, 3))).astype(np.float32).reshape(-1, 3)
        return v, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)

    v, f = mesh(3000, corner - 2, corner + size + 2, 0.15)
    v2, f2 = mesh(20, corner + size * 0.3, corner + size * 0.6, 1.5)
    cell = size / np.float32([1 << k for k in l2d])
    zp = np.float32(corner[2] + 3 * cell[2])   # the plane z = 3 cells: a voxel face
    v3 = np.float32([[corner[0] + 1.1 * cell[0], corner[1] + 0.6 * cell[1], zp], [corner[0] + 4.3 * cell[0], corner[1] + 0.7 * cell[1], zp],
                     [corner[0] + 2.2 * cell[0], corner[1] + 3.9 * cell[1], zp]])
    v, f = np.concatenate([v, v2, v3]), np.concatenate([f, f2 + len(v), np.int32([[0, 1, 2]]) + len(v) + len(v2)])
    ply = tmp_path / "mesh.ply"
    formats.write_ply(ply, v, f, binary=True)
    shape = tuple(1 << k for k in l2d)
    log2dim, tc, ts = torch.tensor(l2d, dtype=torch.int32), torch.from_numpy(corner), torch.from_numpy(size)
    (rvis, rout), (pvis, pout) = [torch.zeros(shape, dtype=torch.bool), torch.zeros(shape, dtype=torch.bool)], \
                                 [torch.zeros(shape, dtype=torch.bool), torch.zeros(shape, dtype=torch.bool)]
    RC.voxelize_mesh(log2dim, tc, ts, str(ply), rvis, init_out, rout)
    voxelize_mesh(log2dim, tc, ts, str(ply), pvis, init_out, pout)
    want_vis, want_out = O.voxelize_mesh(v, f, l2d, corner, size, init_out)
    same_bits(rvis.numpy(), pvis.numpy(), "vis ref/product")
    same_bits(rout.numpy(), pout.numpy(), "outside ref/product")
    same_bits(rvis.numpy(), want_vis, "vis ref/oracle")
    same_bits(rout.numpy(), want_out, "outside ref/oracle")
    assert 0 < want_vis.mean() < 1
    assert rvis[:, :, 2:4].any()   # the in-plane triangle marks the cells on both sides of its plane (the 1.5x box)
