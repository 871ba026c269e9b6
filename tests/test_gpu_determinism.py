"""Launch-to-launch bit-reproducibility of the fused kernels.  No atomics on float data and fixed reduction orders: two
launches on the same inputs must agree bit for bit.  This is also the detector for the f16-MFMA scheduling hazard described in
csrc/render_h3.h / render_t16.h (intermittently wrong sample columns 16-31 of a tile in the second wave of a SIMD), which
tolerance-based parity tests on a few hundred rays miss."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_the_library_under_test_is_the_audited_build():
    """The reproducibility these tests establish belongs to ONE compiled listing per kernel (csrc/isa_manifest.json; no packed-f32
    arithmetic, DESIGN.md §4.1 (last paragraph); profiles/DESIGN_r04_experiment_log.md §4.10).  A library built around the audit (SCANERF_SKIP_ISA_AUDIT=1) or changed after it is refused here."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    st = _capi.audit_state()
    if st["status"] == "unvalidated" and not _capi.audit_required():
        pytest.skip("library built by another compiler build than the validated one (no packed-f32 found): " + st.get("why", ""))
    assert st["status"] == "passed", st


def _setup(B, S, mode_bg=False):
    import scanerf_amd  # noqa: F401
    from scanerf_amd import network, render
    from scanerf_amd.tile_model import TileModel
    torch.manual_seed(0)
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=14)
    with torch.no_grad():
        m.features.mul_(200.0)
    o = torch.rand(B, 3, device=DEV) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1)
    if mode_bg:
        z, dist, _ = m.inverse_z_sampling(o, d, S)
    else:
        z, dist = m.sample(o, d, S)
    wf = network.weight_feature(40000, DEV)
    m.packed.pack(m.decoder.blob(), wf)
    box = (m.min_bbox.tolist(), m.bbox_size.tolist(), render.BG if mode_bg else render.FORE, mode_bg)
    return m, o, d, z, dist, wf, box


@pytest.mark.parametrize("dt,S,bg", [(torch.float32, 64, False), (torch.bfloat16, 64, False), (torch.float16, 64, False),
                                     (torch.float32, 32, True), (torch.float32, 128, False)])
def test_forward_is_bit_reproducible(dt, S, bg):
    from scanerf_amd import render
    B = 32768
    m, o, d, z, dist, wf, box = _setup(B, S, bg)
    table = m.features.detach().to(dt).contiguous()
    ref = None
    for it in range(8):
        out, w = render.render_forward(o, d, z, dist, table, m.resolution, m.packed, *box)
        torch.cuda.synchronize()
        if ref is None:
            ref = (out.clone(), w.clone())
        else:
            nbad = int(((out != ref[0]).any(1) | (w != ref[1]).any(1)).sum())
            assert nbad == 0, f"launch {it}: {nbad} of {B} rays differ from launch 0 (table {dt}, S={S}, bg={bg})"


@pytest.mark.parametrize("arith", ["t16", "h3", "t16s"])
def test_backward_is_bit_reproducible(arith):
    from scanerf_amd import render
    render.set_arith(arith)
    try:
        B, S = 32768, 64
        m, o, d, z, dist, wf, box = _setup(B, S)
        tile_T = torch.empty(B, render.tile_T_columns(S), device=DEV)
        xs = torch.empty(B * S, 32, device=DEV)
        out, _ = render.render_forward(o, d, z, dist, m.features, m.resolution, m.packed, *box, want_weights=False, tile_T=tile_T,
                                       xstash=xs)
        g = torch.randn(B, 16, device=DEV) / B
        ref = None
        for it in range(6):
            dfeat, gblob = render.render_backward(o, d, z, dist, m.features, m.resolution, m.packed, wf, *box, out, tile_T, g,
                                                  xstash=xs)
            torch.cuda.synchronize()
            if ref is None:
                ref = (dfeat.clone(), gblob.clone())
            else:
                assert torch.equal(dfeat, ref[0]), f"{arith}: dfeat of launch {it} differs from launch 0"
                assert torch.equal(gblob, ref[1]), f"{arith}: decoder gradient of launch {it} differs from launch 0"
    finally:
        render.set_arith(render.DEFAULT_ARITH)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_forward_as_the_training_step_calls_it_is_bit_reproducible(dt):
    """Forward with the x-stash and tile_T outputs (what train_step_fused launches) after two training steps: this is the
    configuration in which a vector-memory store picked up a rewritten data register in 1 of ~4e5 tiles before
    SCANERF_STORE_GUARD (a wait-state guard of rounds 1-2; csrc/common.h says why none is needed any more)."""
    from scanerf_amd import render
    from scanerf_amd.tile_model import TileModel, train_step_fused
    torch.manual_seed(9)
    B, S = 16384, 64
    o = torch.rand(B, 3, device=DEV) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1) * (0.5 + torch.rand(B, 1, device=DEV))
    tgt = torch.rand(B, 3, device=DEV)
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=14, seed=1, table_dtype=dt)
    with torch.no_grad():
        m.features.mul_(30.0)
    opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
    for i in range(2):
        train_step_fused(m, opt, o, d, tgt, S, 20000 + i)
    z, dist = m.sample(o, d, S)
    m.packed.pack(m.decoder.blob(), m.weight_feature(20000))
    box = (m.min_bbox.tolist(), m.bbox_size.tolist(), render.FORE, False)
    table = m.gather_table()
    ref = None
    for it in range(120):
        tile_T = torch.empty(B, render.tile_T_columns(S), device=DEV)
        xs = torch.empty(B * S, 32, device=DEV)
        out, _ = render.render_forward(o, d, z, dist, table, m.resolution, m.packed, *box, want_weights=False, tile_T=tile_T, xstash=xs)
        if ref is None:
            ref = (out.clone(), xs.clone(), tile_T.clone())
        else:
            assert torch.equal(out, ref[0]) and torch.equal(xs, ref[1]) and torch.equal(tile_T, ref[2]), f"launch {it} differs (table {dt})"


@pytest.mark.parametrize("dt,pose", [(torch.float32, False), (torch.bfloat16, False), (torch.float32, True)])
def test_forward_with_cold_instruction_caches_is_bit_reproducible(dt, pose):
    """The forward that also counts the scatter plan (and, pose: writes the position-Jacobian stash), 8 192 rays x 128 samples,
    300 launches with the instruction caches swept before each one (scanerf_icache_sweep: 300 KB of straight-line code on every
    CU).  This is the condition under which the forward built with packed-f32 (w, w) weight pairs lost one corner's term in lanes
    48-63 of a tile in 8 % of the launches (DESIGN.md §4.1 (last paragraph); profiles/DESIGN_r04_experiment_log.md §4.10; tools/fault_probe.py: the sweep alone brings the fault out, poisoning
    every register and all LDS between launches does not).  Back-to-back launches of one kernel never showed it."""
    from conftest import need_symbol
    need_symbol("scanerf_icache_sweep")
    from scanerf_amd import _capi, render
    from scanerf_amd.tile_model import TileModel
    torch.manual_seed(9)
    B, S = 8192, 128
    o = torch.rand(B, 3, device=DEV) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1) * (0.5 + torch.rand(B, 1, device=DEV))
    m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=16, seed=1, table_dtype=dt)
    with torch.no_grad():
        m.features.mul_(100.0)
    z, dist = m.sample(o, d, S)
    m.packed.pack(m.decoder.blob(), m.weight_feature(20000))
    box = (m.min_bbox.tolist(), m.bbox_size.tolist(), render.FORE, False)
    table = m.gather_table()
    ref = None
    for it in range(300):
        _capi.check(_capi.lib().scanerf_icache_sweep(_capi.stream()), "icache_sweep")
        tile_T = torch.empty(B, render.tile_T_columns(S), device=DEV)
        xs = torch.empty(B * S, 32, device=DEV)
        js = torch.empty(render.jstash_shape(B, S), dtype=render.JSTASH_DTYPE, device=DEV) if pose else None
        out = render.render_forward(o, d, z, dist, table, m.resolution, m.packed, *box, want_weights=False, tile_T=tile_T, xstash=xs,
                                    plan=render.forward_plan_supported(B, S, table.shape[1]), jstash=js)[0]
        got = (out, xs, tile_T) + ((js,) if pose else ())
        if ref is None:
            ref = tuple(t.clone() for t in got)
        else:
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), f"launch {it} differs (table {dt}, pose {pose})"


@pytest.mark.parametrize("fgbg,pose", [(False, False), (True, False), (False, True), (True, True)])
def test_whole_training_step_is_bit_reproducible(fgbg, pose):
    """The default step end to end -- forward that counts the scatter plan, t16 backward emitting 8-byte records, integer
    accumulate + sparse Adam -- run twelve times from the same state on 8 192 rays x 128 samples, each time on a FRESH model (cold
    caches, new allocations: the context in which a re-allocated forward kernel failed in ~6 % of the first launches, DESIGN.md §4.1 (last paragraph); profiles/DESIGN_r04_experiment_log.md §4.10):
    table, moments and decoder after three iterations agree bit for bit (no float atomics anywhere on the path; the
    reference's scatter is not reproducible).  Also the foreground + background iteration (two record sets, one Adam), and both
    with pose gradients (Jacobian-stash forward, POSE backward; the ray gradients are hashed too)."""
    import hashlib

    import scanerf_amd  # noqa: F401
    from scanerf_amd.tile_model import TileModel, train_step_fgbg, train_step_fused
    torch.manual_seed(11)
    B, S = 8192, 128
    o = torch.rand(B, 3, device=DEV) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1) * (0.5 + torch.rand(B, 1, device=DEV))
    tgt = torch.rand(B, 3, device=DEV)
    digests = set()
    for rep in range(12):
        h = r = None
        m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=16, seed=1)
        with torch.no_grad():
            m.features.mul_(100.0)
        opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
        for i in range(3):
            if fgbg:
                r = train_step_fgbg(m, opt, o, d, tgt, S, S, 20000 + i, pose_grads=pose)
            else:
                r = train_step_fused(m, opt, o, d, tgt, S, 20000 + i, pose_grads=pose)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (m.features.detach(), m.exp_avg, m.exp_avg_sq, m.decoder.blob().detach()) + ((r[1], r[2]) if pose else ()):
            h.update(t.cpu().numpy().tobytes())
        digests.add(h.hexdigest())
    assert len(digests) == 1, f"{len(digests)} distinct results over 12 runs"


@pytest.mark.parametrize("fgbg,pose", [(False, False), (True, True)])
def test_whole_training_step_with_the_instruction_caches_swept_between_all_kernels(fgbg, pose):
    """As test_whole_training_step_is_bit_reproducible, with the instruction caches swept after EVERY library call
    (_capi.SWEEP_ICACHE): every kernel of the step -- sampler, forward, loss, backward, accumulate + Adam -- starts on cold
    instruction caches in every iteration, and the state after three iterations must be the one the plain runs give."""
    from conftest import need_symbol
    need_symbol("scanerf_icache_sweep")
    import hashlib

    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    from scanerf_amd.tile_model import TileModel, train_step_fgbg, train_step_fused
    torch.manual_seed(11)
    B, S = 8192, 128
    o = torch.rand(B, 3, device=DEV) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1) * (0.5 + torch.rand(B, 1, device=DEV))
    tgt = torch.rand(B, 3, device=DEV)
    digests = {}
    try:
        for rep in range(10):
            _capi.SWEEP_ICACHE = rep >= 2
            m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=16, seed=1)
            with torch.no_grad():
                m.features.mul_(100.0)
            opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
            for i in range(3):
                r = (train_step_fgbg(m, opt, o, d, tgt, S, S, 20000 + i, pose_grads=pose) if fgbg
                     else train_step_fused(m, opt, o, d, tgt, S, 20000 + i, pose_grads=pose))
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for t in (m.features.detach(), m.exp_avg, m.exp_avg_sq, m.decoder.blob().detach()) + ((r[1], r[2]) if pose else ()):
                h.update(t.cpu().numpy().tobytes())
            digests.setdefault(h.hexdigest(), []).append(rep)
    finally:
        _capi.SWEEP_ICACHE = False
    assert len(digests) == 1, f"runs by result (0, 1 = plain; 2.. = swept): {sorted(digests.values())}"


def test_compute_ray_backward_is_bit_reproducible():
    """The pose adjoint (cuda/compute_ray_kernel.cu:46-92: float atomics per ray) is summed in a fixed order here: the same rays
    in ANY launch give the same bits, views grouped per camera (tile.py:902-915) or shuffled; and the row of a camera does not
    depend on what other cameras' rays are in the batch."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd.cuda import compute_ray_backward
    gen = torch.Generator().manual_seed(3)
    C, B = 37, 50_000
    Ks = torch.tensor([500, 0, 320.3, 0, 510, 239.6, 0, 0, 1.0]).repeat(C, 1).to(DEV)
    locs = torch.stack([torch.randint(0, C, (B,), generator=gen).sort().values, torch.randint(0, 640, (B,), generator=gen),
                        torch.randint(0, 480, (B,), generator=gen)], 1).int()
    go, gd = torch.randn(B, 3, generator=gen).to(DEV), torch.randn(B, 3, generator=gen).to(DEV)
    for lc in (locs, locs[torch.randperm(B, generator=gen)]):
        lc = lc.to(DEV).contiguous()
        ref = None
        for it in range(50):
            gC = torch.zeros(C, 12, device=DEV)
            compute_ray_backward(go, gd, Ks, gC, lc)
            if ref is None:
                ref = gC
                assert ref.abs().min() > 0
            else:
                assert torch.equal(gC, ref), f"launch {it} differs"
    # camera 5 alone: its row is the row of the full batch (its rays keep their positions; the other cameras' rays are ignored)
    lc = locs.to(DEV).contiguous()
    full = torch.zeros(C, 12, device=DEV)
    compute_ray_backward(go, gd, Ks, full, lc)
    only = lc.clone()
    only[only[:, 0] != 5, 0] = C + 3     # out-of-range view: no camera owns these rays
    part = torch.zeros(C, 12, device=DEV)
    compute_ray_backward(go, gd, Ks, part, only)
    assert torch.equal(part[5], full[5]) and part.abs().sum() == part[5].abs().sum()


def test_reference_default_iteration_is_bit_reproducible():
    """The reference's shipped configuration (T = 2^24 entries per level, foreground + background, pose gradients) on the round-6
    route -- dfeat of both branches -> k_src_points -> count -> k_bin_scatter_seg (records placed through LDS slots: their order
    inside a bucket depends on timing) -> integer accumulate + sparse Adam: four runs of two iterations from the same state end
    with the same table, moments, decoder and ray gradients bit for bit (4 096 rays x (64 + 64) samples)."""
    import hashlib

    import scanerf_amd  # noqa: F401
    from scanerf_amd.tile_model import TileModel, train_step_fgbg
    torch.manual_seed(3)
    B, S = 4096, 64
    o = torch.rand(B, 3, device=DEV) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=-1) * (0.5 + torch.rand(B, 1, device=DEV))
    tgt = torch.rand(B, 3, device=DEV)
    digests = set()
    for rep in range(4):
        m = TileModel([-4, -4, -4], [8, 8, 8], DEV, log2_T=24, seed=1)
        with torch.no_grad():
            m.features.mul_(3000.0)
        opt = torch.optim.Adam(m.decoder.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
        for i in range(2):
            r = train_step_fgbg(m, opt, o, d, tgt, S, S, 20000 + i, pose_grads=True)
        torch.cuda.synchronize()
        assert int((m.exp_avg != 0).sum()) > 1_000_000
        h = hashlib.sha256()
        for t in (m.exp_avg, m.exp_avg_sq, m.decoder.blob().detach(), r[1], r[2]):
            h.update(t.cpu().numpy().tobytes())
        h.update(m.features.detach()[::4, ::64].contiguous().cpu().numpy().tobytes())   # (a 1/256 sample of the 2 GB table; the moments are hashed whole)
        digests.add(h.hexdigest())
        del m, opt
        torch.cuda.empty_cache()
    assert len(digests) == 1, f"{len(digests)} distinct results over 4 runs"
