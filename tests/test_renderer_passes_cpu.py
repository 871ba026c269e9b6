"""The launch plan of TileSetRenderer.render_rays, on CPU tensors: every HIP op the renderer calls through its module-level names is
replaced by a recording fake, so what is checked is the Python above the kernels -- which ops run, in which order, on how many rays,
with which `sample_major` flags and array shapes, which buffers they share, and that the per-ray state of a compacted pass is written
back.  The values come from the fakes: every ray crosses tile 0, the first half of the (padded) batch also tile 1, nothing is ever
opaque.  What the real ops compute is the GPU tests' business (test_gpu_render_many_tiles.py, test_gpu_render_normals.py).
"""
import functools

import pytest
import torch

import render_scenes as RS

N_RAYS, S, SB = 70, 4, 4
SKIP = 4   # HASHGRID.SKIP_UNSAMPLED


def shape(lay, n, s, *tail):
    """a per-sample array of n rays x s samples (include/scanerf_hip.h `sample_major`)"""
    return {0: (n, s), 1: (s, n), 2: (n // 32, s, 32)}[lay] + tail


class Fakes:
    """Replaces the renderer's ops.  calls: (op, rays, sample_major) per launch, in order; masks: per pass (1, 2, ..), whether the
    running mask handed to prepare_points / pts_inference_tracing was all true; colour_buffers: (op, rays, data_ptr of the per-sample diffuse buffer)."""

    def __init__(self, monkeypatch, R, blend=1):
        self.calls, self.masks, self.colour_buffers, self.background, self.blend = [], {}, [], False, blend
        for op in ("ray_block_intersection", "sample_points", "prepare_points", "pts_normals", "pts_inference", "pts_inference_tracing",
                   "accumulate_normal", "accumulate_color", "update_outgoing_bidx", "inverse_z_sampling", "bg_pts_inference_v2"):
            monkeypatch.setattr(R, op, getattr(self, op))

    def mask(self, running):
        n_pass = sum(c[0] == "sample_points" for c in self.calls)
        self.masks.setdefault(n_pass, set()).add(bool(running.all()))

    def rec(self, op, rays, sample_major):
        self.calls.append((op, rays, int(sample_major)))
        return int(sample_major) & 3, rays

    @staticmethod
    def per_ray(n, **arrays):
        for name, (t, cols, dtype) in arrays.items():
            assert tuple(t.shape) == (n, cols) and t.dtype == dtype and t.is_contiguous(), (name, tuple(t.shape), t.dtype)

    @staticmethod
    def per_sample(lay, n, **arrays):
        for name, (t, tail, dtype) in arrays.items():
            s = t.shape[0] if lay == 1 else t.shape[1]
            assert tuple(t.shape) == shape(lay, n, s, *tail) and t.dtype == dtype and t.is_contiguous(), (name, tuple(t.shape), lay, n)
        return s

    def ray_block_intersection(self, rays_o, rays_d, block_corners, block_sizes, intersections):
        n = rays_o.shape[0]
        self.rec("ray_block_intersection", n, 0)
        assert tuple(intersections.shape) == (n, block_corners.shape[0], 2) and bool((intersections == 1e7).all())
        intersections[:, 0, 0], intersections[:, 0, 1] = 1.0, 2.0
        intersections[:n // 2, 1, 0], intersections[:n // 2, 1, 1] = 2.0, 3.0

    def sample_points(self, rays_o, rays_d, block_corners, block_sizes, grid_occupied, grid_starts, grid_log2dim, tracing_blocks,
                      intersections, tracing_idx, z_start, z_vals, dists, sample_major=False):
        lay, n = self.rec("sample_points", rays_o.shape[0], sample_major)
        nb = block_corners.shape[0]
        self.per_ray(n, rays_o=(rays_o, 3, torch.float32), rays_d=(rays_d, 3, torch.float32), tracing_blocks=(tracing_blocks, nb, torch.int32),
                     tracing_idx=(tracing_idx, 1, torch.int32), z_start=(z_start, 1, torch.float32))
        assert tuple(intersections.shape) == (n, nb, 2) and intersections.is_contiguous() and grid_occupied.dtype == torch.bool
        assert self.per_sample(lay, n, z_vals=(z_vals, (), torch.float32), dists=(dists, (), torch.float32)) == S
        assert bool((z_vals == -1).all()) and bool((dists == -1).all()), "the depths are filled per pass"
        tracing_idx += 1
        z_vals.zero_(), dists.zero_()

    def prepare_points(self, z_vals, runing_mask, intersections, block_idxs, sample_major=False):
        lay, n = self.rec("prepare_points", runing_mask.shape[0], sample_major)
        assert runing_mask.dtype == torch.bool and runing_mask.is_contiguous() and intersections.shape[0] == n
        self.per_sample(lay, n, z_vals=(z_vals, (), torch.float32), block_idxs=(block_idxs, (4,), torch.int16))
        assert bool((block_idxs == -1).all()), "the slot lists are filled per pass"
        self.mask(runing_mask)

    def pts_normals(self, rays_o, rays_d, z_vals, dists, block_idxs, features_tables, params, resolution, grid_occupied, grid_starts,
                    grid_log2dim, block_corners, block_sizes, pts_normal, sample_major=False):
        lay, n = self.rec("pts_normals", rays_o.shape[0], sample_major)
        self.per_sample(lay, n, z_vals=(z_vals, (), torch.float32), dists=(dists, (), torch.float32),
                        block_idxs=(block_idxs, (4,), torch.int16), pts_normal=(pts_normal, (3,), torch.float32))
        assert features_tables.dtype == torch.float16 and params.dtype == torch.float32 and grid_occupied.dtype == torch.bool

    def _inference(self, op, n, lay, z_vals, dists, features_tables, block_corners, diffuse, specular, alpha):
        self.per_sample(lay, n, z_vals=(z_vals, (), torch.float32), dists=(dists, (), torch.float32), diffuse=(diffuse, (3,), torch.float32),
                        specular=(specular, (3,), torch.float32), alpha=(alpha, (1,), torch.float32))
        assert features_tables.dtype == torch.float16 and tuple(block_corners.shape[1:]) == (3,)
        self.colour_buffers.append((op, n, diffuse.data_ptr()))

    def pts_inference(self, rays_o, rays_d, z_vals, dists, block_idxs, features_tables, params, resolution, grid_occupied, grid_starts,
                      grid_log2dim, block_corners, block_sizes, diffuse, specular, alpha, sample_major=False):
        lay, n = self.rec("pts_inference", rays_o.shape[0], sample_major)
        self.per_sample(lay, n, block_idxs=(block_idxs, (4,), torch.int16))
        self._inference("pts_inference", n, lay, z_vals, dists, features_tables, block_corners, diffuse, specular, alpha)

    def pts_inference_tracing(self, rays_o, rays_d, z_vals, dists, running_mask, intersections, features_tables, params, resolution,
                              grid_occupied, grid_starts, grid_log2dim, block_corners, block_sizes, diffuse, specular, alpha,
                              sample_major=False):
        lay, n = self.rec("pts_inference_tracing", rays_o.shape[0], sample_major)
        assert running_mask.dtype == torch.bool and tuple(running_mask.shape) == (n,) and intersections.shape[0] == n
        self.mask(running_mask)
        self._inference("pts_inference_tracing", n, lay, z_vals, dists, features_tables, block_corners, diffuse, specular, alpha)

    def accumulate_normal(self, pts_normal, pts_alpha, transparency, z_vals, normal, sample_major=False):
        lay, n = self.rec("accumulate_normal", transparency.shape[0], sample_major)
        self.per_sample(lay, n, pts_normal=(pts_normal, (3,), torch.float32), pts_alpha=(pts_alpha, (1,), torch.float32),
                        z_vals=(z_vals, (), torch.float32))
        self.per_ray(n, transparency=(transparency, 1, torch.float32), normal=(normal, 3, torch.float32))
        normal += 1

    def accumulate_color(self, pts_diffuse, pts_specular, pts_alpha, transparency, z_vals, diffuse, specular, depth, sample_major=False):
        lay, n = self.rec("accumulate_color", transparency.shape[0], sample_major)
        self.per_sample(lay, n, pts_diffuse=(pts_diffuse, (3,), torch.float32), pts_specular=(pts_specular, (3,), torch.float32),
                        pts_alpha=(pts_alpha, (1,), torch.float32), z_vals=(z_vals, (), torch.float32))
        self.per_ray(n, transparency=(transparency, 1, torch.float32), diffuse=(diffuse, 3, torch.float32),
                     specular=(specular, 3, torch.float32), depth=(depth, 1, torch.float32))
        if not self.background:   # (the foreground's passes are what the write-back tests count)
            depth += 1
            diffuse += 1

    def update_outgoing_bidx(self, rays_o, rays_d, block_corners, block_sizes, tracing_blocks, intersections, bg_b, bg_w, overlap, flag):
        n = rays_o.shape[0]
        self.rec("update_outgoing_bidx", n, 0)
        self.per_ray(n, bg_b=(bg_b, 4, torch.int16), bg_w=(bg_w, 4, torch.float32))
        assert bool((bg_b == -1).all()) and bool((bg_w == 0).all()) and (overlap, flag) == (0.12, False)
        bg_b[:, :self.blend], bg_w[:, :self.blend] = 0, 1
        self.background = True

    def inverse_z_sampling(self, intersections, bidx, z_vals, sample_range, sample_major=False):
        lay, n = self.rec("inverse_z_sampling", intersections.shape[0], sample_major)
        assert tuple(bidx.shape) == (n,) and bidx.dtype == torch.int16 and bidx.is_contiguous()
        assert self.per_sample(lay, n, z_vals=(z_vals, (), torch.float32)) == self.bg_samples and bool((z_vals == -1).all())

    def bg_pts_inference_v2(self, rays_o, rays_d, z_vals, bg_b, step, block_corners, block_sizes, resolution, features_tables, params,
                            diffuse, specular, alpha, sample_major=False):
        lay, n = self.rec("bg_pts_inference_v2", rays_o.shape[0], sample_major)
        assert step == sum(c[0] == "bg_pts_inference_v2" for c in self.calls) - 1 and resolution.dtype == torch.int32
        self.per_ray(n, bg_b=(bg_b, 4, torch.int16))
        self._inference("bg_pts_inference_v2", n, lay, z_vals, z_vals, features_tables, block_corners, diffuse, specular, alpha)

    bg_samples = SB

    # ---- views of the record
    def passes(self):
        """the foreground's launches, split at each sample_points: [[(op, rays, sample_major)]]"""
        fg = self.calls[1:[c[0] for c in self.calls].index("update_outgoing_bidx")]
        out = []
        for c in fg:
            if c[0] == "sample_points":
                out.append([])
            out[-1].append(c)
        return out

    def background_calls(self):
        return self.calls[[c[0] for c in self.calls].index("update_outgoing_bidx"):]


def R():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import renderer
    return renderer


def make_renderer(monkeypatch, name):
    """TileSetRenderer on the CPU: the constructor's three device calls replaced by what they document"""
    r = R()
    monkeypatch.setattr(r, "process_occupied_grid", lambda *a: None)
    monkeypatch.setattr(r._HG, "PackedDecoders", lambda params: params)
    monkeypatch.setattr(r, "sort_tracing_blocks", lambda inter: torch.argsort(inter[..., 0], dim=-1, stable=True).int())
    return r.TileSetRenderer("cpu", RS.renderer_tiles(RS.named(name)[0]))


@functools.lru_cache(maxsize=None)
def rays():
    gen = torch.Generator().manual_seed(5)
    return torch.randn(N_RAYS, 3, generator=gen), torch.randn(N_RAYS, 3, generator=gen)


def run(monkeypatch, name, blend=1, switches=(), **kw):
    rnd = make_renderer(monkeypatch, name)
    for k, v in dict(switches).items():
        assert hasattr(rnd, k)
        setattr(rnd, k, v)
    fakes = Fakes(monkeypatch, R(), blend)
    fakes.bg_samples = kw.get("num_bg_sample", SB)
    o, d = rays()
    o0, d0 = o.clone(), d.clone()
    out = rnd.render_rays(o, d, **{"num_sample": S, "num_bg_sample": SB, **kw})
    assert torch.equal(o, o0) and torch.equal(d, d0), "the caller's rays are read only"
    return fakes, out


def pass_ops(fused, normals):
    """the order of one tracing pass"""
    ops = ["sample_points"] + (["prepare_points", "pts_normals"] if normals else [])
    ops += ["pts_inference_tracing"] if fused else (["pts_inference"] if normals else ["prepare_points", "pts_inference"])
    return ops + (["accumulate_normal"] if normals else []) + ["accumulate_color"]


FUSED_FLAGGED = ("pts_inference_tracing", "accumulate_normal", "accumulate_color")


def check_passes(fakes, rows, lay, fused, normals):
    got = fakes.passes()
    assert len(got) == len(rows)
    for p, n in zip(got, rows):
        assert [c[0] for c in p] == pass_ops(fused, normals)
        assert [c[1] for c in p] == [n] * len(p)
        assert [c[2] for c in p] == [lay | (SKIP if fused and c[0] in FUSED_FLAGGED else 0) for c in p]


def check_background(fakes, rows, lay, blend=1):
    bg = fakes.background_calls()
    assert bg[0] == ("update_outgoing_bidx", rows, 0)
    assert bg[1:] == [("inverse_z_sampling", rows, lay), ("bg_pts_inference_v2", rows, lay), ("accumulate_color", rows, lay)] * blend


def check_counts(out, normals, half=48):
    """every output has the caller's 70 rows; depth, diffuse (and the normal) count the passes a ray ran: the first half of the padded
    batch (48 of 96; unpadded: 35 of 70) crosses two tiles, the rest one.  Transparency stays 1, and the background's colours are zero."""
    assert len(out) == (5 if normals else 4)
    assert [tuple(t.shape) for t in out] == [(N_RAYS, 3), (N_RAYS, 3), (N_RAYS, 1), (N_RAYS, 1)] + ([(N_RAYS, 3)] if normals else [])
    want = torch.cat([torch.full((half, 1), 2.0), torch.full((N_RAYS - half, 1), 1.0)])
    assert torch.equal(out[2], want) and torch.equal(out[0], want.expand(N_RAYS, 3))
    assert bool((out[1] == 0).all()) and bool((out[3] == 1).all())
    if normals:
        assert torch.equal(out[4], want.expand(N_RAYS, 3))


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("name", ["G8", "G9"])
def test_default_route_pads_then_compacts(name, normals, monkeypatch):
    """layout 2: 70 rays padded to 96 for the first pass (all running: full size); 48 still run, below nine tenths: the second pass
    takes them alone, padded to 64.  G8 derives the slot lists in the inference kernel (flags | SKIP_UNSAMPLED on it and on the two
    accumulations), G9 (nine tiles) runs prepare_points + pts_inference."""
    fakes, out = run(monkeypatch, name, normals=normals)
    assert fakes.calls[0] == ("ray_block_intersection", 96, 0)
    check_passes(fakes, [96, 64], 2, fused=name == "G8", normals=normals)
    check_background(fakes, 96, 2)
    check_counts(out, normals)
    assert fakes.masks == {1: {True}, 2: {True}}   # (all 96 run in the first pass; a compacted pass gets an all-true mask)


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("name", ["G8", "G9"])
def test_layouts_0_and_1_run_unpadded(name, lay, normals, monkeypatch):
    fakes, out = run(monkeypatch, name, layout=lay, normals=normals)
    assert fakes.calls[0] == ("ray_block_intersection", N_RAYS, 0)
    check_passes(fakes, [70, 35], lay, fused=name == "G8", normals=normals)
    check_background(fakes, 70, lay)
    check_counts(out, normals, half=35)


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("name", ["G8", "G9"])
@pytest.mark.parametrize("tenths,rows,all_true", [(0, [96, 96], [True, False]), (9, [96, 64], [True, True]), (11, [96, 64], [True, True])])
def test_compact_below_tenths(tenths, rows, all_true, name, normals, monkeypatch):
    """0: every pass full size (the second one's mask names the 48 running rays); 11: every pass compacted, the first one too -- all
    96 rays gathered, an all-true mask, buffers of its own; 9 is the default."""
    fakes, out = run(monkeypatch, name, switches={"compact_below_tenths": tenths}, normals=normals)
    check_passes(fakes, rows, 2, fused=name == "G8", normals=normals)
    check_background(fakes, 96, 2)
    check_counts(out, normals, half=N_RAYS if tenths == 0 else 48)   # (the fakes count launches: a full-size pass covers every ray)
    assert fakes.masks == {k + 1: {v} for k, v in enumerate(all_true)}
    # full-size passes and a background of as many samples share ONE set of colour buffers; a compacted pass has its own
    fg = [b for b in fakes.colour_buffers if b[0] != "bg_pts_inference_v2"]
    bg = [b for b in fakes.colour_buffers if b[0] == "bg_pts_inference_v2"]
    if tenths == 0:
        assert fg[0][2] == fg[1][2] == bg[0][2]
    elif tenths == 9:
        assert fg[0][2] == bg[0][2] != fg[1][2]
    else:
        assert bg[0][2] not in (fg[0][2], fg[1][2])


@pytest.mark.parametrize("normals", [False, True])
def test_fuse_slots_off_gives_the_two_op_sequence(normals, monkeypatch):
    fakes, out = run(monkeypatch, "G8", switches={"fuse_slots": False}, normals=normals)
    check_passes(fakes, [96, 64], 2, fused=False, normals=normals)
    check_background(fakes, 96, 2)
    check_counts(out, normals)


@pytest.mark.parametrize("name,arith", [("G8", "f32"), ("G65", "t16")])
def test_single_pass_fallback_is_layout_0_without_fused_slots(name, arith, monkeypatch):
    """INFER_ARITH = "f32", or more than 64 tiles: the reference's [B,S] arrays, unpadded, two-op route, whatever layout was asked for"""
    monkeypatch.setattr(R()._HG, "INFER_ARITH", arith)
    fakes, out = run(monkeypatch, name, normals=True)
    assert fakes.calls[0] == ("ray_block_intersection", N_RAYS, 0)
    check_passes(fakes, [70, 35], 0, fused=False, normals=True)
    check_background(fakes, 70, 0)
    check_counts(out, True, half=35)


@pytest.mark.parametrize("lay", [0, 2])
def test_background_blend_steps_and_buffers_of_their_own_size(lay, monkeypatch):
    """three exit tiles: three blend steps; num_bg_sample != num_sample: the background allocates its colour buffers (the fakes check
    every per-sample shape against the sample count)"""
    fakes, out = run(monkeypatch, "G9", blend=3, layout=lay, num_bg_sample=6)
    rows = 96 if lay == 2 else 70
    check_background(fakes, rows, lay, blend=3)
    bg = [b[2] for b in fakes.colour_buffers if b[0] == "bg_pts_inference_v2"]
    assert len(bg) == 3 and len(set(bg)) == 1   # (one set for all blend steps; of 6 samples, so not the foreground's of 4)
    check_counts(out, False, half=48 if lay == 2 else 35)


def test_a_batch_that_misses_every_tile_runs_no_pass(monkeypatch):
    rnd = make_renderer(monkeypatch, "G9")
    fakes = Fakes(monkeypatch, R())
    monkeypatch.setattr(R(), "ray_block_intersection", lambda ro, *a: fakes.rec("ray_block_intersection", ro.shape[0], 0))
    out = rnd.render_rays(*rays(), num_sample=S, num_bg_sample=SB)
    assert fakes.passes() == []
    check_background(fakes, 96, 2)
    assert all(bool((t == 0).all()) for t in out[:3]) and bool((out[3] == 1).all()) and out[0].shape[0] == N_RAYS
