"""Cost of the fused surface normals (csrc/normals.hip, render.render_normals) against the two things they stand next to:

  * `normals`  the fused kernel: one launch per batch of rays;
  * `ops`      HashGrid.render_batch_rays(out_normal=True) on the same rays -- the op-by-op route with torch autograd through the
               encoder and decoder ops (the only route to a normal before the fused kernel);
  * `forward`  render.render_forward (the fused forward render) on the same rays and the same box: the same gather traffic per
               sample, more MACs -- the expectation the normals are reported against;
  * `view`     one 1920 x 1080 view through TileModel.render_image_rays with and without its normal map.

    python tools/bench_normals.py [--steps 20] [--warmup 3] [--log2-T 19] [--samples 128] [--legs normals,ops,forward,view] [--f16]

Batches of 16 384 and 65 536 rays x `samples`.  Host clock around work that ends in a device synchronise.  One JSON line.  For a
counter pass run one leg on its own under `rocprofv3 --pmc ... -- python tools/bench_normals.py --legs normals --batches 65536`."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2-T", type=int, default=19)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--batches", default="16384,65536")
    ap.add_argument("--legs", default="normals,ops,forward,view")
    ap.add_argument("--f16", action="store_true", help="gather from an f16 table (as exported tiles are); the ops leg keeps f32")
    ap.add_argument("--view", default="1080x1920")
    args = ap.parse_args()
    import scanerf_amd  # noqa
    from scanerf_amd import network, render
    from scanerf_amd import tile_model as tm
    from scanerf_amd.hashgrid import HashGrid
    dev = "cuda:0"
    S, legs = args.samples, args.legs.split(",")
    g = torch.Generator(device=dev).manual_seed(31)
    hg = HashGrid(dev, [-4.0, -4.0, -4.0], [8.0, 8.0, 8.0], log2_hashmap_size=args.log2_T, grid_resolution=[32, 2048], sampler_log2dim=4)
    with torch.no_grad():
        hg.HE.features.copy_(torch.randn(hg.HE.features.shape, device=dev, generator=g) * 0.5)
    dec = network.ShallowMLP(32).to(dev)
    table = hg.HE.features.detach().half().contiguous() if args.f16 else hg.HE.features.detach()
    res_t = hg.HE.resolution.to(dev).int().contiguous()
    step = 20000
    wf = hg.weight_feature(step).repeat_interleave(2, dim=-1).contiguous()
    box = (hg.min_bbox.tolist(), hg.bbox_size.tolist())
    out = {"log2_T": args.log2_T, "samples": S, "table": "f16" if args.f16 else "f32", "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        o = (torch.rand(B, 3, device=dev, generator=g) - 0.5) * 4.0
        d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=g), dim=-1)
        z = torch.sort(torch.rand(B, S, device=dev, generator=g) * 3.5 + 0.1, dim=1)[0].contiguous()
        dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((B, 1), 0.03, device=dev)], 1).contiguous()
        row = {}
        if "normals" in legs:
            blob = dec.blob().detach().contiguous()
            fn = lambda: render.render_normals(o, d, z, dist, table, res_t, blob, wf, *box, False)
            row["normals_ms"] = timed(fn, args.warmup, args.steps)
        if "forward" in legs:
            pk = render.PackedDecoder(dev).pack(dec.blob().detach().contiguous(), wf)
            fn = lambda: render.render_forward(o, d, z, dist, table, res_t, pk, *box, render.FORE, False, want_weights=False)
            row["forward_ms"] = timed(fn, args.warmup, args.steps)
        if "ops" in legs:
            fn = lambda: hg.render_batch_rays(o, d, z, dist, dec, 1, hg.contract_fore, out_normal=True, global_step=step)[0]["normal"]
            row["ops_out_normal_ms"] = timed(fn, 1, max(2, args.steps // 5))
            if "normals" in legs and not args.f16:   # the two routes on the same rays: what they compute
                a = render.render_normals(o, d, z, dist, table, res_t, dec.blob().detach().contiguous(), wf, *box, False)[0][:, :3]
                b = fn().detach()
                row["ops_vs_fused_rel_l2"] = float((a - b).norm() / b.norm())
            torch.cuda.empty_cache()
        if "normals_ms" in row and "forward_ms" in row:
            row["normals_over_forward"] = row["normals_ms"] / row["forward_ms"]
        if "normals_ms" in row and "ops_out_normal_ms" in row:
            row["ops_over_normals"] = row["ops_out_normal_ms"] / row["normals_ms"]
        row["samples_total"] = B * S
        out["batches"][str(B)] = row
    if "view" in legs:
        H, W = (int(v) for v in args.view.split("x"))
        m = tm.TileModel([-4.0, -4.0, -4.0], [8.0, 8.0, 8.0], dev, log2_T=args.log2_T, seed=24, table_dtype=torch.float16 if args.f16 else torch.float32)
        with torch.no_grad():
            m.features.mul_(0.5 / float(m.features.std()))
        m.invalidate_gather_table()
        ys, xs = torch.meshgrid(torch.linspace(-0.56, 0.56, H, device=dev), torch.linspace(-1.0, 1.0, W, device=dev), indexing="ij")
        dv = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(-1, 3).contiguous()
        ov = torch.tensor([0.1, -0.2, -3.0], device=dev).expand(H * W, 3).contiguous()
        view = {"H": H, "W": W, "S_fg": S, "S_bg": S}
        for flag in (False, True):
            fn = lambda: m.render_image_rays(ov, dv, S, S, step, normals=flag)
            view["render_image_rays_normals_%s_ms" % ("on" if flag else "off")] = timed(fn, 1, max(2, args.steps // 5))
        view["normal_map_ms"] = view["render_image_rays_normals_on_ms"] - view["render_image_rays_normals_off_ms"]
        view["fore_valid_rays"] = int(m.render_rays_fused(ov[:16384], dv[:16384], S, S, step)["fore_valid"].sum())
        out["view"] = view
    print(json.dumps(out))


if __name__ == "__main__":
    main()
