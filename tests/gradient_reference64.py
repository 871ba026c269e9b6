"""A position-pinned float64 reference for the training gradients (test infrastructure; CPU only).

The float32 oracle (oracle/oracle.py render_batch_rays + torch autograd) is itself off by ~3e-6 relative L2 per table level, and
a run with EVERYTHING in float64 is no reference either: it moves the sample points by an ulp, and the cell offset t = v - b
amplifies that by the level's resolution (1e-4 .. 5e-4 per group: input rounding, not arithmetic).  So this reference pins, in
float32 and exactly as the oracle computes them,

  * the sample points o + z d and their contraction (contract_fore / contract_bg),
  * each level's cell b and offset t (scanerf_oracle.c locate_bg: v = (p + 2) / 4 * (res - 1), b = (int) v, t = v - b),
  * the level mask's values (weight_feature: an INPUT of the kernels, handed to them as a float32 tensor),

and runs float64 from there on: trilinear weights from t, interpolation of the (upcast) table, the mask product, the oracle's own
mlp_forward / cal_integrate_weight (infinity included) on float64 tensors, the accumulations, the clamp, the l2_reg_specular
numerator, torch autograd, and the table gradient as a float64 scatter of dfeat with those weights (np.add.at).

    r = Branch64(o, d, z, dist, table, res, sd, bg, mn, sz, step)      # one render_batch_rays
    g = r.gradients(loss_of(r.out))                                   # {"out", "dfeat" [N,L,2], "table" [L,T,2], "decoder" {name: ..}}
    r = RenderRays64(tile, table, sd, o, d, S_fg, S_bg, step, ...)     # render_rays: fg + T_left * bg
    g = r.gradients(r.photometric_loss(target))
    oracle32_branch(...) / oracle32_render_rays(...)                  # the float32 oracle's autograd, in the same layout
    group_errors(got, ref)                                            # relative L2 + largest element error per level / per tensor
"""
import contextlib

import numpy as np
import torch

from oracle import oracle as O

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ pinned float32 part
def pinned_points(o, d, z, bg, mn, sz):
    """[B*S,3] float32 contracted sample points, by the oracle's own float32 expressions (render_batch_rays :489-490)."""
    o, d, z = (torch.as_tensor(v, dtype=torch.float32) for v in (o, d, z))
    mn, sz = torch.as_tensor(mn, dtype=torch.float32), torch.as_tensor(sz, dtype=torch.float32)
    samples = o[:, None, :] + z[..., None] * d[:, None, :]
    fn = O.contract_bg if bg else O.contract_fore
    return fn(samples.reshape(-1, 3), mn, sz).numpy()


def pinned_cells(points, res):
    """scanerf_oracle.c locate_bg in numpy float32 (no product feeds a sum there: nothing for a compiler to contract) ->
    b [N,L,3] int32, t [N,L,3] float32."""
    p = np.asarray(points, np.float32)[:, None, :]
    r1 = (np.asarray(res, np.int32) - 1).astype(np.float32)[None, :, :]
    p01 = (p + np.float32(2.0)) / np.float32(4.0)
    v = p01 * r1
    assert v.dtype == np.float32
    b = v.astype(np.int32)          # C (int): truncation
    t = v - b.astype(np.float32)
    return b, t


def corner_indices(b, T):
    """orc_hash of the 8 corners (z fastest) -> [N,L,8] int64."""
    idx = np.empty(b.shape[:2] + (8,), np.int64)
    bu = b.astype(np.uint32)
    for c in range(8):
        x = bu[..., 0] + np.uint32((c >> 2) & 1)
        y = bu[..., 1] + np.uint32((c >> 1) & 1)
        zc = bu[..., 2] + np.uint32(c & 1)
        r = x ^ (y * np.uint32(2654435761)) ^ (zc * np.uint32(805459861))
        idx[..., c] = (r & np.uint32(T - 1)).astype(np.int64)
    return idx


def corner_weights64(t):
    """linear_weight from the pinned t, in float64 -> [N,L,8]."""
    t = t.astype(np.float64)
    w = np.empty(t.shape[:2] + (8,), np.float64)
    for c in range(8):
        wx = t[..., 0] if (c >> 2) & 1 else 1.0 - t[..., 0]
        wy = t[..., 1] if (c >> 1) & 1 else 1.0 - t[..., 1]
        wz = t[..., 2] if c & 1 else 1.0 - t[..., 2]
        w[..., c] = wx * wy * wz
    return w


def _table64(table):
    t = torch.as_tensor(table)
    return t.detach().to(F64).numpy()   # (bf16 / f16: exact upcast)


def _sd64(sd):
    return {k: torch.as_tensor(v).detach().to(F64).clone().requires_grad_(True) for k, v in sd.items()}


def mask64(step, L=16):
    """The level mask as the kernels receive it: the oracle's float32 weight_feature values, exactly upcast -> [2L]."""
    return O.weight_feature(step)[:L].to(F64).repeat_interleave(2)


# ------------------------------------------------------------------------------------------------ one branch
class Branch64:
    """render_batch_rays (TRAIN) with float64 arithmetic behind float32-pinned positions.  `out` holds the per-ray outputs
    with their autograd graph: depth [B,1], tint / diffuse / specular / rgb [B,3], T_left [B], weights [B,S,1],
    l2_reg_specular (scalar, weights detached) and w_spec2 [B] = its per-ray numerator (sum over samples and channels)."""

    def __init__(self, o, d, z, dist, table, res, sd, bg, mn, sz, step, infinity=None, sd64=None):
        z = torch.as_tensor(z, dtype=torch.float32)
        self.B, self.S = z.shape
        res = np.asarray(torch.as_tensor(res).numpy(), np.int32)
        self.L = L = res.shape[0]
        self.table = _table64(table)
        self.T = self.table.shape[1]
        b, t = pinned_cells(pinned_points(o, d, z, bg, mn, sz), res)
        self.idx, self.w = corner_indices(b, self.T), corner_weights64(t)
        lv = np.arange(L)[None, :, None]
        feats = (self.w[..., None] * self.table[lv, self.idx]).sum(2)             # [N,L,2]
        self.feats = torch.from_numpy(feats).requires_grad_(True)
        self.sd = _sd64(sd) if sd64 is None else sd64
        self.mask = mask64(step, L)
        d64 = torch.as_tensor(d, dtype=torch.float32).to(F64)
        x = torch.cat([self.feats.reshape(self.B, self.S, 2 * L), d64[:, None, :].repeat(1, self.S, 1)], -1)
        dec = O.mlp_forward(self.sd, x, self.mask[None, None, :])
        infinity = bool(bg) if infinity is None else infinity
        weights, T_left = O.cal_integrate_weight(dec["sigma"], torch.as_tensor(dist, dtype=torch.float32).to(F64), d64, infinity=infinity)
        assert weights.dtype == F64 and T_left.dtype == F64
        acc = lambda a: torch.sum(weights * a, 1)
        out = {"depth": acc(z.to(F64)[..., None]), "tint": acc(dec["tint"]), "diffuse": acc(dec["diffuse"]),
               "specular": acc(dec["tint"] * dec["specular"]), "T_left": T_left, "weights": weights}
        out["rgb"] = torch.clamp(out["diffuse"] + out["specular"], 0, 1)
        out["w_spec2"] = torch.sum(weights.detach() * dec["specular"] ** 2, (1, 2))
        out["l2_reg_specular"] = torch.mean(torch.sum(weights.detach() * dec["specular"] ** 2, 1))
        self.out = out

    def scatter(self, dfeat):
        """Float64 table gradient of dfeat [N,L,2] with the pinned cells' float64 weights."""
        g = np.zeros((self.L, self.T, 2), np.float64)
        lv = np.broadcast_to(np.arange(self.L)[None, :, None], self.idx.shape)
        np.add.at(g, (lv, self.idx), self.w[..., None] * dfeat[:, :, None, :])
        return g

    def gradients(self, loss):
        loss.backward()
        dfeat = self.feats.grad.numpy().copy()
        return {"out": {k: v.detach() for k, v in self.out.items()}, "dfeat": dfeat, "table": self.scatter(dfeat),
                "decoder": {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().copy() for k, v in self.sd.items()}}


# ------------------------------------------------------------------------------------------------ fg + bg
class RenderRays64:
    """oracle.render_rays (TRAIN): the samplers and both valid-ray rules are the oracle's own float32 ones (pinned: they are
    inputs of the render kernels), the two branches are Branch64 over ONE set of float64 decoder parameters, and the merge
    fg + T_left * bg runs in float64."""

    def __init__(self, tile, table, sd, o, d, S_fg, S_bg, step, invalid_underground=False):
        o, d = torch.as_tensor(o, dtype=torch.float32), torch.as_tensor(d, dtype=torch.float32)
        B = o.shape[0]
        z, dist = O.sample_points_grid(o, d, tile.occ_corner, tile.occ_size, tile.occ, tile.log2dim, S_fg)
        z, dist = torch.from_numpy(z), torch.from_numpy(dist)
        vf = torch.all(z != -1, dim=-1)
        zb, db, vb = O.inverse_z_sampling(o, d, tile.bbox_center, tile.bbox_size, S_bg, invalid_underground)
        self.fore_valid, self.bg_valid, self.sd = vf, vb, _sd64(sd)
        self.z_fg, self.dist_fg, self.z_bg, self.dist_bg = z, dist, zb.contiguous(), db.contiguous()
        z3, o1 = torch.zeros(B, 3, dtype=F64), torch.ones(B, 1, dtype=F64)
        fg = {"rgb": z3, "depth": torch.zeros(B, 1, dtype=F64), "T_left": o1, "specular": z3, "diffuse": z3}
        bg = dict(fg)
        self.fg = self.bg = None
        l2 = 0.0
        mn, sz = tile.min_bbox, tile.bbox_size
        if vf.any():
            self.fg = r = Branch64(o[vf], d[vf], z[vf], dist[vf], table, tile.res, None, False, mn, sz, step, infinity=False, sd64=self.sd)
            fg = {k: fg[k].index_put((vf,), r.out[k] if k != "T_left" else r.out[k][:, None]) for k in fg}
            l2 = l2 + r.out["l2_reg_specular"]
        if vb.any():
            self.bg = r = Branch64(o[vb], d[vb], zb[vb], db[vb], table, tile.res, None, True, mn, sz, step, infinity=True, sd64=self.sd)
            bg = {k: bg[k].index_put((vb,), r.out[k] if k != "T_left" else r.out[k][:, None]) for k in bg}
            l2 = l2 + r.out["l2_reg_specular"]
        self.out = {"pred_color": fg["rgb"] + fg["T_left"] * bg["rgb"], "pred_depth": fg["depth"] + fg["T_left"] * bg["depth"],
                    "pred_specular": fg["specular"] + fg["T_left"] * bg["specular"],
                    "pred_diffuse": fg["diffuse"] + fg["T_left"] * bg["diffuse"], "T_left": fg["T_left"], "l2_reg_specular": l2}

    def photometric_loss(self, target, reg_weight=0.01):
        """tile.py's loss: MSE over the rays valid in either branch (criterions.py:121-138) + reg_weight * l2_reg_specular."""
        vu = self.fore_valid | self.bg_valid
        tgt = torch.as_tensor(target, dtype=torch.float32).to(F64)
        return torch.nn.functional.mse_loss(self.out["pred_color"][vu], tgt[vu]) + reg_weight * self.out["l2_reg_specular"]

    def gradients(self, loss):
        loss.backward()
        res = {"out": {k: (v.detach() if torch.is_tensor(v) else v) for k, v in self.out.items()}, "loss": float(loss.detach())}
        table = 0.0
        for tag, r in (("fg", self.fg), ("bg", self.bg)):
            if r is not None:
                res["dfeat_" + tag] = r.feats.grad.numpy().copy()
                table = table + r.scatter(res["dfeat_" + tag])
        res["table"] = table
        res["decoder"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().copy() for k, v in self.sd.items()}
        return res


# ------------------------------------------------------------------------------------------------ the float32 oracle, same layout
@contextlib.contextmanager
def _capture_encoder_outputs(store):
    """The oracle's render_batch_rays keeps its encoder output to itself: retain its gradient (= the oracle's dfeat)."""
    orig = O.encode_bg

    def wrapped(points, features, res):
        y = orig(points, features, res)
        if y.requires_grad:
            y.retain_grad()
        store.append(y)
        return y
    O.encode_bg = wrapped
    try:
        yield
    finally:
        O.encode_bg = orig


def _grads32(sd):
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().copy() for k, v in sd.items()}


def oracle32_branch(o, d, z, dist, table, res, sd, bg, mn, sz, step, loss_of, infinity=None):
    """The float32 oracle's autograd through render_batch_rays, as Branch64.gradients lays it out.
    loss_of(out) -> scalar; out carries w_spec2-free oracle keys, so write the l2 term with out["l2_reg_specular"]."""
    t32 = lambda v: torch.as_tensor(v, dtype=torch.float32)
    mn, sz = t32(mn), t32(sz)
    sd = {k: t32(v).detach().clone().requires_grad_(True) for k, v in sd.items()}
    F = torch.as_tensor(table).detach().float().clone().requires_grad_(True)
    fn = (lambda x: O.contract_bg(x, mn, sz)) if bg else (lambda x: O.contract_fore(x, mn, sz))
    enc = []
    with _capture_encoder_outputs(enc):
        out = O.render_batch_rays(t32(o), t32(d), t32(z), t32(dist), F, torch.as_tensor(res), sd, O.TRAIN, fn, step,
                                  infinity=bool(bg) if infinity is None else infinity)
    loss_of(out).backward()
    L = int(torch.as_tensor(res).shape[0])
    return {"out": {k: v.detach() for k, v in out.items()}, "dfeat": enc[0].grad.numpy().reshape(-1, L, 2).copy(),
            "table": F.grad.numpy().copy(), "decoder": _grads32(sd)}


def oracle32_render_rays(tile, table, sd, o, d, S_fg, S_bg, step, target, invalid_underground=False, reg_weight=0.01):
    """The float32 oracle's autograd through render_rays and tile.py's loss, as RenderRays64.gradients lays it out."""
    t32 = lambda v: torch.as_tensor(v, dtype=torch.float32)
    sd = {k: t32(v).detach().clone().requires_grad_(True) for k, v in sd.items()}
    F = torch.as_tensor(table).detach().float().clone().requires_grad_(True)
    enc = []
    with _capture_encoder_outputs(enc):
        ref = O.render_rays(tile, F, sd, t32(o), t32(d), S_fg, S_bg, O.TRAIN, step, invalid_underground=invalid_underground)
    vu = ref["fore_valid"] | ref["bg_valid"]
    loss = torch.nn.functional.mse_loss(ref["pred_color"][vu], t32(target)[vu]) + reg_weight * ref["l2_reg_specular"]
    loss.backward()
    L = int(tile.res.shape[0])
    res = {"loss": float(loss.detach()), "table": F.grad.numpy().copy(), "decoder": _grads32(sd), "fore_valid": ref["fore_valid"],
           "bg_valid": ref["bg_valid"]}
    tags = (["fg"] if ref["fore_valid"].any() else []) + (["bg"] if ref["bg_valid"].any() else [])
    for tag, y in zip(tags, enc):
        res["dfeat_" + tag] = y.grad.numpy().reshape(-1, L, 2).copy()
    return res


# ------------------------------------------------------------------------------------------------ per-group errors
def _f64(a):
    return a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)


def _pairs(kind, got, ref):
    """(group name, got, ref) of one kind, converted to float64 one group at a time (a 2^22-entry table stays affordable)."""
    if isinstance(ref, dict):
        assert set(got) == set(ref), (kind, sorted(got), sorted(ref))
        for k in ref:
            yield f"{kind}/{k}", _f64(got[k]), _f64(ref[k])
    else:
        assert tuple(got.shape) == tuple(ref.shape), (kind, tuple(got.shape), tuple(ref.shape))
        for l in range(ref.shape[0]):
            yield f"{kind}/L{l:02d}", _f64(got[l]), _f64(ref[l])


def group_errors(got, ref):
    """got / ref: {kind: array with the LEVEL axis first, or {name: array}} (e.g. {"table": [L,T,2], "decoder": {...}}).
    -> {group: {"rel_l2", "max_err" (largest element error / largest reference element of the group), "ref_norm", "err_norm",
    "kind"}}, plus one "<kind>/*" entry per kind: the same figures over all of that kind's groups pooled."""
    res = {}
    for kind in ref:
        d2 = n2 = dmax = rmax = 0.0
        for name, a, b in _pairs(kind, got[kind], ref[kind]):
            assert a.shape == b.shape, (name, a.shape, b.shape)
            diff = a - b
            dn, rn = float(np.sqrt((diff * diff).sum())), float(np.sqrt((b * b).sum()))
            dm, rm = (float(np.abs(diff).max()), float(np.abs(b).max())) if b.size else (0.0, 0.0)
            res[name] = {"kind": kind, "rel_l2": dn / rn if rn > 0 else (0.0 if dn == 0 else float("inf")),
                         "max_err": dm / rm if rm > 0 else (0.0 if dm == 0 else float("inf")), "ref_norm": rn, "err_norm": dn}
            d2, n2, dmax, rmax = d2 + dn * dn, n2 + rn * rn, max(dmax, dm), max(rmax, rm)
        res[kind + "/*"] = {"kind": kind, "rel_l2": float(np.sqrt(d2 / n2)) if n2 > 0 else 0.0,
                            "max_err": dmax / rmax if rmax > 0 else 0.0, "ref_norm": float(np.sqrt(n2)), "err_norm": float(np.sqrt(d2))}
    return res


def format_table(title, errs, bounds=None, e32=None):
    """One table: group | reference norm | relative L2 | largest element error [| float32 oracle's relative L2 | bound]."""
    lines = [f"--- {title}", f"{'group':<34}{'ref norm':>11}{'rel L2':>11}{'max err':>11}" + (f"{'e32':>11}" if e32 else "")
             + (f"{'bound':>11}" if bounds else "")]
    for name, e in errs.items():
        row = f"{name:<34}{e['ref_norm']:>11.3e}{e['rel_l2']:>11.2e}{e['max_err']:>11.2e}"
        if e32:
            row += f"{e32[name]['rel_l2']:>11.2e}"
        if bounds:
            row += f"{bounds[name]:>11.2e}" if name in bounds else f"{'':>11}"
        lines.append(row)
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ the shared single-branch case
class BackwardCase:
    """The inputs of tests/test_gpu_parity.py _backward_vs_oracle (same generator, same draws: B = 200 rays, T = 2^12, decoder
    seed 5 with biases, random upstream gradients on rgb / depth / T_left and 0.37 on the l2_reg numerator) at a chosen
    step / shape / table size, with an optional ray_valid mask (every `invalid_every`-th ray is left out).

    in_domain: 1.7 % of the foreground samples of that generator lie outside the encoder's domain [-2, 2]^3 (up to 3.45), where
    the plain ops extrapolate like the reference but the compact-record routes are undefined (include/scanerf_hip.h, Domain):
    the rays owning such a sample are masked out through ray_valid as well -- for the tests of those routes."""

    G_L2 = 0.37

    def __init__(self, bg, S_, step, B=200, log2_T=12, seed=12, invalid_every=0, table_dtype=torch.float32, in_domain=False, mlp_seed=5):
        rng = np.random.default_rng(seed)
        T = 2 ** log2_T
        self.bg, self.S, self.step, self.B, self.T = bool(bg), S_, step, B, T
        o = rng.uniform(-3, 3, (B, 3)).astype(np.float32)
        d = rng.normal(size=(B, 3)).astype(np.float32) * rng.uniform(0.5, 1.5, (B, 1)).astype(np.float32)
        if bg:
            z = np.sort(rng.uniform(9, 70, (B, S_)), 1).astype(np.float32)
            dist = np.concatenate([np.diff(z, axis=1), np.full((B, 1), 1e-6, np.float32)], 1).astype(np.float32)
        else:
            z = np.sort(rng.uniform(0.2, 3.2, (B, S_)), 1).astype(np.float32)
            dist = np.concatenate([np.diff(z, axis=1), np.full((B, 1), 0.05, np.float32)], 1).astype(np.float32)
        if log2_T <= 14:
            feat = (rng.normal(size=(16, T, 2)) * 0.5).astype(np.float32)
        else:   # (large tables: float32 draws, a fraction of the time)
            feat = rng.standard_normal(size=(16, T, 2), dtype=np.float32) * np.float32(0.5)
        self.o, self.d, self.z, self.dist = o, d.astype(np.float32), z, dist
        # a bf16 / f16 table IS the parameter: the reference reads the rounded values
        self.table = torch.from_numpy(feat).to(table_dtype)
        self.sd = O.init_mlp(seed=mlp_seed, bias_scale=0.05)
        self.res = O.level_resolutions(torch.tensor([32, 32, 32]), torch.tensor([2048, 2048, 2048]))
        self.mn, self.sz = torch.tensor([-8.0, -8.0, -8.0]), torch.tensor([16.0, 16.0, 16.0])
        self.g_rgb, self.g_depth, self.g_T = (rng.normal(size=s).astype(np.float32) for s in ((B, 3), (B, 1), (B,)))
        self.valid = np.ones(B, bool)
        if invalid_every:
            self.valid[::invalid_every] = False
        if in_domain:
            p = pinned_points(self.o, self.d, self.z, self.bg, self.mn, self.sz).reshape(B, S_, 3)
            self.valid &= (np.abs(p) <= 2.0).all((1, 2))
        self.masked = [l for l in range(16) if float(O.weight_feature(step)[l]) == 0.0]

    def _loss(self, out, dtype):
        v = torch.from_numpy(self.valid)
        g_rgb, g_depth, g_T = (torch.from_numpy(a)[v].to(dtype) for a in (self.g_rgb, self.g_depth, self.g_T))
        nv = int(self.valid.sum())
        return (out["rgb"] * g_rgb).sum() + (out["depth"] * g_depth).sum() + (out["T_left"] * g_T).sum() + \
            self.G_L2 * out["l2_reg_specular"] * (3 * nv)   # = G_L2 * sum over rays of the l2_reg numerator

    def _expand(self, g):
        """dfeat of the valid rays -> dfeat of all rays (an invalid ray's samples get no gradient)."""
        if self.valid.all():
            return g
        full = np.zeros((self.B, self.S) + g["dfeat"].shape[1:], g["dfeat"].dtype)
        full[self.valid] = g["dfeat"].reshape((-1, self.S) + g["dfeat"].shape[1:])
        return dict(g, dfeat=full.reshape((-1,) + g["dfeat"].shape[1:]))

    def reference64(self):
        v = self.valid
        r = Branch64(self.o[v], self.d[v], self.z[v], self.dist[v], self.table, self.res, self.sd, self.bg, self.mn, self.sz, self.step)
        return self._expand(r.gradients(self._loss(r.out, F64)))

    def oracle32(self):
        v = self.valid
        return self._expand(oracle32_branch(self.o[v], self.d[v], self.z[v], self.dist[v], self.table, self.res, self.sd, self.bg,
                                            self.mn, self.sz, self.step, lambda out: self._loss(out, torch.float32)))


def level_major(dfeat):
    """dfeat [N,L,2] -> [L,N,2]: the layout group_errors splits by level."""
    return np.ascontiguousarray(np.asarray(dfeat).transpose(1, 0, 2))
