"""Float64 torch restatement of the warp loss (warp_loss.py:390-660, view_selection_kernel.cu:19-349), steps 2-6 of
scanerf_amd.warp: the yardstick the HIP kernels are checked against (tests/test_warp_cpu.py pins it to golden G21, which the
reference's own torch code produced).  Test helper only; runs on any device."""
import torch

VALID_COST = 0.176


def _split(rts):
    return rts[..., :3, :3], rts[..., :3, 3]


def centres(rts):
    R, t = _split(rts)
    return -(R.transpose(-1, -2) @ t[..., None])[..., 0]


def view_costs(rays_o, rays_d, pts, ks, rts, H, W):
    """computeViewcost_kernel (view_selection_kernel.cu:19-72) -> [B,N]."""
    R, t = _split(rts)
    q = torch.einsum("nij,bj->bni", R, pts) + t[None]
    uv = torch.einsum("nij,bnj->bni", ks, q)
    z = uv[..., 2]
    x, y = uv[..., 0] / z, uv[..., 1] / z
    e = pts[:, None, :] - centres(rts)[None]
    en = e.norm(dim=-1)
    d = rays_d / rays_d.norm(dim=-1, keepdim=True)
    angle = 1.0 - (d[:, None, :] * e).sum(-1) / en
    dis = torch.clamp(1.0 - (pts - rays_o).norm(dim=-1)[:, None] / en, min=0.0)
    cost = 0.9 * angle + 0.1 * dis
    bad = (z <= 0.001) | (x <= 0) | (x >= W - 1) | (y <= 0) | (y >= H - 1)
    return torch.where(bad, torch.ones_like(cost), cost)


def select(costs, K, ray_valid=None):
    """The K lowest costs per ray (ties: lower camera index) -> views [B,K] long, cost [B,K], valid [B,K] (warp_loss.py:390-413)."""
    c, v = torch.sort(costs, dim=1, stable=True)
    c, v = c[:, :K], v[:, :K]
    valid = c <= VALID_COST
    if ray_valid is not None:
        valid = valid & ray_valid[:, None]
    return v, c, valid


def project(pts, ks, rts, views):
    """proj2neighbor_forward + the grid / depth split of warp_loss.py:415-439 -> grid [B,K,2], proj_depth [B,K], nei_origin,
    nei_direction [B,K,3].  Differentiable in pts and rts."""
    R, t = _split(rts[views])
    q = (R @ pts[:, None, :, None])[..., 0] + t
    pix = (ks[views] @ q[..., None])[..., 0]
    grid = pix[..., :2] / (pix[..., 2:3] + 1e-8) - 0.5
    cam_d = torch.cat([q[..., :2] / (q[..., 2:3] + 1e-8), torch.ones_like(q[..., 2:3])], -1)
    direction = (R.transpose(-1, -2) @ cam_d[..., None])[..., 0]
    return grid, pix[..., 2], centres(rts)[views], direction


def sample_color(images, occlusions, grid, views, valid, corner_grid=None):
    """sample_neighbor_color (warp_loss.py:441-521): bilinear from images [N,H,W,3], top-left corner grid.long() (truncation),
    weights from grid - corner (the gradient reaches grid through them), valid AND occlusions at (grid + 0.5).long().
    corner_grid: take the corners (and the occlusion pixel) from this grid instead (a float32 run's), so that a float64 restatement
    picks the same pixels where the two sit on either side of a pixel boundary."""
    H, W = images.shape[1], images.shape[2]
    cg = (grid if corner_grid is None else corner_grid).detach()
    lt = cg.long()
    lx, ly = lt[..., 0].clamp(0, W - 2), lt[..., 1].clamp(0, H - 2)   # (bounds of slots that are not valid anyway)
    off = grid - torch.stack([lx, ly], -1).to(grid.dtype)
    n = (cg + 0.5).long()
    nx, ny = n[..., 0].clamp(0, W - 1), n[..., 1].clamp(0, H - 1)
    v = views.long()
    if occlusions is not None:
        valid = valid & occlusions[v, ny, nx]
    ox, oy = off[..., 0:1], off[..., 1:2]
    color = ((1 - ox) * (1 - oy) * images[v, ly, lx] + ox * (1 - oy) * images[v, ly, lx + 1] +
             (1 - ox) * oy * images[v, ly + 1, lx] + ox * oy * images[v, ly + 1, lx + 1])
    return color, valid


def soft_vis(depth_diff, alpha, voxel_size):
    return torch.exp(-alpha * depth_diff / voxel_size)


def soft_diffuse(specular, gamma):
    return torch.exp(-gamma * specular.mean(-1))


def scores(vis, nei_specular, ref_specular, valid, gamma):
    """warping_score of warp_loss.py:640-650: vis x neighbour diffuse score on the valid slots, x the ray's diffuse score."""
    s = torch.where(valid, vis * soft_diffuse(nei_specular, gamma), torch.zeros_like(vis))
    return s * soft_diffuse(ref_specular, gamma)[:, None]


def compute_loss(diffuse, specular, color, score, n_rays):
    """compute_loss (warp_loss.py:332-337) on clamp(diffuse + specular, 0, 1) (warp_loss.py:652-653): mean over n_rays x K."""
    pred = torch.clamp(diffuse + specular, 0, 1)
    per = ((pred[:, None, :] - color) ** 2).mean(-1) * score
    return per.sum() / (n_rays * color.shape[1])


def warp_loss(rays_o, rays_d, depth, diffuse, specular, rts, ks, images, occlusions, views, valid, score, scale=1.0,
              ray_valid=None, corner_grid=None):
    """The whole differentiable term with selection and scores frozen: scale * mean over B x K.  Inputs may require grad."""
    pts = rays_o + depth[:, None] * rays_d
    grid, _, _, _ = project(pts, ks, rts, views)
    color, valid = sample_color(images, occlusions, grid, views, valid, corner_grid)
    score = torch.where(valid, score, torch.zeros_like(score))
    if ray_valid is not None:
        score = score * ray_valid[:, None].to(score.dtype)
        n = int(ray_valid.sum())
    else:
        n = rays_o.shape[0]
    return scale * compute_loss(diffuse, specular, color, score, max(n, 1)) if n else (score.sum() * 0.0)
