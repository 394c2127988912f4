"""Scenes and the numpy replay for the live quadrant masks (tests/test_gpu_live_masks.py).

tile_scene(): small Gaussians that each touch one tile only, so every tile's sorted list has the length the case
names; centres, sizes and opacities spread so that many (entry, quadrant) visits are blended by no pixel -- the
binning's quadrant bit is a conservative reach test -- and with planted cases:
  * `faint`: opacity 0.0045 on a pixel corner with a footprint narrower than a pixel: alpha < 1/255 at every pixel;
  * `wall` + `hidden`: near-opaque blobs in front of one spot of a tile stop its pixels early, and narrow entries
    behind the spot reach only those stopped pixels: alpha and power pass, pos < n_contrib does not;
  * `tail`: faint entries deepest in a tile, at or past every quadrant's bound;
  * planted_conics(): indefinite conics written into the render records, for pairs with `power > 0`.
replay(): the definition of the live bit in numpy from the library's own records, list and n_contrib.
Everything here runs on the CPU; the GPU test feeds replay() with gslm_inspect's copies."""
import math

import numpy as np
import torch

from gslm.cameras import orbit_cameras
from scenes import _world_from_pixel

THR = np.float32(1.0 / 255.0)
# A pair (entry, pixel) whose decision the replay's float64 exp could take differently from the kernels' hardware
# exp2 (2 ulp, plus the rounding of power * log2(e): relative 5e-7 of alpha at power -5.5) is one with alpha within
# ALPHA_MARGIN (relative) of 1/255, or a nonzero power within POWER_MARGIN (relative to its two terms) of zero.
ALPHA_MARGIN = 2e-6
POWER_MARGIN = 1e-6

# case -> (W, H, per-tile list lengths in tile order, SH degree, seed)
CASES = {
    "16x16_len1": (16, 16, (1,), 0, 1),
    "16x16_len64": (16, 16, (64,), 3, 2),
    "16x16_len129": (16, 16, (129,), 3, 3),
    "17x9": (17, 9, (65, 63), 3, 4),                                # 2 tiles: the second holds one pixel column
    "48x40": (48, 40, (1, 63, 64, 65, 127, 128, 129, 300, 20), 3, 5),  # 3 x 3 tiles, the last row 8 pixels high
    "48x40_sh0": (48, 40, (65, 20, 129, 1, 300, 64, 63, 128, 127), 0, 6),
    "48x40_pow": (48, 40, (1, 63, 64, 65, 127, 128, 129, 300, 20), 3, 5),  # 48x40 with planted_conics()
}
N_FAINT, N_WALL, N_HIDDEN, N_TAIL = 3, 8, 10, 4  # planted entries of a tile of 100 or more (tail: TAIL_LENGTHS)
TAIL_LENGTHS = (20, 300)


def _tile_entries(L, gen):
    """(u, v, sigma_px, opacity, kind) of one tile's L entries in depth order, tile-relative pixel coordinates."""
    u = 5.2 + 5.6 * torch.rand(L, generator=gen)
    v = 5.2 + 5.6 * torch.rand(L, generator=gen)
    sig = 0.4 + 0.65 * torch.rand(L, generator=gen)
    op = torch.exp(math.log(0.0042) + (math.log(0.5) - math.log(0.0042)) * torch.rand(L, generator=gen))
    kind = ["rand"] * L
    def put(i, uu, vv, ss, oo, kk):
        u[i], v[i], sig[i], op[i], kind[i] = uu, vv, ss, oo, kk
    if L >= 100:
        for j in range(N_WALL):  # in front of everything, around (9.5, 9.5): pixels 9..10 x 9..10 stop at the 6th
            put(j, 9.5, 9.5, 1.0, 0.995, "wall")
        for j in range(N_HIDDEN):  # reach those four pixels only
            put(N_WALL + 5 + 3 * j, 9.5, 9.5, 0.4, 0.02, "hidden")
        for j in range(N_FAINT):
            put(L // 2 + 7 * j, 5.5 + j, 6.5, 0.3, 0.0045, "faint")
    n_tail = N_TAIL if L in TAIL_LENGTHS else 0  # (the other tiles' bounds are their list lengths)
    for j in range(n_tail):
        put(L - 1 - j, 6.5 + j, 10.5, 0.3, 0.0045, "tail")
    # the deepest entry ahead of the tail reaches the four pixels around the tile's centre, one per quadrant
    put(L - 1 - n_tail, 7.5, 7.5, 1.05, 0.9, "last")
    return u, v, sig, op, kind


def tile_scene(case):
    """(model, cam, kinds): the model and camera on the CPU, kinds[i] the role of Gaussian i (see the module text).
    Gaussians are numbered tile by tile in depth order."""
    from gslm.model import GaussianModel, RGB2SH, inverse_sigmoid
    W, H, lengths, D, seed = CASES[case]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert len(lengths) == gx * gy
    cam = orbit_cameras(1, W, H, seed=1)[0]
    gen = torch.Generator().manual_seed(4000 + seed)
    cam.original_image = torch.rand(3, H, W, generator=gen)
    cam.alpha_mask = 0.25 + 0.7 * torch.rand(1, H, W, generator=gen)
    cam.alpha_mask[:, : H // 3, : W // 4] = 0.0
    fx = W / (2.0 * math.tan(cam.FoVx * 0.5))
    px, py, z, sig, op, kinds = [], [], [], [], [], []
    for t, L in enumerate(lengths):
        u, v, s, o, k = _tile_entries(L, gen)
        px.append(16.0 * (t % gx) + u)
        py.append(16.0 * (t // gx) + v)
        z.append(2.0 + 0.002 * torch.arange(L, dtype=torch.float64) + 0.0005 * t)
        sig.append(s)
        op.append(o)
        kinds += k
    px, py, z, sig, op = torch.cat(px), torch.cat(py), torch.cat(z), torch.cat(sig), torch.cat(op)
    P = px.numel()
    K = (D + 1) ** 2
    scaling = torch.log((sig / fx) * z.float())[:, None].repeat(1, 3)
    m = GaussianModel(D)
    m.set_params(_world_from_pixel(cam, px, py, z), RGB2SH(torch.rand(P, 1, 3, generator=gen)),
                 0.05 * torch.randn(P, K - 1, 3, generator=gen), scaling, torch.randn(P, 4, generator=gen),
                 inverse_sigmoid(op[:, None]), torch.eye(3, 4)[None])
    m.active_sh_degree = D
    return m, cam, kinds


def threshold_scene(W=48, H=48, seed=7):
    """(model, cam) for the alpha == 1/255 edge: one narrow Gaussian per pixel (sigma 0.3 px), its centre 0.3 to 0.5
    pixels off the pixel's, with the opacity that puts its alpha AT that pixel on 1/255 as the CPU oracle's preprocess
    and a float64 exp predict it; every other pixel sees less than 0.75 of that.  On the GPU the alpha then lands within
    a few ulp of the threshold -- sigmoid's lattice is 8 ulp wide there, the hardware exp2 adds 2 -- so about half of
    the entries blend at their pixel, as its only and therefore last contributor, and about a tenth sit exactly on
    1/255, where `>=` blends and `>` would not.  Which ones is the GPU's to say: the forward's n_contrib names every
    pixel's last contributor, by the same test."""
    from gslm.model import GaussianModel, RGB2SH, inverse_sigmoid
    from oracle import torch_raster as tr
    cam = orbit_cameras(1, W, H, seed=1)[0]
    gen = torch.Generator().manual_seed(5000 + seed)
    cam.original_image = torch.rand(3, H, W, generator=gen)
    fx = W / (2.0 * math.tan(cam.FoVx * 0.5))
    n = W * H
    i = torch.arange(n)
    sign = lambda: 2.0 * (torch.rand(n, generator=gen) < 0.5).double() - 1.0
    ox = sign() * (0.25 + 0.15 * torch.rand(n, generator=gen).double())
    oy = sign() * (0.10 + 0.20 * torch.rand(n, generator=gen).double())
    px, py = (i % W).double() + ox, (i // W).double() + oy
    z = 2.0 + 0.0001 * i.double()
    sig = 0.3 * (0.9 + 0.2 * torch.rand(n, generator=gen))
    m = GaussianModel(0)
    m.set_params(_world_from_pixel(cam, px, py, z), RGB2SH(torch.rand(n, 1, 3, generator=gen)), torch.zeros(n, 0, 3),
                 torch.log((sig / fx) * z.float())[:, None].repeat(1, 3), torch.randn(n, 4, generator=gen),
                 inverse_sigmoid(torch.full((n, 1), 0.5)), torch.eye(3, 4)[None])
    m.active_sh_degree = 0
    st = tr.settings_from_camera(cam, torch.zeros(3), 0)
    with torch.no_grad():
        pre = tr.preprocess(m.get_xyz, torch.zeros_like(m.get_xyz), m.get_opacity, m.get_features, None,
                            m.get_scaling, m.get_rotation, None, st)
    f32 = np.float32
    xy, con = pre["xy"].numpy().astype(f32), pre["conic"].numpy().astype(f32)
    dx, dy = xy[:, 0] - (i % W).numpy().astype(f32), xy[:, 1] - (i // W).numpy().astype(f32)
    s_ = (con[:, 0] * dx) * dx + (con[:, 2] * dy) * dy
    power = (-0.5 * s_.astype(np.float64) - ((con[:, 1] * dx) * dy).astype(np.float64)).astype(f32)
    op = float(THR) / np.exp(power.astype(np.float64))
    assert op.max() < 0.0065 and np.abs(power).min() > 0.03
    m._opacity.data[:] = inverse_sigmoid(torch.from_numpy(op)[:, None]).float()
    return m, cam


def planted_conics(kinds):
    """(ids, abc) for the `power > 0` case: every 9th ordinary Gaussian gets the indefinite conic (0.3, +-1, 0.3),
    written over its render record between the preprocess and the binning (the geometry workspace is the caller's).
    power = -0.15 dx^2 -+ dx dy - 0.15 dy^2 is positive in two opposite sectors around the centre and negative in the
    other two, so such an entry meets pixels it must skip for `power > 0` beside pixels it blends; the binning gives
    an indefinite conic every quadrant of its tile (quad_cull_prep, mode 1)."""
    ids = torch.tensor([i for i, k in enumerate(kinds) if k == "rand"][::9])
    abc = torch.tensor([[0.3, 1.0, 0.3], [0.3, -1.0, 0.3]])[torch.arange(ids.numel()) % 2]
    return ids, abc


def empty_scene(W=48, H=40, P=64):
    """Every Gaussian behind the camera: nothing rendered."""
    from gslm.model import synthetic_gaussians
    cam = orbit_cameras(1, W, H, seed=1)[0]
    cam.original_image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3))
    m = synthetic_gaussians(P, 3, seed=0, s0=0.03)
    c = cam.camera_center.float().cpu()
    f = -c / c.norm()
    gen = torch.Generator().manual_seed(9)
    m._xyz.data[:] = c - f * (0.5 + torch.rand(P, 1, generator=gen)) + 0.3 * (torch.rand(P, 3, generator=gen) - 0.5)
    return m, cam


def replay(records, ids, ranges, n_contrib, W, H):
    """The live bits by the definition, in the kernels' float32 arithmetic up to the exponential.

    records [P, 12] float32 (x, y, conic a, b | conic c, opacity, ...), ids [N] the sorted list's Gaussian ids, ranges
    [ntiles, 2], n_contrib [H, W].  Returns a dict: live [N] uint8 (bit q: some pixel of quadrant q blends the entry),
    below [N] uint8 (bit q: the entry's list position is below the quadrant's bound neff[q]), neff [ntiles, 4],
    pairs (entry-pixel pairs evaluated: inside the image, below the quadrant's bound), near (those within the margins
    of a threshold), power_pos (pairs with power > 0), stopped (pairs that pass power and alpha at pos >= n_contrib)."""
    f32 = np.float32
    records = np.asarray(records, dtype=f32).reshape(-1, 12)
    gx = (W + 15) // 16
    ntiles = ranges.shape[0]
    N = ids.shape[0]
    live = np.zeros(N, dtype=np.uint8)
    below = np.zeros(N, dtype=np.uint8)
    neff = np.zeros((ntiles, 4), dtype=np.int64)
    pairs = near = power_pos = stopped = 0
    for t in range(ntiles):
        r0, r1 = int(ranges[t, 0]), int(ranges[t, 1])
        L = r1 - r0
        tx, ty = t % gx, t // gx
        g = ids[r0:r1]
        x, y, a, b, c, o = (records[g, k][:, None] for k in (0, 1, 2, 3, 4, 5))
        pos = np.arange(L)[:, None]
        for q in range(4):
            xs = 16 * tx + 8 * (q & 1) + np.arange(8)
            ys = 16 * ty + 8 * (q >> 1) + np.arange(8)
            xs, ys = xs[xs < W], ys[ys < H]
            if L == 0 or xs.size == 0 or ys.size == 0:
                continue  # neff = 0: nothing below the bound
            PX, PY = np.meshgrid(xs, ys)
            nc = n_contrib[PY.reshape(-1), PX.reshape(-1)].astype(np.int64)[None, :]
            neff[t, q] = min(int(nc.max()), L)
            pxf, pyf = PX.reshape(-1).astype(f32)[None, :], PY.reshape(-1).astype(f32)[None, :]
            dx, dy = x - pxf, y - pyf                                  # float32, one rounding each
            s = (a * dx) * dx + (c * dy) * dy                          # gpower's sum, as written
            tt = (b * dx) * dy
            power64 = -0.5 * s.astype(np.float64) - tt.astype(np.float64)  # one FMA: a single rounding
            power = power64.astype(f32)
            alpha = o.astype(np.float64) * np.exp(power.astype(np.float64))
            c_pow = ~(power > 0)
            c_alpha = np.minimum(alpha, 0.99) >= np.float64(THR)
            c_last = pos < nc
            inb = pos < neff[t, q]
            ok = c_last & c_pow & c_alpha
            live[r0:r1] |= (np.any(ok, axis=1).astype(np.uint8) << q)
            below[r0:r1] |= (inb[:, 0].astype(np.uint8) << q)
            ev = np.broadcast_to(inb, ok.shape)
            pairs += int(ev.sum())
            scale = np.abs(0.5 * s.astype(np.float64)) + np.abs(tt.astype(np.float64))
            n_pow = (np.abs(power64) <= POWER_MARGIN * scale) & (scale > 0)
            n_alpha = np.abs(alpha - np.float64(THR)) <= ALPHA_MARGIN * np.float64(THR)
            near += int(((n_pow | n_alpha) & ev).sum())
            power_pos += int(((power > 0) & ev).sum())
            stopped += int((c_pow & c_alpha & ~c_last & ev).sum())
    return dict(live=live, below=below, neff=neff, pairs=pairs, near=near, power_pos=power_pos, stopped=stopped)
