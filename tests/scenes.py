"""Seeded test scenes shared by the CPU and GPU tests (SURVEY §8(d) input recipe)."""
import math

import torch

from gslm.cameras import orbit_cameras
from gslm.model import synthetic_gaussians
from oracle import torch_raster as tr

# name -> (P, sh_degree, W, H, s0, n_views)
SCENES = {
    "cfg1_2k_sh0_256": (2000, 0, 256, 256, 0.005, 1),     # BASELINE config 1 (sparse)
    "dense_2k_sh3_64x48": (2000, 3, 64, 48, 0.03, 1),      # many overlaps, early termination
    "mid_8k_sh1_96x80": (8000, 1, 96, 80, 0.02, 1),        # ragged tiles (96x80 = 6x5 tiles)
    "tiny_300_sh2_40x33": (300, 2, 40, 33, 0.06, 2),       # partial tiles both axes, 2 views
}


def make_scene(name, device="cpu"):
    P, D, W, H, s0, nv = SCENES[name]
    model = synthetic_gaussians(P, D, seed=0, s0=s0, device="cpu", n_cams=nv)
    cams = orbit_cameras(nv, W, H, seed=1)
    return model, cams


# ---- LM scenes with a visible background, saturated pixels and alpha masks (tests/test_gpu_lm_background.py,
# tests/test_oracle_lm_background.py).  name -> (P, sh_degree, W, H, s0, model seed, camera seed)
LM_BG_SCENES = {
    "sh2_64x48": (1500, 2, 64, 48, 0.04, 90, 4),
    "sh3_40x33": (1500, 3, 40, 33, 0.04, 11, 4),   # ragged on both axes
    "sh1_33x17": (600, 1, 33, 17, 0.06, 11, 4),    # one tile plus one pixel on each axis
}
BG_WHITE = (1.0, 1.0, 1.0)       # the reference's white_background
BG_GENERIC = (0.2, 0.5, 0.9)
BG_ZERO = (0.0, 0.0, 0.0)
# The model seeds are chosen (on the CPU oracle) so that in every scene and view whose GPU weights are compared with the
# oracle's no covered pixel-channel lies within 4e-5 of the clamp's corners 0 and 1 (the tests assert 1e-5): the two
# sides' 1[0 <= R <= 1] then agree whatever the host's or the GPU's rounding.
OCCLUDER_SEED = 28


def lm_bg_scene(name, n_views=1, occluders=False, seed=None, brighten=True):
    """A synthetic scene whose every 2nd Gaussian is brightened (SH DC + 2..3, colour + 0.56..0.85) so that blended
    pixels exceed 1 and the residual's clamp is active; random ground-truth images.  occluders: eight stacked
    near-opaque Gaussians in front of the first camera and a quarter of the Gaussians behind it (as the "mixed" scenes
    of tests/test_gpu_active_set.py, but leaving the background visible around the occluders), so that the view's
    active list is a proper subset.  Returns (model, cams) on the CPU."""
    from gslm.model import inverse_sigmoid
    P, D, W, H, s0, seed0, cseed = LM_BG_SCENES[name]
    seed = (OCCLUDER_SEED if occluders else seed0) if seed is None else seed
    model = synthetic_gaussians(P, D, seed=seed, s0=s0, device="cpu", n_cams=n_views)
    gen = torch.Generator().manual_seed(seed + 100)
    cams = orbit_cameras(n_views, W, H, seed=cseed)
    for i, c in enumerate(cams):
        c.original_image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(8 + i))
    with torch.no_grad():
        n = model._features_dc[::2].shape[0]
        bright = 2.0 + torch.rand(n, 1, 1, generator=gen)  # (drawn either way: the draws below do not depend on it)
        if brighten:
            model._features_dc[::2] += bright
        if occluders:
            c = cams[0].camera_center.float()
            f = -c / c.norm()  # orbit cameras look at the origin
            perm = torch.randperm(P, generator=gen)
            occ, out = perm[:8], perm[8:8 + P // 4]
            jitter = 0.02 * (torch.rand(8, 3, generator=gen) - 0.5)
            model._xyz[occ] = c + f * (1.2 + 0.01 * torch.arange(8.0)[:, None]) + jitter
            model._scaling[occ] = math.log(0.2)
            model._opacity[occ] = inverse_sigmoid(torch.tensor(0.999))
            back = 0.5 + torch.rand(len(out), 1, generator=gen)
            model._xyz[out] = c - f * back + 0.3 * (torch.rand(len(out), 3, generator=gen) - 0.5)
    return model, cams


# name -> (x0, y0, x1, y1) of the masks' block of exact zeros.  On the 64x48 scene it is two whole tiles (bottom right),
# so a Gaussian whose tile rect lies inside touches masked-out pixels only; on the ragged scenes it cuts through tiles.
ZERO_BLOCKS = {"sh2_64x48": (32, 32, 64, 48), "sh3_40x33": (21, 9, 37, 30), "sh1_33x17": (5, 3, 19, 12)}


def lm_bg_mask(name, seed=0, block=True):
    """A [1, H, W] alpha mask with values in [0.25, 0.95) and (block=True) ZERO_BLOCKS[name] of exact zeros."""
    W, H = LM_BG_SCENES[name][2:4]
    m = 0.25 + 0.7 * torch.rand(1, H, W, generator=torch.Generator().manual_seed(900 + seed))
    if block:
        x0, y0, x1, y1 = ZERO_BLOCKS[name]
        m[:, y0:y1, x0:x1] = 0.0
    return m


def place_in_zero_block(model, cam, block, n=12, seed=0):
    """Moves the first n Gaussians that are not brightened (odd index) in front of the camera so that they project
    well inside `block` (whole tiles), and shrinks them (radius 2 px) so their tile rects stay inside it.  Returns
    their ids."""
    W, H = cam.image_width, cam.image_height
    x0, y0, x1, y1 = block
    assert x0 % 16 == 0 and y0 % 16 == 0 and x1 - x0 >= 12 and y1 - y0 >= 12
    ids = torch.arange(1, 2 * n, 2)
    gen = torch.Generator().manual_seed(700 + seed)
    px = x0 + 5.0 + (x1 - x0 - 10.0) * torch.rand(n, generator=gen)
    py = y0 + 5.0 + (y1 - y0 - 10.0) * torch.rand(n, generator=gen)
    z = 2.0 + torch.rand(n, generator=gen)
    fx, fy = W / (2.0 * math.tan(cam.FoVx * 0.5)), H / (2.0 * math.tan(cam.FoVy * 0.5))
    pv = torch.stack([(px + 0.5 - 0.5 * W) / fx * z, (py + 0.5 - 0.5 * H) / fy * z, z, torch.ones(n)], dim=1)
    world = pv @ torch.linalg.inv(cam.world_view_transform.float().cpu())  # row vectors: p_view = p_world @ V
    with torch.no_grad():
        model._xyz[ids] = world[:, :3]
        model._scaling[ids] = math.log(0.005)
    return ids


def lm_bg_stats(model, cam, bg):
    """What a background / saturation scene must exercise, measured on the oracle's render: the share of pixel-channels
    with raw > 1, the share of pixels that are covered and still show the background (n_contrib > 0, T_final > 0.05),
    and the number of covered pixel-channels within 1e-5 of the clamp's corners 0 and 1 (where the GPU's and the
    oracle's 1[0 <= R <= 1] could fall on different sides through rounding)."""
    a = activated(model)
    st = oracle_settings(cam, model.active_sh_degree, torch.as_tensor(bg, dtype=a["means3D"].dtype))
    with torch.no_grad():
        raw, _, _, I = tr.rasterize(a["means3D"], torch.zeros_like(a["means3D"]), a["opacities"], st, shs=a["shs"],
                                    scales=a["scales"], rotations=a["rotations"], return_internals=True)
    covered = I["n_contrib"] > 0
    near = ((raw - 1).abs() < 1e-5) | (raw.abs() < 1e-5)
    return dict(saturated=float((raw > 1).float().mean()), below_zero=float((raw < 0).float().mean()),
                background=float((covered & (I["final_T"] > 0.05)).float().mean()),
                boundary=int((near & covered[None]).sum()), rect=I["pre"]["rect"], tiles=I["pre"]["tiles_touched"],
                raw=raw)


def assert_lm_bg_scene(model, cam, bg):
    """The conditions every background / saturation scene must meet (on oracle data only); returns the stats."""
    s = lm_bg_stats(model, cam, bg)
    assert s["saturated"] >= 0.05, s["saturated"]
    assert s["background"] >= 0.20, s["background"]
    assert s["boundary"] == 0, s["boundary"]
    return s


# ---- the branch-heavy scene of the per-Gaussian chain tests (tests/chain_jacobian.py, tests/test_gpu_chain_rules.py,
# tests/test_oracle_chain_jacobian.py)
# per-axis scale factors of every Gaussian: a Gaussian with three nearly equal scales has a nearly zero rotation derivative,
# and float32 rounding (of the oracle as of the kernels) then dominates any relative measure of it
ANISOTROPY = (0.5, 1.0, 2.0)


def chain_branch_scene(P=768, D=3, W=64, H=48, n_views=2, seed=5):
    """A scene that runs the derivative branches of csrc/gslm_chain.hpp the standard scenes leave idle: Gaussians
    outside the +-1.3 tan-FoV clamp (xyz spread to +-1.6 and every 4th Gaussian 0.25 wide, so they stay visible there),
    Gaussians under the antialiasing clamp max(2.5e-5, det0 / det) (every 8th, offset 1: 4e-4 wide and anisotropic --
    with equal scales the rotation derivative is exactly zero), SH colour clamps on every channel (every 3rd, offset 2,
    darkened; the SH rest four times as strong), |q_raw| spread over 0.2 .. 6 instead of ~2, and every Gaussian's
    scales spread by ANISOTROPY.  Random ground-truth images.  Returns (model, cams) on the CPU; what it must exercise is asserted by assert_chain_branch_scene."""
    model = synthetic_gaussians(P, D, seed=seed, s0=0.04, device="cpu", n_cams=n_views)
    cams = orbit_cameras(n_views, W, H, seed=4)
    for i, c in enumerate(cams):
        c.original_image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(8 + i))
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        model._xyz *= 1.6
        n = model._scaling[::4].shape[0]
        model._scaling[::4] = math.log(0.25) + 0.3 * torch.randn(n, 3, generator=gen)
        n = model._scaling[1::8].shape[0]
        model._scaling[1::8] = math.log(4e-4) + 0.4 * torch.randn(n, 3, generator=gen)
        n = model._features_dc[2::3].shape[0]
        model._features_dc[2::3] -= 1.2 * torch.rand(n, 1, 3, generator=gen)
        model._features_rest *= 4.0
        model._rotation *= 0.2 + 3.0 * torch.rand(P, 1, generator=gen)
        model._scaling += torch.log(torch.tensor(ANISOTROPY))
    return model, cams


def sh_subset(model, max_degree, active_degree):
    """A copy of the model that stores SH up to max_degree (the leading coefficients of the rest) with active_degree
    active."""
    import copy
    m = copy.deepcopy(model)
    K = (max_degree + 1) ** 2
    m.set_params(m._xyz, m._features_dc, m._features_rest[:, :K - 1], m._scaling, m._rotation, m._opacity, m._exposure,
                 requires_grad=True)
    m.max_sh_degree, m.active_sh_degree = max_degree, active_degree
    return m


def chain_branch_stats(model, cam, aa, scale_modifier=1.0):
    """The float64 oracle's per-Gaussian branch data of one view: preprocess's dict plus `outx` / `outy` (outside the
    tan-FoV clamp), `under_aa` (det0 / det below the antialiasing clamp; computed whatever aa is), `near_fov` /
    `near_aa` (relative distance to those thresholds), `res` (the SH colour + 0.5 before its clamp) and `boundary`
    (Gaussians whose visibility decision lies within float32 rounding of flipping: the pre-ceil radius within 1e-4 of
    an integer, a tile-rect bound within 1e-4 of a tile edge, or t.z within 1e-6 of 0.2)."""
    mc, (cc,) = to_float64(model, [cam])
    st = tr.settings_from_camera(cc, torch.zeros(3, dtype=torch.float64), mc.active_sh_degree,
                                 scale_modifier=scale_modifier, antialiasing=aa)
    with torch.no_grad():
        xyz = mc.get_xyz
        pre = tr.preprocess(xyz, torch.zeros_like(xyz), mc.get_opacity, mc.get_features, None, mc.get_scaling,
                            mc.get_rotation, None, st)
        pv = torch.cat([xyz, torch.ones(len(xyz), 1, dtype=xyz.dtype)], dim=1) @ cc.world_view_transform
        limx, limy = 1.3 * st.tanfovx, 1.3 * st.tanfovy
        rx, ry = (pv[:, 0] / pv[:, 2]).abs() / limx, (pv[:, 1] / pv[:, 2]).abs() / limy
        a, b, c = pre["cov2d"].unbind(1)
        det, det0 = a * c - b * b, (a - 0.3) * (c - 0.3) - b * b
        ratio = det0 / det
        d = xyz - cc.camera_center[None]
        res = tr.eval_sh(st.sh_degree, mc.get_features, d / d.norm(dim=1, keepdim=True)) + 0.5
        mid = 0.5 * (a + c)
        r0 = 3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp_min(mid * mid - det, 0.1)))
        radius = torch.ceil(r0)

        def near_int(t):
            return (t - torch.round(t)).abs() < 1e-4
        edges = [(pre["xy"][:, k] + s * radius + o) / 16.0 for k in (0, 1) for s, o in ((-1.0, 0.0), (1.0, 15.0))]
        boundary = near_int(r0) | ((pv[:, 2] - 0.2).abs() < 1e-6)
        for e in edges:
            boundary |= near_int(e)
    out = dict(pre)
    out.update(outx=rx > 1, outy=ry > 1, near_fov=torch.minimum((rx - 1).abs(), (ry - 1).abs()),
               under_aa=ratio < 0.000025, near_aa=(ratio / 0.000025 - 1).abs(), res=res, boundary=boundary)
    return out


def assert_chain_branch_scene(model, cam, aa, scale_modifier=1.0):
    """The conditions the chain-rule tests rely on (on float64 oracle data only); returns chain_branch_stats.
    Every branch is populated among the visible Gaussians, and no Gaussian sits so close to the tan-FoV limit or the
    antialiasing threshold that float32 and float64 could take different sides of the branch."""
    s = chain_branch_stats(model, cam, aa, scale_modifier)
    vis = s["visible"]
    P = vis.numel()
    assert int((vis & (s["outx"] | s["outy"])).sum()) >= 10
    for ch in range(3):
        assert int((vis & s["clamped"][:, ch]).sum()) >= 50, ch
    assert int((vis & s["under_aa"]).sum()) >= 40
    assert P - int(vis.sum()) >= 60
    assert int((s["near_fov"] < 1e-3).sum()) == 0
    assert int((s["near_aa"] < 1e-2).sum()) == 0
    return s


# ---- scenes whose tile lists have a controlled depth (tests/blend_reference.py, tests/test_oracle_blend_depths.py,
# tests/test_gpu_blend_depths.py)
STACK_DZ = 0.002      # view-depth step between consecutive stack entries
STACK_Z0 = 2.0
STACK_SIGMA_PX = 14.0  # screen sigma of the middle ANISOTROPY axis
BLOB_GRID = (1.0, 3.5, 6.0)
WALL_POWER_MIN = 2.2e-4  # nominal: the perspective Jacobian off the axis widens the footprint, measured 1.2e-4


def _world_from_pixel(cam, px, py, z):
    """World positions of the points that project to pixel (px, py) at view depth z (float64 arithmetic, float32
    result)."""
    W, H = cam.image_width, cam.image_height
    fx, fy = W / (2.0 * math.tan(cam.FoVx * 0.5)), H / (2.0 * math.tan(cam.FoVy * 0.5))
    px, py, z = px.double(), py.double(), z.double()
    pv = torch.stack([(px + 0.5 - 0.5 * W) / fx * z, (py + 0.5 - 0.5 * H) / fy * z, z, torch.ones_like(z)], dim=1)
    world = pv @ torch.linalg.inv(cam.world_view_transform.double().cpu())  # row vectors: p_view = p_world @ V
    return world[:, :3].float()


def stack_scene(n, W, H, a=0.02, seed=0, blobs=None, wall=None, sigma_px=STACK_SIGMA_PX, jitter=0.15):
    """n Gaussians stacked along the optical axis of orbit_cameras(1, W, H, seed=1)[0], entry i at view depth
    STACK_Z0 + STACK_DZ i, so that every tile's sorted list is the index order and (every Gaussian reaching every pixel
    with alpha >= 1/255) every tile's list depth is n.  Wide anisotropic Gaussians (ANISOTROPY around sigma_px
    pixels, sigma_px of the middle axis), opacity a U[0.75, 1.25], SH degree 1, random rotations; the centres are
    jittered perpendicular to the axis only, by at most `jitter` pixels around the pixel corner nearest the image centre
    (a centre on a pixel would put that pixel's exponent at 0, the `power > 0` decision's edge).  Random ground-truth
    image.

    blobs=(q, k): the last 27 entries become small near-opaque Gaussians (sigma 2.5 px, opacity 0.97) on a 3x3 grid
    inside quadrant q (pixels [8 (q & 1), +7] x [8 (q >> 1), +7]) of tile 0, three deep, between stack entries k - 1
    and k: the quadrant's pixels stop early, each at a depth of its own, and the other quadrants run to the end.
    wall=k: the last 3 entries become near-opaque Gaussians (opacity 0.999, centred outside the image, wide enough
    that 0.999 G >= 0.99 -- their alpha is the clamp's 0.99 -- at every pixel) between stack entries k - 1 and k: every
    pixel blends the first and stops at the second, so every tile's n_eff is k + 1 under a list of n.
    Returns (model, cam) on the CPU; what a case must exercise is asserted by tests/blend_reference.py."""
    from gslm.model import GaussianModel, RGB2SH, inverse_sigmoid
    cam = orbit_cameras(1, W, H, seed=1)[0]
    cam.original_image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(8))
    g = torch.Generator().manual_seed(1000 + seed)
    fx = W / (2.0 * math.tan(cam.FoVx * 0.5))
    n_extra = 27 if blobs is not None else (3 if wall is not None else 0)
    assert blobs is None or wall is None
    ns = n - n_extra
    assert ns >= 1
    z = STACK_Z0 + STACK_DZ * torch.arange(ns, dtype=torch.float64)
    cx, cy = math.floor(0.5 * (W - 1)) + 0.5, math.floor(0.5 * (H - 1)) + 0.5
    px = cx + 2 * jitter * (torch.rand(ns, generator=g) - 0.5)
    py = cy + 2 * jitter * (torch.rand(ns, generator=g) - 0.5)
    s_world = (sigma_px / fx) * z.float()
    scaling = torch.log(s_world[:, None] * (0.9 + 0.2 * torch.rand(ns, 3, generator=g)) * torch.tensor(ANISOTROPY))
    rotation = torch.randn(ns, 4, generator=g)
    opacity = a * (0.75 + 0.5 * torch.rand(ns, 1, generator=g))
    dc = RGB2SH(torch.rand(ns, 1, 3, generator=g))
    rest = 0.05 * torch.randn(ns, 3, 3, generator=g)
    if n_extra:
        ge = torch.Generator().manual_seed(2000 + seed)
        if blobs is not None:
            q, k = blobs
            assert 1 <= k <= ns
            gx, gy = torch.meshgrid(torch.tensor(BLOB_GRID), torch.tensor(BLOB_GRID), indexing="ij")
            ex = (8.0 * (q & 1) + gx.reshape(-1)).repeat(3) + 0.3 * (torch.rand(27, generator=ge) - 0.5)
            ey = (8.0 * (q >> 1) + gy.reshape(-1)).repeat(3) + 0.3 * (torch.rand(27, generator=ge) - 0.5)
            e_sigma, e_op = torch.full((27,), 2.5), torch.full((27, 1), 0.97)
        else:
            k = wall
            assert 1 <= k <= ns
            # outside the image (just inside the tan-FoV clamp's 0.15 W, 0.15 H), |exponent| from WALL_POWER_MIN at the
            # nearest pixel to 66 times that at the farthest (measured 1.2e-4 .. 0.0078): below -ln(0.99 / 0.999) = 0.00905, where
            # the alpha would leave the 0.99 clamp
            ex = -0.145 * W + 0.1 * (torch.rand(3, generator=ge) - 0.5)
            ey = -0.145 * H + 0.1 * (torch.rand(3, generator=ge) - 0.5)
            e_sigma = torch.full((3,), math.hypot(0.145 * W - 0.05, 0.145 * H - 0.05) / math.sqrt(2 * WALL_POWER_MIN))
            e_op = torch.full((3, 1), 0.999)
        ez = STACK_Z0 + STACK_DZ * (k - 1 + (1.0 + torch.arange(n_extra, dtype=torch.float64)) / (n_extra + 1))
        z, px, py = torch.cat([z, ez]), torch.cat([px, ex]), torch.cat([py, ey])
        scaling = torch.cat([scaling, torch.log((e_sigma / fx) * ez.float())[:, None].repeat(1, 3)])
        rotation = torch.cat([rotation, torch.randn(n_extra, 4, generator=ge)])
        opacity = torch.cat([opacity, e_op])
        dc = torch.cat([dc, RGB2SH(torch.rand(n_extra, 1, 3, generator=ge))])
        rest = torch.cat([rest, 0.05 * torch.randn(n_extra, 3, 3, generator=ge)])
    m = GaussianModel(1)
    m.set_params(_world_from_pixel(cam, px, py, z), dc, rest, scaling, rotation, inverse_sigmoid(opacity),
                 torch.eye(3, 4)[None])
    m.active_sh_degree = 1
    return m, cam


def to_float64(model, cams):
    """Deep copies of the model and cameras on the CPU in float64 (the oracle then runs in double)."""
    import copy
    mc = copy.deepcopy(model).to("cpu")
    for t in mc.params():
        t.data = t.data.double()
    ccs = []
    for c in cams:
        cc = copy.deepcopy(c).to("cpu")
        for k in ("original_image", "alpha_mask", "world_view_transform", "projection_matrix", "full_proj_transform",
                  "camera_center"):
            setattr(cc, k, getattr(cc, k).double())
        ccs.append(cc)
    return mc, ccs


def activated(model):
    """The tensors render() hands to the rasterizer (gaussian_renderer/__init__.py:54-73)."""
    with torch.no_grad():
        return dict(means3D=model.get_xyz.detach().clone(), opacities=model.get_opacity.detach().clone(),
                    scales=model.get_scaling.detach().clone(), rotations=model.get_rotation.detach().clone(),
                    shs=model.get_features.detach().clone())


def oracle_settings(cam, D, bg=None, scale_modifier=1.0, antialiasing=False):
    bg = torch.zeros(3) if bg is None else bg
    return tr.settings_from_camera(cam, bg, D, scale_modifier=scale_modifier, antialiasing=antialiasing)


def gpu_settings(cam, D, bg=None, device="cuda", scale_modifier=1.0, antialiasing=False):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    bg = torch.zeros(3) if bg is None else bg
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width),
        tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg.to(device),
        scale_modifier=float(scale_modifier), viewmatrix=cam.world_view_transform.to(device),
        projmatrix=cam.full_proj_transform.to(device), sh_degree=D, campos=cam.camera_center.to(device),
        prefiltered=False, debug=False, antialiasing=bool(antialiasing))
