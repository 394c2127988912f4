"""Float64 references for the tile blend passes at controlled list depths (tests/test_oracle_blend_depths.py on the
CPU, tests/test_gpu_blend_depths.py on the GPU).

Everything here is the CPU oracle run in double (oracle/torch_raster.py, oracle/lm_ref.py; derivatives by reverse- and
forward-mode AD through it) on scenes.stack_scene; nothing restates a kernel.  Each function takes dtype: float64 is the
expected value of the GPU tests, float32 the same oracle in the kernels' precision, whose distance from float64 (e32) is
what the GPU bounds are derived from (bound() below).
"""
import copy
import functools
import types

import torch
import torch.autograd.forward_ad as fwAD

from oracle import torch_raster as tr
from oracle.lm_ref import OracleLMProblem
from scenes import BG_GENERIC, BG_ZERO, activated, stack_scene, to_float64

# the round sizes of the tile passes (64: the wave passes, 96: the drop-in backward, 128: the LM backward and product,
# 256: the drop-in JVP) and their neighbours
DEPTHS = (1, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300)


def _case(n, W, H, a=0.02, seed=0, blobs=None, wall=None, bg=BG_GENERIC, n_eff=None, stopped=None, sigma_px=14.0,
          jitter=0.15):
    """n_eff: the depth every tile must reach (the largest n_contrib of its pixels); for a blob case the depth of the
    three running quadrants, `stopped` the largest n_contrib of the stopped one."""
    if n_eff is None:
        n_eff = n if wall is None else wall + 1
    return types.SimpleNamespace(n=n, W=W, H=H, a=a, seed=seed, blobs=blobs, wall=wall, bg=bg, n_eff=n_eff,
                                 stopped=stopped, sigma_px=sigma_px, jitter=jitter)


CASES = {}
for _i, _n in enumerate(DEPTHS):
    CASES[f"stack{_n}_16x16"] = _case(_n, 16, 16, bg=BG_GENERIC if _i % 2 == 0 else BG_ZERO)
WIDE = dict(sigma_px=20.0, jitter=0.05)  # 33x17: the farthest pixel is 18.6 px from the centres
for _n in (64, 96, 128, 256):
    CASES[f"stack{_n}_33x17"] = _case(_n, 33, 17, bg=BG_ZERO if _n == 96 else BG_GENERIC, **WIDE)
CASES["stack97_40x33"] = _case(97, 40, 33, a=0.04, sigma_px=20.0, jitter=0.1)
# walls: every pixel stops at list position k + 1, a tail of n - k - 1 entries nobody blends behind it
CASES["wall64_of200_16x16"] = _case(200, 16, 16, wall=63)
CASES["wall96_of300_33x17"] = _case(300, 33, 17, wall=95, **WIDE)
CASES["wall97_of300_16x16"] = _case(300, 16, 16, wall=96, bg=BG_ZERO)
CASES["wall128_of300_33x17"] = _case(300, 33, 17, wall=127, bg=BG_ZERO, **WIDE)
CASES["wall129_of300_16x16"] = _case(300, 16, 16, wall=128)
CASES["wall256_of400_16x16"] = _case(400, 16, 16, a=0.01, wall=255, sigma_px=18.0, jitter=0.05)
# blobs: quadrant q of the single tile stops early, its pixels at many different depths of which `stopped` is the
# largest (measured on the float64 oracle; k + 26 or so: the blobs leave T near 3e-3, which the stack then takes below
# 1e-4); the other three quadrants run to the end of the list
for _n, _q, _k, _s, _bg in ((128, 0, 38, 64, BG_GENERIC), (128, 0, 39, 65, BG_ZERO), (129, 3, 71, 96, BG_GENERIC),
                            (129, 3, 72, 97, BG_ZERO), (192, 1, 101, 127, BG_GENERIC), (192, 1, 102, 128, BG_ZERO),
                            (192, 1, 104, 129, BG_GENERIC), (300, 2, 71, 97, BG_ZERO)):
    CASES[f"blobs_q{_q}_stop{_s}_of{_n}"] = _case(_n, 16, 16, blobs=(_q, _k), bg=_bg, stopped=_s)
SSIM_CASE = "stack128_16x16"
WALLS = [k for k, c in CASES.items() if c.wall is not None]
BLOBS = [k for k, c in CASES.items() if c.blobs is not None]

# ---- bounds: per quantity and case max(8 e32, n_eff 2^-22 scale), never above the suite's present bar.
# e32 is the float32 oracle's own error against float64 in the measure the quantity is compared in (images L-inf,
# final_T absolute, gradients / tangents / LM vectors relative to the reference's max, loss relative); E32 is its
# largest value over CASES, reached at E32_AT, as measured on the CPU (tests/test_oracle_blend_depths.py re-measures
# it).  The factor 8 covers the kernels' fast exp, rcp_f, FMA contraction and cross-wave summation order (the margin of
# the chain-rule tests).  The floor is about four float32 roundings per blend step of the case's own depth (the
# largest n_contrib of the scene); every scale is 1 (images and final_T are O(1), the other measures are relative).
# No bound comes from a GPU number.
BAR = {"image": 1e-4, "final_T": 1e-5, "grad": 1e-4, "colour_tangent": 1e-4, "depth_tangent": 1e-4, "lm_vector": 1e-4,
       "ssim_vector": 1e-4, "loss": 1e-5}
E32 = {"image": 9.9e-7, "final_T": 1.6e-7, "grad": 1.9e-6, "colour_tangent": 2.3e-6, "depth_tangent": 3.5e-5,
       "lm_vector": 1.8e-6, "ssim_vector": 8.8e-6, "loss": 5.6e-8}
E32_AT = {"image": "blobs_q2_stop97_of300", "final_T": "stack64_33x17", "grad": "stack64_33x17",
          "colour_tangent": "stack256_33x17", "depth_tangent": "wall256_of400_16x16", "lm_vector": "stack300_16x16",
          "ssim_vector": SSIM_CASE, "loss": "stack257_16x16"}


def bound(quantity, name):
    return min(BAR[quantity], max(8.0 * E32[quantity], CASES[name].n_eff * 2.0 ** -22))


def build(name):
    c = CASES[name]
    return stack_scene(c.n, c.W, c.H, a=c.a, seed=c.seed, blobs=c.blobs, wall=c.wall, sigma_px=c.sigma_px,
                       jitter=c.jitter)


def of_max(got, ref):
    """max |got - ref| relative to max |ref| (the suite's measure for gradients, tangents and LM vectors)."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def linf(got, ref):
    return float((got.double() - ref.double()).abs().max())


# ---------------------------------------------------------------- the drop-in rasterizer
def dropin_inputs(name):
    """The activated float32 tensors the drop-in rasterizer is given, the cotangents of its two outputs and the
    tangents of its inputs (float32, seeded)."""
    model, cam = build(name)
    a = activated(model)
    gen = torch.Generator().manual_seed(4)
    H, W = cam.image_height, cam.image_width
    cot = dict(color=torch.randn(3, H, W, generator=gen), depth=torch.randn(1, H, W, generator=gen))
    tang = {k: torch.randn(v.shape, generator=gen) for k, v in a.items()}
    tang["means2D"] = torch.randn(a["means3D"].shape, generator=gen)
    return model, cam, a, cot, tang


def to_float64_cam(cam):
    c = copy.deepcopy(cam)
    for k in ("original_image", "alpha_mask", "world_view_transform", "projection_matrix", "full_proj_transform",
              "camera_center"):
        setattr(c, k, getattr(c, k).double())
    return c


def dropin(name, dtype):
    """The oracle's forward, backward (with and without the depth cotangent) and JVP (tangents on everything; on
    everything but means3D / means2D) of the drop-in's call, in dtype.  The inputs are the float32 activated tensors
    cast to dtype: the GPU is given the same values."""
    model, cam, a32, cot, tang = dropin_inputs(name)
    bg = CASES[name].bg
    cc = to_float64_cam(cam) if dtype == torch.float64 else cam
    st = tr.settings_from_camera(cc, torch.tensor(bg, dtype=dtype), 1)
    a = {k: v.to(dtype).requires_grad_(True) for k, v in a32.items()}
    m2 = torch.zeros_like(a["means3D"], requires_grad=True)
    c, r, d, I = tr.rasterize(a["means3D"], m2, a["opacities"], st, shs=a["shs"], scales=a["scales"],
                              rotations=a["rotations"], return_internals=True)
    out = types.SimpleNamespace(color=c.detach(), invdepth=d.detach(), radii=r, final_T=I["final_T"].detach(),
                                n_contrib=I["n_contrib"], point_list=I["point_list"], ranges=I["ranges"],
                                pre={k: (v.detach() if torch.is_tensor(v) else v) for k, v in I["pre"].items()},
                                grads={}, tangents={})
    leaves = list(a.values()) + [m2]
    names = list(a) + ["means2D"]
    for with_depth in (False, True):
        obj = (c * cot["color"].to(dtype)).sum()
        if with_depth:
            obj = obj + (d * cot["depth"].to(dtype)).sum()
        gs = torch.autograd.grad(obj, leaves, retain_graph=True)
        out.grads[with_depth] = {k: g.detach() for k, g in zip(names, gs)}
    for with_xy in (True, False):
        with torch.no_grad(), fwAD.dual_level():
            dual = {k: (fwAD.make_dual(v.detach(), tang[k].to(dtype)) if (with_xy or k != "means3D") else v.detach())
                    for k, v in a.items()}
            z = torch.zeros_like(a["means3D"]).detach()
            m2d = fwAD.make_dual(z, tang["means2D"].to(dtype)) if with_xy else z
            ct, _, dt = tr.rasterize(dual["means3D"], m2d, dual["opacities"], st, shs=dual["shs"],
                                     scales=dual["scales"], rotations=dual["rotations"])
            out.tangents[with_xy] = (fwAD.unpack_dual(ct).tangent.clone(), fwAD.unpack_dual(dt).tangent.clone())
    return out


@functools.lru_cache(maxsize=None)
def dropin64(name):
    return dropin(name, torch.float64)


# ---------------------------------------------------------------- decision margins
def decision_margins(ref):
    """Over every (pixel, entry) pair the float64 blend evaluates (oracle.torch_raster.tile_decisions: each pixel's
    list positions up to and including the one it stops at) the smallest |255 alpha - 1| (the alpha >= 1/255 test),
    |test_T / 1e-4 - 1| (the stop test, where the entry passes the other two), |power| (the power > 0 test; absolute,
    i.e. relative to 1) and |alpha_raw / 0.99 - 1| (the clamp, on whose two sides the alpha's derivative differs).  A
    float32 evaluation that differs from float64 by less takes every decision the same way."""
    H, W = ref.final_T.shape
    gx, gy = ref.pre["grid"]
    m_alpha = m_T = m_pow = m_clamp = float("inf")
    for t in range(gx * gy):
        d = tr.tile_decisions(ref.pre, ref.point_list, ref.ranges, t, H, W)
        if d is None:
            continue
        seen = d["seen"]
        alpha = torch.clamp_max(d["alpha_raw"], 0.99)
        m_pow = min(m_pow, float(d["power"].abs()[seen].min()))
        m_alpha = min(m_alpha, float((255.0 * alpha - 1.0).abs()[seen].min()))
        m_T = min(m_T, float((d["test_T"] / 0.0001 - 1.0).abs()[seen & d["valid"]].min()))
        m_clamp = min(m_clamp, float((d["alpha_raw"] / 0.99 - 1.0).abs()[seen].min()))
    return dict(alpha=m_alpha, T=m_T, power=m_pow, clamp=m_clamp)


def wall_clamped(ref, c):
    """Whether the two wall entries every pixel evaluates (list positions c.wall, c.wall + 1) have alpha_raw >= 0.99 at
    every pixel."""
    H, W = ref.final_T.shape
    gx, gy = ref.pre["grid"]
    ok = True
    for t in range(gx * gy):
        d = tr.tile_decisions(ref.pre, ref.point_list, ref.ranges, t, H, W)
        ok = ok and bool((d["alpha_raw"][:, c.wall:c.wall + 2] >= 0.99).all())
    return ok


def tile_depths(ref):
    """Per tile the largest n_contrib of its pixels (n_eff) and its list length."""
    H, W = ref.final_T.shape
    gx, gy = ref.pre["grid"]
    out = []
    for t in range(gx * gy):
        py, px = tr._tile_pixels(t, gx, H, W)
        out.append((int(ref.n_contrib[py, px].max()), int(ref.ranges[t, 1] - ref.ranges[t, 0])))
    return out


def quadrant_depths(ref):
    """Tile 0's largest n_contrib per 8x8 quadrant s (pixels [8 (s & 1), +7] x [8 (s >> 1), +7])."""
    nc = ref.n_contrib
    return [int(nc[8 * (s >> 1):8 * (s >> 1) + 8, 8 * (s & 1):8 * (s & 1) + 8].max()) for s in range(4)]


# ---------------------------------------------------------------- the LM path
def lm_direction(layout, mask_xyz, seed=9):
    v = torch.randn(layout.numel, generator=torch.Generator().manual_seed(seed))
    a, b = layout.offsets["exposure"]
    v[a:b] = 0
    a, b = layout.offsets["xyz"]
    if mask_xyz:
        v[a:b] = 0
    else:
        v[a:b] *= 0.05
    return v


def lm(name, dtype, mask_xyz=True, ssim=False):
    """The oracle's LM quantities of the case's single view in dtype: loss, J^T b, the direction v (float32 values),
    (J^T J + D) v, the residual tangent J v and the raw render."""
    model, cam = build(name)
    bg = CASES[name].bg
    if dtype == torch.float64:
        model, (cam,) = to_float64(model, [cam])
    op = OracleLMProblem(model, [cam], torch.tensor(bg, dtype=dtype), mask_xyz=mask_xyz, ssim=ssim)
    loss = float(op.evaluate())
    g = op.rhs()
    v = lm_direction(op.layout, mask_xyz)
    y = op.matvec(v.to(dtype), torch.zeros(op.layout.numel, dtype=dtype)).clone()
    jv = None if ssim else op._jr_v(op._mask(v.to(dtype).clone()))[0]
    with torch.no_grad():
        raw = tr.render_model(op.model, cam, op.bg)[3]
    return types.SimpleNamespace(loss=loss, g=g, v=v, y=y, jv=jv, raw=raw, op=op)


@functools.lru_cache(maxsize=None)
def lm64(name, mask_xyz=True, ssim=False):
    return lm(name, torch.float64, mask_xyz, ssim)


def clamp_distance(raw):
    """The smallest distance of a raw pixel-channel from the residual clamp's corners 0 and 1."""
    return float(torch.minimum(raw.abs(), (raw - 1).abs()).min())
