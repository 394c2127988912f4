"""CPU: the oracle's LM algebra under a nonzero background, an alpha mask and saturated pixels.

tests/golden/solver_golden.npz was produced with a zero background and all-ones masks, so no golden pins how
oracle/lm_ref.py treats the background (the T * bg term of the render and its tangent / adjoint), the mask
(m * clamp01(R) - gt) or the clamp's derivative 1[0 <= R <= 1].  tests/test_gpu_lm_background.py takes this oracle as
the expected value of the HIP LM path on exactly those axes; here the oracle's J v and J^T u are pinned from first
principles, in float64, on the 600-Gaussian 33x17 scene of tests/scenes.py with bg = (0.2, 0.5, 0.9), the fractional
mask with its block of zeros, and every 2nd Gaussian brightened:
  * J v (OracleLMProblem._jr_v, forward-mode AD through the renderer, the mask and the clamp) equals the central finite
    difference of the residual along v at h = 1e-4 and 1e-5: the error shrinks with h and is <= 1e-6 of max |J v| at the
    smaller step (pixel-channels whose raw render crosses 0 or 1 inside the step excluded: the clamp has a kink there);
  * <J v, u> = <v, J^T u> to 1e-10 relative, J^T u by reverse-mode AD (what rhs() and the product's adjoint half use).
Both with xyz masked (the LM path) and with a direction that moves xyz (mask_xyz=False)."""
import math

import pytest
import torch

from oracle import torch_raster as tr
from oracle.lm_ref import OracleLMProblem
from scenes import BG_GENERIC, assert_lm_bg_scene, lm_bg_mask, lm_bg_scene, to_float64

NAME = "sh1_33x17"


def _problem():
    model, cams = lm_bg_scene(NAME)
    stats = assert_lm_bg_scene(model, cams[0], BG_GENERIC)  # measured: 15.1 % saturated, 46.2 % show the background
    cams[0].alpha_mask = lm_bg_mask(NAME)
    mc, cc = to_float64(model, cams)
    return OracleLMProblem(mc, cc, torch.tensor(BG_GENERIC, dtype=torch.float64)), stats


def _direction(op, mask_xyz, seed=5):
    v = torch.randn(op.layout.numel, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    a, b = op.layout.offsets["exposure"]
    v[a:b] = 0
    if mask_xyz:
        a, b = op.layout.offsets["xyz"]
        v[a:b] = 0
    else:
        a, b = op.layout.offsets["xyz"]
        v[a:b] *= 0.05  # world units: small against the Gaussians' extent (s0 = 0.06)
        # Gaussians outside 1.3 tan(FoV / 2) keep their position: there the reference (computeCov2D's backward) and the
        # oracle treat the clamped view coordinate as a constant, which is not the derivative of the value (measured:
        # 17 such Gaussians, 12 of them visible; moving them leaves an h-independent 3.0e-5 between FD and J v)
        cam = op.cams[0]
        xyz = op.model._xyz.detach()
        pv = torch.cat([xyz, torch.ones(len(xyz), 1, dtype=xyz.dtype)], dim=1) @ cam.world_view_transform
        outside = ((pv[:, 0] / pv[:, 2]).abs() > 1.3 * math.tan(cam.FoVx * 0.5)) | \
                  ((pv[:, 1] / pv[:, 2]).abs() > 1.3 * math.tan(cam.FoVy * 0.5))
        assert 0 < int(outside.sum()) < 0.1 * len(xyz)
        v[a:b].view(-1, 3)[outside] = 0
    return v


def _at(op, v, h):
    """(residual, raw render) of the single view at theta + h v."""
    leaves = op._leaves()
    views = op.layout.views(v)
    names = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "exposure")
    with torch.no_grad():
        for t, n in zip(leaves, names):
            t.add_(h * views[n].reshape(t.shape))
        try:
            r = op._residuals()[0].clone()
            raw = tr.render_model(op.model, op.cams[0], op.bg)[3].clone()
        finally:
            for t, n in zip(leaves, names):
                t.sub_(h * views[n].reshape(t.shape))
    return r, raw


@pytest.mark.parametrize("mask_xyz", [True, False])
def test_jv_equals_central_difference_of_the_residual(mask_xyz):
    op, stats = _problem()
    v = _direction(op, mask_xyz)
    jv = op._jr_v(v)[0]
    scale = float(jv.abs().max())
    assert scale > 0
    m = op.cams[0].alpha_mask
    # the tangent is zero where the mask is zero and where the render is saturated, and nowhere else in bulk
    assert float(jv[:, m[0] == 0].abs().max()) == 0.0
    assert float(jv[stats["raw"] > 1].abs().max()) == 0.0
    errs = []
    for h in (1e-4, 1e-5):
        (rp, rawp), (rm, rawm) = _at(op, v, h), _at(op, v, -h)
        fd = (rp - rm) / (2 * h)
        lo, hi = torch.minimum(rawp, rawm), torch.maximum(rawp, rawm)
        crossing = ((lo < 0) & (hi > 0)) | ((lo < 1) & (hi > 1))
        assert int(crossing.sum()) <= 0.01 * crossing.numel()
        errs.append(float(((fd - jv).abs() * (~crossing)).max()) / scale)
    print(f"mask_xyz={mask_xyz}: |FD - J v| / max |J v| = {errs[0]:.3e} (h = 1e-4), {errs[1]:.3e} (h = 1e-5)")
    assert errs[1] < errs[0], errs
    assert errs[1] <= 1e-6, errs


@pytest.mark.parametrize("mask_xyz", [True, False])
def test_adjoint_identity(mask_xyz):
    op, _ = _problem()
    v = _direction(op, mask_xyz)
    jv = op._jr_v(v)[0]
    u = torch.randn(jv.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    leaves = op._leaves()
    r = op._residuals()[0]
    grads = torch.autograd.grad((r * u).sum(), leaves, allow_unused=True)
    jtu = torch.cat([(g if g is not None else torch.zeros_like(t)).reshape(-1) for g, t in zip(grads, leaves)])
    lhs, rhs = float((jv * u).sum()), float((v * jtu).sum())
    print(f"mask_xyz={mask_xyz}: <J v, u> = {lhs!r}, <v, J^T u> = {rhs!r}, rel {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs) > 0
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)
