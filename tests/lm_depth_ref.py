"""Yardsticks of the inverse-depth residual of the LM step (tests/test_oracle_lm_depth.py, tests/test_gpu_lm_depth.py).

The loss is 2 sum ||m clamp01(R) - gt||^2 + lambda_d sum (m_d (D - Dgt))^2, D the rendered inverse depth (no
background term, no clamp); the depth block enters once, not aliased [r; r].
DepthOracleLMProblem    oracle.lm_ref.OracleLMProblem whose residual block of a camera with a depth target is the
                        [4, H, W] cat([m clamp01(R) - gt, sqrt(lambda_d / 2) m_d (D - Dgt)]): the oracle's factor 2 on
                        every block then yields lambda_d.  One block per camera (_jr_v zips blocks against cameras); a
                        camera without depth_reliable or without an invdepthmap keeps its [3, H, W] block.  It runs in
                        the model's dtype (float64 via scenes.to_float64).
DepthOracleLossEvaluator    the matching line-search loss (OracleLossEvaluator's interface).
epilogue_f32            gslm_lm_residual_depth restated in float32 torch on the CPU, operation by operation: residual,
                        weight, seed as floats and the per-pixel loss terms in double.
set_depth_targets       the target recipe: Dgt = D (0.7 + 0.6 u), m_d = 1[u' > 0.2], u and u' uniform draws of one
                        generator (seed 3 + view), D the float32 oracle's inverse depth of the scene as it stands.

Bounds of the GPU comparison: 8 x the float32 oracle's own distance from the float64 one (F32_FLOOR, measured and
asserted by tests/test_oracle_lm_depth.py::test_float32_floor), per group relative to the group's max, capped at
MAX_TOL -- the convention of tests/lm_robust_ref.py.  No bound comes from a GPU number."""
import torch

from oracle import torch_raster as tr
from oracle.lm_ref import OracleLMProblem, OracleLossEvaluator
from scenes import lm_bg_mask, lm_bg_scene, to_float64

SCENES = ("sh1_33x17", "sh3_40x33")
GROUPS5 = ("features_dc", "features_rest", "scaling", "rotation", "opacity")
DEPTH_GROUPS = ("scaling", "rotation", "opacity")  # the groups J_D has columns in (xyz frozen: through alpha only)
# At lambda_d = 4 the depth term is 0.9-3 % of the colour's J^T b; LAMBDA_D is the smallest power of two at which the
# depth share of J^T b and of the product reaches 0.25 of the colour part's group max in every DEPTH_GROUPS group of
# both scenes (tests/test_oracle_lm_depth.py::test_lambda_is_large_enough_to_matter prints and asserts the shares).
LAMBDA_D = 128.0
TARGET_SEED = 3
PRODUCT_SEED = 5  # the random direction of the product's floor (float64 randn of the reference's layout)
MAX_TOL = 1e-3
# float32 oracle vs float64 oracle (DepthOracleLMProblem in both) at LAMBDA_D, max |x32 - x64| / max |x64| per group
# (relative for the loss), measured on sh1_33x17 (masked) one view | two views, the second without depth, and
# sh3_40x33 one view | two views likewise, generic background (tests/test_oracle_lm_depth.py::test_float32_floor prints
# the measurements and asserts they stay below the floors):
#   loss                   6.3e-9  2.3e-9 | 1.1e-8  1.5e-8
#   J^T b    features_dc   1.0e-6  6.2e-7 | 5.0e-7  4.1e-7      features_rest 8.3e-7  5.4e-7 | 5.1e-7  6.5e-7
#            scaling       2.0e-6  2.0e-6 | 5.1e-6  3.7e-6      rotation      1.5e-6  1.8e-6 | 5.2e-6  4.7e-6
#            opacity       1.9e-6  1.8e-6 | 4.6e-6  2.7e-6
#   product  features_dc   3.6e-7  5.0e-7 | 5.7e-7  6.3e-7      features_rest 3.3e-7  6.0e-7 | 4.4e-7  5.8e-7
#   (randn   scaling       8.6e-7  8.8e-7 | 1.3e-6  1.0e-6      rotation      1.7e-6  1.7e-6 | 3.6e-7  3.6e-7
#   seed 5)  opacity       5.1e-7  4.8e-7 | 7.7e-7  7.2e-7
#   solve    features_dc   1.7e-6  9.6e-7 | 1.5e-6  1.2e-6      features_rest 1.4e-6  9.6e-7 | 1.5e-6  1.6e-6
#   (5 x 5   scaling       1.7e-6  1.2e-6 | 3.2e-6  2.8e-6      rotation      1.4e-6  2.1e-6 | 1.6e-6  1.6e-6
#   cgls)    opacity       2.3e-6  1.7e-6 | 3.8e-6  3.0e-6
F32_FLOOR = {
    "loss": 1.8e-8,
    "rhs": {"features_dc": 1.2e-6, "features_rest": 1.0e-6, "scaling": 5.8e-6, "rotation": 5.8e-6, "opacity": 5.2e-6},
    "product": {"features_dc": 7.2e-7, "features_rest": 7.0e-7, "scaling": 1.5e-6, "rotation": 1.9e-6,
                "opacity": 9.0e-7},
    "solve": {"features_dc": 2.0e-6, "features_rest": 1.8e-6, "scaling": 3.7e-6, "rotation": 2.4e-6, "opacity": 4.4e-6},
}


def _tol(f):
    return {k: min(8.0 * v, MAX_TOL) for k, v in f.items()} if isinstance(f, dict) else min(8.0 * f, MAX_TOL)


GPU_TOL = {q: _tol(f) for q, f in F32_FLOOR.items()}


def group_errors(got, ref, layout, groups=GROUPS5):
    """{group: max |got - ref| / max |ref|} in float64."""
    gv, rv = layout.views(got.double()), layout.views(ref.double())
    return {k: float((gv[k] - rv[k]).abs().max() / rv[k].abs().max().clamp_min(1e-300)) for k in groups
            if rv[k].numel()}


def direction(layout, dtype=torch.float64, seed=PRODUCT_SEED):
    return torch.randn(layout.numel, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def set_depth_targets(model, cams, bg, views=None):
    """The recipe on the cameras `views` (default: all): invdepthmap, depth_mask (float32 [1, H, W]) and
    depth_reliable = True; the other cameras keep depth_reliable = False.  D is rendered once, in float32, from the
    model as it stands, so a float64 copy of the cameras (scenes.to_float64 leaves these fields alone) holds the same
    target values."""
    views = range(len(cams)) if views is None else views
    bg = torch.as_tensor(bg, dtype=torch.float32)
    for i in views:
        c = cams[i]
        with torch.no_grad():
            D = tr.render_model(model, c, bg)[2].float()
        gen = torch.Generator().manual_seed(TARGET_SEED + i)
        u = torch.rand(D.shape, generator=gen)
        u2 = torch.rand(D.shape, generator=gen)
        c.invdepthmap = (D * (0.7 + 0.6 * u)).contiguous()
        c.depth_mask = (u2 > 0.2).float()
        c.depth_reliable = True
    return cams


def scene(name, f64=True, n_views=1, depth_views=None, occluders=False):
    """The scene as every depth test takes it: sh1_33x17 with alpha masks (seed = view), sh3_40x33 without; the depth
    targets of the recipe on `depth_views` (default: every view)."""
    from scenes import BG_GENERIC
    model, cams = lm_bg_scene(name, n_views=n_views, occluders=occluders)
    if name == "sh1_33x17":
        for i, c in enumerate(cams):
            c.alpha_mask = lm_bg_mask(name, seed=i)
    set_depth_targets(model, cams, BG_GENERIC, depth_views)
    return to_float64(model, cams) if f64 else (model, cams)


def has_depth(cam):
    return bool(getattr(cam, "depth_reliable", False)) and getattr(cam, "invdepthmap", None) is not None


class DepthOracleLMProblem(OracleLMProblem):
    def __init__(self, model, cams, bg, depth_weight, colour=True, **kw):
        """colour=False: the depth block alone (the colour residual and its columns dropped), for the depth share."""
        super().__init__(model, cams, bg, **kw)
        self.depth_weight = float(depth_weight)
        self.colour = colour

    def _blocks(self):
        """Per camera (colour residual [3, H, W], unscaled depth residual m_d (D - Dgt) [1, H, W] or None)."""
        out = []
        for c in self.cams:
            img, _, invd, _ = tr.render_model(self.model, c, self.bg)
            rc = img * c.alpha_mask - c.original_image
            rd = None
            if has_depth(c):
                m = torch.ones_like(invd) if c.depth_mask is None else c.depth_mask.to(invd.dtype)
                rd = m * (invd - c.invdepthmap.to(invd.dtype))
            out.append((rc, rd))
        return out

    def _residuals(self):
        s = (0.5 * self.depth_weight) ** 0.5
        out = []
        for rc, rd in self._blocks():
            if not self.colour:
                rc = torch.zeros_like(rc) if rd is None else None
            parts = [t for t in (rc, None if rd is None else s * rd) if t is not None]
            out.append(torch.cat(parts))
        return out

    def stated_loss(self):
        """2 sum ||r_c||^2 + lambda_d sum r_d^2 with its graph, written as the issue states it (not through the
        blocks' common factor): rhs() must be -1/2 of its gradient."""
        total = 0.0
        for rc, rd in self._blocks():
            total = total + 2.0 * (rc * rc).sum()
            if rd is not None:
                total = total + self.depth_weight * (rd * rd).sum()
        return total


class DepthOracleLossEvaluator(OracleLossEvaluator):
    def __init__(self, model, cams, bg, depth_weight, device="cpu", batch=8, reduce=None):
        self.prob = DepthOracleLMProblem(model, cams, bg, depth_weight)
        self.reduce = reduce


def epilogue_f32(invdepth, gt, mask, depth_weight):
    """gslm_lm_residual_depth restated: float32 CPU tensors invdepth / gt [H, W], mask [H, W] or None.  Returns
    residual, weight, seed in float32 and the per-pixel loss terms in float64 (the loss is their sum).
      r = m * (D - gt);  w = (float)lambda_d * (m * m);  seed = (-w) * r;  term = lambda_d * ((double)r * (double)r)."""
    assert invdepth.dtype == torch.float32 and gt.dtype == torch.float32 and invdepth.device.type == "cpu"
    m = torch.ones_like(invdepth) if mask is None else mask.reshape(invdepth.shape).float()
    lam = torch.tensor(depth_weight, dtype=torch.float32)
    r = m * (invdepth - gt)
    w = lam * (m * m)
    seed = (-w) * r
    rd = r.double()
    terms = float(depth_weight) * (rd * rd)
    return r, w, seed, terms
