"""Yardsticks of the robust LM losses (tests/test_oracle_lm_robust.py, tests/test_gpu_lm_robust.py).

The loss is 2 sum rho(r^2) over the residual elements r = m clamp01(R) - gt:
  huber    rho(s) = s where |r| <= delta, 2 delta |r| - delta^2 elsewhere;   rho' = 1, delta / |r|
  cauchy   rho(s) = delta^2 log1p(s / delta^2);                              rho' = 1 / (1 + (r / delta)^2)
RobustOracleLMProblem   oracle.lm_ref.OracleLMProblem whose residual blocks are sqrt(rho').detach() r (iteratively
                        reweighted least squares, the first-order Triggs form) and whose loss is the robust one: rhs()
                        is then -1/2 grad loss exactly, the product 2 J^T diag(rho') J + D, and cgls_ref's monitor the
                        quadratic model of the robust loss.  It runs in the model's dtype (float64 via to_float64).
RobustOracleLossEvaluator   the matching line-search loss (OracleLossEvaluator's interface).
epilogue_f32            the residual epilogue of the HIP kernels restated in float32 torch on the CPU, operation by
                        operation: residual, weight, seed as floats and the per-element rho terms in double.

Bounds of the GPU comparison: 8 x the float32 oracle's own distance from the float64 one (F32_FLOOR, measured and
asserted by tests/test_oracle_lm_robust.py::test_float32_floor), per group relative to the group's max, capped at
MAX_TOL: a weight or seed without its rho' is an O(1) error."""
import torch

from oracle.lm_ref import OracleLMProblem, OracleLossEvaluator

KINDS = ("huber", "cauchy")
# scene -> delta at which the reference alone keeps 25%..75% of the residual elements on each side of |r| = delta
# (tests/test_oracle_lm_robust.py::test_both_branches_busy: 0.601 outside on sh1_33x17, 0.592 on sh3_40x33)
DELTA = {"sh1_33x17": 0.25, "sh3_40x33": 0.25}
GROUPS5 = ("features_dc", "features_rest", "scaling", "rotation", "opacity")
# float32 oracle vs float64 oracle (RobustOracleLMProblem in both), max |x32 - x64| / max |x64| per group (relative for
# the loss), measured on sh1_33x17 (masked) / sh3_40x33, generic background, delta 0.25, huber | cauchy
# (tests/test_oracle_lm_robust.py::test_float32_floor prints the measurements and asserts they stay below the floors):
#   loss                   1.0e-8  2.3e-9 | 5.7e-9  5.0e-9
#   J^T b    features_dc   1.2e-6  5.6e-7 | 1.3e-6  6.7e-7      features_rest 1.2e-6  4.5e-7 | 1.2e-6  5.7e-7
#            scaling       1.2e-6  1.1e-6 | 1.4e-6  2.1e-6      rotation      4.4e-7  7.2e-7 | 3.7e-7  1.1e-6
#            opacity       5.8e-7  7.4e-7 | 5.4e-7  7.6e-7
#   product  features_dc   3.5e-7  5.6e-7 | 3.8e-7  5.3e-7      features_rest 3.4e-7  5.2e-7 | 4.8e-7  4.7e-7
#   (randn   scaling       8.1e-7  9.8e-7 | 7.3e-7  1.2e-6      rotation      1.1e-6  1.0e-6 | 1.0e-6  1.0e-6
#   seed 5)  opacity       7.6e-7  6.6e-7 | 8.1e-7  6.6e-7
#   solve    features_dc   6.0e-6  2.5e-6 | 2.0e-6  2.1e-6      features_rest 5.8e-6  2.0e-6 | 1.5e-6  2.1e-6
#   (5 x 5   scaling       1.4e-5  1.3e-6 | 3.1e-6  2.0e-6      rotation      1.1e-4  2.3e-6 | 2.4e-5  2.7e-6
#   cgls)    opacity       6.8e-6  2.0e-6 | 2.8e-6  1.7e-6
F32_FLOOR = {
    "loss": 1.2e-8,
    "rhs": {"features_dc": 1.4e-6, "features_rest": 1.4e-6, "scaling": 2.2e-6, "rotation": 1.2e-6, "opacity": 8.5e-7},
    "product": {"features_dc": 6.5e-7, "features_rest": 6.0e-7, "scaling": 1.4e-6, "rotation": 1.2e-6,
                "opacity": 9.0e-7},
    "solve": {"features_dc": 6.5e-6, "features_rest": 6.5e-6, "scaling": 1.5e-5, "rotation": 1.2e-4, "opacity": 7.5e-6},
}
MAX_TOL = 1e-3
GPU_TOL = {q: (min(8.0 * f, MAX_TOL) if not isinstance(f, dict) else {k: min(8.0 * v, MAX_TOL) for k, v in f.items()})
           for q, f in F32_FLOOR.items()}
PRODUCT_SEED = 5  # the random direction of the product's floor (float64 randn of the reference's layout)


def group_errors(got, ref, layout, groups=GROUPS5):
    """{group: max |got - ref| / max |ref|} in float64."""
    gv, rv = layout.views(got.double()), layout.views(ref.double())
    return {k: float((gv[k] - rv[k]).abs().max() / rv[k].abs().max().clamp_min(1e-300)) for k in groups
            if rv[k].numel()}


def direction(layout, dtype=torch.float64):
    return torch.randn(layout.numel, generator=torch.Generator().manual_seed(PRODUCT_SEED), dtype=torch.float64).to(dtype)


def rho(r, kind, delta):
    """rho(r^2) elementwise, in r's dtype."""
    a = r.abs()
    if kind == "huber":
        return torch.where(a <= delta, r * r, 2.0 * delta * a - delta * delta)
    if kind == "cauchy":
        return (delta * delta) * torch.log1p((r / delta) ** 2)
    raise ValueError(kind)


def rho_prime(r, kind, delta):
    """rho'(r^2) elementwise, in r's dtype."""
    a = r.abs()
    if kind == "huber":
        return torch.where(a <= delta, torch.ones_like(r), delta / a)
    if kind == "cauchy":
        return 1.0 / (1.0 + (r / delta) ** 2)
    raise ValueError(kind)


class RobustOracleLMProblem(OracleLMProblem):
    def __init__(self, model, cams, bg, robust, **kw):
        super().__init__(model, cams, bg, **kw)
        self.kind, self.delta = robust

    def raw_residuals(self):
        return super()._residuals()

    def _residuals(self):
        return [torch.sqrt(rho_prime(r, self.kind, self.delta)).detach() * r for r in self.raw_residuals()]

    def evaluate(self):
        with torch.no_grad():
            self.loss = torch.zeros((), dtype=torch.float64)
            for r in self.raw_residuals():
                self.loss = self.loss + 2.0 * rho(r, self.kind, self.delta).double().sum()
        return self.loss

    def robust_loss(self):
        """The robust loss with its graph (for autograd: rhs() must be -1/2 of its gradient)."""
        return sum(2.0 * rho(r, self.kind, self.delta).sum() for r in self.raw_residuals())


class RobustOracleLossEvaluator(OracleLossEvaluator):
    def __init__(self, model, cams, bg, robust, device="cpu", batch=8, reduce=None):
        self.prob = RobustOracleLMProblem(model, cams, bg, robust)
        self.reduce = reduce


def epilogue_f32(color, gt, mask, kind, delta):
    """gslm_lm_residual_robust restated: float32 CPU tensors color / gt [3, H, W], mask [H, W] or None.  Returns
    residual, weight, seed in float32 and the per-element rho in float64 (the loss is 2 x their sum).  One float test
    |r| <= delta serves rho' and rho; rho' in float32 (IEEE divisions, products and sums apart); rho in double from
    double(r) and double(float32(delta))."""
    assert color.dtype == torch.float32 and gt.dtype == torch.float32 and color.device.type == "cpu"
    d = torch.tensor(delta, dtype=torch.float32)
    m = torch.ones(color.shape[1:], dtype=torch.float32) if mask is None else mask.reshape(color.shape[1:]).float()
    m = m[None]
    inside = ((color >= 0) & (color <= 1)).float()
    clamped = torch.where(color < 0, torch.zeros_like(color), torch.where(color > 1, torch.ones_like(color), color))
    r = m * clamped - gt
    a = r.abs()
    inl = a <= d
    rd, dd = r.double(), d.double()
    if kind == "huber":
        dr = torch.where(inl, torch.ones_like(r), d / a)
        terms = torch.where(inl, rd * rd, (2.0 * dd) * rd.abs() - dd * dd)
    elif kind == "cauchy":
        t = r / d
        dr = 1.0 / (1.0 + t * t)
        q = rd / dd
        terms = (dd * dd) * torch.log1p(q * q)
    else:
        raise ValueError(kind)
    weight = ((m * m) * inside) * dr
    seed = (((-2.0 * m) * inside) * r) * dr
    return r, weight, seed, terms
