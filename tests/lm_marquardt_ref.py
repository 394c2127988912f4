"""Yardsticks of Marquardt-scaled damping D = lambda max(diag(J^T W J), floor) on the CPU oracle
(tests/test_oracle_lm_marquardt.py, tests/test_gpu_lm_marquardt.py).

MarquardtOracle   A v = A0 v + lambda max(diag, floor) (.) v, with A0 the OracleLMProblem at zero damping and diag
                  lm_diag_ref.jacobian_diag(damp=False) (or any diagonal the caller has: the closed form, which the
                  CPU suite holds to the dense Jacobian at 1e-10).  projected=True: the operator on the single-view
                  projected layout, A v = P (A0 (E v)) + d (.) v with E = Bh (x) . the expansion and P = E^T, and d
                  from the diagonal of (J Bh)^T W (J Bh).  With one view the SH-rest columns of J are B_k (d rgb),
                  so that diagonal is sum_k of the full layout's SH-rest diagonal (|B|^2 S_col = sum_k B_k^2 S_col);
                  projected_diag() forms it that way and dense_jacobian() / projected_diag_dense() from J itself.
                  It has OracleLMProblem's interface as far as lm_diag_ref.pcg_ref uses it (matvec, loss).
rest_basis        Bh_k(dir_i) = B_k / |B_rest| of the view, from torch_raster.eval_sh on unit coefficient vectors.
dense_jacobian    J of the [r; r] residual's one copy r, rows = residual elements, columns = the flat layout.

Bounds of the GPU comparison: 8 x the float32 oracle restatement's own distance from float64, capped at
lm_diag_ref.MAX_TOL (lm_diag_ref's rule).  The floors below were measured by tests/test_oracle_lm_marquardt.py, which
asserts they are not exceeded."""
import torch

import lm_diag_ref as R
from gslm.params import GROUPS, ParamLayout
from oracle import torch_raster as tr
from oracle.lm_ref import OracleLMProblem

ZERO_DAMP = {g: 0.0 for g in GROUPS}
# The cases of the lm_step and solver tests: one lambda on every group, and a floor that is a power of two (so that
# floor / 4 is exact in any format, as the residual-scale tests need).
LAMBDA = 1e-1
FLOOR = 2.0 ** -10
SOLVE_TOL = 1e-4  # |x - x64| / |x64|: the bound the other CGLS tests hold against the float64 helper
# float32 oracle vs float64, the product A v (v = J^T b) per group relative to the group's max, over sh1_33x17 and
# sh3_40x33 (masked, brightened; one view in the full and the projected layout, two views in the full one; floor 0
# and FLOOR), each precision with its own J^T b and diagonal.  Measured, worst over layouts and floors:
#                     features_dc  features_rest  scaling  rotation  opacity
#   sh1_33x17 1 view  1.7e-6       1.7e-6         1.3e-6   1.5e-6    2.2e-6
#   sh3_40x33 1 view  9.1e-7       9.7e-7         2.0e-6   2.1e-6    1.4e-6
#   sh1_33x17 2 views 5.4e-7       5.2e-7         1.4e-6   1.4e-6    5.7e-7
#   sh3_40x33 2 views 8.5e-7       8.6e-7         1.1e-6   1.9e-6    1.5e-6
PRODUCT_F32_FLOOR = {"features_dc": 2.5e-6, "features_rest": 2.5e-6, "scaling": 3.0e-6, "rotation": 3.0e-6,
                     "opacity": 3.2e-6}
PRODUCT_GPU_TOL = {k: min(8.0 * v, R.MAX_TOL) for k, v in PRODUCT_F32_FLOOR.items()}
# float32 oracle restatement of each solve vs float64, |x32 - x64| / |x64|, on sh1_33x17 (no mask, not brightened,
# full layout, lambda = LAMBDA): (precond, max_iter, restart_iter, floor) -> recorded floor.  A schedule qualifies for
# the GPU comparison at SOLVE_TOL when its floor is within SOLVE_TOL / 8.
#   measured       plain F   plain 0   jacobi F   jacobi 0         (F = FLOOR)
#   2 x 1          7.4e-7    7.4e-7    1.7e-6     1.2e-3
#   5 x 5          1.1e-6    1.1e-6    3.6e-6     3.4e-3
#   10 x 1         9.6e-7    9.6e-7    2.3e-6     1.7e-3
#   10 x 10        1.5e-6    1.5e-6    8.2e-6     2.0e-2
# Jacobi without a floor does not qualify at any schedule: M = (1 + lambda) diag down to entries of 1e-15, so z = M^-1 s
# amplifies float32 rounding in s by up to 1e15 on parameters the image barely depends on (|x| = 3e5 .. 5e5 against
# 8 .. 43 with the floor or without the preconditioner).
SOLVE_F32_FLOOR = {
    ("plain", 2, 1, FLOOR): 1.2e-6, ("plain", 2, 1, 0.0): 1.2e-6, ("jacobi", 2, 1, FLOOR): 2.5e-6,
    ("plain", 5, 5, FLOOR): 1.6e-6, ("plain", 5, 5, 0.0): 1.6e-6, ("jacobi", 5, 5, FLOOR): 5.5e-6,
    ("plain", 10, 1, FLOOR): 1.5e-6, ("plain", 10, 1, 0.0): 1.5e-6, ("jacobi", 10, 1, FLOOR): 3.5e-6,
    ("plain", 10, 10, FLOOR): 2.4e-6, ("plain", 10, 10, 0.0): 2.4e-6, ("jacobi", 10, 10, FLOOR): 1.2e-5,
}
SOLVE_NOT_QUALIFIED = {("jacobi", 2, 1, 0.0): 1.2e-3, ("jacobi", 5, 5, 0.0): 3.4e-3, ("jacobi", 10, 1, 0.0): 1.7e-3,
                       ("jacobi", 10, 10, 0.0): 2.0e-2}
# the solves tests/test_gpu_lm_marquardt.py compares with the float64 restatement (and the CPU suite re-measures)
GPU_SOLVE_CASES = (("plain", 2, 1, FLOOR), ("jacobi", 2, 1, FLOOR), ("plain", 5, 5, FLOOR), ("jacobi", 5, 5, FLOOR),
                   ("plain", 2, 1, 0.0), ("jacobi", 10, 1, FLOOR))


def lam_map(lam=LAMBDA):
    return {g: float(lam) for g in GROUPS}


def rest_basis(model, cam):
    """Bh [P, K-1] in the model's dtype: B_k(dir_i) / |B_rest(dir_i)| over the active degree (0 beyond it, and for a
    Gaussian whose B_rest vanishes)."""
    P, K = model._xyz.shape[0], 1 + model._features_rest.shape[1]
    dtype = model._xyz.dtype
    d = model.get_xyz.detach() - cam.camera_center.to(dtype)[None]
    d = d / d.norm(dim=1, keepdim=True)
    B = torch.zeros(P, K, dtype=dtype)
    nc = (model.active_sh_degree + 1) ** 2
    for k in range(min(K, nc)):
        sh = torch.zeros(P, K, 3, dtype=dtype)
        sh[:, k, 0] = 1.0
        B[:, k] = tr.eval_sh(model.active_sh_degree, sh, d)[:, 0]
    rest = B[:, 1:]
    nb = rest.norm(dim=1, keepdim=True)
    return torch.where(nb > 0, rest / nb.clamp_min(1e-300), torch.zeros_like(rest))


def projected_layout(layout):
    return ParamLayout(layout.P, layout.K, layout.n_exposure, rest_projected=True)


def expand(v, Bh, full, proj):
    """projected layout -> full: the SH-rest group Bh_k v[i, c]."""
    out = torch.zeros(full.numel, dtype=v.dtype)
    fv, pv = full.views(out), proj.views(v)
    for g in GROUPS:
        if g != "features_rest":
            fv[g].copy_(pv[g])
    fv["features_rest"].copy_(Bh[:, :, None] * pv["features_rest"].reshape(-1, 1, 3))
    return out


def project(v, Bh, full, proj):
    """full layout -> projected: sum_k Bh_k v[i, k, c] (the transpose of expand)."""
    out = torch.zeros(proj.numel, dtype=v.dtype)
    fv, pv = full.views(v), proj.views(out)
    for g in GROUPS:
        if g != "features_rest":
            pv[g].copy_(fv[g])
    pv["features_rest"].copy_((Bh[:, :, None] * fv["features_rest"]).sum(dim=1, keepdim=True))
    return out


def projected_diag(diag_full, full, proj):
    """diag of (J Bh)^T W (J Bh) from the full layout's diagonal of ONE view: the SH-rest entry of channel c is
    sum_k diag_full[k, c] (see the module docstring); the other groups are the full layout's."""
    out = torch.zeros(proj.numel, dtype=diag_full.dtype)
    fv, pv = full.views(diag_full), proj.views(out)
    for g in GROUPS:
        if g != "features_rest":
            pv[g].copy_(fv[g])
    pv["features_rest"].copy_(fv["features_rest"].sum(dim=1, keepdim=True))
    return out


def dense_jacobian(model, cams, bg):
    """J [rows, layout.numel] of r = m clamp01(R) - gt over the views (one copy of the [r; r] pair: J^T W J of the
    product is 2 J^T J), xyz and exposure columns zeroed as OracleLMProblem._mask does.  The model's dtype."""
    leaves = R._leaves(model)
    lay = R.layout_of(model)
    rows = []
    for cam in cams:
        for _, r, _, _, _ in R.tile_residuals(model, cam, bg):
            flat = r.reshape(-1)
            eye = torch.eye(flat.numel(), dtype=flat.dtype)
            for k0 in range(0, flat.numel(), R.CHUNK):
                grads = torch.autograd.grad(flat, leaves, grad_outputs=eye[k0:k0 + R.CHUNK], retain_graph=True,
                                            allow_unused=True, is_grads_batched=True)
                n = min(R.CHUNK, flat.numel() - k0)
                rows.append(torch.cat([(g if g is not None else torch.zeros(n, *t.shape, dtype=t.dtype)).reshape(n, -1)
                                       for g, t in zip(grads, leaves)], dim=1).detach())
    J = torch.cat(rows, dim=0)
    for name in ("xyz", "exposure"):
        a, b = lay.offsets[name]
        J[:, a:b] = 0
    return J


def projected_diag_dense(J, Bh, full, proj):
    """diag(2 (J E)^T (J E)) from the dense J, E the expansion: the definition of the projected layout's diagonal."""
    a, b = full.offsets["features_rest"]
    P, Km1 = Bh.shape
    Jr = J[:, a:b].reshape(-1, P, Km1, 3)
    JE = (Jr * Bh[None, :, :, None]).sum(dim=2)  # [rows, P, 3]
    out = projected_diag(2.0 * (J * J).sum(dim=0), full, proj)
    proj.views(out)["features_rest"].copy_((2.0 * (JE * JE).sum(dim=0)).reshape(P, 1, 3))
    return out


def damping_vector(diag, layout, lam, floor):
    """lambda[group] max(diag, floor) in diag's dtype (the select form: a NaN diagonal stays NaN)."""
    d = torch.where(diag < floor, torch.full_like(diag, floor), diag)
    for g in GROUPS:
        a, b = layout.offsets[g]
        d[a:b] *= lam[g]
    return d


class MarquardtOracle:
    """A v = A0 v + d (.) v on the oracle; see the module docstring.  `d` may be given (a caller's damping vector in
    the operator's layout) instead of (diag, lam, floor)."""

    def __init__(self, model, cams, bg, diag=None, lam=None, floor=0.0, projected=False, d=None):
        self.op = OracleLMProblem(model, cams, bg, damp=ZERO_DAMP)
        self.full = self.op.layout
        self.projected = bool(projected) and self.full.K > 1
        self.layout = projected_layout(self.full) if self.projected else self.full
        self.Bh = rest_basis(model, cams[0]) if self.projected else None
        if self.projected and len(cams) != 1:
            raise ValueError("the projected layout is a single-view mode")
        if d is None:
            if self.projected:
                diag = projected_diag(diag, self.full, self.layout)
            d = damping_vector(diag, self.layout, lam_map() if lam is None else lam, floor)
        self.d = d
        self.loss = None

    def evaluate(self):
        self.loss = self.op.evaluate()
        return self.loss

    def rhs(self):
        g = self.op.rhs()
        return project(g, self.Bh, self.full, self.layout) if self.projected else g

    def matvec(self, v, y):
        if self.projected:
            yf = self.op.local_normal_matvec(expand(v, self.Bh, self.full, self.layout),
                                             torch.zeros(self.full.numel, dtype=v.dtype), damp=False)
            y.copy_(project(yf, self.Bh, self.full, self.layout))
        else:
            self.op.local_normal_matvec(v, y, damp=False)
        # (the oracle masks xyz and exposure out of v, D included: J has no column there and the iterates are zero)
        y += self.d * self._mask(v.clone())
        return y

    def _mask(self, vec):
        o = self.layout.offsets
        vec[o["xyz"][0]:o["xyz"][1]] = 0
        vec[o["exposure"][0]:o["exposure"][1]] = 0
        return vec


def group_errors(got, ref, layout):
    return R.group_errors(got, ref, layout)
