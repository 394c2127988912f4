"""CPU: the yardsticks of Marquardt-scaled damping (tests/lm_marquardt_ref.py) pinned on the oracle, the invariances
the mode exists for, the float32 floors behind the GPU bounds, and the host-side argument checks.

Scene: lm_bg_scene("sh1_33x17") -- 600 Gaussians, SH 1, 33x17, generic background.  The diagonal of the unmasked,
not brightened scene (float64): per-group medians of the nonzero entries 7e-5 (rotation) .. 1.7e-3 (features_dc), the
smallest nonzero entries 1e-13 .. 1e-15 (features_rest, scaling), 96 % of the entries nonzero.

What is measured here (float64 unless noted; SCHED = 10 plain CG iterations):
  residual halved exactly (mask 0.5, gt x 0.5)   Marquardt x bitwise equal, float64 and float32, floor 0 and floor f
                                                  against f / 4; the fixed damping's x moves by 0.546 in relative norm
  column scaling S in [1/4, 4] (floor 0)         exact solve and Jacobi-PCG iterates equal S^-1 x to 1e-12 .. 1e-14"""
import ctypes
import functools

import pytest
import torch

import lm_diag_ref as R
import lm_marquardt_ref as M
from scenes import BG_GENERIC, lm_bg_mask, lm_bg_scene, to_float64

SCENE = "sh1_33x17"
FAKE = 16  # a non-NULL pointer nothing may dereference
SCHED = (10, 10)
BG64 = torch.tensor(BG_GENERIC, dtype=torch.float64)
BG32 = torch.tensor(BG_GENERIC)


@functools.lru_cache(maxsize=None)
def _plain():
    """(model32, cams32, model64, cams64) of the unmasked, not brightened scene: computed once, not modified."""
    model, cams = lm_bg_scene(SCENE, brighten=False)
    return (model, cams) + to_float64(model, cams)


@functools.lru_cache(maxsize=None)
def _dense():
    """(J, diagonal from lm_diag_ref.jacobian_diag) of the float64 scene."""
    _, _, m64, c64 = _plain()
    return M.dense_jacobian(m64, c64, BG64), R.jacobian_diag(m64, c64, BG64, damp=False)


# ---------------------------------------------------------------- 1. the yardstick is the operator
def test_yardstick_against_unit_products():
    """e_j^T (A e_j) of MarquardtOracle against diag_j + lambda max(diag_j, floor) on the largest and one seeded
    random column of every group, in the full layout and (the SH-rest group) in the projected one, whose diagonal
    is taken from the dense J: diag(2 (J E)^T (J E)).  The sum over k of the full layout's SH-rest diagonal is that
    number (one view: the columns are B_k d rgb)."""
    _, _, m64, c64 = _plain()
    J, d64 = _dense()
    lay = R.layout_of(m64)
    assert float((2.0 * (J * J).sum(dim=0) - d64).abs().max()) <= 1e-12 * float(d64.max())
    op = M.MarquardtOracle(m64, c64, BG64, diag=d64, floor=M.FLOOR)
    want = d64 + op.d
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    floored = 0
    for name in R.DIAG_GROUPS:
        a, b = lay.offsets[name]
        cols = [int(torch.argmax(d64[a:b])), int(torch.randint(0, b - a, (1,), generator=gen))]
        for j in cols:
            e = torch.zeros(lay.numel, dtype=torch.float64)
            e[a + j] = 1.0
            y = op.matvec(e, torch.zeros(lay.numel, dtype=torch.float64))
            err = abs(float(y[a + j]) - float(want[a + j])) / float(want[a + j])
            worst = max(worst, err)
            floored += int(float(d64[a + j]) < M.FLOOR)
            assert err <= 1e-8, (name, j, float(y[a + j]), float(want[a + j]))
    assert floored >= 1  # (a column whose damping is lambda floor was among them)
    # the projected layout: its diagonal from J itself, and the product on it
    pop = M.MarquardtOracle(m64, c64, BG64, diag=d64, floor=M.FLOOR, projected=True)
    dp = M.projected_diag_dense(J, pop.Bh, pop.full, pop.layout)
    short = M.projected_diag(d64, pop.full, pop.layout)
    assert float((dp - short).abs().max()) <= 1e-12 * float(dp.max())
    a, b = pop.layout.offsets["features_rest"]
    for j in (int(torch.argmax(dp[a:b])), 7):
        e = torch.zeros(pop.layout.numel, dtype=torch.float64)
        e[a + j] = 1.0
        y = pop.matvec(e, torch.zeros_like(e))
        w = float(dp[a + j]) + M.LAMBDA * max(float(dp[a + j]), M.FLOOR)
        err = abs(float(y[a + j]) - w) / w
        worst = max(worst, err)
        assert err <= 1e-8, (j, float(y[a + j]), w)
    print(f"yardstick vs e_j^T A e_j: worst relative error {worst:.2e}")
    # the two layouts' Marquardt operators differ on the SH-rest group: diag_full is not a scalar there
    fr = lay.views(d64)["features_rest"]
    top = int(torch.argmax(fr.sum(dim=(1, 2))))
    assert float(fr[top, :, 0].max() - fr[top, :, 0].min()) > 0.1 * float(fr[top, :, 0].max())


# ---------------------------------------------------------------- 2. residual-scale invariance
def _halved(cams):
    """The cameras with the residual halved exactly: alpha mask 0.5, ground truth x 0.5."""
    import copy
    out = []
    for c in cams:
        c = copy.deepcopy(c)
        c.alpha_mask = torch.full_like(c.alpha_mask, 0.5)
        c.original_image = c.original_image * 0.5
        out.append(c)
    return out


def _solve(model, cams, bg, floor, sched=SCHED):
    diag = R.closed_form(model, cams[0], bg)  # (held to the dense Jacobian at 1e-10 by test_oracle_lm_diag.py)
    op = M.MarquardtOracle(model, cams, bg, diag=diag, floor=floor)
    op.evaluate()
    g = op.rhs()
    return R.pcg_ref(op, g, torch.ones_like(g), *sched), g, diag


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_residual_scale_invariance(dtype):
    """Mask 1 against mask 0.5 with gt x 0.5: W and J^T b scale by 2^-2 bitwise, the diagonal with them, and every
    intermediate of the solve by a power of two -- x is bitwise equal, at floor 0 and at floor f against f / 4."""
    model, cams, m64, c64 = _plain()
    m, c, bg = (m64, c64, BG64) if dtype == "float64" else (model, cams, BG32)
    for f in (0.0, M.FLOOR):
        x1, g1, d1 = _solve(m, c, bg, f)
        x2, g2, d2 = _solve(m, _halved(c), bg, f / 4)
        assert torch.equal(g2, 0.25 * g1) and torch.equal(d2, 0.25 * d1)
        assert float(x1.norm()) > 1.0
        assert torch.equal(x1, x2), (dtype, f, float((x1 - x2).norm() / x1.norm()))


def test_fixed_damping_is_not_residual_scale_invariant():
    from oracle.lm_ref import OracleLMProblem
    _, _, m64, c64 = _plain()
    xs = []
    for cams in (c64, _halved(c64)):
        op = OracleLMProblem(m64, cams, BG64)
        op.evaluate()
        g = op.rhs()
        xs.append(R.pcg_ref(op, g, torch.ones_like(g), *SCHED))
    rel = float((xs[0] - xs[1]).norm() / xs[0].norm())
    print(f"fixed damping, residual halved: |x - x'| / |x| = {rel:.3f}")
    assert rel > 0.1


# ---------------------------------------------------------------- 3. column-scaling invariance
class _Dense:
    """(2 J^T J + diag(d)) on the columns `cols`, with pcg_ref's interface."""

    def __init__(self, J, d, b2):
        self.J, self.d, self.loss = J, d, b2

    def matvec(self, v, y):
        y.copy_(2.0 * (self.J.t() @ (self.J @ v)) + self.d * v)
        return y

    def matrix(self):
        return 2.0 * (self.J.t() @ self.J) + torch.diag(self.d)


def test_column_scaling_invariance():
    """J' = J S for a random positive diagonal S: A0' = S A0 S, g' = S g, diag' = S^2 diag, so with floor 0
    (lambda diag') the exact solve and every Jacobi-PCG iterate of the scaled problem are S^-1 x.  Run on the
    sub-problem of the columns whose diagonal is at least 1e-3 of the largest (itself an LM problem, on fewer
    parameters): the Jacobi-scaled matrix is then C + lambda I with C's eigenvalues in [0, n], so the Cholesky solve
    is good to cond x eps ~ 1e-11 and 1e-10 can be asked.  (A floor is an absolute number on the diagonal: it breaks
    this invariance by design, and restores the solve's conditioning.)"""
    _, _, m64, c64 = _plain()
    J, d64 = _dense()
    op = M.MarquardtOracle(m64, c64, BG64, diag=d64)
    b2 = float(op.evaluate())
    g = op.rhs()
    cols = torch.nonzero(d64 >= 1e-3 * d64.max()).reshape(-1)
    assert 500 <= cols.numel() <= 8000, cols.numel()
    Js, gs = J[:, cols], g[cols]
    diag = 2.0 * (Js * Js).sum(dim=0)
    S = 0.25 * 16.0 ** torch.rand(cols.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    a = _Dense(Js, M.LAMBDA * diag, b2)
    Jp = Js * S[None]
    dp = 2.0 * (Jp * Jp).sum(dim=0)
    b = _Dense(Jp, M.LAMBDA * dp, b2)
    solve = lambda op_, rhs: torch.cholesky_solve(rhs[:, None], torch.linalg.cholesky(op_.matrix()))[:, 0]
    x, xp = solve(a, gs), solve(b, S * gs)
    err = float((xp - x / S).norm() / (x / S).norm())
    print(f"column scaling: exact solve |x' - S^-1 x| / |S^-1 x| = {err:.2e}")
    assert err <= 1e-10
    for k in (1, 2, 5):
        xk = R.pcg_ref(a, gs, 1.0 / (diag + a.d), k, k)
        xpk = R.pcg_ref(b, S * gs, 1.0 / (dp + b.d), k, k)
        err = float((xpk - xk / S).norm() / (xk / S).norm())
        print(f"column scaling: Jacobi-PCG iterate {k}: {err:.2e}")
        assert err <= 1e-10, k
    # plain CG is not invariant: the same comparison without the preconditioner
    xk = R.pcg_ref(a, gs, torch.ones_like(gs), 2, 2)
    xpk = R.pcg_ref(b, S * gs, torch.ones_like(gs), 2, 2)
    assert float((xpk - xk / S).norm() / (xk / S).norm()) > 1e-2


# ---------------------------------------------------------------- 4. float32 floors
def _masked(name, n_views=1):
    model, cams = lm_bg_scene(name, n_views=n_views)
    if name == "sh3_40x33":
        model.active_sh_degree = 2
    for i, c in enumerate(cams):
        c.alpha_mask = lm_bg_mask(name, seed=i)
    return model, cams


@pytest.mark.parametrize("name,n_views", [("sh1_33x17", 1), ("sh3_40x33", 1), ("sh1_33x17", 2), ("sh3_40x33", 2)])
def test_float32_floor_of_the_product(name, n_views):
    """The float32 oracle restatement of A v (v = J^T b, its own diagonal) against the float64 one, per group relative
    to the group's max: full layout and (one view) projected, floor 0 and FLOOR.  The GPU bounds are 8 x the recorded
    floors."""
    model, cams = _masked(name, n_views)
    m64, c64 = to_float64(model, cams)
    worst = {}
    for projected in (False, True)[:3 - n_views]:
        ys = {}
        for tag, m, c, bg in (("f64", m64, c64, BG64), ("f32", model, cams, BG32)):
            diag = sum(R.closed_form(m, cam, bg) for cam in c)
            op = M.MarquardtOracle(m, c, bg, d=torch.zeros(1, dtype=diag.dtype), projected=projected)
            g = op.rhs()
            y0 = op.matvec(g, torch.zeros_like(g))  # A0 v, once per layout and precision
            dl = M.projected_diag(diag, op.full, op.layout) if op.projected else diag
            ys[tag] = [y0 + M.damping_vector(dl, op.layout, M.lam_map(), f) * op._mask(g.clone())
                       for f in (0.0, M.FLOOR)]
            lay = op.layout
        for y32, y64 in zip(ys["f32"], ys["f64"]):
            for k, v in M.group_errors(y32, y64, lay).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"float32 floor of the product ({name}, {n_views} view(s)):", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= M.PRODUCT_F32_FLOOR[k], (k, v)
        assert M.PRODUCT_GPU_TOL[k] == min(8.0 * M.PRODUCT_F32_FLOOR[k], R.MAX_TOL)


def _minv(diag, d, precond):
    dg = diag + d
    return torch.where(dg > 0, 1.0 / dg, torch.zeros_like(dg)) if precond == "jacobi" else torch.ones_like(dg)


@pytest.mark.parametrize("case", sorted(k for k in M.SOLVE_F32_FLOOR if k in M.GPU_SOLVE_CASES))
def test_float32_floor_of_the_solves(case):
    """The float32 oracle restatement of each solve the GPU tests compare against float64: its own distance from the
    float64 solve stays within the recorded floor, and the floor within 1/8 of the GPU bound."""
    precond, max_iter, restart, floor = case
    model, cams, m64, c64 = _plain()
    xs = []
    for m, c, bg in ((m64, c64, BG64), (model, cams, BG32)):
        diag = R.closed_form(m, c[0], bg)
        op = M.MarquardtOracle(m, c, bg, diag=diag, floor=floor)
        op.evaluate()
        g = op.rhs()
        xs.append(R.pcg_ref(op, g, _minv(diag, op.d, precond), max_iter, restart).double())
    err = float((xs[1] - xs[0]).norm() / xs[0].norm())
    print(f"float32 floor of the solve {case}: {err:.2e}")
    assert err <= M.SOLVE_F32_FLOOR[case], (case, err)
    assert M.SOLVE_F32_FLOOR[case] <= M.SOLVE_TOL / 8


# ---------------------------------------------------------------- 5. the step descends
@pytest.mark.parametrize("n_train", [1, 2])
def test_float64_step_lowers_the_validation_loss(n_train):
    """The float64 step at the lm_step test's scene, lambda and floor (2 x 1 iterations, both preconditioners): the
    validation loss at the line search's best alpha is below the start's."""
    import copy
    from gslm.lm import update_params
    from oracle.lm_ref import OracleLossEvaluator, line_search_ref
    model, cams = lm_bg_scene(SCENE, n_views=4, brighten=False)
    m64, c64 = to_float64(model, cams)
    train, val = c64[:n_train], c64[n_train:]
    diag = sum(R.closed_form(m64, c, BG64) for c in train)
    lay = R.layout_of(m64)
    for precond in ("plain", "jacobi"):
        mm = copy.deepcopy(m64)
        op = M.MarquardtOracle(mm, train, BG64, diag=diag, floor=M.FLOOR)
        op.evaluate()
        g = op.rhs()
        x = R.pcg_ref(op, g, _minv(diag, op.d, precond), 2, 1)
        ev = OracleLossEvaluator(mm, val, BG64)
        start = float(ev.evaluate())
        alpha, final, _ = line_search_ref(lambda a: update_params(mm, lay, x, a, skip_xyz=True), ev.evaluate)
        print(f"{n_train} view(s), {precond}: validation loss {start:.3f} -> {final:.3f} at alpha {alpha}")
        assert final < start, (n_train, precond, start, final)


# ---------------------------------------------------------------- 6. argument checks (no device call: fake pointers)
def test_marquardt_scale_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    INV, OK = _lib.GSLM_ERR_INVALID, _lib.GSLM_OK
    bounds = (ctypes.c_int64 * 8)(0, 3, 6, 6, 9, 13, 14, 26)
    lam = (ctypes.c_double * 7)(*([0.5] * 7))

    def call(n=26, diag=FAKE, b=bounds, l=lam, ng=7, floor=0.0, d=FAKE):
        return lib.gslm_marquardt_scale(n, diag, b, l, ng, floor, d, None)

    assert call(n=-1) == INV and call(diag=None) == INV and call(d=None) == INV
    assert b"gslm_marquardt_scale" in lib.gslm_last_error()
    assert call(floor=-1.0) == INV and call(floor=float("nan")) == INV and call(floor=float("inf")) == INV
    assert call(ng=9) == INV and call(ng=-1) == INV
    assert call(b=None) == INV and call(l=None) == INV
    assert call(n=0, diag=None, d=None) == OK  # nothing to do: nothing launched


def test_option_handling_raises_before_anything_runs():
    from gslm.lm import BatchedLMProblem, LMProblem, lm_step
    lam = M.lam_map()
    for kw in (dict(damping="levenberg"), dict(damping="marquardt"),  # (damp must be given)
               dict(damping="marquardt", damp=lam, recursion="cgls"),
               dict(damping="marquardt", damp=lam, train_exposure=True),
               dict(damping="marquardt", damp=lam, multiview="batched"),
               dict(damping="marquardt", damp=lam, mask_xyz=False),
               dict(damping="marquardt", damp=lam, backend=(None, None, None)),
               dict(marquardt_floor=1e-3)):
        with pytest.raises(ValueError):
            lm_step(None, [], [], None, **kw)
    for cls, kw in ((LMProblem, dict(damping="levenberg")), (LMProblem, dict(damping="marquardt")),
                    (LMProblem, dict(damping="marquardt", damp=lam, ssim=True)),
                    (LMProblem, dict(damping="marquardt", damp=lam, train_exposure=True)),
                    (LMProblem, dict(damping="marquardt", damp=lam, mask_xyz=False)),
                    (LMProblem, dict(damping="marquardt", damp=lam, marquardt_floor=-1.0)),
                    (LMProblem, dict(marquardt_floor=1e-3)),
                    (BatchedLMProblem, dict(damping="marquardt", damp=lam))):
        with pytest.raises(ValueError):
            cls(None, [], None, device="cpu", **kw)


def test_multi_view_gathers_refuse_the_damping_vector():
    """gslm_gather_views, gslm_gather_views_active and gslm_gather_screen return GSLM_ERR_INVALID on GSLM_MV_DAMP_VEC
    before they read anything (fake pointers)."""
    from gslm import _lib
    from gslm.lm import MV_DAMP_VEC
    lib = _lib.lib
    view = _lib.make_view(64, 64, 0.5, 0.5, [0, 0, 0], 1.0, [0.0] * 16, [0.0] * 16, 0, [0, 0, 0])
    g = _lib.make_gaussians(10, max_coeffs=1, raw=True)
    g.means3D = g.opacities = g.scales = g.rotations = g.sh_dc = FAKE
    g.sh_dc_stride = 3
    v = _lib.GslmGrads()
    v.means3D = v.opacities = v.scales = v.rotations = v.sh_dc = FAKE
    v.sh_dc_stride = 3
    ws = _lib.GslmViewWs()
    opts = _lib.extend_opts(_lib.GslmMatvecOpts(), _lib.GslmMatvecOptsDamp, MV_DAMP_VEC)
    opts.damp_vec = ctypes.addressof(v)
    o = ctypes.addressof(opts)
    INV = _lib.GSLM_ERR_INVALID
    assert lib.gslm_gather_screen(ctypes.byref(view), 1, ctypes.byref(g), FAKE, ctypes.byref(v), ctypes.byref(v), o,
                                  None) == INV
    assert b"GSLM_MV_DAMP_VEC" in lib.gslm_last_error()
    assert lib.gslm_gather_views(ctypes.byref(view), ctypes.byref(ws), 1, ctypes.byref(g), ctypes.byref(v),
                                 ctypes.byref(v), o, None) == INV
    assert b"GSLM_MV_DAMP_VEC" in lib.gslm_last_error()
    assert lib.gslm_gather_views_active(ctypes.byref(view), ctypes.byref(ws), 1, ctypes.byref(g), ctypes.byref(v),
                                        ctypes.byref(v), FAKE, 4, FAKE, 5, FAKE, 4, o, None) == INV
    assert b"GSLM_MV_DAMP_VEC" in lib.gslm_last_error()
