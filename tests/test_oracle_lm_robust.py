"""CPU: the robust LM losses on the oracle (tests/lm_robust_ref.py), the argument checks of the four robust entry points
and the Python layer's refusals -- no GPU is touched.

Float64 unless said, on sh1_33x17 (masked, generic background) and sh3_40x33 at lm_robust_ref.DELTA:
  * rhs() of the reweighted problem is -1/2 grad of 2 sum rho(r^2) by autograd (1e-10);
  * both branches of |r| <= delta are busy (the share outside in [0.25, 0.75]);
  * Huber with delta >= 1 is the plain oracle (every |r| <= 1), torch.equal;
  * five cgls_ref iterations (5 x 5) lower the robust loss at alpha = 1;
  * the float32 oracle's distance from the float64 one stays below lm_robust_ref.F32_FLOOR (the GPU bounds are 8 x)."""
import copy
import ctypes
import functools
import math

import pytest
import torch

import lm_robust_ref as RR
from scenes import BG_GENERIC, lm_bg_mask, lm_bg_scene, to_float64

SCENES = ("sh1_33x17", "sh3_40x33")


def scene(name, f64=True, n_views=1):
    """The scene as every robust test takes it: sh1_33x17 masked (seed = view), sh3_40x33 unmasked."""
    model, cams = lm_bg_scene(name, n_views=n_views)
    if name == "sh1_33x17":
        for i, c in enumerate(cams):
            c.alpha_mask = lm_bg_mask(name, seed=i)
    return to_float64(model, cams) if f64 else (model, cams)


def _bg(dtype):
    return torch.tensor(BG_GENERIC, dtype=dtype)


@functools.lru_cache(maxsize=None)
def solved(name, kind, f64=True, n_views=1):
    """(problem, loss, J^T b, product on lm_robust_ref.direction, the 5 x 5 cgls_ref solution), computed once."""
    from oracle.lm_ref import cgls_ref
    model, cams = scene(name, f64, n_views)
    dtype = torch.float64 if f64 else torch.float32
    prob = RR.RobustOracleLMProblem(model, cams, _bg(dtype), (kind, RR.DELTA[name]))
    loss = float(prob.evaluate())
    g = prob.rhs()
    v = RR.direction(prob.layout, dtype)
    y = prob.matvec(v, prob.zeros().to(dtype)).clone()
    x = cgls_ref(prob, g, 5, 5)
    return prob, loss, g, y, x


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_rhs_is_minus_half_the_gradient_of_the_robust_loss(name, kind):
    prob, _, g, _, _ = solved(name, kind)
    leaves = prob._leaves()
    grads = torch.autograd.grad(prob.robust_loss(), leaves, allow_unused=True)
    ref = prob._mask(-0.5 * torch.cat([(gr if gr is not None else torch.zeros_like(t)).reshape(-1)
                                       for gr, t in zip(grads, leaves)]))
    err = float((g - ref).abs().max() / ref.abs().max())
    print(f"{name} {kind}: rhs vs -1/2 grad (of max) {err:.2e}")
    assert float(ref.abs().max()) > 0 and err <= 1e-10


@pytest.mark.parametrize("name", SCENES)
def test_both_branches_busy(name):
    prob = solved(name, "huber")[0]
    with torch.no_grad():
        r = torch.cat([x.reshape(-1) for x in prob.raw_residuals()])
    share = float((r.abs() > RR.DELTA[name]).double().mean())
    print(f"{name}: share of |r| > delta = {share:.3f}")
    assert 0.25 <= share <= 0.75
    if name == "sh1_33x17":
        assert abs(share - 0.601) < 1e-3


@pytest.mark.parametrize("delta", [1.0, 1e9])
@pytest.mark.parametrize("name", SCENES)
def test_huber_with_every_residual_inside_is_the_plain_problem(name, delta):
    from oracle.lm_ref import OracleLMProblem
    model, cams = scene(name)
    plain = OracleLMProblem(model, cams, _bg(torch.float64))
    rob = RR.RobustOracleLMProblem(model, cams, _bg(torch.float64), ("huber", delta))
    assert torch.equal(rob.evaluate(), plain.evaluate())
    assert torch.equal(rob.rhs(), plain.rhs())
    v = RR.direction(plain.layout)
    assert torch.equal(rob.matvec(v, rob.zeros().double()), plain.matvec(v, plain.zeros().double()))


# the sh1_33x17 figures of the issue (robust loss before -> after the 5 x 5 step at alpha = 1)
DESCENT = {("sh1_33x17", "huber"): (407.76, 375.21), ("sh1_33x17", "cauchy"): (218.01, 205.99)}


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_the_step_descends(name, kind):
    from gslm.lm import update_params
    prob, before, _, _, x = solved(name, kind)
    model = copy.deepcopy(prob.model)
    update_params(model, prob.layout, x, 1.0)
    after = float(RR.RobustOracleLMProblem(model, prob.cams, prob.bg, (kind, RR.DELTA[name])).evaluate())
    print(f"{name} {kind}: robust loss {before:.2f} -> {after:.2f}")
    assert after < before
    if (name, kind) in DESCENT:
        b, a = DESCENT[(name, kind)]
        assert abs(before - b) < 0.01 and abs(after - a) < 0.01


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_float32_floor(name, kind):
    """The float32 oracle against the float64 one: the measurements behind lm_robust_ref.F32_FLOOR."""
    p64, l64, g64, y64, x64 = solved(name, kind)
    _, l32, g32, y32, x32 = solved(name, kind, f64=False)
    lay = p64.layout
    e_loss = abs(l32 - l64) / l64
    print(f"{name} {kind}: loss rel {e_loss:.2e}")
    assert e_loss <= RR.F32_FLOOR["loss"]
    for what, a, b in (("rhs", g32, g64), ("product", y32, y64), ("solve", x32, x64)):
        errs = RR.group_errors(a, b, lay)
        print(f"{name} {kind}: {what} " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= RR.F32_FLOOR[what][k], (what, k, v)
    for q, tol in RR.GPU_TOL.items():
        for t in (tol.values() if isinstance(tol, dict) else (tol,)):
            assert t <= RR.MAX_TOL


# ---------------------------------------------------------------- the entry points' argument checks (no launch)
def _view(W=33, H=17):
    from gslm import _lib
    from gslm.cameras import orbit_cameras
    return _lib.view_from_camera(orbit_cameras(1, W, H, seed=1)[0], torch.zeros(3), 1)


def _rb(kind, delta):
    from gslm import _lib
    return _lib.GslmRobust(kind, delta)


BAD = [(3, 0.25), (-1, 0.25), (1, 0.0), (1, -0.5), (2, math.nan), (2, math.inf), (1, -math.inf)]


def test_library_exports_the_entry_points_and_the_abi_is_still_9():
    import os
    import re
    from gslm import _lib
    for name, plain in (("gslm_lm_residual_robust", "gslm_lm_residual"),
                        ("gslm_rasterize_loss_robust", "gslm_rasterize_loss"),
                        ("gslm_rasterize_loss_slot_robust", "gslm_rasterize_loss_slot"),
                        ("gslm_rasterize_loss_sets_robust", "gslm_rasterize_loss_sets")):
        assert hasattr(_lib.lib, name), name
        assert len(_lib.EXPORTS[name][1]) == len(_lib.EXPORTS[plain][1]) + 1
    assert _lib.lib.gslm_abi_version() == 9
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gslm.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+GSLM_ABI_VERSION\s+9\b", h)
    for name in ("gslm_lm_residual_robust", "gslm_rasterize_loss_robust", "gslm_rasterize_loss_slot_robust",
                 "gslm_rasterize_loss_sets_robust"):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", h, re.S)
        assert m and "const gslm_robust* robust" in m.group(1), name
    assert ctypes.sizeof(_lib.GslmRobust) == 8
    assert (_lib.GSLM_ROBUST_NONE, _lib.GSLM_ROBUST_HUBER, _lib.GSLM_ROBUST_CAUCHY) == (0, 1, 2)
    assert "gslm_rasterize_loss_dev_robust" not in h


def test_lm_residual_robust_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)  # stands for any non-NULL pointer: every check returns before a launch
    nscr = lib.gslm_residual_scratch_bytes(17, 33)

    def call(rb, H=17, W=33, color=a, gt=a, scratch=a, nbytes=nscr, loss=a):
        return lib.gslm_lm_residual_robust(H, W, color, gt, None, ctypes.byref(rb), a, a, a, scratch, nbytes, loss, 0,
                                           None)

    for kind, delta in BAD:
        assert call(_rb(kind, delta)) == _lib.GSLM_ERR_INVALID, (kind, delta)
        assert b"robust" in lib.gslm_last_error()
    ok = _rb(1, 0.25)
    assert call(ok, H=-1) == _lib.GSLM_ERR_INVALID
    assert call(ok, color=None) == _lib.GSLM_ERR_INVALID
    assert call(ok, gt=None) == _lib.GSLM_ERR_INVALID
    assert call(ok, loss=None) == _lib.GSLM_ERR_INVALID
    assert call(ok, scratch=None) == _lib.GSLM_ERR_INVALID
    assert call(ok, nbytes=nscr - 1) == _lib.GSLM_ERR_CAPACITY
    # kind NONE is the plain form: delta is not looked at, the plain checks still hold
    assert call(_rb(0, math.nan), color=None) == _lib.GSLM_ERR_INVALID
    assert b"robust" not in lib.gslm_last_error()


def test_rasterize_loss_robust_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)
    vw = _view()
    H, W, N = vw.image_height, vw.image_width, 10
    nbin, nscr = lib.gslm_binning_bytes(N, H, W), lib.gslm_loss_scratch_bytes(H, W)

    def call(rb, gt=a, scratch=a, nbytes=nscr, loss=a, binning_bytes=nbin):
        return lib.gslm_rasterize_loss_robust(ctypes.byref(vw), 5, a, a, binning_bytes, N, gt, None, ctypes.byref(rb),
                                              scratch, nbytes, loss, 0, None)

    for kind, delta in BAD:
        assert call(_rb(kind, delta)) == _lib.GSLM_ERR_INVALID, (kind, delta)
        assert b"robust" in lib.gslm_last_error()
    ok = _rb(2, 0.05)
    assert call(ok, gt=None) == _lib.GSLM_ERR_INVALID
    assert call(ok, scratch=None) == _lib.GSLM_ERR_INVALID
    assert call(ok, loss=None) == _lib.GSLM_ERR_INVALID
    assert call(ok, nbytes=nscr - 1) == _lib.GSLM_ERR_CAPACITY
    assert call(ok, binning_bytes=nbin - 1) == _lib.GSLM_ERR_CAPACITY


def test_rasterize_loss_slot_robust_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)
    vw = _view()
    H, W, N, P = vw.image_height, vw.image_width, 10, 5
    nbin, nscr, nset = (lib.gslm_union_binning_bytes(N, H, W), lib.gslm_loss_scratch_bytes(H, W),
                        lib.gslm_depth_records_bytes(P))

    def call(rb, slot=0, n_sets=6, nbytes=nscr, set_bytes=nset, gt=a, binning_bytes=nbin):
        return lib.gslm_rasterize_loss_slot_robust(ctypes.byref(vw), P, a, set_bytes, a, binning_bytes, N, slot, n_sets,
                                                   gt, None, ctypes.byref(rb), a, nbytes, a, 0, None)

    for kind, delta in BAD:
        assert call(_rb(kind, delta)) == _lib.GSLM_ERR_INVALID, (kind, delta)
        assert b"robust" in lib.gslm_last_error()
    ok = _rb(1, 0.25)
    assert call(ok, slot=6) == _lib.GSLM_ERR_INVALID
    assert call(ok, slot=-1) == _lib.GSLM_ERR_INVALID
    assert call(ok, n_sets=9, slot=8) == _lib.GSLM_ERR_INVALID
    assert call(ok, gt=None) == _lib.GSLM_ERR_INVALID
    assert call(ok, nbytes=nscr - 1) == _lib.GSLM_ERR_CAPACITY
    assert call(ok, set_bytes=nset - 1) == _lib.GSLM_ERR_CAPACITY
    assert call(ok, binning_bytes=nbin - 1) == _lib.GSLM_ERR_CAPACITY


def test_rasterize_loss_sets_robust_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)
    vw = _view()
    H, W, N, P = vw.image_height, vw.image_width, 10, 5
    nbin, nset = lib.gslm_union_binning_bytes(N, H, W), lib.gslm_depth_records_bytes(P)

    def ptrs(n, hole=None):
        return (ctypes.c_void_p * max(n, 1))(*[None if k == hole else a for k in range(max(n, 1))])

    def call(rb, n=3, first=0, nbytes=None, geoms=None):
        nbytes = lib.gslm_loss_sets_scratch_bytes(n, H, W) if nbytes is None else nbytes
        return lib.gslm_rasterize_loss_sets_robust(ctypes.byref(vw), P, ptrs(n) if geoms is None else geoms, n, first,
                                                   nset, a, nbin, N, a, None, ctypes.byref(rb), a, nbytes, ptrs(n), 0,
                                                   None)

    for kind, delta in BAD:
        assert call(_rb(kind, delta)) == _lib.GSLM_ERR_INVALID, (kind, delta)
        assert b"robust" in lib.gslm_last_error()
    ok = _rb(2, 0.25)
    for n in (0, 9, -1):
        assert call(ok, n=n) == _lib.GSLM_ERR_INVALID, n
    assert call(ok, n=3, first=6) == _lib.GSLM_ERR_INVALID
    assert call(ok, n=1, first=-1) == _lib.GSLM_ERR_INVALID
    assert call(ok, nbytes=lib.gslm_loss_sets_scratch_bytes(3, H, W) - 1) == _lib.GSLM_ERR_CAPACITY
    assert call(ok, geoms=ptrs(3, hole=1)) == _lib.GSLM_ERR_INVALID


# ---------------------------------------------------------------- the Python layer's refusals (before anything runs)
BAD_OPTIONS = ["huber", ("huber",), ("huber", 0.0), ("huber", -1.0), ("cauchy", math.nan), ("cauchy", math.inf),
               ("tukey", 0.25), ("huber", "0.25"), (1, 0.25), ("huber", 0.25, 1), ("huber", True)]


def test_robust_option_forms():
    from gslm.lm import robust_option
    assert robust_option(None) is None
    assert robust_option(("huber", 0.25)) == ("huber", 0.25)
    assert robust_option(["cauchy", 1]) == ("cauchy", 1.0)
    for bad in BAD_OPTIONS:
        with pytest.raises(ValueError, match="robust"):
            robust_option(bad)


def _tiny():
    model, cams = lm_bg_scene("sh1_33x17")
    return model, cams, torch.tensor(BG_GENERIC)


def test_problem_refusals():
    from gslm.lm import BatchedLMProblem, LMProblem, cgls_residual
    model, cams, bg = _tiny()
    for bad in BAD_OPTIONS:
        for cls in (LMProblem, BatchedLMProblem):
            with pytest.raises(ValueError, match="robust"):
                cls(model, cams, bg, device="cpu", robust=bad)
    for kw in (dict(ssim=True), dict(train_exposure=True), dict(mask_xyz=False)):
        with pytest.raises(ValueError, match="robust"):
            LMProblem(model, cams, bg, device="cpu", robust=("huber", 0.25), **kw)

    class Robust:  # (cgls_residual looks at the attribute before it touches the problem)
        ssim, damping, _dvec, train_exposure, robust = False, "fixed", None, False, ("huber", 0.25)

    with pytest.raises(ValueError, match="robust"):
        cgls_residual(Robust())


def test_evaluator_refusals():
    from gslm.lm import LossEvaluator
    model, cams, bg = _tiny()
    for bad in BAD_OPTIONS:
        with pytest.raises(ValueError, match="robust"):
            LossEvaluator(model, cams, bg, device="cpu", robust=bad)
    for kw in (dict(device_count=True), dict(train_exposure=True), dict(train_exposure=True, fused_exposure=True)):
        with pytest.raises(ValueError, match="robust"):
            LossEvaluator(model, cams, bg, device="cpu", robust=("cauchy", 0.25), **kw)


def test_lm_step_refusals(monkeypatch):
    from gslm import lm
    from oracle.lm_ref import OracleLMProblem, OracleLossEvaluator, cgls_solver
    model, cams, bg = _tiny()

    def never(*a, **k):
        raise AssertionError("lm_step built a problem before refusing")

    monkeypatch.setattr(lm, "LMProblem", never)
    monkeypatch.setattr(lm, "BatchedLMProblem", never)
    rob = ("huber", 0.25)
    for bad in BAD_OPTIONS:
        with pytest.raises(ValueError, match="robust"):
            lm.lm_step(model, cams, cams, bg, device="cpu", robust=bad)
    for kw in (dict(recursion="cgls"), dict(train_exposure=True), dict(mask_xyz=False),
               dict(backend=(OracleLMProblem, OracleLossEvaluator, cgls_solver))):
        with pytest.raises(ValueError, match="robust"):
            lm.lm_step(model, cams, cams, bg, device="cpu", robust=rob, **kw)
    monkeypatch.setenv("GSLM_FORCE_COLLECTIVES", "1")  # a sharded run (one rank forced through the collectives)
    try:
        with pytest.raises(ValueError, match="robust"):
            lm.lm_step(model, cams, cams, bg, device="cpu", robust=rob)
    except RuntimeError:
        pytest.fail("the sharded refusal came after the process group was needed")
