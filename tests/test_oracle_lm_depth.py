"""CPU: the inverse-depth residual of the LM step on the oracle (tests/lm_depth_ref.py) and the Python layer's refusals
-- no GPU is touched.

Float64 unless said, on sh1_33x17 (alpha masks, generic background) and sh3_40x33 at lm_depth_ref.LAMBDA_D:
  * rhs() is -1/2 grad of the loss as the issue states it, 2 sum r_c^2 + lambda_d sum r_d^2, by autograd (1e-12);
  * the depth block's columns are exactly zero in xyz (frozen), dc, rest and exposure;
  * a Gaussian whose colour column is zero has a zero depth column (the active-list claim; occluder scene);
  * lambda_d is large enough to matter: the depth share of J^T b and of the product is >= 0.25 of the colour part's
    group max in scaling, rotation and opacity;
  * the float32 oracle's distance from the float64 one stays below lm_depth_ref.F32_FLOOR (the GPU bounds are 8 x);
  * a 5 x 5 LM step with depth lowers the combined validation loss, for one and two training views."""
import copy
import functools
import math

import pytest
import torch

import lm_depth_ref as DR
from scenes import BG_GENERIC, lm_bg_scene

LAM = DR.LAMBDA_D
# (name, views, the views with a depth target)
CONFIGS = [("sh1_33x17", 1, None), ("sh1_33x17", 2, (0,)), ("sh3_40x33", 1, None), ("sh3_40x33", 2, (0,))]


def _bg(dtype):
    return torch.tensor(BG_GENERIC, dtype=dtype)


@functools.lru_cache(maxsize=None)
def solved(name, f64=True, n_views=1, depth_views=None, lam=LAM):
    """(problem, loss, J^T b, product on lm_depth_ref.direction, the 5 x 5 cgls_ref solution), computed once."""
    from oracle.lm_ref import cgls_ref
    model, cams = DR.scene(name, f64, n_views, depth_views)
    dtype = torch.float64 if f64 else torch.float32
    prob = DR.DepthOracleLMProblem(model, cams, _bg(dtype), lam)
    loss = float(prob.evaluate())
    g = prob.rhs()
    v = DR.direction(prob.layout, dtype)
    y = prob.matvec(v, prob.zeros().to(dtype)).clone()
    x = cgls_ref(prob, g, 5, 5)
    return prob, loss, g, y, x


@pytest.mark.parametrize("name,n_views,depth_views", CONFIGS)
def test_rhs_is_minus_half_the_gradient_of_the_stated_loss(name, n_views, depth_views):
    prob, loss, g, _, _ = solved(name, True, n_views, depth_views)
    leaves = prob._leaves()
    stated = prob.stated_loss()
    assert abs(float(stated.detach()) - loss) <= 1e-12 * loss
    grads = torch.autograd.grad(stated, leaves, allow_unused=True)
    ref = prob._mask(-0.5 * torch.cat([(gr if gr is not None else torch.zeros_like(t)).reshape(-1)
                                       for gr, t in zip(grads, leaves)]))
    err = float((g - ref).abs().max() / ref.abs().max())
    print(f"{name} x{n_views}: rhs vs -1/2 grad (of max) {err:.2e}")
    assert float(ref.abs().max()) > 0 and err <= 1e-12


@pytest.mark.parametrize("name", DR.SCENES)
def test_depth_columns_are_zero_outside_scaling_rotation_opacity(name):
    model, cams = DR.scene(name)
    d = DR.DepthOracleLMProblem(model, cams, _bg(torch.float64), LAM, colour=False)
    lay = d.layout
    g = d.rhs()
    y = d.local_normal_matvec(DR.direction(lay), d.zeros().double()).clone()
    for vec in (g, y):
        views = lay.views(vec)
        for k in ("xyz", "features_dc", "features_rest", "exposure"):
            assert not bool(views[k].any()), k
        for k in DR.DEPTH_GROUPS:
            assert float(views[k].abs().max()) > 0, k


def test_a_gaussian_without_a_colour_column_has_no_depth_column():
    """The active-list claim on the oracle: with random cotangents, the Gaussians whose gradient of <cot, raw render>
    is exactly zero in every group get an exactly zero gradient of <cot_d, inverse depth> too -- and on the occluder
    scene they are a proper, non-empty subset."""
    from oracle import torch_raster as tr
    from scenes import to_float64
    model, cams = to_float64(*lm_bg_scene("sh1_33x17", occluders=True))
    cam = cams[0]
    _, _, invd, raw = tr.render_model(model, cam, _bg(torch.float64))
    gen = torch.Generator().manual_seed(12)
    cot = torch.randn(raw.shape, generator=gen, dtype=torch.float64)
    cot_d = torch.randn(invd.shape, generator=gen, dtype=torch.float64)
    leaves = [model._features_dc, model._features_rest, model._scaling, model._rotation, model._opacity]
    P = model._xyz.shape[0]

    def per_gaussian(obj):
        gs = torch.autograd.grad(obj, leaves, allow_unused=True, retain_graph=True)
        return sum((torch.zeros(P, dtype=torch.float64) if g is None else g.reshape(P, -1).abs().sum(1)) for g in gs)

    colour, depth = per_gaussian((raw * cot).sum()), per_gaussian((invd * cot_d).sum())
    dead = colour == 0
    print(f"occluder scene: {int(dead.sum())} of {P} Gaussians without a colour column")
    assert 0 < int(dead.sum()) < P
    assert not bool(depth[dead].any())
    assert int((depth > 0).sum()) > 0


SHARES = {}  # the figures behind LAMBDA_D, printed by the test below


@pytest.mark.parametrize("name", DR.SCENES)
def test_lambda_is_large_enough_to_matter(name):
    """Depth share = the depth block's vector over the colour block's, by group max, for J^T b and the (undamped)
    product on lm_depth_ref.direction: >= 0.25 in scaling, rotation and opacity at LAMBDA_D -- and below it in some
    group at LAMBDA_D / 2, so LAMBDA_D is the smallest power of two that does (the shares scale with lambda_d)."""
    from oracle.lm_ref import OracleLMProblem
    model, cams = DR.scene(name)
    plain = OracleLMProblem(model, cams, _bg(torch.float64))
    depth = DR.DepthOracleLMProblem(model, cams, _bg(torch.float64), LAM, colour=False)
    lay = plain.layout
    v = DR.direction(lay)
    pairs = {"rhs": (depth.rhs(), plain.rhs()),
             "product": (depth.local_normal_matvec(v, depth.zeros().double()).clone(),
                         plain.local_normal_matvec(v, plain.zeros().double()).clone())}
    for what, (d, c) in pairs.items():
        dv, cv = lay.views(d), lay.views(c)
        share = {k: float(dv[k].abs().max() / cv[k].abs().max()) for k in DR.DEPTH_GROUPS}
        SHARES[(name, what)] = share
        print(f"{name}: depth share of {what} at lambda_d = {LAM:g}: " +
              "  ".join(f"{k} {s:.3f}" for k, s in share.items()))
        assert min(share.values()) >= 0.25, (what, share)
    if name == "sh1_33x17":  # measured 0.346 in rotation at 128: half of it is below the bar
        assert SHARES[(name, "rhs")]["rotation"] * 0.5 < 0.25


@pytest.mark.parametrize("name,n_views,depth_views", CONFIGS)
def test_float32_floor(name, n_views, depth_views):
    """The float32 oracle against the float64 one: the measurements behind lm_depth_ref.F32_FLOOR."""
    p64, l64, g64, y64, x64 = solved(name, True, n_views, depth_views)
    _, l32, g32, y32, x32 = solved(name, False, n_views, depth_views)
    lay = p64.layout
    e_loss = abs(l32 - l64) / l64
    print(f"{name} x{n_views}: loss rel {e_loss:.2e}")
    assert e_loss <= DR.F32_FLOOR["loss"]
    for what, a, b in (("rhs", g32, g64), ("product", y32, y64), ("solve", x32, x64)):
        errs = DR.group_errors(a, b, lay)
        print(f"{name} x{n_views}: {what} " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= DR.F32_FLOOR[what][k], (what, k, v)
    for q, tol in DR.GPU_TOL.items():
        for t in (tol.values() if isinstance(tol, dict) else (tol,)):
            assert 0 < t <= DR.MAX_TOL


@pytest.mark.parametrize("n_train", [1, 2])
def test_the_step_lowers_the_combined_validation_loss(n_train):
    """cgls_ref 5 x 5 on n_train training views with depth, then the reference's line search on two further views with
    depth: the combined (colour + depth) validation loss after the step is below the one before it."""
    from gslm.lm import update_params
    from oracle.lm_ref import cgls_ref, line_search_ref
    model, cams = DR.scene("sh1_33x17", True, n_train + 2)
    model = copy.deepcopy(model)
    bg = _bg(torch.float64)
    prob = DR.DepthOracleLMProblem(model, cams[:n_train], bg, LAM)
    prob.evaluate()
    s = cgls_ref(prob, prob.rhs(), 5, 5)
    val = DR.DepthOracleLossEvaluator(model, cams[n_train:], bg, LAM)
    before = float(val.evaluate())
    alpha, after, trace = line_search_ref(lambda a: update_params(model, prob.layout, s, a), val.evaluate)
    print(f"{n_train} training view(s): combined validation loss {before:.3f} -> {after:.3f} at alpha {alpha}")
    assert after < before


# ---------------------------------------------------------------- the Python layer's refusals (before anything runs)
BAD_WEIGHTS = [-1.0, math.nan, math.inf, "4", True, (4.0,)]


def _tiny(n_views=1):
    model, cams = DR.scene("sh1_33x17", False, n_views)
    return model, cams, torch.tensor(BG_GENERIC)


def test_depth_option_forms():
    from gslm.lm import depth_option
    assert depth_option(None) is None
    assert depth_option(0) == 0.0 and depth_option(4) == 4.0 and depth_option(0.5) == 0.5
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="depth_weight"):
            depth_option(bad)


def test_camera_carries_a_depth_mask():
    from gslm.cameras import orbit_cameras
    c = orbit_cameras(1, 8, 8, seed=1)[0]
    assert c.depth_mask is None and c.invdepthmap is None and c.depth_reliable is False


def test_problem_refusals():
    from gslm.lm import BatchedLMProblem, LMProblem
    from gslm.parallel import ShardedLMProblem
    model, cams, bg = _tiny()
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="depth_weight"):
            LMProblem(model, cams, bg, device="cpu", depth_weight=bad)
    for kw in (dict(ssim=True), dict(train_exposure=True), dict(robust=("huber", 0.25)), dict(mask_xyz=False),
               dict(damping="marquardt", damp={"xyz": 1.0})):
        with pytest.raises(ValueError, match="depth_weight"):
            LMProblem(model, cams, bg, device="cpu", depth_weight=4.0, **kw)
    with pytest.raises(ValueError, match="depth"):
        BatchedLMProblem(model, cams, bg, device="cpu", depth_weight=4.0)
    with pytest.raises(ValueError, match="depth"):
        ShardedLMProblem(model, cams, bg, device="cpu", depth_weight=4.0)
    with pytest.raises(ValueError, match="depth_weight"):  # targets without a weight
        LMProblem(model, cams, bg, device="cpu", invdepths=[cams[0].invdepthmap])


def test_target_shapes_are_validated():
    from gslm.lm import depth_targets
    model, cams, bg = _tiny(2)
    H, W = cams[0].image_height, cams[0].image_width
    ok = torch.zeros(1, H, W)
    got = depth_targets(cams, None, None, "cpu")
    assert all(t is not None and t[0].shape == (1, H, W) and t[1].shape == (1, H, W) for t in got)
    cams[1].depth_reliable = False
    assert depth_targets(cams, None, None, "cpu")[1] is None
    cams[1].depth_reliable, cams[1].invdepthmap = True, None
    assert depth_targets(cams, None, None, "cpu")[1] is None
    assert depth_targets(cams, [ok, None], [None, None], "cpu")[0][1] is None
    for bad in (torch.zeros(H, W), torch.zeros(1, H, W + 1), torch.zeros(1, H, W, dtype=torch.float64),
                torch.zeros(3, H, W), [0.0]):
        with pytest.raises(ValueError, match="inverse-depth target"):
            depth_targets(cams, [bad, None], None, "cpu")
        with pytest.raises(ValueError, match="depth mask"):
            depth_targets(cams, [ok, None], [bad, None], "cpu")
    with pytest.raises(ValueError, match="invdepths"):
        depth_targets(cams, [ok], None, "cpu")
    with pytest.raises(ValueError, match="depth_masks"):
        depth_targets(cams, [ok, ok], [ok], "cpu")


def test_consumers_without_a_depth_term_refuse():
    """diagonal (cgls_jacobi, Marquardt), set_damping_vector, the residual-space recursion and the sharded exchange
    refuse a problem that carries depth -- before they touch a device."""
    from gslm.lm import LMProblem
    model, cams, bg = _tiny()
    prob = LMProblem.__new__(LMProblem)
    prob.depth_weight = 4.0
    prob.ssim = prob.train_exposure = False
    for call in (lambda: prob.diagonal(), lambda: prob.set_damping_vector(torch.zeros(3)),
                 lambda: prob.jv_residual(None, None, None), lambda: prob.jt_residual(None, None, None),
                 lambda: prob.screen_products(None, None)):
        with pytest.raises(ValueError, match="depth"):
            call()


def test_evaluator_refusals():
    from gslm.lm import LossEvaluator
    model, cams, bg = _tiny()
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="depth_weight"):
            LossEvaluator(model, cams, bg, device="cpu", depth_weight=bad)
    for kw in (dict(device_count=True), dict(train_exposure=True), dict(train_exposure=True, fused_exposure=True),
               dict(robust=("cauchy", 0.25))):
        with pytest.raises(ValueError, match="depth_weight"):
            LossEvaluator(model, cams, bg, device="cpu", depth_weight=4.0, **kw)
    with pytest.raises(ValueError, match="depth_weight"):
        LossEvaluator(model, cams, bg, device="cpu", depth_masks=[None])


def test_lm_step_refusals(monkeypatch):
    from gslm import lm
    from oracle.lm_ref import OracleLMProblem, OracleLossEvaluator, cgls_solver
    model, cams, bg = _tiny(2)

    def never(*a, **k):
        raise AssertionError("lm_step built a problem before refusing")

    monkeypatch.setattr(lm, "LMProblem", never)
    monkeypatch.setattr(lm, "BatchedLMProblem", never)
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="depth_weight"):
            lm.lm_step(model, cams, cams, bg, device="cpu", depth_weight=bad)
    damp = {k: 1e-2 for k in ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "exposure")}
    for kw in (dict(recursion="cgls"), dict(train_exposure=True), dict(mask_xyz=False), dict(robust=("huber", 0.25)),
               dict(precond="jacobi"), dict(damping="marquardt", damp=damp), dict(multiview="batched"),
               dict(backend=(OracleLMProblem, OracleLossEvaluator, cgls_solver))):
        with pytest.raises(ValueError, match="depth_weight"):
            lm.lm_step(model, cams, cams, bg, device="cpu", depth_weight=4.0, **kw)
    monkeypatch.setenv("GSLM_FORCE_COLLECTIVES", "1")  # a sharded run (one rank forced through the collectives)
    try:
        with pytest.raises(ValueError, match="depth_weight"):
            lm.lm_step(model, cams, cams, bg, device="cpu", depth_weight=4.0)
    except RuntimeError:
        pytest.fail("the sharded refusal came after the process group was needed")
