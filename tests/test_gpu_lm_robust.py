"""GPU: the Huber and Cauchy robust losses of the fused LM step -- gslm_lm_residual_robust, the three robust loss
blends, LMProblem / BatchedLMProblem / LossEvaluator / lm_step with `robust`.

References (tests/lm_robust_ref.py, pinned on the CPU by tests/test_oracle_lm_robust.py):
  epilogue    the float32 torch restatement on the CPU, by torch.equal for residual, weight and seed; the loss against
              the float64 sum of the restatement's rho terms at 1e-12 of sum |terms|;
  blends      gslm_rasterize + gslm_lm_residual_robust (and the restatement on gslm_rasterize's image) at 1e-12 of the
              loss, the plain pair's bound; slot against the set's own render and sets against slot by ==;
  problem     RobustOracleLMProblem in float64, per group relative to the group's max, at 8 x the float32 oracle's own
              distance (lm_robust_ref.GPU_TOL);
  lm_step     union against exact by ==; the float64 restatement (cgls_ref 5 x 5 + line_search_ref on the robust
              oracle): the same alpha, losses to 1e-6."""
import ctypes
import itertools
import math

import pytest
import torch

import lm_diag_ref as D
import lm_robust_ref as RR
from margins import record
from scenes import BG_GENERIC, BG_ZERO, lm_bg_mask, lm_bg_scene
from test_oracle_lm_robust import scene, solved

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -7777.0
KIND = {"huber": 1, "cauchy": 2}
DELTAS = (0.05, 0.25)


def _rb(kind, delta):
    from gslm import _lib
    return _lib.GslmRobust(KIND.get(kind, kind), delta)


# ---------------------------------------------------------------- 1. the residual epilogue
def _images(H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    color = -0.3 + 1.6 * torch.rand(3, H, W, generator=gen)  # a fifth of it outside [0, 1]
    color.view(-1)[::7] = torch.tensor([0.0, 1.0, -0.0, 1.5, -0.5])[torch.arange(color.numel())[::7] % 5]
    gt = torch.rand(3, H, W, generator=gen)
    mask = 0.25 + 0.7 * torch.rand(H, W, generator=gen)
    mask.view(-1)[::5] = 0.0
    mask.view(-1)[1::11] = 1.0
    return color, gt, mask


def _guarded(n, on):
    """A NaN-filled float32 output of n elements between two guard elements (None when the output is not asked for)."""
    if not on:
        return None
    t = torch.full((n + 2,), math.nan, dtype=torch.float32, device=DEV)
    t[0] = t[n + 1] = GUARD
    return t


def _run_epilogue(fn_args, H, W, color, gt, mask, outs, accumulate, base=3.5):
    """One call of an epilogue entry point: (residual, weight, seed) as CPU tensors or None, and the loss."""
    from gslm._lib import check, lib
    n = 3 * H * W
    bufs = [_guarded(n, on) for on in outs]
    scr = torch.empty(lib.gslm_residual_scratch_bytes(H, W) // 8, dtype=torch.float64, device=DEV)
    loss = torch.full((3,), base, dtype=torch.float64, device=DEV)
    ptrs = [None if b is None else b.data_ptr() + 4 for b in bufs]
    name, extra = fn_args
    check(getattr(lib, name)(H, W, color.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), *extra,
                             *ptrs, scr.data_ptr(), scr.numel() * 8, loss.data_ptr() + 8, accumulate, None), name)
    torch.cuda.synchronize()
    assert float(loss[0]) == base and float(loss[2]) == base
    got = []
    for b in bufs:
        if b is None:
            got.append(None)
            continue
        c = b.cpu()
        assert float(c[0]) == GUARD and float(c[n + 1]) == GUARD
        got.append(c[1:n + 1].reshape(3, H, W))
    return got, float(loss[1])


SIZES = [(1, 255), (1, 256), (1, 257), (17, 33), (512, 520)]  # (H, W): around a block, ragged, past the 1024-block grid


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("kind", RR.KINDS)
def test_epilogue_bitwise_against_the_torch_restatement(kind, H, W):
    """residual, weight and seed by torch.equal, the loss at 1e-12 of sum |terms|: both deltas, masked and unmasked,
    every NULL-output combination on NaN-filled destinations between guard elements, accumulate 0 and 1."""
    color, gt, mask = _images(H, W, seed=H * 1000 + W)
    dc, dg, dm = color.to(DEV), gt.to(DEV), mask.to(DEV)
    base = 3.5
    for delta, masked in itertools.product(DELTAS, (True, False)):
        r, w, s, terms = RR.epilogue_f32(color, gt, mask if masked else None, kind, delta)
        assert not bool(torch.isnan(w).any() | torch.isnan(s).any())
        share = float((r.abs() > delta).float().mean())
        assert 0.05 < share < 0.95  # both branches
        want_loss, scale = 2.0 * float(terms.sum()), 2.0 * float(terms.abs().sum())
        rb = _rb(kind, delta)
        combos = [(c, 0) for c in itertools.product((True, False), repeat=3)] + [((True,) * 3, 1), ((False,) * 3, 1)]
        for outs, acc in combos:
            got, loss = _run_epilogue(("gslm_lm_residual_robust", (ctypes.byref(rb),)), H, W, dc, dg,
                                      dm if masked else None, outs, acc, base)
            for g, ref, what in zip(got, (r, w, s), ("residual", "weight", "seed")):
                if g is not None:
                    assert torch.equal(g, ref), (what, delta, masked, outs, float((g - ref).abs().max()))
            want = want_loss + (base if acc else 0.0)
            assert abs(loss - want) <= 1e-12 * (scale + (base if acc else 0.0)), (delta, masked, outs, acc, loss, want)


@pytest.mark.parametrize("kind", RR.KINDS)
def test_epilogue_nan_colour_gives_nan_loss_weight_and_seed(kind):
    H, W = 17, 33
    color, gt, mask = _images(H, W, seed=77)
    color[1, 3, 4] = math.nan
    got, loss = _run_epilogue(("gslm_lm_residual_robust", (ctypes.byref(_rb(kind, 0.25)),)), H, W, color.to(DEV),
                              gt.to(DEV), None, (True, True, True), 0)
    assert math.isnan(loss)
    for g in got:
        assert math.isnan(float(g[1, 3, 4])) and int(torch.isnan(g).sum()) == 1


@pytest.mark.parametrize("H,W", [(17, 33), (512, 520)])
def test_epilogue_plain_equivalence(H, W):
    """Huber with every |r| <= delta = 2, kind NONE and a NULL block are gslm_lm_residual, bitwise (the loss too)."""
    color, gt, mask = _images(H, W, seed=5)
    dc, dg, dm = color.to(DEV), gt.to(DEV), mask.to(DEV)
    for m in (dm, None):
        plain, lp = _run_epilogue(("gslm_lm_residual", ()), H, W, dc, dg, m, (True, True, True), 0)
        for extra in ((ctypes.byref(_rb("huber", 2.0)),), (ctypes.byref(_rb(0, math.nan)),), (None,)):
            got, lr = _run_epilogue(("gslm_lm_residual_robust", extra), H, W, dc, dg, m, (True, True, True), 0)
            assert lr == lp
            for a, b in zip(got, plain):
                assert torch.equal(a, b)


def test_epilogue_error_returns_leave_the_outputs():
    from gslm import _lib
    H, W = 17, 33
    color, gt, _ = _images(H, W, seed=6)
    dc, dg = color.to(DEV), gt.to(DEV)
    out = torch.full((3, 3 * H * W), 7.0, dtype=torch.float32, device=DEV)
    loss = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
    scr = torch.empty(1024, dtype=torch.float64, device=DEV)
    for kind, delta in ((3, 0.25), (1, 0.0), (2, -1.0), (1, math.nan), (2, math.inf)):
        rb = _rb(kind, delta)
        st = _lib.lib.gslm_lm_residual_robust(H, W, dc.data_ptr(), dg.data_ptr(), None, ctypes.byref(rb),
                                              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), scr.data_ptr(),
                                              scr.numel() * 8, loss.data_ptr(), 0, None)
        assert st == _lib.GSLM_ERR_INVALID, (kind, delta)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and float(loss) == 7.0


# ---------------------------------------------------------------- 2. the loss blends
def _gpu_scene(name, n_views, masked):
    model, cams = lm_bg_scene(name, n_views=n_views)
    for i, c in enumerate(cams):
        if masked:
            c.alpha_mask = lm_bg_mask(name, seed=i)
    return model.to(DEV), [c.to(DEV) for c in cams]


def _restated_loss(params, cam, bg, kind, delta):
    """2 sum rho of the restatement on gslm_rasterize's image of `params` (a model or a param_snapshot): the float64
    value and sum |terms|."""
    from gslm import _lib
    from gslm.lm import ViewRaster
    from gslm.params import raw_gaussians
    vr = ViewRaster(_lib.view_from_camera(cam, bg, params.active_sh_degree), DEV)
    R = vr.forward(raw_gaussians(params), _lib.stream_handle(DEV), want_invdepth=False)
    torch.cuda.synchronize()
    m = cam.alpha_mask
    terms = RR.epilogue_f32(R.cpu(), cam.original_image.cpu().float(), None if m is None else m.cpu().float()[0], kind,
                            delta)[3]
    return 2.0 * float(terms.sum()), 2.0 * float(terms.abs().sum()), vr.N


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("bgv", [BG_GENERIC, BG_ZERO])
@pytest.mark.parametrize("name", ["sh1_33x17", "sh3_40x33"])
def test_loss_blend_against_rasterize_and_the_residual_epilogue(name, bgv, masked):
    """gslm_rasterize_loss_robust (LossEvaluator.evaluate) against gslm_rasterize + gslm_lm_residual_robust
    (LMProblem.evaluate) and against the restatement on the rendered image: 1e-12 of the loss, both kinds."""
    from gslm.lm import LMProblem, LossEvaluator
    model, cams = _gpu_scene(name, 2, masked)
    bg = torch.tensor(bgv)
    for kind in RR.KINDS:
        rob = (kind, RR.DELTA[name])
        ev = LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2, robust=rob)
        got = float(ev.evaluate())
        pair = float(LMProblem(model, cams, bg, device=DEV, robust=rob).evaluate())
        parts = [_restated_loss(model, c, bg, *rob) for c in cams]
        want = sum(p[0] for p in parts)
        assert all(p[2] > 0 for p in parts) and want > 0
        T = "test_loss_blend_against_rasterize_and_the_residual_epilogue"
        record(T, f"{name} {kind} bg={bgv[0]} mask={int(masked)}: blend vs pair (rel)", abs(got - pair) / pair, 1e-12)
        assert abs(got - pair) <= 1e-12 * pair, (kind, got, pair)
        assert abs(got - want) <= 1e-12 * want, (kind, got, want)
        plain = float(LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2).evaluate())
        assert abs(got - plain) > 1e-3 * plain  # (the robust loss is another number)


@pytest.mark.parametrize("kind", RR.KINDS)
def test_loss_blend_one_tile_and_a_view_that_renders_nothing(kind):
    from gslm.cameras import orbit_cameras
    from gslm.lm import LMProblem, LossEvaluator
    from gslm.model import synthetic_gaussians
    model = synthetic_gaussians(300, 1, seed=2, s0=0.08).to(DEV)
    cams = orbit_cameras(2, 16, 16, seed=3)
    for i, c in enumerate(cams):
        c.original_image = torch.rand(3, 16, 16, generator=torch.Generator().manual_seed(20 + i))
        c.to(DEV)
    bg = torch.tensor(BG_GENERIC)
    rob = (kind, 0.25)
    got = float(LossEvaluator(model, cams, bg, device=DEV, batch=1, streams=1, robust=rob).evaluate())
    pair = float(LMProblem(model, cams, bg, device=DEV, robust=rob).evaluate())
    assert abs(got - pair) <= 1e-12 * pair
    # every Gaussian behind the cameras: nothing is rendered, the loss is the background's
    with torch.no_grad():
        model._xyz.mul_(0.0).add_(cams[0].camera_center.float()[None] * 3.0)
    ev = LossEvaluator(model, cams[:1], bg, device=DEV, batch=1, streams=1, robust=rob)
    got = float(ev.evaluate())
    want, scale, N = _restated_loss(model, cams[0], bg, *rob)
    assert N == 0 and ev.num_rendered == [0]
    assert abs(got - want) <= 1e-12 * scale and want > 0


def _points_setup(kind, nviews=3, name="sh3_40x33"):
    """Six line-search points on a masked scene: the union evaluator, the sets, each set's own robust render."""
    import test_gpu_line_search as tls
    from gslm.lm import LossEvaluator
    model, cams = _gpu_scene(name, nviews, True)
    bg = torch.tensor(BG_GENERIC)
    rob = (kind, RR.DELTA[name])
    lay, s = tls._step(model, scale=0.5)
    ev_x = LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2, robust=rob)
    ev_u = LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2, robust=rob)
    sets, exact, _, _ = tls._points(model, lay, s, ev_x)
    return model, cams, bg, rob, ev_u, sets, exact


@pytest.mark.parametrize("kind", RR.KINDS)
def test_slot_and_sets_forms(kind):
    """Slot a of a six-set union binning is bitwise that set's own render (gslm_rasterize_loss_robust); the sets form is
    bitwise the slot form for n = 1, 2, 3, 5, 6, 8 and for groups starting past slot 0."""
    model, cams, bg, rob, ev_u, sets, exact = _points_setup(kind)
    assert len(set(exact)) == 6
    ev_u.loss_sets = 1
    assert [float(x) for x in ev_u.evaluate_points(sets)] == exact
    eight = sets + [sets[1], sets[4]]
    slot8 = [float(x) for x in ev_u.evaluate_points(eight)]
    assert slot8 == exact + [exact[1], exact[4]]
    for n in (1, 2, 3, 5, 6, 8):
        ev_u.loss_sets = 8  # one group of n sets
        assert [float(x) for x in ev_u.evaluate_points(eight[:n])] == slot8[:n], n
    for k in (2, 3, 4):  # groups starting at slots k, 2 k, ...: a ragged last group for 4
        ev_u.loss_sets = k
        assert [float(x) for x in ev_u.evaluate_points(sets)] == exact, k


@pytest.mark.parametrize("loss_sets", [1, 3])
@pytest.mark.parametrize("kind", RR.KINDS)
def test_slot_and_sets_forms_against_the_restatement(kind, loss_sets):
    """The slot form (loss_sets = 1) and the sets form (groups of 3: sets 4 and 5 are not their group's first) against
    the restatement on each set's own gslm_rasterize image, 1e-12 of the loss."""
    model, cams, bg, rob, ev_u, sets, _ = _points_setup(kind, nviews=2)
    ev_u.loss_sets = loss_sets
    got = [float(x) for x in ev_u.evaluate_points(sets)]
    for a in (0, 4, 5):
        parts = [_restated_loss(sets[a], c, bg, *rob) for c in cams]
        want = sum(p[0] for p in parts)
        assert abs(got[a] - want) <= 1e-12 * want, (a, got[a], want)


def test_blends_plain_equivalence():
    """Huber with delta = 2 and kind NONE give the three blends' plain losses, bitwise."""
    import test_gpu_line_search as tls
    from gslm import _lib
    from gslm.lm import LossEvaluator
    model, cams = _gpu_scene("sh3_40x33", 3, True)
    bg = torch.tensor(BG_GENERIC)
    lay, s = tls._step(model, scale=0.5)
    ev_p = LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2)
    sets, exact, _, _ = tls._points(model, lay, s, ev_p)
    ev_h = LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2, robust=("huber", 2.0))
    ev_n = LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2, robust=("huber", 2.0))
    ev_n._robust = _lib.GslmRobust(_lib.GSLM_ROBUST_NONE, math.nan)  # the entry points with kind NONE
    plain = float(ev_p.evaluate())
    for ev in (ev_h, ev_n):
        assert float(ev.evaluate()) == plain
        for k in (1, 3, 8):
            ev.loss_sets = k
            assert [float(x) for x in ev.evaluate_points(sets)] == exact, k


# ---------------------------------------------------------------- 3. the problem against the float64 yardstick
def _check_groups(T, tag, what, got, ref, layout):
    errs = RR.group_errors(got, ref, layout)
    for k, v in errs.items():
        record(T, f"{tag}: {what} {k} (of max)", v, RR.GPU_TOL[what][k])
    bad = {k: (v, RR.GPU_TOL[what][k]) for k, v in errs.items() if not v <= RR.GPU_TOL[what][k]}
    assert not bad, (tag, what, bad)


def _problem(name, kind, n_views=1, cls=None, **kw):
    from gslm.lm import LMProblem
    model, cams = scene(name, f64=False, n_views=n_views)
    prob = (cls or LMProblem)(model.to(DEV), [c.to(DEV) for c in cams], torch.tensor(BG_GENERIC), device=DEV,
                              robust=(kind, RR.DELTA[name]), **kw)
    return prob


def _loss_rhs_product(T, tag, prob, ref):
    p64, l64, g64, y64, _ = ref
    lay = p64.layout
    loss = float(prob.evaluate())
    e = record(T, f"{tag}: loss rel", abs(loss - l64) / l64, RR.GPU_TOL["loss"])
    assert e <= RR.GPU_TOL["loss"], (tag, loss, l64)
    g = prob.rhs(prob.zeros())
    _check_groups(T, tag, "rhs", prob.expand(g).cpu(), g64, lay)
    v_full = RR.direction(lay, torch.float32).to(DEV)
    if prob.layout.numel == lay.numel:
        v, yo = v_full, y64
    else:  # a direction of the problem's own coordinates, expanded for the oracle
        v = prob.project(v_full)
        yo = p64.matvec(prob.expand(v).cpu().double(), p64.zeros().double())
    y = prob.matvec(v, prob.zeros())
    _check_groups(T, tag, "product", prob.expand(y).cpu(), yo, lay)
    # the weights and seeds carry rho': residuals stay raw
    r = prob.residuals[0].cpu()
    with torch.no_grad():
        r64 = p64.raw_residuals()[0]
    assert float((r.double() - r64).abs().max()) < 1e-5
    return g


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("name", ["sh1_33x17", "sh3_40x33"])
def test_problem_one_view_projected_layout(name, kind):
    prob = _problem(name, kind, sh_projection=True)
    assert prob.layout.rest_projected
    _loss_rhs_product("test_problem_one_view_projected_layout", f"{name} {kind}", prob, solved(name, kind))


@pytest.mark.parametrize("kind", RR.KINDS)
def test_problem_two_views_full_layout(kind):
    prob = _problem("sh1_33x17", kind, n_views=2)
    assert not prob.layout.rest_projected and len(prob.views) == 2
    _loss_rhs_product("test_problem_two_views_full_layout", f"sh1_33x17 x2 {kind}", prob,
                      solved("sh1_33x17", kind, True, 2))


@pytest.mark.parametrize("union_active", [False, True])
@pytest.mark.parametrize("kind", RR.KINDS)
def test_batched_problem_two_views(kind, union_active):
    from gslm.lm import BatchedLMProblem, cgls_fused
    prob = _problem("sh3_40x33", kind, n_views=2, cls=BatchedLMProblem, union_active=union_active)
    ref = solved("sh3_40x33", kind, True, 2)
    T = "test_batched_problem_two_views"
    g = _loss_rhs_product(T, f"sh3_40x33 x2 batched {kind}", prob, ref)
    x, _ = cgls_fused(prob, g, max_iter=5, restart_iter=5, check_every=True)
    _check_groups(T, f"sh3_40x33 x2 batched union={int(union_active)} {kind}", "solve", prob.expand(x).cpu(), ref[4],
                  ref[0].layout)


@pytest.mark.parametrize("kind", RR.KINDS)
def test_diagonal_is_the_robust_products(kind):
    """diagonal(damp=True) against e_j^T (A e_j) of the float64 robust product on two columns per group -- the group's
    largest entry (the scale of the bound, lm_diag_ref.GPU_TOL per group) and one more."""
    name = "sh1_33x17"
    prob = _problem(name, kind)
    prob.evaluate()
    prob.rhs(prob.zeros())
    d = prob.diagonal().cpu().double()
    p64 = solved(name, kind)[0]
    lay = p64.layout
    T = "test_diagonal_is_the_robust_products"
    for gname in D.DIAG_GROUPS:
        a, b = lay.offsets[gname]
        top = a + int(d[a:b].argmax())
        nz = (d[a:b] > 0.05 * d[top]).nonzero().reshape(-1)
        cols = [top, a + int(nz[len(nz) // 2])]
        want = []
        for j in cols:
            e = torch.zeros(lay.numel, dtype=torch.float64)
            e[j] = 1.0
            want.append(float(p64.matvec(e, p64.zeros().double())[j]))
        err = max(abs(float(d[j]) - w) for j, w in zip(cols, want)) / want[0]
        record(T, f"{kind} {gname}: diagonal vs e^T A e (of the group's max)", err, D.GPU_TOL[gname])
        assert want[0] > 0 and err <= D.GPU_TOL[gname], (gname, cols, [float(d[j]) for j in cols], want)


@pytest.mark.parametrize("mode", ["list", "no_list", "jacobi"])
@pytest.mark.parametrize("kind", RR.KINDS)
def test_solves_against_the_float64_recursion(kind, mode, monkeypatch):
    """cgls_fused with the active list and with GSLM_CG_ACTIVE=0 against cgls_ref, and cgls_jacobi against pcg_ref with
    the same preconditioner (the device diagonal, checked above), all 5 x 5 on the float64 robust oracle."""
    from gslm.lm import cgls_fused, cgls_jacobi
    name = "sh1_33x17"
    if mode == "no_list":
        monkeypatch.setenv("GSLM_CG_ACTIVE", "0")
    prob = _problem(name, kind, sh_projection=(mode != "jacobi"))
    p64, _, g64, _, x64 = solved(name, kind)
    prob.evaluate()
    g = prob.rhs(prob.zeros())
    if mode == "jacobi":
        x, info = cgls_jacobi(prob, g, max_iter=5, restart_iter=5, check_every=True)
        assert info["precond"] == "jacobi"
        dg = prob.diagonal().cpu().double()
        minv = torch.where(dg > 0, 1.0 / dg, torch.zeros_like(dg))
        x64 = D.pcg_ref(p64, g64, minv, 5, 5)
    else:
        x, info = cgls_fused(prob, g, max_iter=5, restart_iter=5, check_every=True)
        if mode == "list":
            assert prob.active_view() is not None
    assert float(x64.abs().max()) > 0
    _check_groups("test_solves_against_the_float64_recursion", f"{name} {kind} {mode}", "solve",
                  prob.expand(x).cpu(), x64, p64.layout)


# ---------------------------------------------------------------- 4. lm_step
def _step_scene():
    model, cams = scene("sh1_33x17", f64=False, n_views=3)
    return model, cams


def _lm_step(kind, **kw):
    from gslm.lm import clear_val_cache, lm_step
    model, cams = _step_scene()
    m = model.to(DEV)
    cams = [c.to(DEV) for c in cams]
    rob = None if kind is None else (kind, RR.DELTA["sh1_33x17"])
    out = lm_step(m, cams[:1], cams[1:], torch.tensor(BG_GENERIC), max_iter=5, restart_iter=5, val_at_start=True,
                  cache_val=False, **({"robust": rob} if kind != "absent" else {}), **kw)
    clear_val_cache()
    return out, [t.detach().clone() for t in m.params()]


@pytest.mark.parametrize("kind", RR.KINDS)
def test_lm_step_union_equals_exact_and_matches_the_float64_restatement(kind):
    from gslm.lm import update_params
    from oracle.lm_ref import cgls_ref, line_search_ref
    (u, pu), (x, px) = _lm_step(kind, line_search="union"), _lm_step(kind, line_search="exact")
    assert u["line_search"] == "union" and x["line_search"] == "exact"
    assert u["robust"] == x["robust"] == (kind, RR.DELTA["sh1_33x17"])
    assert u["trace"] == x["trace"] and u["best_alpha"] == x["best_alpha"]
    assert u["final_val_loss"] == x["final_val_loss"] and u["val_start_loss"] == x["val_start_loss"]
    assert u["start_loss"] == x["start_loss"]
    for a, b in zip(pu, px):
        assert torch.equal(a, b)
    # the robust validation loss falls
    assert u["final_val_loss"] < u["val_start_loss"]
    # the float64 restatement of the step
    m64, c64 = scene("sh1_33x17", f64=True, n_views=3)
    bg64 = torch.tensor(BG_GENERIC, dtype=torch.float64)
    rob = (kind, RR.DELTA["sh1_33x17"])
    p64 = RR.RobustOracleLMProblem(m64, c64[:1], bg64, rob)
    start64 = float(p64.evaluate())
    s64 = cgls_ref(p64, p64.rhs(), 5, 5)
    val = RR.RobustOracleLossEvaluator(m64, c64[1:], bg64, rob)
    vstart64 = float(val.evaluate())
    alpha64, final64, trace64 = line_search_ref(lambda a: update_params(m64, p64.layout, s64, a), val.evaluate)
    T = "test_lm_step_union_equals_exact_and_matches_the_float64_restatement"
    print("float64 trace", trace64, "gpu trace", u["trace"])
    assert u["best_alpha"] == alpha64
    worst = max([abs(a[1] - b[1]) / b[1] for a, b in zip(u["trace"], trace64)]
                + [abs(u["final_val_loss"] - final64) / final64, abs(u["val_start_loss"] - vstart64) / vstart64,
                   abs(u["start_loss"] - start64) / start64])
    record(T, f"{kind}: losses vs float64 step (rel, worst)", worst, 1e-6)
    assert worst <= 1e-6, (u["trace"], trace64)


def test_lm_step_robust_none_is_the_existing_step():
    (a, pa), (b, pb) = _lm_step("absent"), _lm_step(None)
    assert "robust" not in a and "robust" not in b
    assert a["trace"] == b["trace"] and a["best_alpha"] == b["best_alpha"]
    assert a["final_val_loss"] == b["final_val_loss"] and a["start_loss"] == b["start_loss"]
    assert torch.equal(a["step"], b["step"])
    for s, t in zip(pa, pb):
        assert torch.equal(s, t)
    # and the robust step is another step
    c, _ = _lm_step("huber")
    assert c["start_loss"] != a["start_loss"] and not torch.equal(c["step"], a["step"])


@pytest.mark.parametrize("kw", [dict(multiview="batched"), dict(multiview="batched", union_active=True),
                                dict(precond="jacobi"), dict(damping="marquardt")])
def test_lm_step_robust_with_the_other_options(kw):
    """The combinations the step allows run and descend on the robust validation loss."""
    from gslm.lm import clear_val_cache, lm_step
    model, cams = scene("sh1_33x17", f64=False, n_views=4)
    m = model.to(DEV)
    cams = [c.to(DEV) for c in cams]
    extra = dict(kw)
    if "damping" in kw:
        extra.update(damp={k: 1e-2 for k in ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity",
                                             "exposure")}, marquardt_floor=1e-6)
    out = lm_step(m, cams[:2], cams[2:], torch.tensor(BG_GENERIC), max_iter=5, restart_iter=5, val_at_start=True,
                  cache_val=False, robust=("cauchy", 0.25), **extra)
    clear_val_cache()
    assert out["robust"] == ("cauchy", 0.25)
    assert math.isfinite(out["final_val_loss"]) and out["final_val_loss"] < out["val_start_loss"]
