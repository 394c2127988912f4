"""GPU: the inverse-depth residual of the fused LM product -- gslm_lm_residual_depth, GSLM_MV_DEPTH on
gslm_matvec_view_ex / gslm_matvec_view_active (k_render_matvec_depth, k_render_bwd_lm_depth), the loss blends
gslm_rasterize_loss_depth / gslm_rasterize_loss_slot_depth, and LMProblem / LossEvaluator / lm_step with `depth_weight`.

References (tests/lm_depth_ref.py, pinned on the CPU by tests/test_oracle_lm_depth.py):
  epilogue     the float32 torch restatement on the CPU, by torch.equal for residual, weight and seed; the loss against
               the float64 sum of the restatement's terms at 1e-12 relative;
  neutrality   a fourth plane of zeros (depth_weight = 0) against the problem without the option, bitwise;
  operator     DepthOracleLMProblem in float64, per group relative to the group's max, at 8 x the float32 oracle's own
               distance (lm_depth_ref.GPU_TOL); the measured margins go to the parity log (tests/margins.py);
  list depths  the stack scenes of tests/blend_reference.py at depths on and next to the J v pass's 64-entry rounds and
               the back-to-front pass's 128-entry batches, at blend_reference.BAR["lm_vector"], each case's float64
               decisions inside that bar's margins;
  composition  cgls_fused with and without the active list and the lean loop, bitwise; the projected layout against
               the full one within tests/test_gpu_shproj.py's bounds;
  blends       gslm_rasterize + both epilogues (LMProblem.evaluate) at 1e-12 of the loss and the oracle at the loss
               floor; the slot form against each point's own render by ==;
  lm_step      the float64 restatement (cgls_ref 5 x 5 + line_search_ref on the depth oracle): the same alpha, the step
               within the solve bound, the combined validation loss lower than before the step."""
import copy
import ctypes
import functools
import itertools
import math
import types

import pytest
import torch

import blend_reference as br
import lm_depth_ref as DR
from margins import record
from scenes import BG_GENERIC, activated, stack_scene, to_float64
from test_oracle_lm_depth import solved

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -7777.0
LAM = DR.LAMBDA_D


# ---------------------------------------------------------------- 1. the residual epilogue
def _planes(H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    D = 0.05 + 1.5 * torch.rand(H, W, generator=gen)
    gt = D * (0.7 + 0.6 * torch.rand(H, W, generator=gen))
    mask = (torch.rand(H, W, generator=gen) > 0.2).float()
    mask[H // 4:H // 4 + max(1, H // 3), W // 5:W // 5 + max(1, W // 2)] = 0.0  # a block of exact zeros
    frac = 0.25 + 0.7 * torch.rand(H, W, generator=gen)  # and a fractional mask: the arithmetic is stated for any m
    return D, gt, mask, frac


def _guarded(n, on):
    """A NaN-filled float32 output of n elements between two guard elements (None when the output is not asked for)."""
    if not on:
        return None
    t = torch.full((n + 2,), math.nan, dtype=torch.float32, device=DEV)
    t[0] = t[n + 1] = GUARD
    return t


def _run_epilogue(H, W, D, gt, mask, lam, outs, accumulate, base=3.5):
    """One call of gslm_lm_residual_depth: (residual, weight, seed) as CPU tensors or None, and the loss."""
    from gslm._lib import check, lib
    n = H * W
    bufs = [_guarded(n, on) for on in outs]
    scr = torch.empty(lib.gslm_residual_scratch_bytes(H, W) // 8, dtype=torch.float64, device=DEV)
    loss = torch.full((3,), base, dtype=torch.float64, device=DEV)
    ptrs = [None if b is None else b.data_ptr() + 4 for b in bufs]
    check(lib.gslm_lm_residual_depth(H, W, D.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), lam,
                                     *ptrs, scr.data_ptr(), scr.numel() * 8, loss.data_ptr() + 8, accumulate, None),
          "gslm_lm_residual_depth")
    torch.cuda.synchronize()
    assert float(loss[0]) == base and float(loss[2]) == base
    got = []
    for b in bufs:
        if b is None:
            got.append(None)
            continue
        c = b.cpu()
        assert float(c[0]) == GUARD and float(c[n + 1]) == GUARD
        got.append(c[1:n + 1].reshape(H, W))
    return got, float(loss[1])


SIZES = [(1, 1), (16, 16), (17, 33), (33, 40), (512, 520)]  # (H, W); the last: past the 1024-block grid's one pass


@pytest.mark.parametrize("H,W", SIZES)
def test_epilogue_bitwise_against_the_torch_restatement(H, W):
    """residual, weight and seed by torch.equal, the loss at 1e-12 relative: mask NULL, a mask with a block of zeros
    and a fractional one, two weights, every NULL-output combination (the loss-only mode among them) on NaN-filled
    destinations between guard elements, accumulate 0 and 1."""
    D, gt, mask, frac = _planes(H, W, seed=H * 1000 + W)
    dD, dg = D.to(DEV), gt.to(DEV)
    base = 3.5
    for lam, m in itertools.product((LAM, 0.3), (None, mask, frac)):
        r, w, s, terms = DR.epilogue_f32(D, gt, m, lam)
        want_loss = float(terms.sum())
        dm = None if m is None else m.to(DEV)
        combos = [(c, 0) for c in itertools.product((True, False), repeat=3)] + [((True,) * 3, 1), ((False,) * 3, 1)]
        for outs, acc in combos:
            got, loss = _run_epilogue(H, W, dD, dg, dm, lam, outs, acc, base)
            for g, ref, what in zip(got, (r, w, s), ("residual", "weight", "seed")):
                if g is not None:
                    assert torch.equal(g, ref), (what, lam, outs, float((g - ref).abs().max()))
            want = want_loss + (base if acc else 0.0)
            assert abs(loss - want) <= 1e-12 * want, (lam, outs, acc, loss, want)
    if H * W > 1:
        assert float(mask.mean()) < 1.0 and float((mask == 0).float().mean()) > 0.1


def test_epilogue_zero_weight_and_nan():
    """depth_weight = 0: weight, seed and the loss term are exact zeros; a NaN inverse depth stays a NaN in the
    residual, the seed and the loss (the weight does not depend on it)."""
    H, W = 17, 33
    D, gt, mask, _ = _planes(H, W, seed=77)
    (r, w, s), loss = _run_epilogue(H, W, D.to(DEV), gt.to(DEV), mask.to(DEV), 0.0, (True, True, True), 0)
    assert not bool(w.any()) and not bool(s.any()) and loss == 0.0 and float(r.abs().max()) > 0
    D[3, 4] = math.nan
    mask[3, 4] = 1.0
    (r, w, s), loss = _run_epilogue(H, W, D.to(DEV), gt.to(DEV), mask.to(DEV), LAM, (True, True, True), 0)
    assert math.isnan(loss)
    for g in (r, s):
        assert math.isnan(float(g[3, 4])) and int(torch.isnan(g).sum()) == 1
    assert not bool(torch.isnan(w).any())


def test_epilogue_error_returns_leave_the_outputs():
    from gslm import _lib
    H, W = 17, 33
    D, gt, _, _ = _planes(H, W, seed=6)
    dD, dg = D.to(DEV), gt.to(DEV)
    out = torch.full((3, H * W), 7.0, dtype=torch.float32, device=DEV)
    loss = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
    scr = torch.empty(1024, dtype=torch.float64, device=DEV)

    def call(H=H, W=W, D=dD.data_ptr(), gt=dg.data_ptr(), lam=LAM, scratch=scr.data_ptr(), nbytes=scr.numel() * 8,
             lossp=loss.data_ptr()):
        return _lib.lib.gslm_lm_residual_depth(H, W, D, gt, None, lam, out[0].data_ptr(), out[1].data_ptr(),
                                               out[2].data_ptr(), scratch, nbytes, lossp, 0, None)

    for kw in (dict(H=-1), dict(W=-1), dict(D=None), dict(gt=None), dict(lam=-1.0), dict(lam=math.nan),
               dict(lam=math.inf), dict(scratch=None), dict(lossp=None)):
        assert call(**kw) == _lib.GSLM_ERR_INVALID, kw
    assert call(nbytes=scr.numel() * 8 - 1) == _lib.GSLM_ERR_CAPACITY
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and float(loss) == 7.0


# ---------------------------------------------------------------- 2. problems
def _problem(name, n_views=1, depth_views=None, lam=LAM, occluders=False, **kw):
    from gslm.lm import LMProblem
    model, cams = DR.scene(name, False, n_views, depth_views, occluders=occluders)
    extra = {} if lam is None else {"depth_weight": lam}
    return LMProblem(model.to(DEV), [c.to(DEV) for c in cams], torch.tensor(BG_GENERIC), device=DEV, **extra, **kw)


def _dot(prob, v, y):
    """(y, <v, y>) of matvec_dot with the dot fused into the gather (single view)."""
    d = torch.zeros(1, dtype=torch.float64, device=DEV)
    fused = prob.matvec_dot(v, y, d.data_ptr())
    torch.cuda.synchronize()
    return y, float(d), fused


@pytest.mark.parametrize("sh_projection", [False, True])
@pytest.mark.parametrize("name", DR.SCENES)
def test_zero_fourth_planes_are_the_plain_call_bitwise(name, sh_projection):
    """depth_weight = 0.0: the flag is on (the depth kernels run, on [4, H, W] weights and seeds whose fourth plane is
    zero) and the loss, J^T b, y, the fused dot and a 5 x 5 solve are bitwise those of the problem without the option."""
    from gslm.lm import cgls_fused
    plain = _problem(name, lam=None, sh_projection=sh_projection)
    zero = _problem(name, lam=0.0, sh_projection=sh_projection)
    assert float(plain.evaluate()) == float(zero.evaluate())
    assert zero.weights[0].shape[0] == 4 and plain.weights[0].shape[0] == 3 and zero._depth_flag(0) == 32
    assert not bool(zero.weights[0][3].any()) and not bool(zero.seeds[0][3].any())
    assert float(zero.residuals[0][3].abs().max()) > 0  # (the residual itself is there)
    gp, gz = plain.rhs(plain.zeros()), zero.rhs(zero.zeros())
    assert torch.equal(gp, gz) and float(gp.abs().max()) > 0
    v = DR.direction(plain.full_layout, torch.float32).to(DEV)
    v = plain.project(v) if sh_projection else v
    yp, dp, fp = _dot(plain, v, plain.zeros())
    yz, dz, fz = _dot(zero, v, zero.zeros())
    assert fp and fz and torch.equal(yp, yz) and dp == dz and dp > 0
    xp, _ = cgls_fused(plain, gp, max_iter=5, restart_iter=5, check_every=True)
    xz, _ = cgls_fused(zero, gz, max_iter=5, restart_iter=5, check_every=True)
    assert torch.equal(xp, xz) and float(xp.abs().max()) > 0


def _check_groups(T, tag, what, got, ref, layout):
    errs = DR.group_errors(got, ref, layout)
    for k, v in errs.items():
        record(T, f"{tag}: {what} {k} (of max)", v, DR.GPU_TOL[what][k])
    bad = {k: (v, DR.GPU_TOL[what][k]) for k, v in errs.items() if not v <= DR.GPU_TOL[what][k]}
    assert not bad, (tag, what, bad)


@pytest.mark.parametrize("entry", ["ex", "active"])
@pytest.mark.parametrize("sh_projection", [False, True])
@pytest.mark.parametrize("name", DR.SCENES)
def test_one_view_against_the_float64_oracle(name, sh_projection, entry):
    """Loss, J^T b and the product of one view with depth, full and projected layout, through gslm_matvec_view_ex and
    through the active-list entry point (the direction restricted to the listed Gaussians, so that both sides apply
    the same D v); J^T b through the drop-in backward (rhs(fused=False)) agrees with the fused one."""
    T = "test_one_view_against_the_float64_oracle"
    tag = f"{name} proj={int(sh_projection)} {entry}"
    p64, l64, g64, y64, _ = solved(name)
    lay = p64.layout
    prob = _problem(name, sh_projection=sh_projection)
    assert prob.layout.rest_projected == sh_projection
    loss = float(prob.evaluate())
    e = record(T, f"{tag}: loss rel", abs(loss - l64) / l64, DR.GPU_TOL["loss"])
    assert e <= DR.GPU_TOL["loss"], (tag, loss, l64)
    g = prob.rhs(prob.zeros())
    _check_groups(T, tag, "rhs", prob.expand(g).cpu(), g64, lay)
    v = DR.direction(lay, torch.float32).to(DEV)
    v = prob.project(v) if sh_projection else v
    if entry == "active":
        act = prob.active_view()
        assert act is not None and 0 < act._active[1] <= lay.P
        va = act.pack(v)
        v = act.unpack(va)  # zero off the list
        y = act.unpack(act.matvec(va, act.zeros()))
        assert torch.equal(y, prob.matvec(v, prob.zeros()))  # the list form is the same product, bitwise
    else:
        y = prob.matvec(v, prob.zeros())
    if sh_projection or entry == "active":
        yo = p64.matvec(prob.expand(v).cpu().double(), p64.zeros().double())
    else:
        yo = y64
    _check_groups(T, tag, "product", prob.expand(y).cpu(), yo, lay)
    if entry == "ex":
        gd = prob.rhs(prob.zeros(), fused=False)
        worst = max(DR.group_errors(gd.cpu(), g.cpu(), prob.layout).values())
        record(T, f"{tag}: drop-in backward vs fused J^T b (of max, worst group)", worst, 1e-5)
        assert worst <= 1e-5  # tests/test_gpu_shproj.py's bound for the same pair without depth


@pytest.mark.parametrize("name", DR.SCENES)
def test_two_views_one_without_depth(name):
    """View 0 with depth ([4, H, W], GSLM_MV_DEPTH), view 1 without (depth_reliable False: the plain kernels)."""
    T, tag = "test_two_views_one_without_depth", f"{name} x2"
    p64, l64, g64, y64, _ = solved(name, True, 2, (0,))
    prob = _problem(name, n_views=2, depth_views=(0,))
    loss = float(prob.evaluate())
    assert [w.shape[0] for w in prob.weights] == [4, 3] and [prob._depth_flag(b) for b in (0, 1)] == [32, 0]
    e = record(T, f"{tag}: loss rel", abs(loss - l64) / l64, DR.GPU_TOL["loss"])
    assert e <= DR.GPU_TOL["loss"], (tag, loss, l64)
    g = prob.rhs(prob.zeros())
    _check_groups(T, tag, "rhs", g.cpu(), g64, p64.layout)
    y = prob.matvec(DR.direction(p64.layout, torch.float32).to(DEV), prob.zeros())
    _check_groups(T, tag, "product", y.cpu(), y64, p64.layout)


@pytest.mark.parametrize("name", DR.SCENES)
def test_depth_only(name):
    """Alpha mask 0 and ground truth 0: the colour residual and weight vanish, and the product is
    J_D^T W_d J_D v + D v alone -- the features rows exactly D v; J^T b is the depth term alone."""
    from gslm.lm import LMProblem
    T = "test_depth_only"
    model, cams = DR.scene(name, False, 1)
    for c in cams:
        c.alpha_mask = torch.zeros_like(c.alpha_mask)
        c.original_image = torch.zeros_like(c.original_image)
    m64, c64 = to_float64(model, cams)
    bg64 = torch.tensor(BG_GENERIC, dtype=torch.float64)
    p64 = DR.DepthOracleLMProblem(m64, c64, bg64, LAM)
    only = DR.DepthOracleLMProblem(m64, c64, bg64, LAM, colour=False)
    lay = p64.layout
    v64 = DR.direction(lay)
    y64 = p64.matvec(v64, p64.zeros().double()).clone()
    assert torch.equal(y64, only.matvec(v64, only.zeros().double()))  # the oracle's colour block is exactly absent
    prob = LMProblem(model.to(DEV), [c.to(DEV) for c in cams], torch.tensor(BG_GENERIC), device=DEV, depth_weight=LAM)
    prob.evaluate()
    assert not bool(prob.weights[0][:3].any()) and not bool(prob.seeds[0][:3].any())
    g = prob.rhs(prob.zeros())
    v = v64.float().to(DEV)
    y = prob.matvec(v, prob.zeros())
    gv, yv, vv = prob.layout.views(g), prob.layout.views(y), prob.layout.views(v)
    for k in ("features_dc", "features_rest"):
        assert not bool(gv[k].any()), k
        assert torch.equal(yv[k], vv[k] * torch.tensor(prob.damp[k], dtype=torch.float32)), f"{k}: not exactly D v"
    for what, got, ref in (("rhs", g, p64.rhs()), ("product", y, y64)):
        errs = DR.group_errors(got.cpu(), ref, lay, DR.DEPTH_GROUPS)
        for k, e in errs.items():
            record(T, f"{name}: depth-only {what} {k} (of max)", e, DR.GPU_TOL[what][k])
            assert e <= DR.GPU_TOL[what][k], (what, k, e)


# ---------------------------------------------------------------- 3. list depths around the passes' batch sizes
STACK_DEPTHS = (63, 64, 65, 127, 128, 129, 257)
STACK_SIZES = {"16x16": dict(W=16, H=16), "33x17": dict(W=33, H=17, **br.WIDE)}


@functools.lru_cache(maxsize=None)
def _stack_ref(n, size):
    """The float64 oracle of the stack scene of depth n with depth targets: (model, cam) in float32 for the GPU, J^T b,
    the direction, the product, and the decision margins of the float64 blend."""
    from oracle import torch_raster as tr
    model, cam = stack_scene(n, **STACK_SIZES[size])
    DR.set_depth_targets(model, [cam], BG_GENERIC)
    m64, (c64,) = to_float64(model, [cam])
    bg64 = torch.tensor(BG_GENERIC, dtype=torch.float64)
    p64 = DR.DepthOracleLMProblem(m64, [c64], bg64, LAM)
    g = p64.rhs()
    v = br.lm_direction(p64.layout, True)
    y = p64.matvec(v.double(), p64.zeros().double()).clone()
    st = tr.settings_from_camera(c64, bg64, 1)
    with torch.no_grad():
        a = activated(m64)
        _, _, _, I = tr.rasterize(a["means3D"], torch.zeros_like(a["means3D"]), a["opacities"], st, shs=a["shs"],
                                  scales=a["scales"], rotations=a["rotations"], return_internals=True)
    ref = types.SimpleNamespace(final_T=I["final_T"], n_contrib=I["n_contrib"], point_list=I["point_list"],
                                ranges=I["ranges"], pre=I["pre"])
    return model, cam, g, v, y, br.decision_margins(ref), br.tile_depths(ref)


@pytest.mark.parametrize("size", list(STACK_SIZES))
@pytest.mark.parametrize("n", STACK_DEPTHS)
def test_list_depths(n, size):
    """J^T b (k_render_bwd_lm_depth: 128-entry batches) and the product (k_render_matvec_depth: 64-entry rounds of the
    J v pass with its 1/z plane, then the batches) at depths 63 / 64 / 65 and 127 / 128 / 129 / 257."""
    from gslm.lm import LMProblem
    T = "test_list_depths"
    model, cam, g64, v, y64, m, depths = _stack_ref(n, size)
    # every tile blends the whole stack, and float32 takes every decision as float64 does (the bar's margins)
    assert all(d == (n, n) for d in depths), depths
    assert m["alpha"] >= 1e-4 and m["T"] >= 1e-4 and m["power"] >= 1e-4 and m["clamp"] >= 1e-4, m
    prob = LMProblem(copy.deepcopy(model).to(DEV), [copy.deepcopy(cam).to(DEV)], torch.tensor(BG_GENERIC), device=DEV,
                     depth_weight=LAM)
    prob.evaluate()
    g = prob.rhs(prob.zeros())
    y = prob.matvec(v.to(DEV), prob.zeros())
    bar = br.BAR["lm_vector"]
    eg = record(T, f"stack{n}_{size} J^T b (of max)", br.of_max(g.cpu(), g64), bar)
    ey = record(T, f"stack{n}_{size} (J^T J + D) v (of max)", br.of_max(y.cpu(), y64), bar)
    assert eg <= bar and ey <= bar, (eg, ey)
    # and the depth term is a visible part of both (a build without it fails the bar)
    plain = LMProblem(copy.deepcopy(model).to(DEV), [copy.deepcopy(cam).to(DEV)], torch.tensor(BG_GENERIC),
                      device=DEV)
    plain.evaluate()
    assert br.of_max(plain.rhs(plain.zeros()).cpu(), g64) > 100 * bar


# ---------------------------------------------------------------- 4. composition
@pytest.mark.parametrize("occluders", [True, False])
def test_solve_is_bitwise_with_and_without_the_active_list_and_the_lean_loop(occluders, monkeypatch):
    """cgls_fused 5 x 5 with depth on: x bitwise equal between GSLM_CG_ACTIVE=0 and the default, and between
    GSLM_CG_LEAN=0 and the default, at Pa < P (occluders) and Pa = P."""
    from gslm.lm import cgls_fused
    name = "sh1_33x17"

    def solve(env):
        for k in ("GSLM_CG_ACTIVE", "GSLM_CG_LEAN"):
            monkeypatch.delenv(k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        if occluders:
            prob = _problem(name, occluders=True, sh_projection=True)
        else:
            prob = _visible_problem()
        prob.evaluate()
        g = prob.rhs(prob.zeros())
        x, info = cgls_fused(prob, g, max_iter=5, restart_iter=5, check_every=False)
        na = prob.views[0].active_list(prob.layout.P, prob.stream)[1]
        return prob.expand(x).clone(), na, prob.layout.P

    x0, na, P = solve({})
    assert (na < P) if occluders else (na == P), (na, P)
    assert float(x0.abs().max()) > 0
    for env in ({"GSLM_CG_ACTIVE": "0"}, {"GSLM_CG_LEAN": "0"}):
        x1, _, _ = solve(env)
        assert torch.equal(x0, x1), env


def _visible_problem():
    """A one-view problem with depth in which every Gaussian owns a head row (Pa = P): the stack scene of depth 65."""
    from gslm.lm import LMProblem
    model, cam = _stack_ref(65, "16x16")[:2]
    return LMProblem(copy.deepcopy(model).to(DEV), [copy.deepcopy(cam).to(DEV)], torch.tensor(BG_GENERIC), device=DEV,
                     depth_weight=LAM, sh_projection=True)


@pytest.mark.parametrize("name", DR.SCENES)
def test_projected_layout_against_the_full_layout(name):
    """tests/test_gpu_shproj.py's comparisons with depth on: loss 1e-7, J^T b and the product 1e-5 of the max."""
    pf, pp = _problem(name), _problem(name, sh_projection=True)
    assert abs(float(pf.evaluate()) - float(pp.evaluate())) <= 1e-7 * float(pf.loss)
    gf, gp = pf.rhs(pf.zeros()), pp.rhs(pp.zeros())

    def close(a, b, tol):
        return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-12)

    assert close(pp.expand(gp), gf, 1e-5) and close(pp.project(gf), gp, 1e-5)
    vp = pp.project(DR.direction(pf.layout, torch.float32).to(DEV))
    yp = pp.matvec(vp, pp.zeros())
    yf = pf.matvec(pp.expand(vp), pf.zeros())
    assert close(pp.expand(yp), yf, 1e-5)


# ---------------------------------------------------------------- 5. refusals on a live problem
def test_flag_refusals_leave_the_outputs_untouched():
    """GSLM_MV_DEPTH with GSLM_MV_EXPOSURE, GSLM_MV_DAMP_VEC, jv_out, the SCREEN stage or mask_xyz = 0 on a live view:
    GSLM_ERR_INVALID and y as it was."""
    from gslm import _lib
    from gslm.params import raw_gaussians
    prob = _problem("sh1_33x17")
    prob.evaluate()
    prob.rhs(prob.zeros())
    vr, g = prob.views[0], raw_gaussians(prob.model)
    v = DR.direction(prob.layout, torch.float32).to(DEV)
    y = torch.full_like(v, 7.0)
    side = torch.full((8 * prob.layout.P + 3 * vr.H * vr.W,), 7.0, dtype=torch.float32, device=DEV)
    vs, ys = prob.layout.grads_struct(v), prob.layout.grads_struct(y)
    cases = [dict(flags=32 | 8), dict(flags=32 | 16), dict(flags=32, stages=1 | 2, jv_out=side.data_ptr()),
             dict(flags=32, stages=1 | 2 | 16, screen_out=side.data_ptr()), dict(flags=32, mask_xyz=0)]
    for kw in cases:
        kw = dict(kw)
        mask_xyz = kw.pop("mask_xyz", 1)
        o = _lib.GslmMatvecOpts()
        o.stages = 7 | 8
        for k, val in kw.items():
            setattr(o, k, val)
        st = _lib.lib.gslm_matvec_view_ex(ctypes.byref(vr.view), ctypes.byref(g), ctypes.byref(vs),
                                          prob.weights[0].data_ptr(), mask_xyz, vr.geom.data_ptr(),
                                          vr.binning.data_ptr(), vr.N, vr.image.data_ptr(), vr.scratch.data_ptr(),
                                          vr.scratch.numel(), ctypes.byref(ys), ctypes.byref(o), prob.stream)
        assert st == _lib.GSLM_ERR_INVALID, kw
        assert b"GSLM_MV_DEPTH" in _lib.lib.gslm_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((side == 7.0).all())
    for call in (prob.diagonal, lambda: prob.set_damping_vector(torch.zeros_like(v))):
        with pytest.raises(ValueError, match="depth"):
            call()


# ---------------------------------------------------------------- 6. the loss blends
def _gpu_scene(name, n_views, depth_views=None):
    model, cams = DR.scene(name, False, n_views, depth_views)
    return model.to(DEV), [c.to(DEV) for c in cams]


@pytest.mark.parametrize("name", DR.SCENES)
def test_loss_blend_against_forward_and_both_epilogues(name):
    """gslm_rasterize_loss_depth (LossEvaluator.evaluate) against gslm_rasterize + gslm_lm_residual +
    gslm_lm_residual_depth (LMProblem.evaluate) at 1e-12 of the loss, and against the float64 oracle at the loss floor:
    two views with depth (sh1_33x17: alpha masks too), and two views of which the second has none."""
    from gslm.lm import LMProblem, LossEvaluator
    T = "test_loss_blend_against_forward_and_both_epilogues"
    bg = torch.tensor(BG_GENERIC)
    for depth_views in (None, (0,)):
        model, cams = _gpu_scene(name, 2, depth_views)
        ev = LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2, depth_weight=LAM)
        got = float(ev.evaluate())
        pair = float(LMProblem(model, cams, bg, device=DEV, depth_weight=LAM).evaluate())
        record(T, f"{name} depth_views={depth_views}: blend vs forward + epilogues (rel)", abs(got - pair) / pair, 1e-12)
        assert abs(got - pair) <= 1e-12 * pair, (got, pair)
        m64, c64 = DR.scene(name, True, 2, depth_views)
        want = float(DR.DepthOracleLMProblem(m64, c64, torch.tensor(BG_GENERIC, dtype=torch.float64), LAM).evaluate())
        e = record(T, f"{name} depth_views={depth_views}: blend vs float64 oracle (rel)", abs(got - want) / want,
                   DR.GPU_TOL["loss"])
        assert e <= DR.GPU_TOL["loss"], (got, want)
        plain = float(LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2).evaluate())
        assert got - plain > 1e-3 * plain  # (the depth term is a visible part of the loss)
        zero = float(LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2, depth_weight=0.0).evaluate())
        assert zero == plain  # depth_weight = 0: the depth blend's loss is the plain blend's, bitwise


@pytest.mark.parametrize("name,depth_views", [("sh1_33x17", None), ("sh3_40x33", (0, 2))])
def test_slot_form_equals_each_points_own_render(name, depth_views, monkeypatch):
    """evaluate_points == evaluate() at each of the six line-search points (tests/test_gpu_line_search.py's
    comparison), on views with alpha masks (sh1_33x17) and without, all with depth or one without; GSLM_LOSS_SET_GROUP
    above 1 falls back to per set on the views with depth and gives the same losses."""
    import test_gpu_line_search as tls
    from gslm.lm import LossEvaluator
    model, cams = _gpu_scene(name, 3, depth_views)
    bg = torch.tensor(BG_GENERIC)
    lay, s = tls._step(model, scale=0.5)
    kw = dict(device=DEV, batch=2, streams=2, depth_weight=LAM)
    ev_x, ev_u = LossEvaluator(model, cams, bg, **kw), LossEvaluator(model, cams, bg, **kw)
    sets, exact, _, _ = tls._points(model, lay, s, ev_x)
    assert len(set(exact)) == 6
    assert [float(x) for x in ev_u.evaluate_points(sets)] == exact
    for k in (3, 8):
        ev_u.loss_sets = k
        assert [float(x) for x in ev_u.evaluate_points(sets)] == exact, k
    # and the depth term is in every point's loss
    plain = LossEvaluator(model, cams, bg, device=DEV, batch=2, streams=2)
    assert all(a > b for a, b in zip(exact, [float(x) for x in plain.evaluate_points(sets)]))


def test_blend_error_returns_leave_the_loss():
    from gslm import _lib
    model, cams = _gpu_scene("sh1_33x17", 1)
    bg = torch.tensor(BG_GENERIC)
    from gslm.lm import LossEvaluator
    ev = LossEvaluator(model, cams, bg, device=DEV, batch=1, streams=1, depth_weight=LAM)
    ev.evaluate()
    sl, vw, N = ev.slots[0], ev.views[0], ev.num_rendered[0]
    loss = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
    scr = ev.loss_scratch[0]
    dt = ev.depth[0]

    def call(gtd=dt[0].data_ptr(), lam=LAM):
        return _lib.lib.gslm_rasterize_loss_depth(ctypes.byref(vw), model._xyz.shape[0], sl["geom"].data_ptr(),
                                                  sl["binning"].data_ptr(), sl["binning"].numel(), N,
                                                  ev.gts[0].data_ptr(), None, gtd, None, lam, scr.data_ptr(),
                                                  scr.numel() * 8, loss.data_ptr(), 0, None)

    for kw in (dict(gtd=None), dict(lam=-1.0), dict(lam=math.nan), dict(lam=math.inf)):
        assert call(**kw) == _lib.GSLM_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert float(loss) == 7.0


# ---------------------------------------------------------------- 7. lm_step
def _lm_step(n_train, lam, **kw):
    from gslm.lm import clear_val_cache, lm_step
    model, cams = DR.scene("sh1_33x17", False, n_train + 2)
    m = model.to(DEV)
    cams = [c.to(DEV) for c in cams]
    extra = {} if lam == "absent" else {"depth_weight": lam}
    out = lm_step(m, cams[:n_train], cams[n_train:], torch.tensor(BG_GENERIC), max_iter=5, restart_iter=5,
                  val_at_start=True, cache_val=False, **extra, **kw)
    clear_val_cache()
    return out, [t.detach().clone() for t in m.params()]


@pytest.mark.parametrize("n_train", [1, 2])
def test_lm_step_against_the_float64_restatement(n_train):
    """lm_step(depth_weight=...) with one and two training views against cgls_ref 5 x 5 + line_search_ref on the depth
    oracle: the same chosen alpha, the step within the solve bound, losses to 1e-6, and the combined validation loss
    lower than before the step; union against exact by ==."""
    from gslm.lm import update_params
    from oracle.lm_ref import cgls_ref, line_search_ref
    T = "test_lm_step_against_the_float64_restatement"
    (u, pu), (x, px) = _lm_step(n_train, LAM, line_search="union"), _lm_step(n_train, LAM, line_search="exact")
    assert u["line_search"] == "union" and x["line_search"] == "exact" and u["depth_weight"] == LAM
    assert u["trace"] == x["trace"] and u["best_alpha"] == x["best_alpha"]
    assert u["final_val_loss"] == x["final_val_loss"] and u["start_loss"] == x["start_loss"]
    for a, b in zip(pu, px):
        assert torch.equal(a, b)
    assert u["final_val_loss"] < u["val_start_loss"]
    m64, c64 = DR.scene("sh1_33x17", True, n_train + 2)
    bg64 = torch.tensor(BG_GENERIC, dtype=torch.float64)
    p64 = DR.DepthOracleLMProblem(m64, c64[:n_train], bg64, LAM)
    start64 = float(p64.evaluate())
    s64 = cgls_ref(p64, p64.rhs(), 5, 5)
    _check_groups(T, f"sh1_33x17 x{n_train}", "solve", u["step"].cpu(), s64, p64.layout)
    val = DR.DepthOracleLossEvaluator(m64, c64[n_train:], bg64, LAM)
    vstart64 = float(val.evaluate())
    alpha64, final64, trace64 = line_search_ref(lambda a: update_params(m64, p64.layout, s64, a), val.evaluate)
    print("float64 trace", trace64, "gpu trace", u["trace"])
    assert u["best_alpha"] == alpha64
    worst = max([abs(a[1] - b[1]) / b[1] for a, b in zip(u["trace"], trace64)]
                + [abs(u["final_val_loss"] - final64) / final64, abs(u["val_start_loss"] - vstart64) / vstart64,
                   abs(u["start_loss"] - start64) / start64])
    record(T, f"x{n_train}: losses vs float64 step (rel, worst)", worst, 1e-6)
    assert worst <= 1e-6, (u["trace"], trace64)  # tests/test_gpu_lm_robust.py's bound for the same comparison


def test_lm_step_with_zero_weight_is_the_existing_step():
    (a, pa), (b, pb) = _lm_step(1, "absent"), _lm_step(1, 0.0)
    assert "depth_weight" not in a and b["depth_weight"] == 0.0
    assert a["trace"] == b["trace"] and a["best_alpha"] == b["best_alpha"]
    assert a["final_val_loss"] == b["final_val_loss"] and a["start_loss"] == b["start_loss"]
    assert a["val_start_loss"] == b["val_start_loss"] and torch.equal(a["step"], b["step"])
    for s, t in zip(pa, pb):
        assert torch.equal(s, t)
    c, _ = _lm_step(1, LAM)
    assert c["start_loss"] != a["start_loss"] and not torch.equal(c["step"], a["step"])
