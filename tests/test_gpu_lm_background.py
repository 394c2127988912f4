"""GPU: the LM path under a nonzero background, alpha masks and saturated pixels, against the CPU oracle.

The reference LM loop renders over a white or random background, multiplies every render by the camera's alpha mask
and clamps it to [0, 1] before the residual.  The LM path carries code for all three -- the background tangent
u = 2 w (dC + dT bg) of k_render_matvec and k_render_jv_wave, the background adjoint tb = -T_final <bg, dL/dpix> of
vjp_init, the weight m^2 1[0 <= R <= 1] and seed -2 m 1[..] r of gslm_lm_residual, the loss blends'
m clamp01(C + T bg) - gt -- and every other LM test passes bg = 0, an all-ones mask and unsaturated renders, where a
wrong dT recurrence, a missing tb or a blend without T bg changes no asserted number.

Scenes (tests/scenes.py, lm_bg_scene): 1500 Gaussians / SH 2 / 64x48, 1500 / SH 3 (active degree 2) / 40x33 and
600 / SH 1 / 33x17, every 2nd Gaussian's SH DC raised by 2..3 so blended pixels exceed 1; backgrounds white,
(0.2, 0.5, 0.9) and zero; [1, H, W] masks with values in [0.25, 0.95) and a block of exact zeros.  What each scene
must exercise is asserted on oracle data in the tests (scenes.assert_lm_bg_scene).  Measured on the CPU oracle:

  scene / view         raw > 1 (white, generic, zero bg)   covered and T_final > 0.05   nearest covered pixel-channel
                                                                                     to a clamp corner (asserted > 1e-5)
  sh2_64x48 view 0       21.1 %  11.6 %   8.1 %               54.7 %                    6.1e-5 (white), 1.2e-4 (generic)
  sh2_64x48 view 1       19.9 %  10.2 %   7.1 %               50.9 %                    2.3e-4 (generic)
  sh2_64x48 view 2       22.2 %  12.1 %   8.5 %               53.3 %                    (losses only)
  sh2_64x48 occluders     5.9 %                               53.8 %                    5.0e-5 (white)
  sh3_40x33              23.8 %  13.3 %   9.9 %               48.3 %                    4.0e-5 (white), 8.2e-5 (generic)
  sh1_33x17              24.5 %  15.1 %  12.3 %               46.2 %                    3.7e-5 (white), 4.5e-4 (generic)

  oracle float32, ||y(bg) - y(0)|| / ||y(bg)|| over the three scenes: J^T b 0.58 - 0.68 (white), 0.50 - 0.54 (generic);
  (J^T J + D) v 0.61 - 0.76 (white), 0.34 - 0.43 (generic).  ||y(mask) - y(ones)|| / ||y(mask)||: J^T b 3.5 - 4.0,
  product 1.2 - 1.8.

The control (bg = 0, no mask, no brightened Gaussians: the oracle's raw render stays inside [0, 1), max 0.95) runs the
same scenes through the same code: a failure of a case above that the control does not share belongs to the new axes.

The expected values' own background / mask / clamp handling is pinned in float64 by
tests/test_oracle_lm_background.py.  Bounds: those of the tests this file extends (tests/test_gpu_edge.py's
test_lm_product_sh_degrees_and_sizes and test_lm_ssim_product_small_and_ragged_images: loss rel 1e-5, vectors 1e-4 of
the reference's max; test_gpu_lm.py, test_gpu_cull.py, test_gpu_active_set.py, test_gpu_dist.py and
test_gpu_line_search.py for the internal equalities), none widened."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

from margins import record
from scenes import (BG_GENERIC, BG_WHITE, BG_ZERO, LM_BG_SCENES, ZERO_BLOCKS, assert_lm_bg_scene, lm_bg_mask,
                    lm_bg_scene, lm_bg_stats, place_in_zero_block, to_float64)

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAIN = "sh2_64x48"
BGS = {"white": BG_WHITE, "generic": BG_GENERIC, "zero": BG_ZERO}


def _scene(name, n_views=1, masked=True, brighten=True, occluders=False):
    """(model, cams, ids) on the CPU: the masks on the cameras (view i's from seed i), on the 64x48 scene twelve small
    Gaussians moved into the masks' zero block (ids)."""
    model, cams = lm_bg_scene(name, n_views=n_views, brighten=brighten, occluders=occluders)
    if name == "sh3_40x33":
        model.active_sh_degree = 2  # below the stored degree (train_jvp.py's progressive oneupSHdegree)
    ids = place_in_zero_block(model, cams[0], ZERO_BLOCKS[name]) if name == MAIN else None
    if masked:
        for i, c in enumerate(cams):
            c.alpha_mask = lm_bg_mask(name, seed=i)
    return model, cams, ids


def _direction(layout, ids, mask_xyz=True, seed=9):
    """A random vector with exposure (and, on the LM path, xyz) zeroed, and zero on the Gaussians `ids`."""
    v = torch.randn(layout.numel, generator=torch.Generator().manual_seed(seed))
    for name in (("xyz", "exposure") if mask_xyz else ("exposure",)):
        a, b = layout.offsets[name]
        v[a:b] = 0
    if ids is not None:
        for name, t in layout.views(v).items():
            if name != "exposure":
                t[ids] = 0
    return v


def _check_conditions(model, cams, bg, control, boundary=True):
    """The scene conditions, on the oracle's render of every view.  boundary=False: a comparison between two GPU paths
    that share gslm_lm_residual's weight and seed, where a pixel near a corner of the clamp falls on the same side for
    both -- saturation and visible background only."""
    out = []
    for c in cams:
        if control:
            # no new axis: nothing saturates and nothing is near the clamp's upper corner.  (The lower corner cannot
            # split the two sides: colours, alphas and bg are >= 0, so R >= 0 and 1[0 <= R] = 1 on both.)
            s = lm_bg_stats(model, c, bg)
            assert s["saturated"] == 0.0 and s["below_zero"] == 0.0 and float(s["raw"].max()) < 1 - 1e-5
            assert s["background"] >= 0.20
        elif boundary:
            s = assert_lm_bg_scene(model, c, bg)
        else:
            s = lm_bg_stats(model, c, bg)
            assert s["saturated"] >= 0.05 and s["background"] >= 0.20, (s["saturated"], s["background"])
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def _expected(name, bgname, masked, n_views=1, ssim=False, mask_xyz=True, brighten=True):
    """The oracle's loss, J^T b and (J^T J + D) v (float32, full layout; computed once per case and not modified)."""
    from oracle.lm_ref import OracleLMProblem
    model, cams, ids = _scene(name, n_views, masked, brighten)
    bg = torch.tensor(BGS[bgname])
    # (bg = 0 on the brightened scene is the oracle-only baseline of the sensitivity test: no GPU value is compared)
    stats = _check_conditions(model, cams, BGS[bgname], control=not brighten, boundary=bgname != "zero")
    op = OracleLMProblem(model, cams, bg, ssim=ssim, mask_xyz=mask_xyz)
    loss = float(op.evaluate())
    g = op.rhs()
    v = _direction(op.layout, ids, mask_xyz)
    y = op.matvec(v, op.zeros())
    return types.SimpleNamespace(op=op, loss=loss, g=g, v=v, y=y, ids=ids, stats=stats)


def _of_max(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def _gpu_problem(name, bgname, masked, n_views=1, projected=False, via_kw=False, brighten=True, **kw):
    from gslm.lm import LMProblem
    model, cams, ids = _scene(name, n_views, masked, brighten)
    masks = None
    if via_kw:  # the mask through alpha_masks= instead of the camera
        masks = [c.alpha_mask.clone().to(DEV) for c in cams]
        for c in cams:
            c.alpha_mask = torch.ones_like(c.alpha_mask)
    prob = LMProblem(model.to(DEV), [c.to(DEV) for c in cams], torch.tensor(BGS[bgname]), device=DEV,
                     sh_projection=projected, alpha_masks=masks, **kw)
    return prob, ids


def _parity(T, name, bgname, masked, projected=False, n_views=1, ssim=False, mask_xyz=True, via_kw=False,
            brighten=True):
    """Loss (rel 1e-5), J^T b and (J^T J + D) v (1e-4 of the reference's max) of the HIP LM path against the oracle."""
    ref = _expected(name, bgname, masked, n_views, ssim, mask_xyz, brighten)
    prob, ids = _gpu_problem(name, bgname, masked, n_views, projected, via_kw, brighten, ssim=ssim, mask_xyz=mask_xyz)
    proj = prob.layout.rest_projected
    assert proj == bool(projected)
    tag = (f"{name} bg={bgname} mask={int(masked)} proj={int(proj)} views={n_views} ssim={int(ssim)} "
           f"xyz={int(not mask_xyz)}")
    e_loss = record(T, f"{tag}: loss rel", abs(float(prob.evaluate()) - ref.loss) / ref.loss, 1e-5)
    assert all(n > 0 for n in prob.num_rendered())
    g = prob.rhs(prob.zeros())
    e_g = record(T, f"{tag}: J^T b (of max)", _of_max((prob.expand(g) if proj else g).cpu(), ref.g), 1e-4)
    if proj:  # a direction of the projected layout, expanded for the oracle
        v = _direction(prob.layout, ids, mask_xyz).to(DEV)
        yo = ref.op.matvec(prob.expand(v).cpu(), ref.op.zeros())
    else:
        v, yo = ref.v.to(DEV), ref.y
    y = prob.matvec(v, prob.zeros())
    e_y = record(T, f"{tag}: (J^T J + D) v (of max)", _of_max((prob.expand(y) if proj else y).cpu(), yo), 1e-4)
    assert e_loss <= 1e-5, (tag, e_loss)
    assert e_g < 1e-4, (tag, e_g)
    assert e_y < 1e-4, (tag, e_y)
    return prob, ids, g, v, y, ref


def _rows(layout, vec, ids):
    return torch.cat([t.reshape(layout.P, -1)[ids.to(vec.device)].reshape(-1) for k, t in layout.views(vec).items()
                      if k != "exposure" and t.numel()])


# ---------------------------------------------------------------- 1. what the expected values depend on
@pytest.mark.parametrize("name", list(LM_BG_SCENES))
def test_expected_values_depend_on_background_and_mask(name):
    """On the oracle (float32): moving bg from zero to white / generic, and the mask from ones to the fractional one,
    each changes J^T b and (J^T J + D) v by >= 5 % of their norm (measured 34 - 76 % and 120 - 400 %), so a kernel that
    ignored either could not meet the 1e-4 bounds below."""
    zero = _expected(name, "zero", False)
    for bgname in ("white", "generic"):
        e = _expected(name, bgname, False)
        for what, a, b in (("J^T b", e.g, zero.g), ("product", e.y, zero.y)):
            d = float((a - b).norm() / a.norm())
            print(f"{name}: {what} bg={bgname} vs zero: {d:.3f}")
            assert d >= 0.05, (what, bgname, d)
    e, m = _expected(name, "generic", False), _expected(name, "generic", True)
    for what, a, b in (("J^T b", m.g, e.g), ("product", m.y, e.y)):
        d = float((a - b).norm() / a.norm())
        print(f"{name}: {what} mask vs ones: {d:.3f}")
        assert d >= 0.05, (what, d)


# ---------------------------------------------------------------- 2. operator parity
@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("bgname", ["white", "generic"])
def test_lm_operator_background_and_mask(bgname, masked, projected):
    """One view of the 64x48 scene: white / generic background x no mask / fractional mask with a zero block x the
    full and the projected SH-rest layout.  With the mask: the Gaussians whose every touched pixel lies in the zero
    block (>= 10, verified from the oracle's rects) have exactly zero rows of J^T b and of the product, and the
    product is bitwise reproducible."""
    T = "test_lm_operator_background_and_mask"
    prob, ids, g, v, y, ref = _parity(T, MAIN, bgname, masked, projected, via_kw=(bgname == "generic"))
    if not masked:
        return
    x0, y0, x1, y1 = ZERO_BLOCKS[MAIN]
    rect, tiles = ref.stats[0]["rect"][ids] * 16, ref.stats[0]["tiles"][ids]
    inside = (tiles > 0) & (rect[:, 0] >= x0) & (rect[:, 1] >= y0) & (rect[:, 2] <= x1) & (rect[:, 3] <= y1)
    assert int(inside.sum()) >= 10, (rect.tolist(), tiles.tolist())
    hidden = ids[inside]
    assert float(_rows(prob.layout, v, hidden).abs().max()) == 0.0
    assert float(_rows(prob.layout, g, hidden).abs().max()) == 0.0
    assert float(_rows(prob.layout, y, hidden).abs().max()) == 0.0
    y1_ = y.clone()
    assert torch.equal(y1_, prob.matvec(v, prob.zeros()))  # determinism, as test_matvec_deterministic


@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("name", ["sh3_40x33", "sh1_33x17"])
def test_lm_operator_ragged_images(name, projected):
    """The ragged 40x33 (SH 3 stored, degree 2 active) and 33x17 (SH 1) scenes, generic background and mask."""
    _parity("test_lm_operator_ragged_images", name, "generic", True, projected)


def test_lm_operator_two_views_different_masks():
    """Two views, one shared background, a different mask each: the per-view accumulation into y (STAGE_OVERWRITE on
    view 0 only)."""
    _parity("test_lm_operator_two_views_different_masks", MAIN, "generic", True, n_views=2)


@pytest.mark.parametrize("name", ["sh1_33x17", "sh3_40x33"])
def test_lm_ssim_operator_background_and_mask(name):
    """The SSIM residual's product: its J v image comes from k_render_jv_wave, whose background term is code of its
    own (bounds of test_lm_ssim_product_small_and_ragged_images)."""
    _parity("test_lm_ssim_operator_background_and_mask", name, "generic", True, ssim=True)


def test_lm_operator_moving_xyz():
    """mask_xyz=False: the product runs k_render_matvec<true> (the block-cooperative jvp_tile with screen-position
    tangents), J^T b the drop-in backward; v nonzero on xyz."""
    _parity("test_lm_operator_moving_xyz", MAIN, "white", True, mask_xyz=False)


@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("name", list(LM_BG_SCENES))
def test_lm_operator_control(name, projected):
    """bg = 0, no mask, nothing saturated, on the same scenes through the same code."""
    _parity("test_lm_operator_control", name, "zero", False, projected, brighten=False)


def test_lm_operator_control_two_views_ssim_xyz():
    """The control for the two-view, SSIM and mask_xyz=False cases."""
    T = "test_lm_operator_control_two_views_ssim_xyz"
    _parity(T, MAIN, "zero", False, n_views=2, brighten=False)
    _parity(T, "sh1_33x17", "zero", False, ssim=True, brighten=False)
    _parity(T, MAIN, "zero", False, mask_xyz=False, brighten=False)


# ---------------------------------------------------------------- 3. the LM path's internal equalities
def _main_problem(**kw):
    prob, ids = _gpu_problem(MAIN, "white", True, **kw)
    return prob, ids


def test_fused_rhs_matches_dropin_backward_with_background():
    """J^T b on the LM rows (vjp_init's tb in k_render_bwd<false, false, 2>) against the drop-in backward's, white
    background, mask and saturation (1e-5 of max, test_fused_rhs_matches_dropin_backward)."""
    _expected(MAIN, "white", True)  # the scene's conditions
    prob, _ = _main_problem()
    prob.evaluate()
    gf = prob.rhs(prob.zeros()).clone()
    gd = prob.rhs(prob.zeros(), fused=False)
    e = record("test_fused_rhs_matches_dropin_backward_with_background", "fused vs drop-in J^T b (of max)",
               _of_max(gf, gd), 1e-5)
    assert e <= 1e-5, e


def test_cull_bitwise_with_background():
    """Culled against exhaustive traversal (view.debug = 1): J^T b and the product bitwise equal
    (test_cull_lm_matvec_bitwise)."""
    _expected(MAIN, "white", True)
    out = []
    for debug in (0, 1):
        prob, ids = _main_problem()
        for vr in prob.views:
            vr.view.debug = debug
        prob.evaluate()
        g = prob.rhs(prob.zeros()).clone()
        v = _direction(prob.layout, ids).to(DEV)
        out.append((g, prob.matvec(v, prob.zeros()).clone()))
    assert float(out[0][0].abs().max()) > 0 and float(out[0][1].abs().max()) > 0
    assert torch.equal(out[0][0], out[1][0]), "J^T b differs between culled and exhaustive traversal"
    assert torch.equal(out[0][1], out[1][1]), "(J^T J + D) v differs between culled and exhaustive traversal"


def test_active_set_path_with_background(monkeypatch):
    """The compact single-view path on a scene with occluders and a quarter of the Gaussians behind the camera, white
    background, mask and saturation: pack(A_full v) == A_active(pack v) bitwise, and cgls_fused with GSLM_CG_ACTIVE
    1 / 0 gives the same iteration count and stop code and x within rel 1e-4 (tests/test_gpu_active_set.py)."""
    import test_gpu_active_set as tas
    from gslm.lm import LMProblem
    model, cams, _ = _scene(MAIN, occluders=True)
    _check_conditions(model, cams, BG_WHITE, control=False)
    s = tas.Scene.__new__(tas.Scene)
    s.model, s.cam, s.P = model.to(DEV), cams[0].to(DEV), model._xyz.shape[0]
    s.prob = LMProblem(s.model, [s.cam], torch.tensor(BG_WHITE), device=DEV, sh_projection="auto")
    s.prob.evaluate()
    s.g = s.prob.rhs(s.prob.zeros())
    s.vr = s.prob.views[0]
    s.ids, s.Pa = s.vr.active_list(s.P, s.prob.stream)
    s.act = s.prob.active_view()
    torch.cuda.synchronize()
    print(f"active list: Pa {s.Pa} of P {s.P}")
    assert 0.2 * s.P <= s.Pa <= 0.8 * s.P, (s.Pa, s.P)
    for seed in (11, 12):
        v = s.restrict(s.random_v(seed))
        vp = s.act.pack(v)
        yf, df, _, _ = tas._product(s.prob, v)
        ya, da, _, _ = tas._product(s.act, vp)
        assert float(yf.abs().max()) > 0
        assert torch.equal(s.act.pack(yf), ya)
        assert torch.equal(s.act.unpack(ya), s.restrict(yf))
        assert abs(df - da) <= 1e-12 * float((v.double() * yf.double()).abs().sum())
    kw = dict(max_iter=5, restart_iter=5, check_every=True)
    xf, inf, nf = tas._solve(s, s.g, False, monkeypatch, **kw)
    xa, ina, na = tas._solve(s, s.g, True, monkeypatch, **kw)
    assert nf == 0 and na > 0
    assert ina["iters"] == inf["iters"] and ina.get("stop") == inf.get("stop")
    rel = record("test_active_set_path_with_background", "compact vs full CGLS x (rel)",
                 float((xa.double() - xf.double()).norm() / xf.double().norm()), 1e-4)
    assert rel < 1e-4, rel
    np.testing.assert_allclose(ina["residuals"], inf["residuals"], rtol=1e-4)


def test_gaussian_sharded_operator_with_background():
    """GaussianShardedOperator at world size 1 (its RENDER | SCREEN stages run vjp_init with the same v.bg) against the
    fused single-process product: two views with different masks, white background
    (test_gaussian_sharded_single_rank_equals_lmproblem's bounds)."""
    import test_gpu_dist as tgd
    from gslm.lm import LMProblem
    from gslm.parallel import GaussianShardedOperator
    model, cams, _ = _scene(MAIN, n_views=2)
    _check_conditions(model, cams, BG_WHITE, control=False, boundary=False)
    model = model.to(DEV)
    cams = [c.to(DEV) for c in cams]
    bg = torch.tensor(BG_WHITE)
    op = GaussianShardedOperator(LMProblem(model, cams, bg), all_cams=cams)
    got = tgd._run(op, op.layout)
    lp = LMProblem(model, cams, bg)
    ref = tgd._run(lp, lp.layout, v=got["v"])
    T = "test_gaussian_sharded_operator_with_background"
    assert abs(float(got["loss"]) - float(ref["loss"])) <= 1e-12 * float(ref["loss"])
    assert record(T, "J^T b (of max)", _of_max(got["g"], ref["g"]), 1e-6) <= 1e-6
    assert record(T, "product (of max)", _of_max(got["y"], ref["y"]), 1e-5) <= 1e-5
    assert record(T, "3 CG iterations x (rel)", float((got["x"] - ref["x"]).norm() / ref["x"].norm()), 1e-4) <= 1e-4


def test_cgls_against_float64_oracle_with_background():
    """Five CGLS iterations (5 x 5) of cgls_fused against cgls_ref on the float64 oracle, white background, mask and
    saturation: x within rel 1e-4 in norm, the LM model decrease within 1e-5
    (test_recursions_against_float64_oracle's helpers and bounds)."""
    from gslm.lm import cgls_fused
    from oracle.lm_ref import OracleLMProblem, cgls_ref
    from test_gpu_lm import _model_gap
    model, cams, _ = _scene(MAIN)
    _check_conditions(model, cams, BG_WHITE, control=False)
    mc, ccs = to_float64(model, cams)
    op = OracleLMProblem(mc, ccs, torch.tensor(BG_WHITE, dtype=torch.float64))
    op.evaluate()
    x64 = cgls_ref(op, op.rhs(), 5, 5)
    prob, _ = _main_problem()
    prob.evaluate()
    g = prob.rhs(prob.zeros())
    x, info = cgls_fused(prob, g, max_iter=5, restart_iter=5, check_every=True)
    T = "test_cgls_against_float64_oracle_with_background"
    gap = record(T, "model decrease rel vs float64", _model_gap(prob, g, x, x64.float().numpy()), 1e-5)
    err = record(T, "x vs float64 oracle (rel)", float((x.double().cpu() - x64).norm() / x64.norm()), 1e-4)
    assert float(x64.norm()) > 0
    assert gap <= 1e-5, gap
    assert err < 1e-4, err


# ---------------------------------------------------------------- 4. line-search losses
def _line_search_setup(bgname="generic"):
    """Three masked views of the 64x48 scene: the model and cameras on the GPU, CPU copies for the oracle.  (The loss
    is continuous across the clamp's corners, so only the saturation and background conditions are asserted here; the
    line-search points change the render, and each point's saturated share is checked where it is used.)"""
    model, cams, _ = _scene(MAIN, n_views=3)
    _check_conditions(model, cams, BGS[bgname], control=False, boundary=False)
    mc, ccs = copy.deepcopy(model), [copy.deepcopy(c) for c in cams]
    return model.to(DEV), [c.to(DEV) for c in cams], mc, ccs


def test_line_search_losses_match_oracle():
    """LossEvaluator.evaluate() (k_render_loss) and evaluate_points (k_render_loss_sets / the per-slot blend) against
    OracleLossEvaluator at the six line-search points, generic background and three different masks: each loss to rel
    1e-5; and the union evaluator equals the exact one with == for loss_sets default, 2 and 8."""
    import test_gpu_line_search as tls
    from gslm.lm import LossEvaluator
    from oracle.lm_ref import OracleLossEvaluator
    m, cams, mc, ccs = _line_search_setup()
    bg = torch.tensor(BG_GENERIC)
    lay, s = tls._step(m)
    ev_x = LossEvaluator(m, cams, bg, batch=2, streams=2)
    ev_u = LossEvaluator(m, cams, bg, batch=2, streams=2)
    sets, exact, _, _ = tls._points(m, lay, s, ev_x)
    names = ("_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
    cpu_sets = [types.SimpleNamespace(**{k: getattr(st, k).cpu() for k in names}) for st in sets]
    want = [float(x) for x in OracleLossEvaluator(mc, ccs, bg).evaluate_points(cpu_sets)]
    assert len(set(want)) == 6  # six different renders
    union = [float(x) for x in ev_u.evaluate_points(sets)]
    T = "test_line_search_losses_match_oracle"
    worst_x = record(T, "exact evaluator vs oracle (rel, worst point)",
                     max(abs(a - b) / b for a, b in zip(exact, want)), 1e-5)
    worst_u = record(T, "union evaluator vs oracle (rel, worst point)",
                     max(abs(a - b) / b for a, b in zip(union, want)), 1e-5)
    assert worst_x <= 1e-5 and worst_u <= 1e-5, (exact, union, want)
    assert union == exact
    for k in (2, 8):
        ev_u.loss_sets = k
        assert [float(x) for x in ev_u.evaluate_points(sets)] == exact, k


def test_lm_step_union_equals_exact_with_white_background():
    """lm_step with the union and the exact line search, white background and masks: identical traces, best_alpha and
    final loss (test_lm_step_union_equals_exact_line_search), and the step descends."""
    from gslm.lm import clear_val_cache, lm_step
    outs, params = [], []
    bg = torch.tensor(BG_WHITE)
    for ls in ("union", "exact"):
        model, cams, _ = _scene(MAIN, n_views=2)
        if not outs:
            _check_conditions(model, cams, BG_WHITE, control=False, boundary=False)
        m = model.to(DEV)
        cams = [c.to(DEV) for c in cams]
        outs.append(lm_step(m, cams, cams, bg, max_iter=5, restart_iter=5, line_search=ls, val_at_start=True,
                            cache_val=False))
        params.append([t.detach().clone() for t in m.params()])
    clear_val_cache()
    u, x = outs
    assert u["line_search"] == "union" and x["line_search"] == "exact"
    print("trace", u["trace"], "start", u["start_loss"], "final", u["final_val_loss"])
    assert u["trace"] == x["trace"]
    assert u["best_alpha"] == x["best_alpha"]
    assert u["final_val_loss"] == x["final_val_loss"]
    assert u["val_start_loss"] == x["val_start_loss"]
    for a, b in zip(*params):
        assert torch.equal(a, b)
    assert u["final_val_loss"] <= u["start_loss"]
