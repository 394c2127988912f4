"""CPU: the yardstick of the exposure tests (tests/lm_exposure_ref.py) checked in float64 -- the exposure columns of
its J against central differences, the adjoint identity of its product, the scenes' distance from the clamp's corners,
and the SH-rest span's invariance under the product with exposure (the claim that keeps sh_projection valid)."""
import pytest
import torch

from lm_exposure_ref import (SCENES, X0, ExposureOracleLMProblem, ExposureOracleLossEvaluator, assert_exposure_scene,
                             direction, exposure_scene, set_exposures)
from scenes import BG_GENERIC, BG_ZERO, to_float64

BGS = {"zero": BG_ZERO, "generic": BG_GENERIC}


def _op64(name, bgname, masked=True):
    model, cams = exposure_scene(name, masked)
    mc, ccs = to_float64(model, cams)
    mc.exposure_mapping = dict(model.exposure_mapping)
    return ExposureOracleLMProblem(mc, ccs, torch.tensor(BGS[bgname], dtype=torch.float64))


@pytest.mark.parametrize("bgname", list(BGS))
@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_stay_clear_of_the_clamp_corners(name, bgname):
    """No pixel-channel of C within 1e-5 of 0 or 1 in either view (float32 oracle, as the GPU tests assert it); C > 1
    somewhere in every view, and with the zero background C < 0 too: both sides of the clamp are live."""
    model, cams = exposure_scene(name)
    stats = assert_exposure_scene(model, cams, BGS[bgname])
    print(name, bgname, stats)
    if bgname == "zero":
        assert all(s["below"] > 0 for s in stats), stats


@pytest.mark.parametrize("name", list(SCENES))
def test_exposure_columns_match_central_differences(name):
    """J's exposure columns: the residual is linear in X away from the clamp, so central differences are exact up to
    rounding -- every pixel-channel of both views within 1e-8."""
    op = _op64(name, "zero")
    lay = op.layout
    v = torch.zeros(lay.numel, dtype=torch.float64)
    a, b = lay.offsets["exposure"]
    v[a:b] = torch.randn(b - a, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    jv = op._jr_v(v)
    X = op.model._exposure
    V = v[a:b].view_as(X)
    eps = 1e-6
    with torch.no_grad():
        saved = X.detach().clone()
        X.copy_(saved + eps * V)
        rp = [r.clone() for r in op._residuals()]
        X.copy_(saved - eps * V)
        rm = [r.clone() for r in op._residuals()]
        X.copy_(saved)
    for t, p, m in zip(jv, rp, rm):
        fd = (p - m) / (2 * eps)
        assert float(t.abs().max()) > 0
        assert float((t - fd).abs().max()) <= 1e-8, float((t - fd).abs().max())


@pytest.mark.parametrize("bgname", list(BGS))
@pytest.mark.parametrize("name", list(SCENES))
def test_adjoint_identity_with_exposure(name, bgname):
    """<J u, J u> = <u, J^T J u> to 1e-12 with a nonzero exposure tail in u ([r; r]: both sides carry the factor 2)."""
    op = _op64(name, bgname)
    u = direction(op.layout, seed=5).double()
    lhs = 2.0 * sum(float((t * t).sum()) for t in op._jr_v(u))
    y = op.local_normal_matvec(u, torch.zeros_like(u), damp=False)
    rhs = float((u * y).sum())
    a, b = op.layout.offsets["exposure"]
    assert float(y[a:b].abs().min()) > 0  # every exposure row of both cameras takes part
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def test_exposure_rows_outside_the_batch_are_damping_only():
    """A camera outside the batch has a zero column block: its rows of J^T b are 0 and of the product D v."""
    model, cams = exposure_scene("sh1_33x17")
    op = ExposureOracleLMProblem(model, cams[:1], torch.tensor(BG_GENERIC))
    g = op.rhs()
    a, b = op.layout.offsets["exposure"]
    assert float(g[a:a + 12].abs().min()) > 0 and float(g[a + 12:b].abs().max()) == 0
    v = direction(op.layout)
    y = op.matvec(v, op.zeros())
    assert torch.equal(y[a + 12:b], op.damp["exposure"] * v[a + 12:b])


def test_single_view_krylov_space_keeps_sh_rest_in_basis_span_with_exposure():
    """tests/test_oracle_properties.py's span test with exposure: it mixes channels, and span{Bh (x) e_c, c = 0..2} is
    closed under that, so J^T b and the product of a span vector with a nonzero exposure tail stay in the span."""
    from test_oracle_properties import _rest_basis
    from scenes import make_scene
    model, cams = make_scene("tiny_300_sh2_40x33")
    cam = cams[0]
    cam.original_image = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(3))
    set_exposures(model, [cam], rows=(X0,))
    op = ExposureOracleLMProblem(model, [cam], torch.tensor(BG_GENERIC))
    op.evaluate()
    Bh = _rest_basis(model, cam).float()
    a, b = op.layout.offsets["features_rest"]
    P, Km1 = Bh.shape

    def off_span(vec):
        R = vec[a:b].view(P, Km1, 3)
        coef = (Bh[:, :, None] * R).sum(1)
        resid = R - Bh[:, :, None] * coef[:, None, :]
        return float(resid.abs().max()), float(R.abs().max())

    g = op.rhs()
    e0, e1 = op.layout.offsets["exposure"]
    assert float(g[e0:e0 + 12].abs().min()) > 0
    r, scale = off_span(g)
    assert scale > 0 and r <= 1e-5 * scale
    v = torch.randn(op.layout.numel, generator=torch.Generator().manual_seed(4))
    v[a:b] = (Bh[:, :, None] * torch.randn(P, 1, 3, generator=torch.Generator().manual_seed(5))).reshape(-1)
    y = op.matvec(v, op.zeros())
    r, scale = off_span(y)
    assert scale > 0 and r <= 1e-5 * scale


def test_float64_lm_step_descends_on_the_helper():
    """gslm.lm.lm_step's driver on the float64 helper (backend=...): ground truths rendered under X0 / X1, the model
    starting from identity exposures -- the chosen point's validation loss is below the start's, the batch's exposure
    rows move and the line search runs in the exact order."""
    from gslm.lm import lm_step
    from oracle.lm_ref import cgls_solver
    model, cams = exposure_scene("sh1_33x17", masked=False)
    mc, ccs = to_float64(model, cams)
    mc.exposure_mapping = dict(model.exposure_mapping)
    bg = torch.tensor(BG_GENERIC, dtype=torch.float64)
    op = ExposureOracleLMProblem(mc, ccs, bg)
    with torch.no_grad():
        for c in ccs:
            c.original_image = op.exposed(c).clamp(0, 1)
        mc._exposure.copy_(torch.eye(3, 4, dtype=torch.float64)[None].repeat(2, 1, 1))
    before = mc._exposure.detach().clone()
    out = lm_step(mc, ccs, ccs, bg, max_iter=5, restart_iter=5, device="cpu", train_exposure=True, val_at_start=True,
                  cache_val=False, backend=(ExposureOracleLMProblem, ExposureOracleLossEvaluator, cgls_solver))
    print(out["val_start_loss"], out["final_val_loss"], out["best_alpha"])
    assert out["line_search"] == "exact"
    assert out["final_val_loss"] < out["val_start_loss"]
    assert float((mc._exposure.detach() - before).abs().min()) > 0
