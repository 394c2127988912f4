"""gslm.lm.BatchedLMProblem (one tangent pass, V tile passes and one gather per product) against LMProblem's per-view
loop on the same model and cameras, at the bounds tests/test_gpu_dist.py uses for the same comparison between the
Gaussian-sharded pipeline and the loop: the loss equal, J^T b (expanded) within 1e-6 of its max, a product within
1e-5 of its max, three CG iterations within 1e-4 in norm.  V = 2 and 5 run in SH-rest coordinates; V = 9 is past
GSLM_MAX_REST_VIEWS and runs the full layout with one 9-view call.  The scenes are those of tests/test_gpu_dist.py."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

from gslm.cameras import orbit_cameras
from gslm.model import GaussianModel, synthetic_gaussians

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 96, 72
CASES = [(2, 6000), (5, 6001), (9, 2000)]


def _scene(nv, P):
    model = synthetic_gaussians(P, 3, seed=0, s0=0.03, n_cams=nv)
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(10 + i)) for i in range(nv)]
    cams = orbit_cameras(nv, W, H, seed=1, images=gts)
    model = model.to("cuda")
    for c in cams:
        c.to("cuda")
    return model, cams


def _direction(layout):
    v = torch.randn(layout.numel, generator=torch.Generator().manual_seed(3))
    for grp in ("xyz", "exposure"):
        a, b = layout.offsets[grp]
        v[a:b] = 0
    return v.cuda()


@functools.lru_cache(maxsize=None)
def _pair(nv, P):
    """(loop, batched, reference results of the loop): built and evaluated once per case, then only read."""
    from gslm.lm import BatchedLMProblem, LMProblem, cgls_fused
    model, cams = _scene(nv, P)
    A = LMProblem(model, cams, torch.zeros(3))
    B = BatchedLMProblem(model, cams, torch.zeros(3))
    la, lb = A.evaluate(), B.evaluate()
    ga = A.rhs(A.zeros())
    v = B.expand(B.project(_direction(A.layout)))  # in the views' span, where every CG iterate lives
    ref = {"loss": float(la), "loss_b": float(lb), "g": ga, "v": v, "y": A.matvec(v, A.zeros())}
    for ce in (False, True):
        ref["x", ce] = cgls_fused(A, ga, max_iter=3, restart_iter=3, check_every=ce)[0]
    torch.cuda.synchronize()
    return A, B, ref


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("nv,P", CASES)
def test_layout_loss_rhs_and_product_match_the_loop(nv, P):
    A, B, ref = _pair(nv, P)
    assert B.rest_views == (nv if nv <= 8 else 0)
    assert B.layout.numel == (A.layout.numel - P * 3 * (15 - nv) if nv <= 8 else A.layout.numel)
    assert B.full_layout.numel == A.layout.numel and B.active_view() is None
    assert ref["loss_b"] == ref["loss"]  # the same forwards and residual epilogues
    g = B.rhs(B.zeros())
    assert B.exposure_is_zero(g)
    eg = _rel(B.expand(g), ref["g"])
    y = B.expand(B.matvec(B.project(ref["v"]), B.zeros()))
    ey = _rel(y, ref["y"])
    print(f"V {nv} P {P}: J^T b {eg:.2e} of max, product {ey:.2e} of max")
    assert eg <= 1e-6
    assert ey <= 1e-5
    # <v, y> comes fused for any V
    dot = torch.zeros(1, dtype=torch.float64, device="cuda")
    vb = B.project(ref["v"])
    yb = B.zeros()
    assert B.matvec_dot(vb, yb, dot.data_ptr()) is True
    scale = float((vb.double() * yb.double()).abs().sum())
    assert abs(float(dot) - float((vb.double() * yb.double()).sum())) <= 1e-12 * scale


@pytest.mark.parametrize("check_every", [False, True])
@pytest.mark.parametrize("nv,P", CASES)
def test_three_cg_iterations_match_the_loop(nv, P, check_every):
    from gslm.lm import cgls_fused
    A, B, ref = _pair(nv, P)
    g = B.rhs(B.zeros())
    x, _ = cgls_fused(B, g, max_iter=3, restart_iter=3, check_every=check_every)
    xr = ref["x", check_every]
    err = float((B.expand(x) - xr).norm() / xr.norm())
    print(f"V {nv} P {P} check_every {check_every}: |x - x_loop| / |x_loop| {err:.2e}")
    assert err <= 1e-4


def test_golden_product_two_views():
    """The reference solver's (J^T J + D) v of tests/golden/solver_golden.npz (the scene recipe of
    tests/test_gpu_lm.py), at that test's 1e-5 of the max.  The golden direction is a generic vector: its SH-rest
    part off the two views' span is seen by no row of J, so (J^T J + D) v = expand(A_c project(v)) + D (v - Q Q^T v)."""
    from gslm.lm import BatchedLMProblem
    d = np.load(os.path.join(HERE, "golden", "solver_golden.npz"))
    P, D, w, h, s0, nv = d["scene"]
    P, D, w, h, nv = int(P), int(D), int(w), int(h), int(nv)
    assert nv == 2
    m = GaussianModel(D)
    t = lambda k: torch.from_numpy(d[f"in_{k}"]).cuda()
    m.set_params(t("xyz"), t("features_dc"), t("features_rest"), t("scaling"), t("rotation"), t("opacity"),
                 t("exposure"))
    m.active_sh_degree = D
    cams = orbit_cameras(nv, w, h, seed=1, images=[torch.from_numpy(d[f"gt{i}"]) for i in range(nv)])
    for c in cams:
        c.to("cuda")
    B = BatchedLMProblem(m, cams, torch.zeros(3))
    assert B.rest_views == 2
    loss = float(B.evaluate())
    assert abs(loss - float(d["loss"])) <= 1e-5 * float(d["loss"])
    g = B.expand(B.rhs(B.zeros()))
    Jtb = torch.from_numpy(d["Jtb"]).cuda()
    assert _rel(g, Jtb) <= 1e-5
    v = torch.from_numpy(d["v"]).cuda()
    y = B.expand(B.matvec(B.project(v), B.zeros()))
    a, b = B.full_layout.offsets["features_rest"]
    off_span = v - B.expand(B.project(v))
    y[a:b] += float(B._damps[2]) * off_span[a:b]
    Av = torch.from_numpy(d["Av"]).cuda()
    err = _rel(y, Av)
    print(f"golden product: {err:.2e} of max")
    assert err <= 1e-5


@pytest.mark.parametrize("nv,P", [(5, 6001), (9, 2000)])
def test_nan_poison_and_reproducibility(nv, P):
    """Nothing of a product depends on what the record table, y or the rest-factor buffer's tail held before."""
    A, B, ref = _pair(nv, P)
    vb = B.project(ref["v"])
    g1 = B.rhs(B.zeros())
    y1 = B.matvec(vb, B.zeros())
    assert torch.equal(g1, B.rhs(B.zeros())) and torch.equal(y1, B.matvec(vb, B.zeros()))

    def poison():
        B._trec.fill_(math.nan)
        if B._rest_R is not None:
            B._rest_R[B._rest_n:].fill_(math.nan)
        return torch.full_like(y1, math.nan)

    g2 = B.rhs(poison())
    y2 = B.matvec(vb, poison())
    assert torch.isfinite(g2).all() and torch.isfinite(y2).all()
    assert torch.equal(g1, g2) and torch.equal(y1, y2)


def test_forward_between_products_rebuilds_the_row_maps():
    """The GSLM_MV_TAIL_CLEAN protocol: a forward clears it, the next product rebuilds the maps, y is the same."""
    from gslm.params import raw_gaussians
    A, B, ref = _pair(5, 6001)
    vb = B.project(ref["v"])
    y1 = B.matvec(vb, B.zeros())
    assert all(vr.tail_clean for vr in B.views)
    g = raw_gaussians(B.model)
    for vr in B.views:
        vr.forward(g, B.stream, want_invdepth=False)
    assert not any(vr.tail_clean for vr in B.views)
    y2 = B.matvec(vb, B.zeros())
    assert all(vr.tail_clean for vr in B.views)
    assert torch.equal(y1, y2)


def test_problem_rejects_what_it_does_not_cover():
    from gslm.lm import BatchedLMProblem
    model, cams = _scene(2, 500)
    with pytest.raises(ValueError):
        BatchedLMProblem(model, cams, torch.zeros(3), mask_xyz=False)
    with pytest.raises(ValueError):
        BatchedLMProblem(model, cams, torch.zeros(3), ssim=True)
    with pytest.raises(ValueError):
        BatchedLMProblem(model, [], torch.zeros(3))


def test_full_layout_switch(monkeypatch):
    """GSLM_SHARD_REST=full keeps the reference's layout (as in the sharded operator): same product."""
    from gslm.lm import BatchedLMProblem
    A, B, ref = _pair(2, 6000)
    monkeypatch.setenv("GSLM_SHARD_REST", "full")
    F = BatchedLMProblem(A.model, A.cams, torch.zeros(3))
    assert F.rest_views == 0 and F.layout.numel == A.layout.numel
    F.evaluate()
    assert _rel(F.rhs(F.zeros()), ref["g"]) <= 1e-6
    assert _rel(F.matvec(ref["v"], F.zeros()), ref["y"]) <= 1e-5


def _close(a, b, tol):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-12)


def test_lm_step_batched_matches_loop():
    """3 training and 4 validation views, at the bounds of test_gpu_shproj.py::test_projected_lm_step_matches_full."""
    from gslm.lm import clear_val_cache, lm_step
    m, cams = _scene(7, 4000)
    m2 = copy.deepcopy(m)
    a = lm_step(m, cams[:3], cams[3:], torch.zeros(3), max_iter=3, restart_iter=3, multiview="loop")
    b = lm_step(m2, cams[:3], cams[3:], torch.zeros(3), max_iter=3, restart_iter=3, multiview="batched")
    clear_val_cache()
    print(f"lm_step: alpha {a['best_alpha']} / {b['best_alpha']}, final {a['final_val_loss']!r} / "
          f"{b['final_val_loss']!r}")
    assert a["best_alpha"] == b["best_alpha"]
    assert abs(a["final_val_loss"] - b["final_val_loss"]) <= 1e-4 * a["final_val_loss"]
    assert b["step"].numel() == a["step"].numel()  # the step comes back in the reference's layout
    for t1, t2 in zip(m.params(), m2.params()):
        assert _close(t2.detach(), t1.detach(), 1e-4)


def test_lm_step_option_handling():
    from gslm.lm import clear_val_cache, lm_step
    m, cams = _scene(3, 2000)
    with pytest.raises(ValueError):
        lm_step(copy.deepcopy(m), cams[:2], cams[2:], torch.zeros(3), mask_xyz=False, multiview="batched")
    with pytest.raises(ValueError):
        lm_step(copy.deepcopy(m), cams[:2], cams[2:], torch.zeros(3), recursion="cgls", multiview="batched")
    with pytest.raises(ValueError):
        lm_step(copy.deepcopy(m), cams[:2], cams[2:], torch.zeros(3), multiview="fused")
    # one training view: the existing path, bit for bit
    m1, m2 = copy.deepcopy(m), copy.deepcopy(m)
    a = lm_step(m1, cams[:1], cams[1:], torch.zeros(3), max_iter=3, restart_iter=3)
    b = lm_step(m2, cams[:1], cams[1:], torch.zeros(3), max_iter=3, restart_iter=3, multiview="batched")
    clear_val_cache()
    assert a["best_alpha"] == b["best_alpha"] and a["final_val_loss"] == b["final_val_loss"]
    assert torch.equal(a["step"], b["step"])
    for t1, t2 in zip(m1.params(), m2.params()):
        assert torch.equal(t1, t2)
