"""Conditioning guard of tests/test_gpu_ssim_operator.py (CPU): on every case that file runs, the float32 oracle agrees
with the float64 oracle, under the same tile-local metric, to a quarter of the bar the GPU test applies.  A case whose
reference moves by more than that under float32 rounding would pin the GPU bar on the reference's conditioning and not
on the kernel; such a case is rebuilt (seed, construction), never dropped, and the bar is never widened.

Also the float64 identities the GPU tests lean on: N_lambda = (1 - lambda) N_0 + lambda N_1 (so a failure at
lambda = 0 or 1 names one half of the operator), and the x == gt fixed point (S = 1, zero seed, zero operator).
"""
import numpy as np
import pytest
import torch

import ssim_cases as sc
from oracle import ssim_ref

GUARD = 0.25


def _guard(case, lam, ref=None):
    r1, r2, loss, seed, njv = sc.oracle(*case, lam, torch.float64) if ref is None else ref
    q1, q2, qloss, qseed, qnjv = sc.oracle(*case, lam, torch.float32)
    got = {"r1": sc.tile_rel(q1, r1), "r2": sc.tile_rel(q2, r2), "loss": abs(qloss - loss) / loss,
           "seed": sc.tile_rel(qseed, seed), "Njv": sc.tile_rel(qnjv, njv)}
    print({k: f"{v:.2e}" for k, v in got.items()})
    assert got["r1"] < GUARD * sc.BAR_RES
    assert got["r2"] < GUARD * sc.BAR_RES
    assert got["loss"] < GUARD * sc.BAR_RES
    assert got["seed"] < GUARD * sc.BAR_OP
    assert got["Njv"] < GUARD * sc.BAR_OP


@pytest.mark.parametrize("H,W,mask_kind,lam", sc.PURE_SSIM + sc.PURE_L1 + sc.MIXED)
def test_float32_oracle_within_a_quarter_of_the_bar(H, W, mask_kind, lam):
    _guard(sc.gapped(H, W, mask_kind), lam, sc.gapped_oracle(H, W, mask_kind, lam))


@pytest.mark.parametrize("mask_kind,lam", sc.GATE)
def test_float32_oracle_on_the_clamp_gate_case(mask_kind, lam):
    _guard(sc.clamp_gate_case(mask_kind), lam)


@pytest.mark.parametrize("H,W,mask_kind", [(H, W, mk) for (H, W) in sc.SHAPES for mk in sc.MASKS])
def test_gapped_case_properties(H, W, mask_kind):
    R, gt, m, jv = sc.gapped(H, W, mask_kind)
    assert all(t.dtype == torch.float32 and not t.is_cuda for t in (R, gt, m, jv))
    assert R.shape == gt.shape == jv.shape == (3, H, W) and m.shape == (1, H, W)
    assert sc.assert_gap(R, gt, m) >= 0.02 - 1e-6
    assert gt.min() >= 0.1 and gt.max() <= 0.9
    levels = {"none": {1.0}, "binary": {0.0, 1.0}, "levels": {0.0, 0.5, 1.0}}[mask_kind]
    assert set(m.unique().tolist()) <= levels
    if H * W >= 512:
        assert set(m.unique().tolist()) == levels
    x = m * R.clamp(0, 1)
    assert (x[(m == 0).expand_as(x)] == 0).all()


def test_clamp_gate_case_reaches_every_tile_corner():
    R, gt, m, jv = sc.clamp_gate_case("none")
    H, W = sc.GATE_HW
    special = (R == 0) | (R == 1) | ((R < 0) & (R > -1e-30)) | ((R > 1) & (R < 1 + 2e-7))
    for y0 in range(0, H, sc.TILE_H):
        for x0 in range(0, W, sc.TILE_W):
            y1, x1 = min(y0 + sc.TILE_H, H) - 1, min(x0 + sc.TILE_W, W) - 1
            for (y, x) in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
                assert special[:, y, x].all()
    edge = R[special]
    for v in (0.0, 1.0):
        assert (edge == v).any()
    assert (torch.signbit(edge) & (edge == 0)).any()          # -0.0
    assert ((edge < 0) & (edge > -1e-30)).any() and ((edge > 1) & (edge < 1 + 2e-7)).any()
    # autograd's clamp passes the gradient at both bounds inclusive, as the kernel's gate plane does
    r = torch.tensor([0.0, 1.0, -0.0, edge.min().item(), edge.max().item()], requires_grad=True)
    r.clamp(0, 1).sum().backward()
    assert r.grad.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("H,W,mask_kind", [(17, 33, "levels"), (33, 65, "none"), (10, 11, "binary")])
def test_operator_is_affine_in_lambda(H, W, mask_kind):
    """N_lambda = (1 - lambda) N_0 + lambda N_1, and the same for the seed (float64)."""
    o0, o1, o2 = (sc.gapped_oracle(H, W, mask_kind, lam) for lam in (0.0, 1.0, 0.2))
    for k in (3, 4):
        mix = 0.8 * o0[k] + 0.2 * o1[k]
        assert np.abs(mix - o2[k]).max() <= 1e-12 * np.abs(o2[k]).max()
    assert not o0[1].any() and not o1[0].any()  # r2 == 0 at lambda 0, r1 == 0 at lambda 1, exactly


@pytest.mark.parametrize("H,W,mask_kind", sc.XEQ)
def test_x_equal_gt_is_a_fixed_point(H, W, mask_kind):
    """With x == gt the float64 oracle gives S = 1, r = (a, b) 1e-3, a zero seed and a zero operator."""
    R, gt, m, jv = sc.xeq_case(H, W, mask_kind)
    assert torch.equal(m * R.clamp(0, 1), gt)
    lam = 0.2
    a, b = ssim_ref.image_weights(H, W, lam)
    r1, r2, loss, seed, njv = sc.oracle(R, gt, m, jv, lam, torch.float64)
    assert np.abs(r1 - a * 1e-3).max() <= 1e-12 * a and np.abs(r2 - b * 1e-3).max() <= 1e-9 * b
    assert abs(loss - 1e-6 * (a * a + b * b) * 3 * H * W) <= 1e-9 * loss
    assert np.abs(seed).max() <= 1e-9 * a * a and np.abs(njv).max() <= 1e-9 * a * a


@pytest.mark.parametrize("lead", sc.MEAN_LEAD)
@pytest.mark.parametrize("H,W", sc.MEAN_SHAPES)
def test_float32_mean_oracle_within_a_quarter_of_the_bar(lead, H, W):
    x, y = sc.mean_case(lead, H, W)
    s64, g64 = sc.mean_oracle(x, y, torch.float64)
    s32, g32 = sc.mean_oracle(x, y, torch.float32)
    print(f"value {abs(s32 - s64):.2e} grad {np.abs(g32 - g64).max() / np.abs(g64).max():.2e}")
    assert abs(s32 - s64) < GUARD * 1e-6
    assert np.abs(g32 - g64).max() < GUARD * 1e-5 * np.abs(g64).max()


def test_tile_rel_is_tile_local():
    """An error confined to one small-valued tile is measured against that tile, floored at 1e-3 of the global max."""
    b = np.full((3, 33, 65), 1e-2)
    b[0, 0, 0] = 10.0
    a = b.copy()
    a[2, 32, 64] += 1e-3                       # the 1x1 corner tile of channel 2
    assert np.isclose(sc.tile_rel(a, b), 1e-3 / 1e-2)
    assert np.isclose(np.abs(a - b).max() / np.abs(b).max(), 1e-4)
    b[2, 32, 64] = 0.0
    a = b.copy()
    a[2, 32, 64] = 1e-3
    assert np.isclose(sc.tile_rel(a, b), 1e-3 / (1e-3 * 10.0))
    assert sc.tile_rel(b, b) == 0.0 and sc.tile_rel(np.zeros((3, 2, 2)), np.zeros((3, 2, 2))) == 0.0
    assert sc.tile_rel(np.ones((3, 2, 2)), np.zeros((3, 2, 2))) == float("inf")
