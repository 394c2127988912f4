"""CPU: the float64 references and measures of tests/dropin_chain_ref.py, before any GPU value is held to them.

  * the split reference (J per Gaussian, D per pixel) reproduces the float64 oracle's end-to-end autograd gradient and
    forward-mode tangent to 1e-12 of the measure's own denominator, on every case the GPU tests run;
  * no blend decision (alpha < 1 / 255 skip, 0.99 clamp, T < 1e-4 stop) lies within relative 1e-5 of its threshold in
    float64, and the float32 oracle takes every one of them, the radii, the sorted lists and n_contrib as float64 does;
  * the float32 oracle's own distance from float64 in each measure, asserted under dropin_chain_ref.FLOORS (the GPU
    bounds are 8 x these, cut to 2e-4);
  * what the old whole-tensor measure cannot see stays true of the scene;
  * every branch class the GPU tests single out has Gaussians that carry a gradient.
"""
import pytest
import torch

import chain_jacobian as cj
import dropin_chain_ref as dr

REVERSE = dr.reverse_cases()
FORWARD = dr.FORWARD_CFG + [dr.FORWARD_SPLIT]


@pytest.mark.parametrize("cfg", REVERSE, ids=dr.cfg_id)
def test_reverse_reference_equals_autograd(cfg):
    """J^T s of the split reference is the float64 oracle's end-to-end gradient to 1e-12 of mag, exactly 0 where mag
    is 0, and the float32 oracle's radii and n_contrib are float64's."""
    cs = dr.case(cfg)
    ref, mag, _ = dr.reverse_reference(cfg)
    g64, radii, nc = dr.oracle_reverse(cfg, dr.cotangent(cfg), torch.float64)
    assert torch.equal(radii, cs.radii) and torch.equal(nc, cs.n_contrib)
    assert bool(((g64 - ref).abs() <= 1e-12 * mag).all()), float(((g64 - ref).abs() / mag.clamp_min(1e-300)).max())
    _, r32, n32 = dr.oracle_reverse(cfg, dr.cotangent(cfg), torch.float32)
    assert torch.equal(r32, cs.radii) and torch.equal(n32, cs.n_contrib)
    # a Gaussian without any gradient is one no pixel blends
    dead = (mag == 0).all(dim=1)
    assert bool((ref[dead] == 0).all())
    assert 0 < int((dead & (cs.radii > 0)).sum()), "no visible Gaussian that nothing blends"


@pytest.mark.parametrize("cfg", FORWARD, ids=dr.cfg_id)
def test_forward_reference_equals_forward_ad(cfg):
    for name, (v, ref, den) in dr.forward_references(cfg).items():
        t64 = dr.oracle_forward(cfg, v, torch.float64).double()
        assert bool(((t64 - ref).abs() <= 1e-12 * den).all()), name


@pytest.mark.parametrize("cfg", REVERSE + FORWARD, ids=dr.cfg_id)
def test_no_decision_near_its_threshold(cfg):
    m64, k64, pl64, rad64 = dr.decision_margins(cfg, torch.float64)
    for what, m in m64.items():
        assert m > 1e-5, (what, m)
    _, k32, pl32, rad32 = dr.decision_margins(cfg, torch.float32)
    assert torch.equal(pl64, pl32) and torch.equal(rad64, rad32)
    assert len(k64) == len(k32)
    for a, b in zip(k64, k32):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_float32_floors(capsys):
    """The float32 oracle against float64 in every measure and case; prints the measured maxima per FLOORS key."""
    worst = {}
    for cfg in REVERSE:
        cs = dr.case(cfg)
        ref, mag, _ = dr.reverse_reference(cfg)
        g32, _, _ = dr.oracle_reverse(cfg, dr.cotangent(cfg), torch.float32)
        for (name, is_thin), e in dr.reverse_measure(cs, g32, ref, mag).items():
            k = dr.reverse_floor_key(name, cfg.aa, is_thin)
            worst[k] = max(worst.get(k, 0.0), e)
    for cfg in FORWARD:
        for name, (v, ref, den) in dr.forward_references(cfg).items():
            t32 = dr.oracle_forward(cfg, v, torch.float32)
            k = dr.forward_floor_key(name)
            worst[k] = max(worst.get(k, 0.0), float(dr.forward_measure(t32, ref, den).max()))
    with capsys.disabled():
        for k in sorted(worst):
            print(f"[floor] {k}: {worst[k]:.3e} (FLOORS {dr.FLOORS.get(k, float('nan')):.1e})")
    assert set(worst) == set(dr.FLOORS)
    for k, e in worst.items():
        assert e <= dr.FLOORS[k], (k, e)
        assert e >= 0.5 * dr.FLOORS[k], (k, e, "the table is stale: a floor is more than twice the measured value")


def test_the_whole_tensor_measure_cannot_see_most_gaussians():
    """On scenes.chain_branch_scene() as it is (view 0, antialiasing off): the Gaussians with a gradient whose whole
    row lies below 1e-4 and 1e-2 of the tensor's largest element -- garbage in the first set, or 1 % errors in the
    second, pass `max |err| / max |ref| < 1e-4`."""
    cfg = dr.Cfg(0, False, 1.0, opaque_thin=False)
    cs = dr.case(cfg)
    ref, mag, _ = dr.reverse_reference(cfg)
    live = (mag > 0).any(dim=1)
    assert int(live.sum()) >= 500
    for name in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        rows = ref[:, cs.slices[name]].abs().max(dim=1).values
        top = rows.max()
        n4, n2 = int((live & (rows < 1e-4 * top)).sum()), int((live & (rows < 1e-2 * top)).sum())
        print(f"{name}: {n4} rows below 1e-4 of max, {n2} below 1e-2, of {int(live.sum())}")
        assert n4 >= 30, (name, n4)
        assert n2 >= 0.5 * int(live.sum()), (name, n2)


@pytest.mark.parametrize("aa,smod", dr.CONFIGS)
def test_thin_gaussians_are_thin_in_both_views(aa, smod):
    """The two-view accumulate test measures a sum over both views with one classification."""
    a, b = dr.thin(dr.Cfg(0, aa, smod, "raw")), dr.thin(dr.Cfg(1, aa, smod, "raw"))
    assert torch.equal(a, b) and 0 < int(a.sum()) < a.numel()


@pytest.mark.parametrize("cfg", [c for c in REVERSE if c.P == 768 and c.degrees == (3, 3)] + FORWARD, ids=dr.cfg_id)
def test_branch_classes_carry_gradient(cfg):
    """At least 8 Gaussians with mag > 0 outside the tan-FoV clamp, under the antialiasing clamp (with antialiasing on)
    and with a clamped colour channel (where the colour comes from SH)."""
    _, mag, _ = dr.reverse_reference(cfg)
    live = (mag > 0).any(dim=1)
    for name, rows in dr.branch_classes(cfg).items():
        if (name == "under_aa" and not cfg.aa) or (name == "sh_clamped" and cfg.form in ("col", "cov_col")):
            continue
        assert int((rows & live).sum()) >= 8, (name, int((rows & live).sum()))
