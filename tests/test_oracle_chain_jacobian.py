"""CPU: the float64 per-Gaussian Jacobian that tests/test_gpu_chain_rules.py holds chain_jvp / chain_vjp to.

tests/chain_jacobian.py differentiates the oracle's preprocess (float64) per Gaussian by forward-mode AD on the
branch-heavy scene of tests/scenes.py (chain_branch_scene).  Here, without a GPU:
  * the scene's conditions (scenes.assert_chain_branch_scene) for antialiasing off / on and scale_modifier 1.0 / 0.7 on
    both views, and the cap on the Gaussians whose visibility decision float32 could flip (<= 1 % of P);
  * J against central differences of F in float64 (h = 1e-6 relative to each leaf's size).  Gaussians outside the
    tan-FoV clamp are left out in the xyz columns: there the reference treats the clamped view coordinate as a
    constant, which is not the derivative of the value (tests/test_oracle_lm_background.py);
  * the float32 floor: the float32 oracle's own forward-mode J v and reverse-mode J^T s held to the float64 J in the two
    measures of tests/chain_jacobian.py.  The GPU tests' tolerances are 8 x these floors (test_gpu_chain_rules.py).
"""
import pytest
import torch

import chain_jacobian as cj
from chain_jacobian import FLOORS, forward_floor_of, reverse_floor_of
from gslm.params import ParamLayout
from scenes import assert_chain_branch_scene, chain_branch_scene

CASES = [(False, 1.0), (True, 1.0), (False, 0.7), (True, 0.7)]


@pytest.mark.parametrize("aa,smod", CASES)
def test_scene_conditions(aa, smod):
    model, cams = chain_branch_scene()
    for b, cam in enumerate(cams):
        s = assert_chain_branch_scene(model, cam, aa, smod)
        vis = s["visible"]
        print(f"aa={aa} smod={smod} view {b}: visible {int(vis.sum())} of {vis.numel()}, outside x "
              f"{int((vis & s['outx']).sum())}, y {int((vis & s['outy']).sum())}, both "
              f"{int((vis & s['outx'] & s['outy']).sum())}, SH-clamped r/g/b "
              f"{[int((vis & s['clamped'][:, c]).sum()) for c in range(3)]}, under the AA clamp "
              f"{int((vis & s['under_aa']).sum())}, nearest to the tan-FoV limit {float(s['near_fov'].min()):.2e}, "
              f"to the AA threshold {float(s['near_aa'].min()):.2e}, boundary set {int(s['boundary'].sum())}")
        # the Gaussians on which the GPU's visible set may differ from the oracle's (test_flags_from_a_real_preprocess)
        assert int(s["boundary"].sum()) <= 0.01 * vis.numel()


def _leaf_steps(lv):
    return [1e-6 * t.abs().max().clamp_min(1e-3) for t in lv]


@pytest.mark.parametrize("aa,smod", [(False, 1.0), (True, 0.7)])
def test_jacobian_equals_central_differences(aa, smod):
    sub, cams, Js, stats = cj.branch_case(3, 3, aa, smod)
    from scenes import to_float64
    for b, cam in enumerate(cams):
        mc, (cc,) = to_float64(sub, [cam])
        st = cj.settings(cc, 3, aa, smod, torch.float64)
        lv = cj.leaves_of(mc)
        J, s = Js[b], stats[b]
        vis = s["visible"]
        outside = s["outx"] | s["outy"]
        worst, col = 0.0, 0
        with torch.no_grad():
            for g, (t, h) in enumerate(zip(lv, _leaf_steps(lv))):
                for k in range(t.shape[1]):
                    tp, tm = t.clone(), t.clone()
                    tp[:, k] += h
                    tm[:, k] -= h
                    fp = cj.record_fn(lv[:g] + [tp] + lv[g + 1:], st)
                    fm = cj.record_fn(lv[:g] + [tm] + lv[g + 1:], st)
                    fd = (fp - fm) / (2 * h)
                    rows = vis & ~outside if g == 0 else vis
                    # a clamped colour channel's kink is not crossed inside the step: |res| > 1e-5 everywhere near 0
                    scale = J[rows][:, :, col].abs().max(dim=0).values.clamp_min(1e-12)
                    worst = max(worst, float(((fd - J[:, :, col])[rows].abs() / scale).max()))
                    col += 1
        assert col == J.shape[2]
        print(f"aa={aa} smod={smod} view {b}: |FD - J| / max |J| per (output, column) = {worst:.3e}")
        assert worst <= 1e-6, worst
        # the quirk is really there: outside the clamp some xyz column differs from the value's derivative
        assert int((vis & outside).sum()) >= 10


def _floors(max_degree, active_degree, aa, smod):
    sub, cams, Js, stats = cj.branch_case(max_degree, active_degree, aa, smod)
    P = sub._xyz.shape[0]
    K = 1 + sub._features_rest.shape[1]
    lay = ParamLayout(P, K)
    fwd = torch.zeros(cj.N_OUT, dtype=torch.float64)
    v = cj.per_gaussian(lay, cj.direction(lay, seed=21))
    ss = cj.cotangents(P, len(cams), seed=22)
    ys, viss = [], []
    for b, cam in enumerate(cams):
        # the float32 oracle takes its own branch decisions; the scene keeps them equal to float64's except for a colour
        # within rounding of its clamp, which is left out
        vis = stats[b]["visible"] & (stats[b]["res"].abs() > 1e-5).all(dim=1)
        T = cj.float32_forward(sub, cam, aa, smod, v)
        fwd = torch.maximum(fwd, cj.forward_measure(T, Js[b], v, vis))
        ys.append(cj.float32_reverse(sub, cam, aa, smod, ss[b], vis).double())
        viss.append(vis)
    ref, mag = cj.reverse_reference(Js, list(ss), viss)
    rev = cj.reverse_measure(sum(ys), ref, mag, K)
    return fwd, rev


@pytest.mark.parametrize("aa,smod", CASES)
@pytest.mark.parametrize("degrees", cj.DEGREES)
def test_float32_floor(degrees, aa, smod):
    """The float32 oracle's distance from the float64 Jacobian, per output (forward) and per group (reverse), is at
    most the floors the GPU tolerances are built from."""
    fwd, rev = _floors(degrees[0], degrees[1], aa, smod)
    print(f"degrees={degrees} aa={aa} smod={smod}: forward " +
          " ".join(f"{n}={float(x):.2e}" for n, x in zip(cj.OUT_NAMES, fwd)) +
          " | reverse " + " ".join(f"{n}={x:.2e}" for n, x in rev.items()))
    for o, name in enumerate(cj.OUT_NAMES):
        assert float(fwd[o]) <= forward_floor_of(name, aa), (name, float(fwd[o]))
    for name, x in rev.items():
        if name != "xyz":
            assert x <= reverse_floor_of(name, aa), (name, x)
    assert all(cj.forward_tol(n, a) <= 2e-4 and cj.reverse_tol(g, a) <= 2e-4 for a in (False, True)
               for n in cj.OUT_NAMES for g in cj.GROUP_NAMES)


@pytest.mark.parametrize("only,mask_xyz", cj.SINGLE_GROUPS)
def test_float32_floor_single_group(only, mask_xyz):
    """The forward floor with v in one group only (the GPU test's single-group cases: SH 3, scale_modifier 0.7, no
    antialiasing -- a geometry group on its own has no opacity column to cover the cancellation inside d h, and the
    float32 oracle itself then reaches 2.3e-4 on the effective opacity)."""
    aa, smod = cj.SINGLE_GROUP_CASE
    sub, cams, Js, stats = cj.branch_case(3, 3, aa, smod)
    lay = ParamLayout(sub._xyz.shape[0], 16)
    fwd = torch.zeros(cj.N_OUT, dtype=torch.float64)
    for seed in (31, 32):
        v = cj.per_gaussian(lay, cj.direction(lay, seed, only))
        for b, cam in enumerate(cams):
            vis = stats[b]["visible"] & (stats[b]["res"].abs() > 1e-5).all(dim=1)
            fwd = torch.maximum(fwd, cj.forward_measure(cj.float32_forward(sub, cam, aa, smod, v), Js[b], v, vis))
    print(f"only={only}: forward " + " ".join(f"{n}={float(x):.2e}" for n, x in zip(cj.OUT_NAMES, fwd)))
    for o, name in enumerate(cj.OUT_NAMES):
        if mask_xyz and o not in range(2, 9):
            continue
        assert float(fwd[o]) <= forward_floor_of(name, aa, only), (name, float(fwd[o]))
