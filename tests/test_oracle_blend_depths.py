"""CPU: the scenes and the float64 reference of the tile-blend depth tests (tests/test_gpu_blend_depths.py).

The GPU tests compare every tile pass with the oracle run in double on scenes whose list depths sit on and next to the
passes' round sizes (tests/blend_reference.py, scenes.stack_scene).  Asserted here, on oracle data only:
  * the float64 run sorts, bins and stops exactly as the float32 oracle (point list, ranges, n_contrib equal);
  * every tile's n_eff (largest n_contrib of its pixels) is the depth the case names; a blob case's stopped quadrant
    ends at the pinned depth, below the other three, over >= 8 distinct n_contrib values; a wall case leaves a tail of
    n - n_eff >= 64 entries nobody blends, and its plain stacks reach every pixel (n_contrib == n everywhere);
  * decision margins: over every (pixel, entry) pair the float64 blend evaluates, |255 alpha - 1|, |test_T / 1e-4 - 1|
    and |power| are >= 1e-4, and so is |alpha_raw / 0.99 - 1| (the clamp, whose two sides differentiate differently;
    the walls' alpha is on the clamped side at every pixel).  |power| <= ln 255 where it matters and a float32 record error of 2^-24 moves alpha by
    under 1e-5 relative, so float32 on either side takes each decision as float64 does, with 10x to spare.  A
    condition on the scenes (seeds, opacities and widths are chosen to meet it), not a tolerance;
  * no raw pixel-channel within 1e-5 of the residual clamp's corners;
  * the float64 J v of one case against central differences and the adjoint identity (the bounds of
    tests/test_oracle_lm_background.py);
  * the float32 oracle's own error against float64 (e32) stays below blend_reference.E32 for every quantity the GPU
    tests bound, in their measures -- the GPU bounds are derived from E32, never from a GPU number."""
import pytest
import torch

import blend_reference as br
from blend_reference import CASES

FD_CASE = "stack96_33x17"


@pytest.mark.parametrize("name", list(CASES))
def test_scene_conditions(name):
    c = CASES[name]
    r64, r32 = br.dropin64(name), br.dropin(name, torch.float32)
    assert torch.equal(r64.point_list, r32.point_list)
    assert torch.equal(r64.ranges, r32.ranges)
    assert torch.equal(r64.n_contrib, r32.n_contrib)
    assert torch.equal(r64.radii, r32.radii)
    depths = br.tile_depths(r64)
    assert len(depths) == ((c.W + 15) // 16) * ((c.H + 15) // 16)
    for n_eff, length in depths:
        assert n_eff == c.n_eff, (n_eff, c.n_eff)
        assert length == c.n
    if c.blobs is None:
        assert int(r64.n_contrib.min()) == c.n_eff  # every pixel of every tile
    else:
        q = c.blobs[0]
        qd = br.quadrant_depths(r64)
        assert qd[q] == c.stopped and all(qd[s] == c.n for s in range(4) if s != q), qd
        nc = r64.n_contrib[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8]
        assert len(set(nc.reshape(-1).tolist())) >= 8
    if c.wall is not None:
        assert c.n - c.n_eff >= 64
        assert float(r64.final_T.max()) <= 0.011  # the first wall entry's 1 - 0.99, at every pixel
        assert br.wall_clamped(r64, c)  # 0.999 G >= 0.99: the walls' alpha is the clamp's at every pixel
    m = br.decision_margins(r64)
    print(f"{name}: margins alpha {m['alpha']:.2e} T {m['T']:.2e} power {m['power']:.2e} clamp {m['clamp']:.2e}, "
          f"final_T >= {float(r64.final_T.min()):.2e}")
    assert m["alpha"] >= 1e-4 and m["T"] >= 1e-4 and m["power"] >= 1e-4 and m["clamp"] >= 1e-4, m
    if c.blobs is None and c.wall is None:
        assert float(r64.final_T.min()) >= 2.0e-3  # 20x above the 1e-4 stop
    L = br.lm64(name)
    assert br.clamp_distance(L.raw) >= 1e-5


def _e32(name):
    """The float32 oracle's error against float64 in every measure the GPU tests bound, on one case."""
    a, b = br.dropin64(name), br.dropin(name, torch.float32)
    e = {"image": max(br.linf(b.color, a.color), br.linf(b.invdepth, a.invdepth)),
         "final_T": br.linf(b.final_T, a.final_T)}
    e["grad"] = max(br.of_max(b.grads[d][k], a.grads[d][k]) for d in (False, True) for k in a.grads[d])
    e["colour_tangent"] = max(br.of_max(b.tangents[x][0], a.tangents[x][0]) for x in (False, True))
    e["depth_tangent"] = max(br.of_max(b.tangents[x][1], a.tangents[x][1]) for x in (False, True))
    e["loss"] = e["lm_vector"] = 0.0
    for mask_xyz in (True, False):
        a, b = br.lm64(name, mask_xyz), br.lm(name, torch.float32, mask_xyz)
        e["loss"] = max(e["loss"], abs(b.loss - a.loss) / a.loss)
        e["lm_vector"] = max(e["lm_vector"], br.of_max(b.g, a.g), br.of_max(b.y, a.y), br.of_max(b.jv, a.jv))
    if name == br.SSIM_CASE:
        a, b = br.lm64(name, True, True), br.lm(name, torch.float32, True, True)
        e["loss"] = max(e["loss"], abs(b.loss - a.loss) / a.loss)
        e["ssim_vector"] = max(br.of_max(b.g, a.g), br.of_max(b.y, a.y))
    return e


@pytest.mark.parametrize("name", list(CASES))
def test_float32_oracle_error(name):
    """e32 of every quantity the GPU tests bound, per case, against the recorded maximum E32 (x 1.5: float32 sums
    differ by a rounding or two between hosts' vector units; a larger e32 than recorded would only mean a bound tighter
    than the rule allows)."""
    e = _e32(name)
    print(f"{name}: e32 " + ", ".join(f"{k} {x:.2e}" for k, x in e.items()))
    for k, x in e.items():
        assert x <= 1.5 * br.E32[k], (k, x, br.E32[k])


def test_recorded_e32_is_reached():
    """The recorded maxima are not overstated: each is reached, within the same factor, at its case."""
    for k, name in br.E32_AT.items():
        x = _e32(name)[k]
        assert br.E32[k] / 1.5 <= x <= 1.5 * br.E32[k], (k, name, x, br.E32[k])


def test_bounds_follow_the_rule():
    """max(8 E32, n_eff 2^-22) at the case's own depth, capped by the suite's bars; every measure has its own E32."""
    assert set(br.E32) == set(br.BAR) == set(br.E32_AT)
    for name, c in CASES.items():
        for q in br.BAR:
            assert br.bound(q, name) == min(br.BAR[q], max(8 * br.E32[q], c.n_eff * 2.0 ** -22))
    assert br.bound("colour_tangent", "stack300_16x16") == 300 * 2.0 ** -22 < br.BAR["colour_tangent"]
    assert br.bound("image", "stack1_16x16") == 8 * br.E32["image"]


@pytest.mark.parametrize("mask_xyz", [True, False])
def test_jv_equals_central_difference_of_the_residual(mask_xyz):
    from test_oracle_lm_background import _at
    L = br.lm64(FD_CASE, mask_xyz)
    op = L.op
    v = op._mask(L.v.double().clone())
    jv = L.jv
    scale = float(jv.abs().max())
    assert scale > 0
    errs = []
    for h in (1e-4, 1e-5):
        (rp, rawp), (rm, rawm) = _at(op, v, h), _at(op, v, -h)
        fd = (rp - rm) / (2 * h)
        lo, hi = torch.minimum(rawp, rawm), torch.maximum(rawp, rawm)
        assert not bool((((lo < 0) & (hi > 0)) | ((lo < 1) & (hi > 1))).any())
        errs.append(float((fd - jv).abs().max()) / scale)
    print(f"mask_xyz={mask_xyz}: |FD - J v| / max |J v| = {errs[0]:.3e} (h = 1e-4), {errs[1]:.3e} (h = 1e-5)")
    assert errs[1] < errs[0], errs
    assert errs[1] <= 1e-6, errs


@pytest.mark.parametrize("name", [FD_CASE, "wall96_of300_33x17", "blobs_q1_stop128_of192"])
@pytest.mark.parametrize("mask_xyz", [True, False])
def test_adjoint_identity(name, mask_xyz):
    L = br.lm64(name, mask_xyz)
    op = L.op
    v = op._mask(L.v.double().clone())
    u = torch.randn(L.jv.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    leaves = op._leaves()
    r = op._residuals()[0]
    grads = torch.autograd.grad((r * u).sum(), leaves, allow_unused=True)
    jtu = torch.cat([(g if g is not None else torch.zeros_like(t)).reshape(-1) for g, t in zip(grads, leaves)])
    lhs, rhs = float((L.jv * u).sum()), float((v * jtu).sum())
    print(f"{name} mask_xyz={mask_xyz}: <J v, u> = {lhs!r}, <v, J^T u> = {rhs!r}, rel {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs) > 0
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)
