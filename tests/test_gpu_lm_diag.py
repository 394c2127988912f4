"""GPU: diag(J^T W J + D) (gslm_lm_diag_view, LMProblem.diagonal), the Jacobi-preconditioned CG (gslm_pcg_update,
gslm_precond_invert, cgls_jacobi) and lm_step(precond="jacobi").

References (tests/lm_diag_ref.py, pinned on the CPU by tests/test_oracle_lm_diag.py):
  jacobian   the diagonal from the float64 dense Jacobian of the oracle's residual (the yardstick): sh1_33x17 with the
             generic background and the mask, and the 129-deep stack;
  closed     the float64 closed form, which the CPU suite holds to the yardstick at 1e-10 of the group's max: the other
             backgrounds and masks, sh3_40x33, the chain-branch scene and the two-view sum -- where the dense Jacobian
             takes 30 s and more per case (measured: sh3_40x33 31 s, the chain-branch scene 30 s).
Bounds: lm_diag_ref.GPU_TOL, 8 x the float32 oracle's own distance from the float64 diagonal per group, relative to
the group's max.  The depth cases compare with e_j^T (A e_j) of the project's own product, which the oracle tests
hold to 1e-4 of the reference's max: that bound, on the group's max.  The solver's bound is the one the other CGLS
tests hold against the float64 helper (tests/test_gpu_lm.py, tests/test_gpu_lm_exposure.py): |x - x64| / |x64| < 1e-4.
The float32 oracle's own distance from the float64 restatement, measured on the CPU on the test's scene (Jacobi /
plain): 2x1 8.8e-7 / 7.4e-7, 5x5 1.3e-6 / 1.0e-6, 10x1 1.1e-6 / 9.5e-7, 10x10 1.5e-6 / 1.3e-6 -- a margin of 70x and more.

Planted faults (scratch builds, one at a time; the cases that fail are listed in DESIGN.md 4.5e)."""
import copy
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

import lm_diag_ref as R
from margins import record
from scenes import (BG_GENERIC, BG_ZERO, assert_chain_branch_scene, chain_branch_scene, lm_bg_mask, lm_bg_scene,
                    lm_bg_stats, sh_subset, stack_scene, to_float64)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BGS = {"generic": BG_GENERIC, "zero": BG_ZERO}
PCG_TOL = 1e-4


# ---------------------------------------------------------------- scenes and references
def _scene(name, masked, n_views=1, brighten=True):
    model, cams = lm_bg_scene(name, n_views=n_views, brighten=brighten)
    if name == "sh3_40x33":
        model.active_sh_degree = 2  # below the stored degree
    if masked:
        for i, c in enumerate(cams):
            c.alpha_mask = lm_bg_mask(name, seed=i)
    return model, cams


@functools.lru_cache(maxsize=None)
def _ref(name, bgname, masked, kind, n_views=1):
    """The float64 diagonal without D (computed once per case and not modified) and the scene's saturation."""
    model, cams = _scene(name, masked, n_views)
    stats = [lm_bg_stats(model, c, BGS[bgname]) for c in cams]
    m64, c64 = to_float64(model, cams)
    bg = torch.tensor(BGS[bgname], dtype=torch.float64)
    if kind == "jacobian":
        d = R.jacobian_diag(m64, c64, bg, damp=False)
    else:
        d = sum(R.closed_form(m64, c, bg) for c in c64)
    return d, stats


def _problem(model, cams, bgv, projected=False, aa=False, sm=1.0, **kw):
    from gslm.lm import LMProblem
    prob = LMProblem(copy.deepcopy(model).to(DEV), [c.to(DEV) for c in cams], torch.tensor(bgv), device=DEV,
                     sh_projection=projected, **kw)
    for vr in prob.views:
        vr.view.antialiasing, vr.view.scale_modifier = int(aa), float(sm)
    prob.evaluate()
    return prob


def _check(T, tag, got, ref, layout, damp=True):
    """Per-group distance from the float64 diagonal (+ D) against GPU_TOL; xyz and exposure are D alone, exactly."""
    dvec = R.damp_vector(layout) if damp else torch.zeros(layout.numel, dtype=torch.float64)
    want = ref + dvec
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), tag
    for k, v in R.group_errors(got, want, layout).items():
        e = record(T, f"{tag}: {k} (of max)", v, R.GPU_TOL[k])
        assert e <= R.GPU_TOL[k], (tag, k, e)
    for name in ("xyz", "exposure"):
        a, b = layout.offsets[name]
        assert torch.equal(got[a:b], dvec[a:b].float()), (tag, name)


# ---------------------------------------------------------------- 1. the operator against the yardstick
@pytest.mark.parametrize("name,bgname,masked,kind", [
    ("sh1_33x17", "generic", True, "jacobian"), ("sh1_33x17", "generic", False, "closed"),
    ("sh1_33x17", "zero", True, "closed"), ("sh1_33x17", "zero", False, "closed"),
    ("sh3_40x33", "generic", True, "closed"), ("sh3_40x33", "zero", False, "closed")])
def test_diag_view_against_the_yardstick(name, bgname, masked, kind):
    """Partial tiles on both axes, generic and zero background, with and without the alpha mask, brightened so that
    the clamp zeroes weights (asserted on the oracle's render: >= 5 % of the pixel-channels saturate, and no covered
    one lies within 1e-5 of a corner of the clamp, where float32 and float64 weights could differ)."""
    ref, stats = _ref(name, bgname, masked, kind)
    assert stats[0]["saturated"] >= 0.05 and stats[0]["boundary"] == 0, (stats[0]["saturated"], stats[0]["boundary"])
    model, cams = _scene(name, masked)
    prob = _problem(model, cams, BGS[bgname])
    d = prob.diagonal()
    _check("test_diag_view_against_the_yardstick", f"{name} bg={bgname} mask={int(masked)} {kind}", d, ref,
           prob.layout)
    assert prob.views[0].tail_clean  # the row map this call built serves the products after it


def test_diag_chain_branches():
    """Antialiasing on and scale_modifier 0.7 (the do share of scaling and rotation), SH clamps on every channel."""
    model, cams = chain_branch_scene()
    s = assert_chain_branch_scene(model, cams[0], True, 0.7)
    assert all(int((s["visible"] & s["clamped"][:, ch]).sum()) >= 50 for ch in range(3))
    m64, c64 = to_float64(model, cams[:1])
    ref = R.closed_form(m64, c64[0], torch.tensor(BG_GENERIC, dtype=torch.float64), scale_modifier=0.7,
                        antialiasing=True)
    prob = _problem(model, cams[:1], BG_GENERIC, aa=True, sm=0.7)
    _check("test_diag_chain_branches", "chain 64x48 aa sm=0.7", prob.diagonal(), ref, prob.layout)
    # a clamped channel's SH entries are D alone, exactly
    v = prob.layout.views(prob.diagonal(damp=False).cpu())
    cl = s["visible"] & s["clamped"][:, 0]
    assert float(v["features_dc"][cl][:, 0, 0].abs().max()) == 0.0
    assert float(v["features_rest"][cl][:, :, 0].abs().max()) == 0.0


def test_diag_two_views_accumulate():
    ref, _ = _ref("sh1_33x17", "generic", True, "closed", n_views=2)
    one, _ = _ref("sh1_33x17", "generic", True, "jacobian")
    assert max(R.group_errors(one, ref, R.layout_of(_scene("sh1_33x17", True)[0])).values()) > 0.05
    model, cams = _scene("sh1_33x17", True, n_views=2)
    prob = _problem(model, cams, BG_GENERIC)
    _check("test_diag_two_views_accumulate", "sh1_33x17 two views", prob.diagonal(), ref, prob.layout)
    # D is added once: without it the same sum
    _check("test_diag_two_views_accumulate", "sh1_33x17 two views, no D", prob.diagonal(damp=False), ref, prob.layout,
           damp=False)


# ---------------------------------------------------------------- 2. list depths around the batch size
def _unit_products(prob, ids):
    """e_j^T (A e_j) of the problem's own product for every parameter of the Gaussians ids (groups the solve moves)."""
    lay = prob.layout
    out = {}
    y = prob.zeros()
    for name in R.DIAG_GROUPS:
        a, b = lay.offsets[name]
        w = (b - a) // lay.P
        for i in ids:
            for c in range(w):
                e = prob.zeros()
                e[a + i * w + c] = 1.0
                prob.matvec(e, y)
                out[(name, i, c)] = float(y[a + i * w + c])
    return out


@pytest.mark.parametrize("n", [127, 128, 129, 257])
def test_diag_list_depths(n):
    """One 16x16 tile, every list n deep: one entry short of a batch, a full batch, one entry into the second, and
    one into the third -- against e_j^T (A e_j) of the product on the first, a middle and the last two Gaussians."""
    T = "test_diag_list_depths"
    model, cam = stack_scene(n, 16, 16)
    prob = _problem(model, [cam], BG_ZERO)
    assert prob.num_rendered() == [n]
    d = prob.diagonal().cpu()
    lay = prob.layout
    ids = [0, n // 2, n - 2, n - 1]
    want = _unit_products(prob, ids)
    for name in R.DIAG_GROUPS:
        a, b = lay.offsets[name]
        w = (b - a) // lay.P
        keys = [k for k in want if k[0] == name]
        top = max(abs(want[k]) for k in keys)
        err = max(abs(float(d[a + k[1] * w + k[2]]) - want[k]) for k in keys) / top
        assert record(T, f"n={n}: {name} vs e^T A e (of max)", err, 1e-4) <= 1e-4, (n, name, err)
    if n == 129:
        m64, c64 = to_float64(model, [cam])
        ref = R.jacobian_diag(m64, c64, torch.tensor(BG_ZERO, dtype=torch.float64), damp=False)
        _check(T, "stack 129 jacobian", prob.diagonal(), ref, lay)


# ---------------------------------------------------------------- 3. gather blocks
def _truncated(P, seen):
    """The first P Gaussians of sh1_33x17; the first and the last one moved onto the optical axis in front of every
    other Gaussian (seen: the first entries of the centre tiles' lists) or behind the camera (unseen)."""
    model, cams = lm_bg_scene("sh1_33x17")
    m = sh_subset(model, 1, 1)
    m.set_params(m._xyz[:P], m._features_dc[:P], m._features_rest[:P], m._scaling[:P], m._rotation[:P],
                 m._opacity[:P], m._exposure, requires_grad=True)
    c = cams[0].camera_center.float()
    with torch.no_grad():
        for i, t in ((0, 0.6), (P - 1, 0.55)):
            m._xyz[i] = c * t if seen else c * 1.5
            m._scaling[i] = math.log(0.02)
    return m, cams


@pytest.mark.parametrize("seen", [True, False])
@pytest.mark.parametrize("P", [255, 256, 257])
def test_diag_gather_blocks(P, seen):
    """P one short of, equal to and one past a gather block, the first and the last Gaussian seen and unseen.  A
    Gaussian without a head row gets D exactly (0 with damp=False)."""
    model, cams = _truncated(P, seen)
    m64, c64 = to_float64(model, cams)
    ref = R.closed_form(m64, c64[0], torch.tensor(BG_GENERIC, dtype=torch.float64))
    prob = _problem(model, cams, BG_GENERIC)
    d = prob.diagonal()
    _check("test_diag_gather_blocks", f"P={P} seen={int(seen)}", d, ref, prob.layout)
    ids, na = prob.views[0].active_list(P, prob.stream)
    on = torch.zeros(P, dtype=torch.bool)
    on[ids.cpu().long()] = True
    assert bool(on[0]) == seen and bool(on[P - 1]) == seen and 0 < int(on.sum()) < P
    dv = R.damp_vector(prob.layout).float()
    d0 = prob.diagonal(damp=False).cpu()
    for name, t in prob.layout.views(d.cpu()).items():
        if name == "exposure" or not t.numel():
            continue
        a, b = prob.layout.offsets[name]
        rows = t.reshape(P, -1)[~on]
        assert torch.equal(rows, dv[a:b].reshape(P, -1)[~on]), name
        assert float(prob.layout.views(d0)[name].reshape(P, -1)[~on].abs().max()) == 0.0, name


# ---------------------------------------------------------------- 4. layouts
@pytest.mark.parametrize("deg", [0, 1, 3])
def test_diag_full_layout_sh_degrees(deg):
    model, cams = _scene("sh3_40x33", True)
    model = sh_subset(model, deg, deg)
    m64, c64 = to_float64(model, cams)
    ref = R.closed_form(m64, c64[0], torch.tensor(BG_GENERIC, dtype=torch.float64))
    prob = _problem(model, cams, BG_GENERIC, projected=False)
    assert prob.layout.K == (deg + 1) ** 2
    _check("test_diag_full_layout_sh_degrees", f"sh3_40x33 stored/active degree {deg}", prob.diagonal(), ref,
           prob.layout)


def test_diag_projected_layout_and_guards():
    """The single-view projected layout.  Coordinate c's unit vector is Bh (x) e_c (Bh = B_rest / |B_rest|, from
    gslm_sh_rest_project), so its diagonal entry is the quadratic form sum_kk' Bh_k Bh_k' A[(k, c), (k', c)] -- with
    A[(k, c), (k', c)] = B_k B_k' S_col[c] that is (sum_k |Bh_k| sqrt(diag_full[k, c]))^2 = |B_rest|^2 S_col[c], checked
    to float32 rounding (<= 16 terms of a few roundings each, squared: 2e-6 relative) and, on sampled Gaussians,
    against e^T (A e) of the projected product itself (the product's 1e-4 of the max).  (The plain sum
    sum_k Bh_k^2 diag_full[k, c] leaves the off-diagonal terms out: it is |B|^-2 sum_k B_k^4 S_col[c], not the
    diagonal of the projected operator.)  The other groups are bitwise the full layout's.  Overwrite onto a
    NaN-filled destination between guard elements."""
    model, cams = _scene("sh3_40x33", True)
    model.active_sh_degree = 3
    full = _problem(model, cams, BG_GENERIC, projected=False)
    proj = _problem(model, cams, BG_GENERIC, projected=True)
    assert proj.layout.rest_projected and not full.layout.rest_projected
    df = full.diagonal(damp=False)
    n = proj.layout.numel
    buf = torch.full((n + 64,), math.nan, dtype=torch.float32, device=DEV)
    dp = proj.diagonal(out=buf[32:32 + n], damp=False)
    assert bool(torch.isnan(buf[:32]).all()) and bool(torch.isnan(buf[32 + n:]).all())
    assert bool(torch.isfinite(dp).all())
    for name in ("xyz", "features_dc", "scaling", "rotation", "opacity", "exposure"):
        assert torch.equal(full.layout.views(df)[name], proj.layout.views(dp)[name]), name
    ones = proj.zeros()
    a, b = proj.layout.offsets["features_rest"]
    ones[a:b] = 1.0
    Bh = full.layout.views(proj.expand(ones))["features_rest"].double()  # [P, K-1, 3]: Bh_k on every channel
    want = (Bh.abs() * full.layout.views(df)["features_rest"].double().sqrt()).sum(dim=1) ** 2
    got = proj.layout.views(dp)["features_rest"].double().reshape(-1, 3)
    assert float(want.max()) > 0.01
    err = float(((got - want).abs() / want.clamp_min(1e-30))[want > 1e-12].max())
    T = "test_diag_projected_layout_and_guards"
    assert record(T, "projected vs (sum |Bh| sqrt(full))^2 (rel)", err, 2e-6) <= 2e-6
    assert float(got[want == 0].abs().max()) == 0.0
    # the definition itself: e^T (A e) of the projected product on the three largest entries (damping included)
    dd = proj.diagonal()
    y = proj.zeros()
    top = float(dd[a:b].max())
    for j in torch.argsort(dp[a:b], descending=True)[:3].tolist():
        e = proj.zeros()
        e[a + j] = 1.0
        proj.matvec(e, y)
        err = abs(float(y[a + j]) - float(dd[a + j])) / top
        assert record(T, f"projected entry {j} vs e^T A e (of max)", err, 1e-4) <= 1e-4
    # with D: the group's scalar, once
    assert torch.equal(dd[a:b], dp[a:b] + 5e-2)


# ---------------------------------------------------------------- 5. other operator properties
def test_diag_reproducible_and_row_map_built_or_reused():
    """Two runs are bitwise equal; a geometry whose row map this call builds and one that has it from a product give
    the same bits, and the product after a diagonal-built row map is bitwise the product of a fresh problem."""
    model, cams = _scene("sh3_40x33", True)
    a = _problem(model, cams, BG_GENERIC)
    assert not a.views[0].tail_clean
    d1 = a.diagonal()
    assert a.views[0].tail_clean
    d2 = a.diagonal()  # the row map reused
    assert torch.equal(d1, d2)
    b = _problem(model, cams, BG_GENERIC)
    g = b.rhs(b.zeros())  # a product first: its row map
    assert b.views[0].tail_clean
    assert torch.equal(b.diagonal(), d1)
    ya = a.matvec(g, a.zeros())
    yb = b.matvec(g, b.zeros())
    assert torch.equal(ya, yb)
    assert torch.equal(a.rhs(a.zeros()), g)


def test_diag_of_a_view_that_renders_nothing():
    model, cams = _scene("sh1_33x17", False)
    with torch.no_grad():
        model._xyz += 100.0 * cams[0].camera_center.float()  # everything behind the camera
    prob = _problem(model, cams, BG_GENERIC)
    assert prob.num_rendered() == [0]
    d = prob.diagonal().cpu()
    assert torch.equal(d, R.damp_vector(prob.layout).float())
    assert float(prob.diagonal(damp=False).abs().max()) == 0.0


def test_diag_error_returns_leave_the_outputs():
    from gslm import _lib
    from gslm.params import raw_gaussians
    model, cams = _scene("sh1_33x17", False)
    prob = _problem(model, cams, BG_GENERIC)
    lib, vr = _lib.lib, prob.views[0]
    out = torch.full((prob.layout.numel,), 7.0, dtype=torch.float32, device=DEV)
    ys = prob.layout.grads_struct(out)
    g = raw_gaussians(prob.model)
    w = prob.weights[0].data_ptr()

    def call(w=w, mask=1, sbytes=vr.scratch.numel(), ys=ys, flags=0, g=g):
        return lib.gslm_lm_diag_view(ctypes.byref(vr.view), ctypes.byref(g), w, mask, vr.geom.data_ptr(),
                                     vr.binning.data_ptr(), vr.N, vr.image.data_ptr(), vr.scratch.data_ptr(), sbytes,
                                     None if ys is None else ctypes.byref(ys), None, flags, prob.stream)

    INV, CAP = _lib.GSLM_ERR_INVALID, _lib.GSLM_ERR_CAPACITY
    bad = prob.layout.grads_struct(out)
    bad.sh_rest_stride = 6
    assert call(mask=0) == INV and call(w=None) == INV and call(ys=None) == INV and call(flags=64) == INV
    assert call(sbytes=lib.gslm_scratch_bytes(prob.layout.P, vr.N) - 1) == CAP and call(ys=bad) == INV
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == _lib.GSLM_OK
    assert torch.equal(out[prob.layout.offsets["xyz"][1]:prob.layout.offsets["exposure"][0]],
                       prob.diagonal(damp=False)[prob.layout.offsets["xyz"][1]:prob.layout.offsets["exposure"][0]])
    with pytest.raises(ValueError):
        _problem(model, cams, BG_GENERIC, ssim=True).diagonal()


# ---------------------------------------------------------------- 6. the vector kernels
GUARD = -7777.0


def _pad(a):
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(a), np.full(1, GUARD, dtype=a.dtype)])).cuda()


@pytest.mark.parametrize("with_x", [True, False])
@pytest.mark.parametrize("step", [1.5, 0.75])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4 * 1024 * 256 + 259])
def test_pcg_update_exact(n, step, with_x):
    """x += a p ; s -= a q ; z = s (.) minv ; gamma' = <s, z> on integer-valued inputs, a = 3/2 and 3/4, minv in
    {0, 1/2, 1, 2}: every element a multiple of 1/8 below 2^15 and every partial sum a multiple of 1/32 below 2^53 --
    exact in any order, so ==.  The float4 body, the scalar tail, a second sweep past 4 x 1024 x 256 elements, and
    x = NULL."""
    from gslm._lib import check, lib
    rng = np.random.default_rng(700 + n)
    p, q, x, s = (rng.integers(-1000, 1001, size=n).astype(np.float32) for _ in range(4))
    minv = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], dtype=np.float32), size=n)
    z0 = np.full(n, 3.0, dtype=np.float32)
    pd_, qd, xd, sd, md, zd = (_pad(v) for v in (p, q, x, s, minv, z0))
    sc = torch.tensor([3.0, 3.0 / step, 0.0], dtype=torch.float64, device=DEV)
    scratch = torch.zeros(lib.gslm_dot_scratch_bytes(n) // 8, dtype=torch.float64, device=DEV)
    check(lib.gslm_pcg_update(n, sc.data_ptr(), sc.data_ptr() + 8, pd_.data_ptr(), qd.data_ptr(),
                              xd.data_ptr() if with_x else None, sd.data_ptr(), md.data_ptr(), zd.data_ptr(),
                              scratch.data_ptr(), sc.data_ptr() + 16, None), "gslm_pcg_update")
    d = lambda v: v.astype(np.float64)
    s_ref = d(s) - step * d(q)
    z_ref = s_ref * d(minv)
    assert np.array_equal(sd.cpu().numpy()[:n], s_ref.astype(np.float32))
    assert np.array_equal(zd.cpu().numpy()[:n], z_ref.astype(np.float32))
    assert np.array_equal(xd.cpu().numpy()[:n], (d(x) + step * d(p)).astype(np.float32) if with_x else x)
    assert float(sc[2]) == float(np.sum(s_ref * z_ref))
    for t in (pd_, qd, xd, sd, md, zd):
        assert float(t[n]) == GUARD
    assert np.array_equal(pd_.cpu().numpy()[:n], p) and np.array_equal(md.cpu().numpy()[:n], minv)


def test_precond_invert():
    from gslm._lib import check, lib
    m = torch.tensor([4.0, 0.5, 0.0, -2.0, math.nan, 1.0, 3.0, math.inf] * 37 + [8.0], device=DEV)
    out = torch.full((m.numel() + 1,), GUARD, device=DEV)
    check(lib.gslm_precond_invert(m.numel(), m.data_ptr(), out.data_ptr(), None), "gslm_precond_invert")
    want = torch.where(m > 0, 1.0 / m, torch.zeros_like(m))
    assert torch.equal(out[:-1], want) and float(out[-1]) == GUARD


# ---------------------------------------------------------------- 7. cgls_jacobi
def _solver_problem(n_views=1):
    model, cams = _scene("sh1_33x17", False, n_views=n_views, brighten=False)
    prob = _problem(model, cams, BG_GENERIC, projected=False)
    return prob, prob.rhs(prob.zeros())


@functools.lru_cache(maxsize=None)
def _pcg64():
    """The float64 restatement's problem on the oracle: (operator, J^T b, M^-1 from the dense Jacobian)."""
    from oracle.lm_ref import OracleLMProblem
    model, cams = _scene("sh1_33x17", False, brighten=False)
    m64, c64 = to_float64(model, cams)
    bg = torch.tensor(BG_GENERIC, dtype=torch.float64)
    op = OracleLMProblem(m64, c64, bg)
    op.evaluate()
    diag = R.jacobian_diag(m64, c64, bg, damp=True)
    return op, op.rhs(), torch.where(diag > 0, 1.0 / diag, torch.zeros_like(diag))


@pytest.mark.parametrize("sched", [(2, 1), (5, 5)])
def test_cgls_jacobi_with_unit_diagonal_is_cgls_fused(sched):
    """diag = 1: z = s, and every kernel sums as cgls_fused(host_checks=True)'s -- the same x, bitwise."""
    from gslm.lm import cgls_fused, cgls_jacobi
    prob, g = _solver_problem()
    xj, ij = cgls_jacobi(prob, g, max_iter=sched[0], restart_iter=sched[1], diag=torch.ones_like(g))
    xf, info = cgls_fused(prob, g, max_iter=sched[0], restart_iter=sched[1], host_checks=True)
    assert ij["iters"] == info["iters"] == sched[0]
    assert torch.equal(xj, xf)


@pytest.mark.parametrize("sched", [(2, 1), (5, 5), (10, 1)])
def test_cgls_jacobi_against_the_float64_restatement(sched):
    from gslm.lm import cgls_jacobi
    op, g64, minv = _pcg64()
    want = R.pcg_ref(op, g64, minv, *sched)
    prob, g = _solver_problem()
    x, info = cgls_jacobi(prob, g, max_iter=sched[0], restart_iter=sched[1])
    assert info["precond"] == "jacobi" and info["iters"] == sched[0] and len(info["residuals"]) == sched[0]
    err = float((x.cpu().double() - want).norm() / want.norm())
    T = "test_cgls_jacobi_against_the_float64_restatement"
    assert record(T, f"{sched[0]}x{sched[1]}: x vs float64 (rel)", err, PCG_TOL) < PCG_TOL


def _phi(prob, g, x):
    y = prob.matvec(x, prob.zeros())
    return float(0.5 * (x.double() @ y.double()) - g.double() @ x.double())


@pytest.mark.parametrize("k", [2, 5])
def test_cgls_jacobi_model_decrease_and_active_list(k, monkeypatch):
    """phi(x_k) = x^T A x / 2 - g^T x (one extra product, float64 sums) is not above plain CG's; the solve on the
    active list and on the full vectors (GSLM_CG_ACTIVE=0) agree within the solver's float32 bound (their dots group
    differently), and check_every=False gives the iterates of the checked loop."""
    from gslm.lm import cgls_fused, cgls_jacobi
    prob, g = _solver_problem()
    xj, _ = cgls_jacobi(prob, g, max_iter=k, restart_iter=k)
    xp, _ = cgls_fused(prob, g, max_iter=k, restart_iter=k, host_checks=True)
    pj, pp = _phi(prob, g, xj), _phi(prob, g, xp)
    print(f"k={k}: phi jacobi {pj:.4f}, plain {pp:.4f}")
    assert pj <= pp and pj < 0
    xb, _ = cgls_jacobi(prob, g, max_iter=k, restart_iter=k, check_every=False)
    assert torch.equal(xb, xj)
    monkeypatch.setenv("GSLM_CG_ACTIVE", "0")
    xf, _ = cgls_jacobi(prob, g, max_iter=k, restart_iter=k)
    err = float((xf.double() - xj.double()).norm() / xj.double().norm())
    assert record("test_cgls_jacobi_model_decrease_and_active_list", f"k={k}: active vs full (rel)", err,
                  PCG_TOL) < PCG_TOL
    ids, na = prob.views[0].active_list(prob.layout.P, prob.stream)
    assert 0 < na < prob.layout.P  # the list is a proper subset: the two solves differ in their vectors


def test_cgls_jacobi_five_views():
    """The loop problem over five views: the diagonal sums them, and the solve lowers the model below plain CG's."""
    from gslm.lm import cgls_fused, cgls_jacobi
    prob, g = _solver_problem(n_views=5)
    xj, _ = cgls_jacobi(prob, g, max_iter=3, restart_iter=3)
    xp, _ = cgls_fused(prob, g, max_iter=3, restart_iter=3, host_checks=True)
    assert _phi(prob, g, xj) <= _phi(prob, g, xp)


@pytest.mark.parametrize("check_every", [True, False])
def test_cgls_jacobi_nan_raises(check_every):
    from gslm.lm import NonFiniteError, cgls_jacobi
    prob, g = _solver_problem()
    g = g.clone()
    g[prob.layout.offsets["scaling"][0] + 5] = math.nan
    with pytest.raises(NonFiniteError):
        cgls_jacobi(prob, g, max_iter=2, restart_iter=1, check_every=check_every)


# ---------------------------------------------------------------- 8. lm_step
def _step_models():
    model, cams = lm_bg_scene("sh1_33x17", n_views=3, brighten=False)
    return model.to(DEV), [c.to(DEV) for c in cams]


def test_lm_step_jacobi_descends_and_none_is_todays_step():
    from gslm.lm import clear_val_cache, lm_step
    bg = torch.tensor(BG_GENERIC)
    outs = {}
    for tag, kw in (("default", {}), ("none", dict(precond=None)), ("jacobi", dict(precond="jacobi"))):
        model, cams = _step_models()
        clear_val_cache()
        outs[tag] = lm_step(model, cams[:1], cams[1:], bg, max_iter=2, restart_iter=1, device=DEV, val_at_start=True,
                            cache_val=False, **kw)
    assert torch.equal(outs["default"]["step"], outs["none"]["step"])
    assert outs["default"]["final_val_loss"] == outs["none"]["final_val_loss"]
    assert "precond" not in outs["none"] and "precond" not in outs["none"]["cg"]
    j = outs["jacobi"]
    assert j["precond"] == "jacobi" and j["cg"]["precond"] == "jacobi" and j["cg"]["iters"] == 2
    print(f"val loss: start {j['val_start_loss']:.4f}, jacobi {j['final_val_loss']:.4f} (alpha {j['best_alpha']}), "
          f"plain {outs['none']['final_val_loss']:.4f} (alpha {outs['none']['best_alpha']})")
    assert j["final_val_loss"] < j["val_start_loss"]
    assert not torch.equal(j["step"], outs["none"]["step"])


def test_lm_step_jacobi_exclusions():
    from gslm.lm import cgls_jacobi, lm_step
    model, cams = _step_models()
    bg = torch.tensor(BG_GENERIC)
    for kw in (dict(precond="diag"), dict(precond="jacobi", recursion="cgls"),
               dict(precond="jacobi", train_exposure=True), dict(precond="jacobi", multiview="batched"),
               dict(precond="jacobi", mask_xyz=False)):
        with pytest.raises(ValueError):
            lm_step(model, cams[:2], cams[2:], bg, device=DEV, **kw)
    # the SSIM residual (which lm_step does not run) is refused by the solver itself
    prob = _problem(*_scene("sh1_33x17", False), BG_GENERIC, ssim=True)
    with pytest.raises(ValueError):
        cgls_jacobi(prob, prob.rhs(prob.zeros()))
