"""GPU: Marquardt-scaled damping D = lambda max(diag(J^T W J), floor) -- gslm_marquardt_scale, the per-element damping
vector of the LM gather (GSLM_MV_DAMP_VEC), LMProblem(damping="marquardt"), set_damping_vector, and
lm_step(damping="marquardt").

References (tests/lm_marquardt_ref.py, pinned on the CPU by tests/test_oracle_lm_marquardt.py):
  kernels     exact: integer-valued inputs against numpy float32 / float64 by ==, and the damp7 product bitwise for a d
              that is constant per group (the arithmetic per element is the same multiply and add);
  operator    A v = A0 v + lambda max(diag, floor) (.) v in float64 on the oracle (A0: zero damping; diag: the float64
              closed form, which the CPU suite holds to the dense Jacobian at 1e-10), per group relative to the
              group's max, bound 8 x the float32 oracle's own distance capped at 1e-3 (PRODUCT_GPU_TOL);
  solves      lm_diag_ref.pcg_ref in float64, |x - x64| / |x64| < 1e-4 on the schedules whose float32 CPU restatement
              stays within 1/8 of that (GPU_SOLVE_CASES; Jacobi without a floor does not qualify: DESIGN.md 4.5f).
Residual-scale invariance (mask 1 against mask 0.5 with gt x 0.5) is asserted bitwise on the device: every
intermediate scales by a power of two."""
import copy
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import lm_diag_ref as R
import lm_marquardt_ref as M
from margins import record
from scenes import BG_GENERIC, lm_bg_mask, lm_bg_scene, sh_subset, to_float64

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -7777.0
BG64 = torch.tensor(BG_GENERIC, dtype=torch.float64)
# group constants that are exact in float32 and differ from group to group
DMAP = {"xyz": 3.0, "features_dc": 0.25, "features_rest": 0.5, "scaling": 2.0, "rotation": 0.125, "opacity": 1.5,
        "exposure": 4.0}


# ---------------------------------------------------------------- 1. gslm_marquardt_scale
def _pad(a):
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(a), np.full(1, GUARD, dtype=a.dtype)])).cuda()


def _groups(n):
    """Seven groups over [0, n) with a zero-width third one (SH 0's rest group), and their multipliers."""
    b = [0, n // 7, n // 3, n // 3, n // 2, (3 * n) // 4, n - n // 9, n]
    lam = [1.0, 2.0, 64.0, 3.0, 0.5, 4.0, 0.25]
    return (ctypes.c_int64 * 8)(*b), (ctypes.c_double * 7)(*lam), b, lam


@pytest.mark.parametrize("floor", [0.0, 5.0])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4096 * 256 + 259])
def test_marquardt_scale_exact(n, floor):
    """d = lambda[group] max(diag, floor) on integer-valued inputs against numpy float32 by ==: one element, around a
    block, and one size past a full sweep of the 4096 x 256 grid; a zero-width group; NaN in gives NaN out; the
    output starts NaN-filled between guard elements."""
    from gslm._lib import check, lib
    rng = np.random.default_rng(40 + n)
    diag = rng.integers(0, 21, size=n).astype(np.float32)
    nan_at = [k for k in (0, n // 2, n - 1) if 0 <= k < n and n >= 255]
    for k in nan_at:
        diag[k] = np.nan
    bounds, lam, b, l = _groups(n)
    dd = _pad(diag)
    out = torch.full((n + 2,), math.nan, dtype=torch.float32, device=DEV)
    out[0] = out[n + 1] = GUARD
    check(lib.gslm_marquardt_scale(n, dd.data_ptr(), bounds, lam, 7, floor, out.data_ptr() + 4, None),
          "gslm_marquardt_scale")
    w = np.zeros(n, dtype=np.float32)
    for k in range(7):
        w[b[k]:b[k + 1]] = l[k]
    with np.errstate(invalid="ignore"):
        want = w * np.where(diag < np.float32(floor), np.float32(floor), diag)
    got = out.cpu().numpy()
    assert got[0] == GUARD and got[n + 1] == GUARD and float(dd[n]) == GUARD
    assert np.array_equal(got[1:n + 1], want, equal_nan=True)
    assert all(np.isnan(got[1 + k]) for k in nan_at) and int(np.isnan(got[1:n + 1]).sum()) == len(set(nan_at))
    assert np.array_equal(dd.cpu().numpy()[:n], diag, equal_nan=True)  # the input is left alone
    if n:  # in place: d may be diag
        check(lib.gslm_marquardt_scale(n, dd.data_ptr(), bounds, lam, 7, floor, dd.data_ptr(), None),
              "gslm_marquardt_scale")
        assert np.array_equal(dd.cpu().numpy()[:n], want, equal_nan=True) and float(dd[n]) == GUARD


def test_marquardt_scale_error_returns_leave_the_output():
    from gslm import _lib
    lib = _lib.lib
    n = 300
    bounds, lam, _, _ = _groups(n)
    diag = torch.ones(n, device=DEV)
    out = torch.full((n,), 7.0, device=DEV)
    INV = _lib.GSLM_ERR_INVALID

    def call(n=n, diag=diag.data_ptr(), b=bounds, l=lam, ng=7, floor=1.0, d=out.data_ptr()):
        return lib.gslm_marquardt_scale(n, diag, b, l, ng, floor, d, None)

    assert call(n=-1) == INV and call(diag=None) == INV and call(d=None) == INV
    assert call(floor=-1.0) == INV and call(floor=math.nan) == INV and call(floor=math.inf) == INV
    assert call(ng=9) == INV and call(b=None) == INV and call(l=None) == INV
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == _lib.GSLM_OK
    assert call(ng=0, b=None, l=None) == _lib.GSLM_OK  # no groups: lambda = 1
    assert bool((out == 1.0).all())


# ---------------------------------------------------------------- 2. the damping vector in the gather
def _problem(model, cams, bgv=BG_GENERIC, projected=False, **kw):
    from gslm.lm import LMProblem
    prob = LMProblem(copy.deepcopy(model).to(DEV), [copy.deepcopy(c).to(DEV) for c in cams], torch.tensor(bgv),
                     device=DEV, sh_projection=projected, **kw)
    prob.evaluate()
    return prob


def _const_vec(layout, dmap=DMAP):
    d = torch.zeros(layout.numel, dtype=torch.float32)
    for name, (a, b) in layout.offsets.items():
        d[a:b] = dmap[name]
    return d.to(DEV)


def _ints(n, lo, hi, seed):
    return torch.randint(lo, hi, (n,), generator=torch.Generator().manual_seed(seed)).float().to(DEV)


def _product(prob, v, damp=True):
    """(y, <v, y> or None) of one product on NaN-filled y between guard elements; the fused dot when one view."""
    n = prob.layout.numel
    buf = torch.full((n + 64,), math.nan, dtype=torch.float32, device=DEV)
    y = buf[32:32 + n]
    sc = torch.full((1,), math.nan, dtype=torch.float64, device=DEV)
    if damp:
        fused = prob.matvec_dot(v, y, sc.data_ptr())
    else:
        prob.local_normal_matvec(v, y, damp=False)
        fused = False
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:32]).all()) and bool(torch.isnan(buf[32 + n:]).all())
    assert bool(torch.isfinite(y).all())
    return y, (float(sc[0]) if fused else None)


def _forms(prob, form):
    """The problem itself, or its active view (a row map first: rhs)."""
    if form == "full":
        return prob, (lambda t: t)
    prob.rhs(prob.zeros())
    act = prob.active_view()
    assert act is not None
    return act, act.pack


def _check_damp_vec(model, cams, projected, form, tag):
    """The two equivalences of one (scene, layout, form).  Returns the rows of v and y."""
    fixed = _problem(model, cams, projected=projected, damp=DMAP)
    vec = _problem(model, cams, projected=projected, damp=DMAP)
    n = fixed.layout.numel
    assert vec.damping_vector() is None
    vec.set_damping_vector(_const_vec(vec.layout))
    v = torch.randn(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    fa, fpack = _forms(fixed, form)
    va, vpack = _forms(vec, form)
    if form == "active":
        assert va._dvec.numel() == va.layout.numel <= n  # the listed rows of d, packed with the list
    # constant per group, equal to damp7: y and the fused dot are the damp7 product's, bitwise
    yf, df = _product(fa, fpack(v))
    yv, dv = _product(va, vpack(v))
    assert df is not None and dv is not None and math.isfinite(df)
    assert torch.equal(yv, yf), (tag, float((yv - yf).abs().max()))
    assert dv == df, (tag, dv, df)
    # small integers: y == float32(float64(y_nodamp) + d v), and the dot includes the term
    full_n = vec.layout.numel
    d_int, v_int = _ints(full_n, 0, 8, 11), _ints(full_n, -4, 5, 12)
    vec.set_damping_vector(d_int)
    va, vpack = _forms(vec, form)
    pv, pd = vpack(v_int), vpack(d_int)
    y0, _ = _product(va, pv, damp=False)
    y1, d1 = _product(va, pv)
    want = (y0.double() + pd.double() * pv.double()).float()
    assert torch.equal(y1, want), (tag, float((y1 - want).abs().max()))
    e0 = va.layout.offsets["exposure"][0]
    dot = float((pv[:e0].double() * y1[:e0].double()).sum())
    assert abs(d1 - dot) <= 1e-12 * abs(dot), (tag, d1, dot)
    assert float((pd * pv).abs().max()) > 0 and not torch.equal(y1, y0)
    return va.layout.P


def _truncated(P, seen):
    """The first P Gaussians of sh1_33x17; the first and the last one moved onto the optical axis in front of every
    other Gaussian (seen) or behind the camera (unseen)."""
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


@pytest.mark.parametrize("form", ["full", "active"])
@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("seen", [True, False])
@pytest.mark.parametrize("P", [255, 256, 257])
def test_damp_vec_gather_blocks(P, seen, projected, form):
    """P one short of, equal to and one past a gather block, the end Gaussians seen and unseen; the projected and the
    full SH-rest layout; the full-P and the active-list kernel."""
    model, cams = _truncated(P, seen)
    rows = _check_damp_vec(model, cams, projected, form, f"P={P} seen={seen} proj={projected} {form}")
    assert rows == P if form == "full" else 0 < rows < P


@pytest.mark.parametrize("form", ["full", "active"])
@pytest.mark.parametrize("deg", [0, 1, 3])
def test_damp_vec_sh_degrees(deg, form):
    """SH 0 (no rest group: its pointer is NULL and its group zero-wide), 1 and 3, masked and brightened; both
    layouts where there is a rest group."""
    model, cams = lm_bg_scene("sh3_40x33")
    cams[0].alpha_mask = lm_bg_mask("sh3_40x33", seed=0)
    model = sh_subset(model, deg, deg)
    for projected in ((False, True) if deg else (False,)):
        _check_damp_vec(model, cams, projected, form, f"deg={deg} proj={projected} {form}")


def _scene_with_list(target):
    """The first 400 Gaussians of sh1_33x17 with as many listed ones moved behind the camera as it takes for the
    view's active list to have exactly `target` entries (a Gaussian leaving a tile's list can bring another one into
    the head of it, so the count is taken again until it fits)."""
    model, cams = lm_bg_scene("sh1_33x17")
    P = 400
    m = sh_subset(model, 1, 1)
    m.set_params(m._xyz[:P], m._features_dc[:P], m._features_rest[:P], m._scaling[:P], m._rotation[:P],
                 m._opacity[:P], m._exposure, requires_grad=True)
    c = cams[0].camera_center.float()
    for _ in range(12):
        prob = _problem(m, cams)
        prob.rhs(prob.zeros())
        ids, na = prob.views[0].active_list(P, prob.stream)
        if na == target:
            return m, cams
        assert na > target, (na, target)
        with torch.no_grad():
            m._xyz[ids[target:].cpu().long()] = c * 1.5
    raise AssertionError(f"no scene with a list of {target} entries")


@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("na", [255, 256, 257])
def test_damp_vec_list_sizes(na, projected):
    """Active lists one short of, equal to and one past a block of the list-order kernel."""
    model, cams = _scene_with_list(na)
    assert _check_damp_vec(model, cams, projected, "active", f"list={na} proj={projected}") == na


def test_damp_vec_second_view_adds_no_damping():
    """Two views: the first view's gather overwrites with d (.) v, the second accumulates without it -- bitwise the
    damp7 problem's y for a d constant per group, and y - y_nodamp is d (.) v once."""
    model, cams = lm_bg_scene("sh1_33x17", n_views=2)
    fixed = _problem(model, cams, damp=DMAP)
    vec = _problem(model, cams, damp=DMAP)
    d = _const_vec(vec.layout)
    vec.set_damping_vector(d)
    v = torch.randn(vec.layout.numel, generator=torch.Generator().manual_seed(4)).to(DEV)
    yf, _ = _product(fixed, v)
    yv, dot = _product(vec, v)
    assert dot is None  # (two views: the caller takes the dot)
    assert torch.equal(yv, yf)
    y0, _ = _product(vec, v, damp=False)
    lo, hi = vec.layout.offsets["features_dc"][0], vec.layout.offsets["exposure"][0]
    diff = (yv.double() - y0.double())[lo:hi]
    want = (d.double() * v.double())[lo:hi]
    scale = float(yv[lo:hi].abs().max())
    assert float((diff - want).abs().max()) <= 4e-7 * scale  # (a few float32 roundings of y)
    assert float(want.abs().max()) > 1e-2 * scale  # (twice d v would be seen)


def test_damp_vec_error_returns_leave_the_outputs():
    """Every combination the flag refuses returns GSLM_ERR_INVALID before a launch: y and the dot slot keep their
    fill.  gslm_matvec_view_ex and gslm_matvec_view_active."""
    from gslm import _lib
    from gslm.lm import MV_DAMP_VEC, MV_EXPOSURE, MV_LEAN, STAGE_ALL, STAGE_OVERWRITE
    from gslm.params import raw_gaussians
    model, cams = lm_bg_scene("sh1_33x17")
    prob = _problem(model, cams)
    g0 = prob.rhs(prob.zeros())  # (the row map: the active form needs GSLM_MV_TAIL_CLEAN)
    lib, vr, lay = _lib.lib, prob.views[0], prob.layout
    n = lay.numel
    v = g0.clone()
    y = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    d = torch.ones(n, dtype=torch.float32, device=DEV)
    sc = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
    g = raw_gaussians(prob.model)
    vs, ys = lay.grads_struct(v), lay.grads_struct(y)
    ids, na = vr.active_list(lay.P, prob.stream)
    INV = _lib.GSLM_ERR_INVALID
    aux = torch.zeros(3 * vr.H * vr.W + 16 * lay.P, dtype=torch.float32, device=DEV)

    def call(edit=None, mask=1, stages=STAGE_ALL | STAGE_OVERWRITE, dgroup=None, no_vec=False, active=False,
             flags=0):
        opts = prob._opts(vr, stages)
        prob._dot_opts(opts, sc.data_ptr())
        ext = _lib.extend_opts(opts, _lib.GslmMatvecOptsDamp, MV_DAMP_VEC | flags)
        ds = lay.grads_struct(d)
        if dgroup:
            setattr(ds, dgroup, None)
        ext.damp_vec = None if no_vec else ctypes.addressof(ds)
        if edit:
            edit(ext.base)
        ws = (vr.geom.data_ptr(), vr.binning.data_ptr(), vr.N, vr.image.data_ptr(), vr.scratch.data_ptr(),
              vr.scratch.numel())
        w = prob.weights[0].data_ptr()
        if active:
            return lib.gslm_matvec_view_active(ctypes.byref(vr.view), ctypes.byref(g), ctypes.byref(vs), w, mask, *ws,
                                               ctypes.byref(ys), ctypes.byref(ext), ids.data_ptr(),
                                               vr.active_rows.data_ptr(), na, prob.stream)
        return lib.gslm_matvec_view_ex(ctypes.byref(vr.view), ctypes.byref(g), ctypes.byref(vs), w, mask, *ws,
                                       ctypes.byref(ys), ctypes.byref(ext), prob.stream)

    def set_(name, value):
        return lambda o: setattr(o, name, value)

    for active in (False, True):
        assert call(set_("damp7", prob._damps), active=active) == INV
        assert b"GSLM_MV_DAMP_VEC" in lib.gslm_last_error()
        assert call(no_vec=True, active=active) == INV
        for grp in ("means3D", "sh_dc", "sh_rest", "scales", "rotations", "opacities"):
            assert call(dgroup=grp, active=active) == INV, grp
        assert call(set_("pixel_seed", aux.data_ptr()), stages=2 | 4 | STAGE_OVERWRITE, active=active) == INV
        assert call(set_("jv_out", aux.data_ptr()), stages=1 | 2, active=active) == INV
        assert call(set_("screen_out", aux.data_ptr()), stages=1 | 2 | 16, active=active) == INV
        assert call(set_("trec_in", aux.data_ptr()), stages=2 | 4 | STAGE_OVERWRITE, active=active) == INV
        assert call(set_("rest_basis", aux.data_ptr()), active=active) == INV
        assert call(flags=MV_LEAN, active=active) == INV
        assert call(flags=MV_EXPOSURE, active=active) == INV
        assert call(mask=0, active=active) == INV
    bad = lay.grads_struct(d)
    bad.sh_rest_stride = 3  # (the full layout's stride is 9)
    opts = _lib.extend_opts(prob._opts(vr, STAGE_ALL | STAGE_OVERWRITE), _lib.GslmMatvecOptsDamp, MV_DAMP_VEC)
    opts.damp_vec = ctypes.addressof(bad)
    assert lib.gslm_matvec_view_ex(ctypes.byref(vr.view), ctypes.byref(g), ctypes.byref(vs), prob.weights[0].data_ptr(),
                                   1, vr.geom.data_ptr(), vr.binning.data_ptr(), vr.N, vr.image.data_ptr(),
                                   vr.scratch.data_ptr(), vr.scratch.numel(), ctypes.byref(ys), ctypes.byref(opts),
                                   prob.stream) == INV
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and float(sc[0]) == 7.0 and torch.equal(v, g0)
    assert call() == _lib.GSLM_OK
    torch.cuda.synchronize()
    assert bool((y[lay.offsets["features_dc"][0]:lay.offsets["exposure"][0]] != 7.0).any()) and float(sc[0]) != 7.0


# ---------------------------------------------------------------- 3. the operator against the yardstick
def _masked(name, n_views):
    model, cams = lm_bg_scene(name, n_views=n_views)
    if name == "sh3_40x33":
        model.active_sh_degree = 2  # below the stored degree
    for i, c in enumerate(cams):
        c.alpha_mask = lm_bg_mask(name, seed=i)
    return model, cams


@functools.lru_cache(maxsize=None)
def _operator_case(name, n_views, projected):
    """(v, A0 v in float64, the float64 diagonal, the oracle's layout) of one case: computed once, not modified.
    v is the GPU problem's own J^T b, so both sides apply their operator to the same vector."""
    model, cams = _masked(name, n_views)
    prob = _problem(model, cams, projected=projected, damping="marquardt", damp=M.lam_map())
    v = prob.rhs(prob.zeros()).cpu().double()
    m64, c64 = to_float64(model, cams)
    diag = sum(R.closed_form(m64, c, BG64) for c in c64)
    op = M.MarquardtOracle(m64, c64, BG64, d=torch.zeros(1, dtype=torch.float64), projected=projected)
    assert op.layout.numel == v.numel() and op.layout.rest_projected == prob.layout.rest_projected
    y0 = op.matvec(v, torch.zeros_like(v))
    if op.projected:
        diag = M.projected_diag(diag, op.full, op.layout)
    return v, y0, diag, op.layout


@pytest.mark.parametrize("floor", [0.0, M.FLOOR])
@pytest.mark.parametrize("name,n_views,projected", [
    ("sh1_33x17", 1, False), ("sh1_33x17", 1, True), ("sh1_33x17", 2, False),
    ("sh3_40x33", 1, False), ("sh3_40x33", 1, True), ("sh3_40x33", 2, False)])
def test_marquardt_operator_against_the_yardstick(name, n_views, projected, floor):
    """LMProblem(damping="marquardt").matvec on masked, brightened scenes; full and projected layout, one and two
    views, floor zero and nonzero.  Also: the damping vector is lambda max(diagonal(damp=False), floor) bitwise,
    lambda floor on xyz and the exposure tail, and diagonal(damp=True) adds it."""
    T = "test_marquardt_operator_against_the_yardstick"
    v, y0, diag, lay = _operator_case(name, n_views, projected)
    model, cams = _masked(name, n_views)
    prob = _problem(model, cams, projected=projected, damping="marquardt", damp=M.lam_map(), marquardt_floor=floor)
    assert prob.layout.rest_projected == (projected and True)
    d = prob.damping_vector()
    d0 = prob.diagonal(damp=False)
    want_d = torch.where(d0 < floor, torch.full_like(d0, floor), d0) * torch.tensor(M.LAMBDA, device=DEV)
    assert torch.equal(d, want_d)
    lam_floor = float(torch.tensor(M.LAMBDA, dtype=torch.float32) * torch.tensor(floor, dtype=torch.float32))
    for grp in ("xyz", "exposure"):
        a, b = prob.layout.offsets[grp]
        assert bool((d[a:b] == lam_floor).all())
    assert torch.equal(prob.diagonal(), d0 + d)
    y = prob.matvec(v.float().to(DEV), prob.zeros()).cpu()
    want = y0 + M.damping_vector(diag, lay, M.lam_map(), floor) * v
    assert bool(torch.isfinite(y).all())
    tag = f"{name} views={n_views} proj={int(projected)} floor={floor:g}"
    for k, e in M.group_errors(y, want, lay).items():
        record(T, f"{tag}: {k} (of max)", e, M.PRODUCT_GPU_TOL[k])
        assert e <= M.PRODUCT_GPU_TOL[k], (tag, k, e)
    # the damping is part of the number compared: without it the distance is far outside the bound
    assert max(M.group_errors(y0, want, lay).values()) > 10 * max(M.PRODUCT_GPU_TOL.values())


def test_marquardt_vector_is_rebuilt_after_evaluate():
    """Built lazily once per evaluate(): the same tensor until the next evaluate(), a new one after it; an
    active view carries the listed rows."""
    model, cams = lm_bg_scene("sh1_33x17", brighten=False)
    prob = _problem(model, cams, projected="auto", damping="marquardt", damp=M.lam_map(), marquardt_floor=M.FLOOR)
    assert prob.layout.rest_projected
    d1 = prob.damping_vector()
    assert prob.damping_vector() is d1
    with torch.no_grad():
        prob.model._features_dc += 0.05
    prob.evaluate()
    d2 = prob.damping_vector()
    assert d2 is not d1 and not torch.equal(d1, d2)
    act = prob.active_view()
    assert act is not None and torch.equal(act._dvec, act.pack(d2))


# ---------------------------------------------------------------- 4. residual-scale invariance on the device
def _halved(cams):
    out = []
    for c in cams:
        c = copy.deepcopy(c)
        c.alpha_mask = torch.full_like(c.alpha_mask, 0.5)
        c.original_image = c.original_image * 0.5
        out.append(c)
    return out


def _plain_scene(n_views=1):
    return lm_bg_scene("sh1_33x17", n_views=n_views, brighten=False)


@pytest.mark.parametrize("solver", ["fused", "jacobi"])
@pytest.mark.parametrize("floor", [0.0, M.FLOOR])
def test_residual_scale_invariance_on_the_device(solver, floor):
    """Mask 1 against mask 0.5 with gt x 0.5, the floor against floor / 4: W, J^T b and the diagonal scale by 2^-2,
    every dot by a power of two, alpha by 2^2 -- x is bitwise equal (10 iterations, the projected layout)."""
    from gslm.lm import cgls_fused, cgls_jacobi
    model, cams = _plain_scene()
    xs = []
    for cc, f in ((cams, floor), (_halved(cams), floor / 4)):
        prob = _problem(model, cc, projected="auto", damping="marquardt", damp=M.lam_map(), marquardt_floor=f)
        g = prob.rhs(prob.zeros())
        if solver == "fused":
            x, _ = cgls_fused(prob, g, max_iter=10, restart_iter=10, check_every=False)
        else:
            x, _ = cgls_jacobi(prob, g, max_iter=10, restart_iter=10)
        xs.append((x, g, prob.damping_vector()))
    (x1, g1, d1), (x2, g2, d2) = xs
    assert torch.equal(g2, 0.25 * g1) and torch.equal(d2, 0.25 * d1)
    assert float(x1.norm()) > 1.0 and bool(torch.isfinite(x1).all())
    rel = float((x1.double() - x2.double()).norm() / x1.double().norm())
    assert torch.equal(x1, x2), (solver, floor, rel)


def test_fixed_damping_moves_with_the_residual_scale():
    from gslm.lm import cgls_fused
    model, cams = _plain_scene()
    xs = []
    for cc in (cams, _halved(cams)):
        prob = _problem(model, cc, projected="auto")
        x, _ = cgls_fused(prob, prob.rhs(prob.zeros()), max_iter=10, restart_iter=10, check_every=False)
        xs.append(x.double())
    rel = float((xs[0] - xs[1]).norm() / xs[0].norm())
    print(f"fixed damping, residual halved: |x - x'| / |x| = {rel:.3f}")
    assert rel > 0.1


# ---------------------------------------------------------------- 5. solves
@pytest.mark.parametrize("check_every", [False, True])
@pytest.mark.parametrize("projected", [False, True])
def test_group_constant_vector_solves_as_fixed_damping(projected, check_every, monkeypatch):
    """set_damping_vector(the group constants): cgls_fused's x is bitwise the fixed-damping general loop's
    (GSLM_CG_LEAN=0); with a vector the lean loop is not taken whatever the switch says."""
    from gslm.lm import DEFAULT_DAMP, cgls_fused
    model, cams = _plain_scene()
    vec = _problem(model, cams, projected=projected)
    vec.set_damping_vector(_const_vec(vec.layout, DEFAULT_DAMP))
    xv, iv = cgls_fused(vec, vec.rhs(vec.zeros()), max_iter=5, restart_iter=5, check_every=check_every)
    assert getattr(vec, "_lean_state", None) is None
    monkeypatch.setenv("GSLM_CG_LEAN", "0")
    fixed = _problem(model, cams, projected=projected)
    xf, info = cgls_fused(fixed, fixed.rhs(fixed.zeros()), max_iter=5, restart_iter=5, check_every=check_every)
    assert iv["iters"] == info["iters"] == 5
    assert torch.equal(xv, xf)


@functools.lru_cache(maxsize=None)
def _solve64(case):
    """The float64 restatement of one solve (computed once, not modified)."""
    precond, max_iter, restart, floor = case
    model, cams = _plain_scene()
    m64, c64 = to_float64(model, cams)
    diag = R.closed_form(m64, c64[0], BG64)
    op = M.MarquardtOracle(m64, c64, BG64, diag=diag, floor=floor)
    op.evaluate()
    g = op.rhs()
    dg = diag + op.d
    minv = torch.where(dg > 0, 1.0 / dg, torch.zeros_like(dg)) if precond == "jacobi" else torch.ones_like(dg)
    return R.pcg_ref(op, g, minv, max_iter, restart)


@pytest.mark.parametrize("case", M.GPU_SOLVE_CASES)
def test_marquardt_solves_against_the_float64_restatement(case):
    from gslm.lm import cgls_fused, cgls_jacobi
    precond, max_iter, restart, floor = case
    assert M.SOLVE_F32_FLOOR[case] <= M.SOLVE_TOL / 8
    want = _solve64(case)
    model, cams = _plain_scene()
    prob = _problem(model, cams, damping="marquardt", damp=M.lam_map(), marquardt_floor=floor)
    g = prob.rhs(prob.zeros())
    solver = cgls_jacobi if precond == "jacobi" else cgls_fused
    x, info = solver(prob, g, max_iter=max_iter, restart_iter=restart)
    assert info["iters"] == max_iter
    err = float((x.cpu().double() - want).norm() / want.norm())
    T = "test_marquardt_solves_against_the_float64_restatement"
    assert record(T, f"{precond} {max_iter}x{restart} floor={floor:g}: x vs float64 (rel)", err, M.SOLVE_TOL) < M.SOLVE_TOL


@pytest.mark.parametrize("solver", ["fused", "jacobi"])
def test_active_list_on_and_off(solver, monkeypatch):
    """The solve on the active list (d packed with it) against GSLM_CG_ACTIVE=0: within 1e-6 in norm (their dots group
    the same products differently); whether they are bitwise equal is recorded."""
    from gslm.lm import cgls_fused, cgls_jacobi
    model, cams = _plain_scene()
    run = cgls_jacobi if solver == "jacobi" else cgls_fused
    xs = []
    for env in ("1", "0"):
        monkeypatch.setenv("GSLM_CG_ACTIVE", env)
        prob = _problem(model, cams, projected="auto", damping="marquardt", damp=M.lam_map(), marquardt_floor=M.FLOOR)
        x, _ = run(prob, prob.rhs(prob.zeros()), max_iter=5, restart_iter=5)
        xs.append(x.double())
    ids, na = prob.views[0].active_list(prob.layout.P, prob.stream)
    assert 0 < na < prob.layout.P
    err = float((xs[0] - xs[1]).norm() / xs[1].norm())
    record("test_active_list_on_and_off", f"{solver}: active vs full (rel); bitwise={int(torch.equal(xs[0], xs[1]))}", err,
           1e-6)
    assert err <= 1e-6


def test_poisoned_damping_vector_raises():
    """A NaN in D reaches the solve's dots: NonFiniteError from the stopping tests, as for a NaN in J^T b."""
    from gslm.lm import NonFiniteError, cgls_fused
    model, cams = _plain_scene()
    prob = _problem(model, cams)
    g = prob.rhs(prob.zeros())
    ids, na = prob.views[0].active_list(prob.layout.P, prob.stream)
    d = _const_vec(prob.layout, {k: 0.05 for k in DMAP})
    d[prob.layout.offsets["scaling"][0] + 3 * int(ids[0]) + 1] = math.nan
    prob.set_damping_vector(d)
    with pytest.raises(NonFiniteError):
        cgls_fused(prob, g, max_iter=2, restart_iter=1)


# ---------------------------------------------------------------- 6. lm_step and option handling
def _step_models():
    model, cams = lm_bg_scene("sh1_33x17", n_views=4, brighten=False)
    return model.to(DEV), [c.to(DEV) for c in cams]


@pytest.mark.parametrize("precond", [None, "jacobi"])
@pytest.mark.parametrize("n_train", [1, 2])
def test_lm_step_marquardt_descends(n_train, precond):
    from gslm.lm import clear_val_cache, lm_step
    model, cams = _step_models()
    clear_val_cache()
    out = lm_step(model, cams[:n_train], cams[n_train:], torch.tensor(BG_GENERIC), max_iter=2, restart_iter=1,
                  device=DEV, val_at_start=True, cache_val=False, damping="marquardt", damp=M.lam_map(),
                  marquardt_floor=M.FLOOR, precond=precond)
    print(f"{n_train} view(s), precond={precond}: validation loss {out['val_start_loss']:.3f} -> "
          f"{out['final_val_loss']:.3f} at alpha {out['best_alpha']}")
    assert out["damping"] == "marquardt"
    assert (precond is None) == ("precond" not in out)
    assert bool(torch.isfinite(out["step"]).all()) and float(out["step"].abs().max()) > 0
    for k in ("start_loss", "final_val_loss", "val_start_loss", "best_alpha"):
        assert math.isfinite(out[k]), k
    assert all(math.isfinite(a) and math.isfinite(v) for a, v in out["trace"])
    for t in (model._features_dc, model._features_rest, model._scaling, model._rotation, model._opacity):
        assert bool(torch.isfinite(t).all())
    assert out["final_val_loss"] < out["val_start_loss"]


def test_lm_step_defaults_are_todays_step():
    """damping="fixed", marquardt_floor=0.0 and no new argument at all: the same step and the same model, bitwise."""
    from gslm.lm import clear_val_cache, lm_step
    outs, models = [], []
    for kw in ({}, dict(damping="fixed", marquardt_floor=0.0)):
        model, cams = _step_models()
        clear_val_cache()
        outs.append(lm_step(model, cams[:1], cams[1:], torch.tensor(BG_GENERIC), max_iter=2, restart_iter=1, device=DEV,
                            cache_val=False, **kw))
        models.append(model)
    assert torch.equal(outs[0]["step"], outs[1]["step"])
    assert outs[0]["final_val_loss"] == outs[1]["final_val_loss"] and outs[0]["trace"] == outs[1]["trace"]
    assert "damping" not in outs[0] and "damping" not in outs[1]
    for a, b in zip(models[0].params(), models[1].params()):
        assert torch.equal(a, b)


def test_option_handling_on_the_device():
    from gslm.lm import BatchedLMProblem, LMProblem, cgls_residual, lm_step
    model, cams = _step_models()
    bg = torch.tensor(BG_GENERIC)
    lam = M.lam_map()
    for kw in (dict(damping="levenberg"), dict(damping="marquardt"),
               dict(damping="marquardt", damp=lam, recursion="cgls"),
               dict(damping="marquardt", damp=lam, train_exposure=True),
               dict(damping="marquardt", damp=lam, multiview="batched"),
               dict(damping="marquardt", damp=lam, mask_xyz=False),
               dict(damping="marquardt", damp=lam, backend=(None, None, None)),
               dict(marquardt_floor=1e-3)):
        with pytest.raises(ValueError):
            lm_step(model, cams[:2], cams[2:], bg, device=DEV, **kw)
    for cls, kw in ((LMProblem, dict(damping="marquardt")), (LMProblem, dict(damping="marquardt", damp=lam, ssim=True)),
                    (LMProblem, dict(damping="marquardt", damp=lam, train_exposure=True)),
                    (LMProblem, dict(damping="marquardt", damp=lam, mask_xyz=False)),
                    (BatchedLMProblem, dict(damping="marquardt", damp=lam))):
        with pytest.raises(ValueError):
            cls(model, cams[:2], bg, device=DEV, **kw)
    prob = LMProblem(model, cams[:1], bg, device=DEV)
    prob.evaluate()
    n = prob.layout.numel
    for bad in (torch.ones(n - 1, device=DEV), torch.ones(n, dtype=torch.float64, device=DEV), torch.ones(n),
                -torch.ones(n, device=DEV)):
        with pytest.raises(ValueError):
            prob.set_damping_vector(bad)
    for kw in (dict(ssim=True), dict(train_exposure=True), dict(mask_xyz=False)):
        with pytest.raises(ValueError):
            LMProblem(model, cams[:1], bg, device=DEV, **kw).set_damping_vector(torch.ones(n, device=DEV))
    prob.set_damping_vector(torch.ones(n, device=DEV))
    with pytest.raises(ValueError):
        cgls_residual(prob)
    prob.set_damping_vector(None)
    assert prob.damping_vector() is None
