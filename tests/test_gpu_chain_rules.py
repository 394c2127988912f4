"""GPU: chain_jvp and chain_vjp (csrc/gslm_chain.hpp), one Gaussian at a time, against a float64 Jacobian.

The two C-ABI entry points that expose the per-Gaussian derivative chains, gslm_tangent_views (chain_jvp) and
gslm_gather_screen (chain_vjp), are driven directly on the branch-heavy scene of tests/scenes.py
(chain_branch_scene: Gaussians outside the tan-FoV clamp, under the antialiasing clamp, SH colour clamps on every
channel, |q_raw| from 0.2 to 6, every Gaussian anisotropic, 14 % culled) and held to J v and sum_b J_b^T s_b + D v of the float64 per-Gaussian
Jacobian of tests/chain_jacobian.py (the oracle's preprocess under forward-mode AD).  No preprocess runs on the GPU:
the visibility / SH-clamp words are inputs, built from the oracle (bit 31 visible, bits 0-2 clamped).

Measures and bounds (tests/chain_jacobian.py, FLOORS / forward_tol / reverse_tol): per (Gaussian, output)
|T - J v| <= tol_o sum_k |J[o, k]| |v[k]|, per (Gaussian, group) max_k |y - ref| <= tol_g max_k (|J|^T |s| + |d v|),
with tol = 8 x the float32 oracle's own distance from the float64 J in the same measure
(tests/test_oracle_chain_jacobian.py::test_float32_floor), cut to 2e-4:
  forward, any output 6e-5; the effective opacity with antialiasing 2e-4 (8 x 4.5e-5 cut); the conic with v in one
  geometry group alone 2e-4 (8 x 6.5e-5 cut);
  reverse dc / rest / opacity 9.6e-6; scaling 2.4e-5, with antialiasing 9.6e-5; rotation 8.8e-5.
A wrong branch (a sign, a missing mask, a dropped factor) shows as O(1) in these measures.

Also here: the flags word of a real preprocess (gslm_view_flags after LMProblem.evaluate) against the oracle's, and
LMProblem.rhs / matvec on the branch scene against oracle/lm_ref.py at the 1e-4 bar of tests/test_gpu_lm_background.py.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import chain_jacobian as cj
from margins import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELD = {"xyz": "means3D", "features_dc": "sh_dc", "features_rest": "sh_rest", "scaling": "scales",
         "rotation": "rotations", "opacity": "opacities"}
DAMP7 = (0.7, 0.05, 0.3, 0.02, 0.11, 0.5, 3.0)  # xyz, dc, rest, scaling, rotation, opacity, exposure


def _prefix(model, P):
    """The first P Gaussians of the model, on the GPU."""
    import copy
    m = copy.deepcopy(model)
    m.set_params(m._xyz[:P], m._features_dc[:P], m._features_rest[:P], m._scaling[:P], m._rotation[:P],
                 m._opacity[:P], m._exposure, requires_grad=False)
    return m.to(DEV)


def _view_array(cams, D, smod, aa):
    from gslm import _lib
    arr = (_lib.GslmView * len(cams))()
    for k, c in enumerate(cams):
        arr[k] = _lib.view_from_camera(c, torch.zeros(3), D, smod, aa)
    return arr


def _flag_words(stats, P, n_views, stride):
    """int32 [n_views, stride] on the GPU: the oracle's words of the first P Gaussians; the guard entries past P are
    marked visible with every clamp bit (a kernel that read them would write a guard record)."""
    w = np.full((n_views, stride), 0x80000007, dtype=np.uint32)
    for b in range(n_views):
        w[b, :P] = cj.flags_word(stats[b]["visible"], stats[b]["clamped"])[:P].numpy().astype(np.uint32)
    return torch.from_numpy(w.view(np.int32)).to(DEV)


def _case(degrees, aa, smod, P):
    from gslm.params import ParamLayout, raw_gaussians
    sub, cams, Js, stats = cj.branch_case(degrees[0], degrees[1], aa, smod)
    m = _prefix(sub, P)
    K = 1 + m._features_rest.shape[1]
    return m, raw_gaussians(m), ParamLayout(P, K), K, cams, [J[:P] for J in Js], stats


def _tag(degrees, aa, smod, P):
    return f"sh{degrees[0]}/{degrees[1]} aa={int(aa)} smod={smod} P={P}"


# ------------------------------------------------------------------ forward: gslm_tangent_views against J v
def _tangent_views(degrees, aa, smod, mask_xyz, P, only=None, seed=31):
    """Both views in one call with flags_stride and trec_stride above P, the records prefilled with NaN.  Returns
    (T [n_views, P, 10] float64 with NaN where a record holds no such entry, v rows [P, C], Js, visible masks)."""
    from gslm import _lib
    m, g, lay, K, cams, Js, stats = _case(degrees, aa, smod, P)
    n = len(cams)
    v = cj.direction(lay, seed, only)
    vd = v.to(DEV)
    vs = lay.grads_struct(vd)
    if only is not None:
        for name, field in FIELD.items():
            if name != only:
                setattr(vs, field, None)  # NULL: a zero tangent
    R = 8 if mask_xyz else 12
    fstride, tstride = P + 5, P + 3
    flags = _flag_words(stats, P, n, fstride)
    trec = torch.full((n, tstride, R), float("nan"), device=DEV)
    _lib.check(_lib.lib.gslm_tangent_views(_view_array(cams, degrees[1], smod, aa), n, ctypes.byref(g),
                                          ctypes.byref(vs), int(mask_xyz), flags.data_ptr(), fstride,
                                          trec.data_ptr(), tstride, None, _lib.stream_handle(DEV)),
               "gslm_tangent_views")
    torch.cuda.synchronize()
    rec = trec.cpu()
    viss = [s["visible"][:P] for s in stats]
    T = torch.full((n, P, cj.N_OUT), float("nan"), dtype=torch.float64)
    for b in range(n):
        vis = viss[b]
        assert torch.isnan(rec[b, :P][~vis]).all(), "the record of an invisible Gaussian was written"
        assert torch.isnan(rec[b, P:]).all(), "a guard row past the view's block was written"
        assert torch.isfinite(rec[b, :P][vis]).all()
        if mask_xyz:
            T[b, :, 2:9] = rec[b, :P, :7].double()
            assert bool((rec[b, :P, 7][vis] == 0).all())
        else:
            T[b] = rec[b, :P, :10].double()
            assert bool((rec[b, :P, 10:][vis] == 0).all())
    vrows = cj.per_gaussian(lay, v)
    if mask_xyz:
        vrows[:, cj.group_slices(K)["xyz"]] = 0  # v.xyz is ignored
    return T, vrows, Js, viss


def _check_forward(T_name, degrees, aa, smod, mask_xyz, P, only=None):
    T, vrows, Js, viss = _tangent_views(degrees, aa, smod, mask_xyz, P, only)
    outs = range(2, 9) if mask_xyz else range(cj.N_OUT)
    tag = f"{_tag(degrees, aa, smod, P)} xyz={int(not mask_xyz)}" + (f" only={only}" if only else "")
    worst = torch.zeros(cj.N_OUT, dtype=torch.float64)
    for b in range(len(Js)):
        Tb = torch.nan_to_num(T[b], nan=0.0)
        worst = torch.maximum(worst, cj.forward_measure(Tb, Js[b], vrows, viss[b]))
        assert int(viss[b].sum()) > 0.5 * P
    bad = []
    for o in outs:
        name = cj.OUT_NAMES[o]
        e = record(T_name, f"{tag}: {name}", float(worst[o]), cj.forward_tol(name, aa, only))
        if e > cj.forward_tol(name, aa, only):
            bad.append((name, e))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("mask_xyz", [1, 0])
@pytest.mark.parametrize("smod", [1.0, 0.7])
@pytest.mark.parametrize("aa", [False, True])
def test_tangent_views_branches(aa, smod, mask_xyz):
    """SH 3, 768 Gaussians: antialiasing x scale_modifier x the 8-float and the 12-float record."""
    _check_forward("test_tangent_views_branches", (3, 3), aa, smod, mask_xyz, 768)


@pytest.mark.parametrize("mask_xyz", [1, 0])
@pytest.mark.parametrize("degrees", [d for d in cj.DEGREES if d != (3, 3)])
def test_tangent_views_sh_degrees(degrees, mask_xyz):
    """(stored, active) SH degree: no rest group, all active, and an active degree below the stored one (the rest's
    inactive coefficients have a zero column)."""
    _check_forward("test_tangent_views_sh_degrees", degrees, True, 0.7, mask_xyz, 768)


@pytest.mark.parametrize("mask_xyz", [1, 0])
@pytest.mark.parametrize("P", [255, 256, 257])
def test_tangent_views_block_edges(P, mask_xyz):
    """A prefix of the scene one short of, equal to and one past the 256-Gaussian block."""
    _check_forward("test_tangent_views_block_edges", (3, 3), True, 0.7, mask_xyz, P)


@pytest.mark.parametrize("only,mask_xyz", cj.SINGLE_GROUPS)
def test_tangent_views_single_group_null_others(only, mask_xyz):
    """v in one group only, every other group's pointer NULL: a NULL pointer is a zero tangent, and no group's
    tangent leaks into another's outputs."""
    aa, smod = cj.SINGLE_GROUP_CASE
    _check_forward("test_tangent_views_single_group_null_others", (3, 3), aa, smod, mask_xyz, 768, only)


# ------------------------------------------------------------------ reverse: gslm_gather_screen against J^T s + D v
def _screen_rows(ss, stats, P, n, stride):
    """[n, stride, 8] on the GPU: (conic a, b, c, opacity, r, g, b cotangents, flags word); guard rows NaN, visible."""
    scr = torch.full((n, stride, 8), float("nan"))
    scr[:, :P, :7] = ss[:, :, 2:9]
    words = _flag_words(stats, P, n, stride).cpu()
    scr.view(torch.int32)[:, :, 7] = words
    return scr.to(DEV)


def _gather_screen(degrees, aa, smod, P, n_views, overwrite, damp, seed=41):
    """Returns (y rows [P, C] float64, expected rows, magnitude rows, extras)."""
    from gslm import _lib
    from gslm.lm import STAGE_ALL, STAGE_OVERWRITE
    m, g, lay, K, cams, Js, stats = _case(degrees, aa, smod, P)
    cams, Js, stats = cams[:n_views], Js[:n_views], stats[:n_views]
    sl = cj.group_slices(K)
    ss = cj.cotangents(P, n_views, seed)
    viss = [s["visible"][:P] for s in stats]
    v = cj.direction(lay, seed + 1)
    vrows = cj.per_gaussian(lay, v)
    ref, mag = cj.reverse_reference(Js, list(ss), viss)
    ref[:, sl["xyz"]] = 0  # xyz is masked: the rows carry no xy / inverse-depth cotangent and J^T's xyz part is left out
    mag[:, sl["xyz"]] = 0
    d = torch.zeros(ref.shape[1], dtype=torch.float64)
    if damp:
        for k, name in enumerate(cj.GROUP_NAMES):
            d[sl[name]] = float(np.float32(DAMP7[k]))  # the kernel holds the damping in float
    dv = d[None, :] * vrows
    mag = mag + dv.abs()
    gen = torch.Generator().manual_seed(seed + 2)
    if overwrite:
        y0 = torch.full((lay.numel,), float("nan"))
        y0rows = torch.zeros_like(ref)
    else:
        # a random y of each element's own size where a view reaches it (so the sum is exercised at the gradient's
        # scale), plain N(0, 1) elsewhere
        u = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
        y0rows = torch.where(mag > 0, u * mag, u).float().double()
        y0 = torch.full((lay.numel,), float("nan"))
        for name in cj.GROUP_NAMES:
            a, b = lay.offsets[name]
            if b > a:
                y0[a:b] = y0rows[:, sl[name]].reshape(-1).float()
    yd, vd = y0.to(DEV), v.to(DEV)
    stride = P + 7
    scr = _screen_rows(ss, stats, P, n_views, stride)
    dot = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = torch.empty(_lib.lib.gslm_dot_scratch_bytes(P) // 8 + 8, dtype=torch.float64, device=DEV)
    opts = _lib.GslmMatvecOpts()
    opts.stages = STAGE_ALL | (STAGE_OVERWRITE if overwrite else 0)
    damps = (ctypes.c_double * 7)(*DAMP7)
    if damp:
        opts.damp7 = damps
    opts.screen_stride = stride
    opts.dot_vy = dot.data_ptr()
    opts.dot_scratch = scratch.data_ptr()
    opts.dot_scratch_bytes = scratch.numel() * 8
    vs, ys = lay.grads_struct(vd), lay.grads_struct(yd)
    _lib.check(_lib.lib.gslm_gather_screen(_view_array(cams, degrees[1], smod, aa), n_views, ctypes.byref(g),
                                          scr.data_ptr(), ctypes.byref(vs), ctypes.byref(ys), ctypes.byref(opts),
                                          _lib.stream_handle(DEV)), "gslm_gather_screen")
    torch.cuda.synchronize()
    y = yd.cpu()
    e0, e1 = lay.offsets["exposure"]
    assert torch.isnan(y[e0:e1]).all(), "the exposure group is not the gather's"
    x0, x1 = lay.offsets["xyz"]
    yx = y[x0:x1].reshape(P, 3)
    # xyz is masked: overwritten with d v (exactly; +0 without damping), untouched when accumulating
    if overwrite:
        want = (np.float32(DAMP7[0]) * v[x0:x1].numpy()).reshape(P, 3) if damp else np.zeros((P, 3), np.float32)
        assert np.array_equal(yx.numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    else:
        assert np.array_equal(yx.numpy().view(np.uint32), y0[x0:x1].reshape(P, 3).numpy().view(np.uint32))
    yfull = y.clone()
    yfull[e0:e1] = 0
    yrows = cj.per_gaussian(lay, yfull)
    # <v, y> over the elements the gather wrote, from the returned y in float64
    written = [n_ for n_ in cj.GROUP_NAMES if n_ != "xyz" or overwrite]
    want_dot = sum(float((vrows[:, sl[n_]] * yrows[:, sl[n_]]).sum()) for n_ in written)
    got_dot = float(dot.cpu())
    assert abs(got_dot - want_dot) <= 1e-6 * abs(want_dot), (got_dot, want_dot)
    anyvis = torch.stack(viss).any(dim=0)
    return yrows, y0rows + ref + dv, mag, dict(K=K, anyvis=anyvis, y0rows=y0rows, dv=dv, overwrite=overwrite,
                                               damp=damp, vrows=vrows, ss=ss, viss=viss, Js=Js)


def _check_reverse(T_name, degrees, aa, smod, P, n_views, overwrite=True, damp=True):
    yrows, want, mag, x = _gather_screen(degrees, aa, smod, P, n_views, overwrite, damp)
    K, anyvis = x["K"], x["anyvis"]
    sl = cj.group_slices(K)
    tag = (f"{_tag(degrees, aa, smod, P)} views={n_views} {'overwrite' if overwrite else 'accumulate'} "
           f"damp={int(damp)}")
    assert 0 < int((~anyvis).sum()) < P
    # Gaussians no view sees: exactly d v (+0 without damping) in every group; accumulating, y + d v to one rounding
    hid = ~anyvis
    for name in cj.GROUP_NAMES[1:]:
        if sl[name].stop == sl[name].start:
            continue
        got = yrows[hid][:, sl[name]]
        if overwrite:
            dvf = (np.float32(DAMP7[cj.GROUP_NAMES.index(name)]) * x["vrows"][hid][:, sl[name]].numpy().astype(np.float32)
                   if damp else np.zeros(got.shape, np.float32))
            assert np.array_equal(got.numpy().astype(np.float32).view(np.uint32),
                                  dvf.astype(np.float32).view(np.uint32)), name
        else:
            w = want[hid][:, sl[name]]
            size = x["y0rows"][hid][:, sl[name]].abs() + x["dv"][hid][:, sl[name]].abs()
            assert bool(((got - w).abs() <= 2.0 ** -23 * size).all()), name
    meas = cj.reverse_measure(yrows, want, mag, K, rows=anyvis)
    bad = []
    for name, e in meas.items():
        if name == "xyz":
            continue
        record(T_name, f"{tag}: {name}", e, cj.reverse_tol(name, aa))
        if e > cj.reverse_tol(name, aa):
            bad.append((name, e))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("n_views", [1, 2])
@pytest.mark.parametrize("smod", [1.0, 0.7])
@pytest.mark.parametrize("aa", [False, True])
def test_gather_screen_branches(aa, smod, n_views):
    """SH 3, 768 Gaussians: antialiasing x scale_modifier x one / two views, overwriting a NaN-filled y, damped."""
    _check_reverse("test_gather_screen_branches", (3, 3), aa, smod, 768, n_views)


@pytest.mark.parametrize("damp", [True, False])
@pytest.mark.parametrize("overwrite", [True, False])
def test_gather_screen_overwrite_accumulate_damping(overwrite, damp):
    """STAGE_OVERWRITE on a NaN-prefilled y and accumulation into a random y, damp7 set and NULL, two views."""
    _check_reverse("test_gather_screen_overwrite_accumulate_damping", (3, 3), True, 0.7, 768, 2, overwrite, damp)


@pytest.mark.parametrize("degrees", [d for d in cj.DEGREES if d != (3, 3)])
def test_gather_screen_sh_degrees(degrees):
    _check_reverse("test_gather_screen_sh_degrees", degrees, True, 0.7, 768, 2, overwrite=degrees[0] != 2)


@pytest.mark.parametrize("P", [255, 256, 257])
def test_gather_screen_block_edges(P):
    _check_reverse("test_gather_screen_block_edges", (3, 3), True, 0.7, P, 2, overwrite=P != 256)


# ------------------------------------------------------------------ transpose
@pytest.mark.parametrize("aa", [False, True])
def test_tangent_and_gather_are_transposes(aa):
    """<s, T(v)> over the visible (view, Gaussian) pairs equals <v, J^T s> from the two GPU calls (same flags), both
    accumulated in float64, to the larger of the two tolerances times sum |s| |J| |v|."""
    degrees, smod, P = (3, 3), 0.7, 768
    T, vrows, Js, viss = _tangent_views(degrees, aa, smod, 1, P, seed=42)  # the direction of _gather_screen(seed=41)
    yrows, want, mag, x = _gather_screen(degrees, aa, smod, P, 2, True, False, seed=41)
    assert torch.equal(x["vrows"][:, 3:], vrows[:, 3:])
    lhs = sum(float((x["ss"][b].double() * torch.nan_to_num(T[b], nan=0.0))[viss[b]].sum()) for b in range(2))
    rhs = float((vrows * yrows).sum())
    scale = sum(float(torch.einsum("po,poc,pc->p", x["ss"][b].double().abs(), Js[b].abs(), vrows.abs())[viss[b]].sum())
                for b in range(2))
    tol = max(max(cj.forward_tol(n, aa) for n in cj.OUT_NAMES[2:9]),
              max(cj.reverse_tol(n, aa) for n in cj.GROUP_NAMES[1:]))
    e = record("test_tangent_and_gather_are_transposes", f"aa={int(aa)}: |<s, T v> - <v, J^T s>| / sum |s||J||v|",
               abs(lhs - rhs) / scale, tol)
    assert abs(lhs) > 0 and e <= tol, (lhs, rhs, scale)


# ------------------------------------------------------------------ flags from a real preprocess
def test_flags_from_a_real_preprocess():
    """gslm_view_flags after LMProblem.evaluate equals the oracle's word on every Gaussian visible on both sides whose
    colour is not within 1e-5 of its clamp; the visible sets differ only on Gaussians the float64 oracle puts on a
    decision boundary (scenes.chain_branch_stats: <= 1 % of P, asserted on the CPU)."""
    from gslm import _lib
    from gslm.lm import LMProblem
    sub, cams, Js, stats = cj.branch_case(3, 3, False, 1.0)
    P = sub._xyz.shape[0]
    import copy
    prob = LMProblem(copy.deepcopy(sub).to(DEV), [copy.deepcopy(c).to(DEV) for c in cams], torch.zeros(3), device=DEV)
    prob.evaluate()
    for b, vr in enumerate(prob.views):
        out = torch.zeros(P, dtype=torch.int32, device=DEV)
        _lib.check(_lib.lib.gslm_view_flags(vr.geom.data_ptr(), P, out.data_ptr(), prob.stream), "gslm_view_flags")
        torch.cuda.synchronize()
        got = torch.from_numpy(out.cpu().numpy().view(np.uint32).astype(np.int64))
        s = stats[b]
        want = cj.flags_word(s["visible"], s["clamped"])
        gvis = (got >> 31) == 1
        assert bool(((got == 0) | gvis).all()) and bool((got[gvis] & 0x7FFFFFF8 == 0).all())
        differ = gvis != s["visible"]
        assert bool((~differ | s["boundary"]).all()), torch.nonzero(differ & ~s["boundary"]).flatten().tolist()
        assert int(s["boundary"].sum()) <= 0.01 * P
        sure = gvis & s["visible"] & (s["res"].abs() > 1e-5).all(dim=1)
        assert int(sure.sum()) > 0.7 * P
        assert torch.equal(got[sure], want[sure]), b
        assert int(((got & 7) != 0).sum()) >= 100


# ------------------------------------------------------------------ the whole product on the branch scene
def _of_max(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _expected_lm():
    """The oracle's loss, J^T b and (J^T J + D) v on view 0 (float32, full layout; computed once, not modified)."""
    import copy
    from oracle.lm_ref import OracleLMProblem
    sub, cams, _, _ = cj.branch_case(3, 3, False, 1.0)
    op = OracleLMProblem(copy.deepcopy(sub), [copy.deepcopy(cams[0])], torch.zeros(3))
    loss = float(op.evaluate())
    g = op.rhs()
    v = cj.direction(op.layout, 9)
    a, b = op.layout.offsets["xyz"]
    v[a:b] = 0
    return op, loss, g, v, op.matvec(v, op.zeros())


@pytest.mark.parametrize("projected", [False, True])
def test_lm_product_on_the_branch_scene(projected):
    """LMProblem.rhs and matvec against oracle/lm_ref.py, full and SH-rest-projected layout (loss rel 1e-5, vectors
    1e-4 of the reference's max, as tests/test_gpu_lm_background.py)."""
    import copy
    from gslm.lm import LMProblem
    T = "test_lm_product_on_the_branch_scene"
    op, loss, g_ref, v_ref, y_ref = _expected_lm()
    sub, cams, _, _ = cj.branch_case(3, 3, False, 1.0)
    prob = LMProblem(copy.deepcopy(sub).to(DEV), [copy.deepcopy(cams[0]).to(DEV)], torch.zeros(3), device=DEV,
                     sh_projection=projected)
    assert prob.layout.rest_projected == projected
    tag = f"proj={int(projected)}"
    e_loss = record(T, f"{tag}: loss rel", abs(float(prob.evaluate()) - loss) / loss, 1e-5)
    g = prob.rhs(prob.zeros())
    e_g = record(T, f"{tag}: J^T b (of max)", _of_max((prob.expand(g) if projected else g).cpu(), g_ref), 1e-4)
    if projected:
        v = cj.direction(prob.layout, 9).to(DEV)
        a, b = prob.layout.offsets["xyz"]
        v[a:b] = 0
        yo = op.matvec(prob.expand(v).cpu(), op.zeros())
    else:
        v, yo = v_ref.to(DEV), y_ref
    y = prob.matvec(v, prob.zeros())
    e_y = record(T, f"{tag}: (J^T J + D) v (of max)", _of_max((prob.expand(y) if projected else y).cpu(), yo), 1e-4)
    assert e_loss <= 1e-5, e_loss
    assert e_g < 1e-4, e_g
    assert e_y < 1e-4, e_y
