"""GPU: the drop-in rasterizer's VJP and JVP held to float64 per Gaussian and per pixel.

k_preprocess_bwd<RAW> / k_render_bwd (GaussianRasterizer's backward, and gslm_backward with raw leaves as
LMProblem.rhs_full calls it) and the non-compact k_preprocess_jvp<false, false> / k_render_jvp (the forward-mode jvp)
on the branch scene, against the split float64 reference of tests/dropin_chain_ref.py:

  reverse  per (Gaussian, input tensor)  max_k |y - ref| <= tol max_k mag,  mag = |J_i|^T S_i
  forward  per (pixel, channel)          |T - ref| <= tol den,             den = sum |D| |J| |v|

with tol = min(8 x the float32 oracle's own value of the same measure, 2e-4) (dropin_chain_ref.FLOORS, measured and
asserted on the CPU by tests/test_oracle_dropin_chain.py), no Gaussian and no pixel left out, and exact zeros (or the
prior value, bitwise, when accumulating) wherever the reference's measure is zero.  A wrong branch shows at 0.1 .. 0.3.
Before any float comparison the radii, the sorted point list and n_contrib are asserted equal to the float64 oracle's.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import chain_jacobian as cj
import dropin_chain_ref as dr
from margins import record
from scenes import gpu_settings

pytestmark = pytest.mark.gpu
DEV = "cuda"

RASTERIZER_CASES = [c for c in dr.reverse_cases() if c.form != "raw"]
RAW_CASES = [c for c in dr.reverse_cases() if c.form == "raw"]


def _settings(cfg):
    return gpu_settings(dr.camera(cfg), cfg.degrees[1], torch.tensor(dr.BG), DEV, scale_modifier=cfg.smod,
                        antialiasing=cfg.aa)


def _device_inputs(cfg):
    return {n: t.clone().to(DEV) for n, t in dr.case(cfg).x32.items()}


def _gaussians(cfg, x):
    """gslm_gaussians over the flat device tensors x (kept alive by the caller)."""
    from diff_gaussian_rasterization import _gaussians as activated_gaussians
    from gslm import _lib
    P, K = cfg.P, dr.case(cfg).K
    if cfg.form == "raw":
        return _lib.make_gaussians(P, x["xyz"], x["opacity"], x["scaling"], x["rotation"], None,
                                   x["features_dc"].data_ptr(), 3, x["features_rest"].data_ptr() if K > 1 else None,
                                   3 * (K - 1), K, None, raw=True)
    sh = x["shs"].reshape(P, -1, 3) if "shs" in x else None
    dc = x["dc"].reshape(P, 1, 3) if "dc" in x else None
    return activated_gaussians(P, x["means3D"], x["opacities"].reshape(-1), x.get("scales"), x.get("rotations"),
                               x.get("cov3D_precomp"), sh, dc, x.get("colors_precomp"))


def _forward(cfg, x):
    """The forward of one call through the C ABI; radii, point list and n_contrib asserted equal to the float64
    oracle's.  Returns (view, gaussians, geom, binning, image, N)."""
    from diff_gaussian_rasterization import forward_buffers
    from gslm import _lib
    cs = dr.case(cfg)
    view = _lib.view_from_settings(_settings(cfg))
    g = _gaussians(cfg, x)
    color, radii, invd, geom, binning, image, N = forward_buffers(view, g, DEV)
    H, W, P = cs.H, cs.W, cfg.P
    pl = torch.zeros(max(N, 1), dtype=torch.int32, device=DEV)
    rg = torch.zeros(((W + 15) // 16) * ((H + 15) // 16) * 2, dtype=torch.int32, device=DEV)
    tiles = torch.zeros(P, dtype=torch.int32, device=DEV)
    fT = torch.zeros(H * W, dtype=torch.float32, device=DEV)
    nc = torch.zeros(H * W, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.gslm_inspect(geom.data_ptr(), P, binning.data_ptr(), N, H, W, image.data_ptr(), pl.data_ptr(),
                                     rg.data_ptr(), tiles.data_ptr(), fT.data_ptr(), nc.data_ptr(), None,
                                     _lib.stream_handle(DEV)), "gslm_inspect")
    torch.cuda.synchronize()
    assert torch.equal(radii.cpu(), cs.radii), "radii"
    assert N == cs.point_list.numel() and torch.equal(pl[:N].cpu().long(), cs.point_list), "sorted point list"
    assert torch.equal(nc.view(H, W).cpu().long(), cs.n_contrib.long()), "n_contrib"
    return view, g, geom, binning, image, N


@functools.lru_cache(maxsize=None)
def _decisions_checked(cfg):
    _forward(cfg, _device_inputs(cfg))
    return True


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check_reverse(test, cfg, yrows, ref, mag, names=None):
    """Records and asserts the reverse measure of every input tensor (or `names`) and both classes of Gaussian."""
    cs = dr.case(cfg)
    assert bool(torch.isfinite(yrows).all())
    bad = []
    for (name, is_thin), e in dr.reverse_measure(cs, yrows, ref, mag, names).items():
        tol = dr.reverse_tol(name, cfg.aa, is_thin)
        record(test, f"{dr.cfg_id(cfg)}: {name}{' (thin)' if is_thin else ''}", e, tol)
        if not e <= tol:
            bad.append((name, is_thin, e, tol))
    assert not bad, (dr.cfg_id(cfg), bad)


# ------------------------------------------------------------------ reverse through GaussianRasterizer
def _rasterizer_grads(cfg, requires=None, seed=4):
    """name -> gradient (device tensors) of <u, (colour, inverse depth)> for the inputs in `requires` (default all)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    cs = dr.case(cfg)
    x = _device_inputs(cfg)
    for n in (x if requires is None else requires):
        x[n].requires_grad_(True)
    u = dr.cotangent(cfg, seed).to(DEV)
    color, radii, invd = GaussianRasterizer(_settings(cfg))(**dr.gpu_kwargs(cfg.form, x))
    assert torch.equal(radii.cpu(), cs.radii)
    ((color * u[:3]).sum() + (invd * u[3:]).sum()).backward()
    return {n: t.grad for n, t in x.items() if t.grad is not None}


@pytest.mark.parametrize("cfg", RASTERIZER_CASES, ids=dr.cfg_id)
def test_rasterizer_backward(cfg):
    """k_preprocess_bwd<false> with colour and inverse-depth cotangents and means2D a leaf: both views plain and with
    antialiasing at scale_modifier 0.7; cov3D_precomp, colors_precomp, both, the dc split; the (stored, active) SH
    degrees; prefixes around the 256-Gaussian block."""
    cs = dr.case(cfg)
    assert _decisions_checked(cfg)
    ref, mag, _ = dr.reverse_reference(cfg)
    grads = _rasterizer_grads(cfg)
    assert set(grads) == {n for n, w in cs.cols if w}
    yrows = cs.rows(grads)
    dead = (mag == 0).all(dim=1)
    assert bool((yrows[dead] == 0).all()), "a Gaussian nothing blends has a nonzero gradient"
    assert bool((yrows[:, cs.slices["means2D"]][:, 2] == 0).all())
    _check_reverse("test_rasterizer_backward", cfg, yrows, ref, mag)


@pytest.mark.parametrize("cfg", [dr.Cfg(0, True, 0.7), dr.Cfg(0, True, 0.7, "split")], ids=dr.cfg_id)
def test_rasterizer_requires_grad_subsets(cfg):
    """Only means3D (no SH output, the direction term on) and everything but means3D (the direction term off): each
    requested gradient is bitwise the all-outputs call's."""
    cs = dr.case(cfg)
    full = _rasterizer_grads(cfg)
    names = [n for n, w in cs.cols if w]
    for req in (["means3D"], [n for n in names if n != "means3D"]):
        got = _rasterizer_grads(cfg, req)
        assert set(got) == set(req)
        for n in req:
            assert _same_bits(got[n], full[n]), (req, n)


# ------------------------------------------------------------------ reverse through the C ABI
def _abi_backward(cfg, x, fwd, u, out, accumulate):
    """gslm_backward for the forward `fwd` with cotangent u [4, H, W] into `out` (a gslm_grads)."""
    from gslm import _lib
    view, g, geom, binning, image, N = fwd
    scratch = _lib.u8(_lib.lib.gslm_scratch_bytes(cfg.P, N), DEV)
    out.accumulate = int(bool(accumulate))
    _lib.check(_lib.lib.gslm_backward(ctypes.byref(view), ctypes.byref(g), geom.data_ptr(), binning.data_ptr(), N,
                                      image.data_ptr(), u[:3].contiguous().data_ptr(), u[3:].contiguous().data_ptr(),
                                      scratch.data_ptr(), scratch.numel(), ctypes.byref(out),
                                      _lib.stream_handle(DEV)), "gslm_backward")
    torch.cuda.synchronize()


def _abi_outputs(cfg, names, fill=float("nan")):
    """(gslm_grads, name -> NaN-filled device tensor) with a pointer for the tensors in `names` only, NULL elsewhere."""
    from gslm import _lib
    cs = dr.case(cfg)
    P = cfg.P
    t = {n: torch.full((P, w), fill, device=DEV) for n, w in cs.cols if w and n in names}
    kw = dict(means2D=t.get("means2D"), means3D=t.get("means3D"), opacities=t.get("opacities"), scales=t.get("scales"),
              rotations=t.get("rotations"), cov3D=t.get("cov3D_precomp"), colors=t.get("colors_precomp"))
    if cfg.form == "split":
        # dc and rest pointers of their own; either may be NULL
        grads = _lib.make_grads(**kw)
        if "dc" in t:
            grads.sh_dc, grads.sh_dc_stride = t["dc"].data_ptr(), 3
        if "shs" in t:
            grads.sh_rest, grads.sh_rest_stride = t["shs"].data_ptr(), 3 * (cs.K - 1)
    else:
        grads = _lib.make_grads(sh=t["shs"].view(P, cs.K, 3) if "shs" in t else None, **kw)
    return grads, t


@pytest.mark.parametrize("cfg", [dr.Cfg(0, True, 0.7), dr.Cfg(0, True, 0.7, "split"), dr.Cfg(0, True, 0.7, "cov_col")],
                         ids=dr.cfg_id)
def test_abi_null_outputs(cfg):
    """gslm_backward on activated inputs with NULL output pointers: every requested tensor is overwritten entirely and
    is bitwise the all-outputs call's, which is bitwise GaussianRasterizer's."""
    cs = dr.case(cfg)
    names = [n for n, w in cs.cols if w]
    x = _device_inputs(cfg)
    fwd = _forward(cfg, x)
    u = dr.cotangent(cfg).to(DEV)
    grads, full = _abi_outputs(cfg, names)
    _abi_backward(cfg, x, fwd, u, grads, False)
    auto = _rasterizer_grads(cfg)
    for n in names:
        assert bool(torch.isfinite(full[n]).all()), n
        assert _same_bits(full[n], auto[n].reshape(cfg.P, -1)), n
    colour = [n for n in names if n in ("shs", "dc", "colors_precomp")]
    subsets = [["means3D"], [n for n in names if n != "means3D"], colour, [n for n in names if n not in colour],
               ["means2D", "opacities"]]
    if cfg.form == "split":
        subsets += [["dc", "means3D"], ["shs"]]
    for req in subsets:
        grads, got = _abi_outputs(cfg, req)
        _abi_backward(cfg, x, fwd, u, grads, False)
        for n in req:
            assert _same_bits(got[n], full[n]), (req, n)


def _raw_layout(cfg):
    from gslm.params import ParamLayout
    return ParamLayout(cfg.P, dr.case(cfg).K)


def _flat_from_rows(lay, rows, fill=float("nan")):
    """A flat float32 vector of the layout from [P, C] rows (group order of chain_jacobian.GROUP_NAMES); the exposure
    group holds `fill`."""
    flat = torch.full((lay.numel,), fill)
    sl = cj.group_slices(lay.K)
    for n in cj.GROUP_NAMES:
        a, b = lay.offsets[n]
        if b > a:
            flat[a:b] = rows[:, sl[n]].reshape(-1).float()
    return flat


@pytest.mark.parametrize("cfg", RAW_CASES, ids=dr.cfg_id)
def test_abi_raw_overwrite(cfg):
    """gslm_backward with raw = 1 and the full layout's strides, accumulate = 0 into a NaN-filled vector: every element
    of every group is overwritten, Gaussians nothing blends get exactly 0, the rest meets the raw-leaf Jacobian."""
    cs = dr.case(cfg)
    lay = _raw_layout(cfg)
    x = _device_inputs(cfg)
    fwd = _forward(cfg, x)
    y = torch.full((lay.numel,), float("nan"), device=DEV)
    _abi_backward(cfg, x, fwd, dr.cotangent(cfg).to(DEV), lay.grads_struct(y), False)
    y = y.cpu()
    e0, e1 = lay.offsets["exposure"]
    assert bool(torch.isnan(y[e0:e1]).all()), "the exposure group is not gslm_backward's"
    assert bool(torch.isfinite(y[:e0]).all()), "an element was not overwritten"
    y[e0:e1] = 0
    yrows = cj.per_gaussian(lay, y)
    ref, mag, _ = dr.reverse_reference(cfg)
    dead = (mag == 0).all(dim=1)
    assert int((cs.radii == 0).sum()) > 0 and bool((dead | (cs.radii > 0)).all())
    assert bool((yrows[dead] == 0).all()), "a Gaussian nothing blends has a nonzero gradient"
    _check_reverse("test_abi_raw_overwrite", cfg, yrows, ref, mag)


@pytest.mark.parametrize("aa,smod", dr.CONFIGS)
def test_abi_raw_accumulate_two_views(aa, smod):
    """accumulate = 1 over the two views onto a random y0, as LMProblem.rhs_full sums J^T b: against y0 + sum_b ref_b in
    the measure mag = sum_b mag_b + |y0|; a Gaussian no view blends keeps y0 bitwise."""
    cfgs = [dr.Cfg(b, aa, smod, "raw") for b in (0, 1)]
    lay = _raw_layout(cfgs[0])
    refs = [dr.reverse_reference(c) for c in cfgs]
    ref = refs[0][0] + refs[1][0]
    mag = refs[0][1] + refs[1][1]
    u0 = torch.randn(mag.shape, generator=torch.Generator().manual_seed(43), dtype=torch.float64)
    # a prior value of each element's own size where a view reaches it, N(0, 1) elsewhere
    y0rows = torch.where(mag > 0, u0 * mag, u0).float().double()
    y0 = _flat_from_rows(lay, y0rows)
    y = y0.clone().to(DEV)
    out = lay.grads_struct(y)
    x = _device_inputs(cfgs[0])
    for c in cfgs:
        _abi_backward(c, x, _forward(c, x), dr.cotangent(c).to(DEV), out, True)
    y = y.cpu()
    e0, e1 = lay.offsets["exposure"]
    assert bool(torch.isnan(y[e0:e1]).all())
    y[e0:e1] = 0
    yrows = cj.per_gaussian(lay, y)
    dead = (mag == 0).all(dim=1)
    assert int(dead.sum()) > 0
    assert np.array_equal(_bits(yrows[dead].float()), _bits(y0rows[dead].float())), "a prior value was changed"
    cs = dr.case(cfgs[0])
    assert bool(torch.isfinite(yrows).all())
    # a Gaussian is thin in both views or in neither, so view 0's classes serve the sum
    assert torch.equal(dr.thin(cfgs[0]), dr.thin(cfgs[1]))
    bad = []
    for (name, is_thin), e in dr.reverse_measure(cs, yrows, y0rows + ref, mag + y0rows.abs()).items():
        tol = dr.reverse_tol(name, aa, is_thin)
        record("test_abi_raw_accumulate_two_views", f"aa={int(aa)} smod={smod}: {name}{' (thin)' if is_thin else ''}",
               e, tol)
        if not e <= tol:
            bad.append((name, is_thin, e, tol))
    assert not bad, bad


# ------------------------------------------------------------------ forward through the jvp
def _rasterizer_jvp(cfg, vrows, dual):
    """(colour, inverse depth) tangent [4, H, W] with the inputs in `dual` carrying their rows of vrows as tangents and
    every other input plain (a missing tangent is a NULL pointer)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    cs = dr.case(cfg)
    x = _device_inputs(cfg)
    with torch.no_grad(), fwAD.dual_level():
        for n in dual:
            x[n] = fwAD.make_dual(x[n], vrows[:, cs.slices[n]].float().contiguous().to(DEV))
        color, _, invd = GaussianRasterizer(_settings(cfg))(**dr.gpu_kwargs(cfg.form, x))
        tc, td = fwAD.unpack_dual(color).tangent, fwAD.unpack_dual(invd).tangent
        assert tc is not None and td is not None
        return torch.cat([tc, td], dim=0).cpu()


@pytest.mark.parametrize("cfg", dr.FORWARD_CFG + [dr.FORWARD_SPLIT], ids=dr.cfg_id)
def test_jvp_supports(cfg):
    """The forward-mode jvp (12-float tangent records with the means2D tangent and the inverse-depth entry) with every
    input's tangent at once, each input's alone (the others NULL), and each branch class's Gaussians alone."""
    cs = dr.case(cfg)
    assert _decisions_checked(cfg)
    names = [n for n, w in cs.cols if w]
    bad = []
    for support, (v, ref, den) in dr.forward_references(cfg).items():
        dual = [support] if support in names else names
        T = _rasterizer_jvp(cfg, v, dual).double()
        assert bool(torch.isfinite(T).all()), support
        assert bool((T[den == 0] == 0).all()), f"{support}: a tangent where nothing can move the pixel"
        assert int((den > 0).sum()) > 0
        tol = dr.forward_tol(support)
        worst = dr.forward_measure(T, ref, den)
        for c, ch in enumerate(("r", "g", "b", "invdepth")):
            record("test_jvp_supports", f"{dr.cfg_id(cfg)} {support}: {ch}", float(worst[c]), tol)
            if not float(worst[c]) <= tol:
                bad.append((support, ch, float(worst[c]), tol))
    assert not bad, (dr.cfg_id(cfg), bad)
