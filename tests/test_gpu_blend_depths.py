"""GPU: every tile blend pass at list depths on and next to its round size, against the oracle in float64.

The tile passes walk a tile's sorted list in rounds -- 64 positions (k_render_fwd_wave, jvp_wave_packed /
k_render_jv_wave), 96 (the drop-in k_render_bwd<true, *, 3>, whose second hit word is half used), 128
(k_render_bwd<false, false, 2> and k_render_matvec<*>) and 256 (k_render_jvp<*>) -- between the machinery that bounds
the rounds: n_eff from the per-wave maxima of n_contrib, base / cnt of the back-to-front pass, rel of the wave pass, the
quadrant masks and-ed with the per-wave bounds, the hit-word walk, live_update, and the LM row map whose tail rows are
never read.  An off-by-one in any of these is wrong only at particular depths, which the random scenes of the other
tests do not hit (no tile of theirs has n_eff at 96, 128, 192 or 256 or next to them, and none has a tail to speak of).

Scenes (scenes.stack_scene, cases in blend_reference.CASES): Gaussians stacked along the optical axis, list position
== index, every pixel of every tile blending all of them -- depths 1, 63 .. 65, 95 .. 97, 127 .. 129, 191 .. 193,
255 .. 257 and 300 on one 16x16 tile, 64 / 96 / 128 / 256 on 33x17 (six tiles; the right column and the bottom row
leave whole waves outside the image) and 97 on 40x33; "wall" cases, where every pixel stops at n_eff = 64, 96, 97, 128,
129 or 256 under a list of 200 - 400 (a tail of >= 64 entries nobody blends); "blob" cases, where one quadrant of the
tile stops early (at 64, 65, 96, 97, 127, 128 or 129, its pixels at >= 8 different depths) and the other three run to
128 - 300.  Backgrounds (0.2, 0.5, 0.9) and zero.  What each case must exercise, and that float32 takes every skip /
stop decision as float64 does, is asserted on oracle data by tests/test_oracle_blend_depths.py.

Expected values: the oracle in double (blend_reference), derivatives by AD.  Bounds (blend_reference.bound): per
quantity and case max(8 e32, n_eff 2^-22) capped by the suite's bar, where e32 is the float32 oracle's own error
against float64 in that quantity's measure (its largest value over the cases) and n_eff the case's depth -- derived
on the CPU, never from a GPU number.  Integer and index results are compared exactly."""
import ctypes
import types

import pytest
import torch
import torch.autograd.forward_ad as fwAD

import blend_reference as br
from blend_reference import CASES
from margins import record
from scenes import gpu_settings

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = list(CASES)


def _bound(test, name, what, quantity, measured):
    b = br.bound(quantity, name)
    m = record(test, f"{name} {what} [{quantity}]", measured, b)
    assert m <= b, (name, what, quantity, m, b)


def _tail_ids(ref, c):
    """The Gaussians no pixel blends (list positions >= n_eff in every tile); the list is the same in every tile."""
    ntiles = ref.ranges.shape[0]
    lists = [ref.point_list[int(ref.ranges[t, 0]):int(ref.ranges[t, 1])] for t in range(ntiles)]
    assert all(torch.equal(lists[0], L) for L in lists)
    tail = lists[0][c.n_eff:]
    assert tail.numel() == c.n - c.n_eff
    return tail


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("name", NAMES)
def test_forward(name):
    """k_render_fwd_wave: point list, ranges, radii and n_contrib exact; final_T, colour and inverse depth against
    float64.  A blob-stopped quadrant leaves the other three at the full depth."""
    from test_gpu_raster import _gpu_forward_internals
    c = CASES[name]
    ref = br.dropin64(name)
    model, cam = br.build(name)
    G = _gpu_forward_internals(model, cam, 1, torch.tensor(c.bg))
    assert torch.equal(G["radii"], ref.radii)
    assert G["N"] == ref.point_list.numel()
    assert torch.equal(G["point_list"], ref.point_list)
    assert torch.equal(G["ranges"], ref.ranges)
    assert torch.equal(G["n_contrib"].long(), ref.n_contrib.long())
    if c.blobs is not None:
        q = c.blobs[0]
        qd = br.quadrant_depths(types.SimpleNamespace(n_contrib=G["n_contrib"]))
        assert qd[q] == c.stopped and all(qd[s] == c.n for s in range(4) if s != q), qd
    T = "test_forward"
    _bound(T, name, "final_T", "final_T", br.linf(G["final_T"], ref.final_T))
    _bound(T, name, "colour", "image", br.linf(G["color"], ref.color))
    _bound(T, name, "inverse depth", "image", br.linf(G["invdepth"], ref.invdepth))


# ---------------------------------------------------------------- drop-in backward and JVP
def _rasterizer(name):
    from diff_gaussian_rasterization import GaussianRasterizer
    model, cam, a, cot, tang = br.dropin_inputs(name)
    rast = GaussianRasterizer(gpu_settings(cam, 1, torch.tensor(CASES[name].bg)))
    return rast, a, cot, tang


def _gpu_backward(name, with_depth):
    rast, a, cot, _ = _rasterizer(name)
    a = {k: v.to(DEV).requires_grad_(True) for k, v in a.items()}
    m2 = torch.zeros_like(a["means3D"], requires_grad=True)
    col, _, dep = rast(means3D=a["means3D"], means2D=m2, shs=a["shs"], opacities=a["opacities"], scales=a["scales"],
                       rotations=a["rotations"])
    obj = (col * cot["color"].to(DEV)).sum()
    if with_depth:
        obj = obj + (dep * cot["depth"].to(DEV)).sum()
    obj.backward()
    return {k: v.grad.detach().cpu() for k, v in a.items()} | {"means2D": m2.grad.detach().cpu()}


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_dropin_backward(name, with_depth):
    """k_render_bwd<true, with_depth, 3> (96 entries per round): the six input gradients and means2D against float64; a
    second run bitwise equal; in wall cases the tail Gaussians' gradients exactly zero."""
    c = CASES[name]
    ref = br.dropin64(name)
    got = _gpu_backward(name, with_depth)
    again = _gpu_backward(name, with_depth)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
    if c.wall is not None:
        tail = _tail_ids(ref, c)
        for k in got:
            assert float(ref.grads[with_depth][k][tail].abs().max()) == 0.0
            assert float(got[k][tail].abs().max()) == 0.0, f"{k}: tail gradient not exactly zero"
    T = "test_dropin_backward"
    for k in got:
        _bound(T, name, f"depth={int(with_depth)} d{k}", "grad", br.of_max(got[k], ref.grads[with_depth][k]))


@pytest.mark.parametrize("with_xy", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_dropin_jvp(name, with_xy):
    """k_render_jvp<with_xy> (256 entries per round): tangents on every input, and on every input but means3D /
    means2D; the colour and inverse-depth tangents against float64."""
    ref = br.dropin64(name)
    rast, a, _, tang = _rasterizer(name)
    with torch.no_grad(), fwAD.dual_level():
        dual = {k: (fwAD.make_dual(v.to(DEV), tang[k].to(DEV)) if (with_xy or k != "means3D") else v.to(DEV))
                for k, v in a.items()}
        z = torch.zeros_like(a["means3D"]).to(DEV)
        m2 = fwAD.make_dual(z, tang["means2D"].to(DEV)) if with_xy else z
        col, _, dep = rast(means3D=dual["means3D"], means2D=m2, shs=dual["shs"], opacities=dual["opacities"],
                           scales=dual["scales"], rotations=dual["rotations"])
        ct, dt = fwAD.unpack_dual(col).tangent.cpu(), fwAD.unpack_dual(dep).tangent.cpu()
    T = "test_dropin_jvp"
    _bound(T, name, f"xy={int(with_xy)} colour tangent", "colour_tangent", br.of_max(ct, ref.tangents[with_xy][0]))
    _bound(T, name, f"xy={int(with_xy)} inverse-depth tangent", "depth_tangent", br.of_max(dt, ref.tangents[with_xy][1]))


# ---------------------------------------------------------------- the LM path
def _problem(name, mask_xyz=True, ssim=False):
    from gslm.lm import LMProblem
    model, cam = br.build(name)
    model.to(DEV)
    cam.to(DEV)
    prob = LMProblem(model, [cam], torch.tensor(CASES[name].bg), device=DEV, sh_projection=False, mask_xyz=mask_xyz,
                     ssim=ssim)
    return prob, model, cam


def _jv(prob, v):
    """m 1[0 <= R <= 1] (.) (dR / dtheta) v of the single view: LMProblem.jv_residual on the LM rows (k_render_jv_wave);
    with xyz free the same call with mask_xyz = 0 (launch_render_jv's k_render_jvp<true> branch)."""
    from gslm import _lib
    from gslm.params import raw_gaussians
    vr = prob.views[0]
    rm = prob.residual_masks()
    out = [torch.empty(3, vr.H, vr.W, device=DEV)]
    if prob.mask_xyz:
        return prob.jv_residual(v, rm, out)[0]
    g = raw_gaussians(prob.model)
    vs = prob.layout.grads_struct(v)
    opts = _lib.GslmMatvecOpts()
    opts.stages = 1 | 2  # TANGENT | RENDER
    opts.flags = prob.mv_flags
    opts.jv_out = out[0].data_ptr()
    _lib.check(_lib.lib.gslm_matvec_view_ex(ctypes.byref(vr.view), ctypes.byref(g), ctypes.byref(vs), out[0].data_ptr(),
                                            0, vr.geom.data_ptr(), vr.binning.data_ptr(), vr.N, vr.image.data_ptr(),
                                            vr.scratch.data_ptr(), vr.scratch.numel(), ctypes.byref(vs),
                                            ctypes.byref(opts), prob.stream), "gslm_matvec_view_ex(jv)")
    return out[0].mul_(rm[0])


def _rows(layout, vec, ids, skip=("exposure",)):
    return {k: t.reshape(layout.P, -1)[ids.to(vec.device)] for k, t in layout.views(vec).items()
            if k not in skip and t.numel()}


@pytest.mark.parametrize("mask_xyz", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_lm_single_view(name, mask_xyz):
    """LMProblem on the case's view, full SH layout.  mask_xyz=True: k_render_bwd<false, false, 2> (J^T b),
    k_render_matvec<false> (jvp_wave_packed), k_render_jv_wave; mask_xyz=False: the drop-in backward,
    k_render_matvec<true> (jvp_tile) and k_render_jvp<true>.  evaluate(), rhs(), matvec(), J v and the line-search loss
    against float64.  The LM row map is built once by the product and (mask_xyz) once by rhs() after a fresh forward,
    and reused by the call after each: the flag only decides whether launch_lm_rowmap runs, and the results are
    bitwise equal; in wall cases the tail Gaussians' J^T b exactly zero and their (J^T J + D) v exactly D v."""
    from gslm.lm import LossEvaluator
    c = CASES[name]
    ref = br.lm64(name, mask_xyz)
    prob, model, cam = _problem(name, mask_xyz)
    T, tag = "test_lm_single_view", f"xyz={int(not mask_xyz)}"
    loss = float(prob.evaluate())
    assert prob.num_rendered()[0] == br.dropin64(name).point_list.numel()
    vr = prob.views[0]
    v = ref.v.to(DEV)
    assert not vr.tail_clean  # a forward leaves no row map: this product builds it (launch_lm_rowmap)
    y = prob.matvec(v, prob.zeros()).clone()
    assert vr.tail_clean
    y2 = prob.matvec(v, prob.zeros()).clone()  # MV_TAIL_CLEAN: the same kernels on the map the first product built
    assert torch.equal(y, y2), "the product differs between the run that builds the row map and the one that reuses it"
    g = prob.rhs(prob.zeros()).clone()  # mask_xyz: on the product's row map; else the drop-in backward, which drops it
    assert vr.tail_clean == mask_xyz
    assert torch.equal(g, prob.rhs(prob.zeros()))
    if mask_xyz:  # and J^T b as the builder of the map, after a fresh forward
        assert float(prob.evaluate()) == loss and not vr.tail_clean
        assert torch.equal(g, prob.rhs(prob.zeros())) and vr.tail_clean
    jv = _jv(prob, v).cpu()
    ls = float(LossEvaluator(model, [cam], torch.tensor(c.bg), device=DEV, batch=1, streams=1).evaluate())
    if c.wall is not None:
        tail = _tail_ids(br.dropin64(name), c)
        damp = prob.damp
        for k, rows in _rows(prob.layout, g, tail).items():
            assert float(rows.abs().max()) == 0.0, f"J^T b {k}: tail rows not exactly zero"
        vrows = _rows(prob.layout, v, tail)
        for k, rows in _rows(prob.layout, y, tail).items():
            assert torch.equal(rows, vrows[k] * torch.tensor(damp[k], dtype=torch.float32)), f"product {k}: tail != D v"
    _bound(T, name, tag + " evaluate() loss", "loss", abs(loss - ref.loss) / ref.loss)
    _bound(T, name, tag + " line-search loss", "loss", abs(ls - ref.loss) / ref.loss)
    _bound(T, name, tag + " J^T b", "lm_vector", br.of_max(g.cpu(), ref.g))
    _bound(T, name, tag + " (J^T J + D) v", "lm_vector", br.of_max(y.cpu(), ref.y))
    _bound(T, name, tag + " J v", "lm_vector", br.of_max(jv, ref.jv))


def test_lm_ssim_depth_128():
    """The SSIM residual at depth 128: its J v image comes from k_render_jv_wave and its adjoint half from the seeded
    k_render_bwd<false, false, 2>."""
    name = br.SSIM_CASE
    ref = br.lm64(name, True, True)
    prob, _, _ = _problem(name, ssim=True)
    T = "test_lm_ssim_depth_128"
    loss = float(prob.evaluate())
    g = prob.rhs(prob.zeros()).clone()
    y = prob.matvec(ref.v.to(DEV), prob.zeros()).clone()
    assert torch.equal(y, prob.matvec(ref.v.to(DEV), prob.zeros()))
    _bound(T, name, "SSIM loss", "loss", abs(loss - ref.loss) / ref.loss)
    _bound(T, name, "SSIM J^T b", "ssim_vector", br.of_max(g.cpu(), ref.g))
    _bound(T, name, "SSIM (J^T J + D) v", "ssim_vector", br.of_max(y.cpu(), ref.y))
