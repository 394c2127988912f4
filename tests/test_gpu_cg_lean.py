"""GPU: the lean single-view CG loop (gslm.lm._cgls_lean) against the loops it must reproduce.

Benchmark-mode cgls_fused on an active view sums every dot's block partials in the kernel that needs the scalar
(no finalising launch), reads the chains' parameters from a list-order block, and starts / ends a solve with one
launch each.  All arithmetic keeps its operands and order, so on one small scene (3001 Gaussians, SH 3, one 64 x 48
view, a tenth of the Gaussians behind the camera, vector lengths odd: no multiple of 4 or 256):
  * x is bitwise the full-layout loop's (GSLM_CG_ACTIVE=0) and the active loop's without the lean path
    (GSLM_CG_LEAN=0), for 1 / 2 / 3 / 10 iterations with restarts every 1 / 2 / max_iter iterations (restarts take
    the flush -> matvec path);
  * the gamma and delta slots the consumers stored equal gslm_dot_finalize of the same partials to the last bit, and
    both are within 1e-12 relative of a float64 dot of the vectors read back;
  * the parameter block equals the scene arrays indexed by the list, and the inverse map inverts the list;
  * after the parameters change and evaluate() runs again, the next solve equals a fresh problem's bitwise;
  * the checked loop (check_every=True), which the lean path leaves alone, agrees with the full-layout loop.
The first and the second point are repeated on the layouts that scene does not have (LAYOUT_SCENES): the full SH-rest
group at SH 3 and SH 1 (45 and 9 floats per row, LMProblem's default sh_projection=False), SH 0 (a rest group of
width 0), a list that holds every Gaussian, and one shorter than a block of the per-Gaussian kernels.
The scenes, J^T b and each reference solve are computed once per module."""
import functools
import math

import numpy as np
import pytest
import torch

from gslm.cameras import orbit_cameras
from gslm.model import synthetic_gaussians

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, SH, W, H = 3001, 3, 64, 48
CASES = sorted({(m, r) for m in (1, 2, 3, 10) for r in (1, 2, m)})


def _camera():
    rng = np.random.default_rng(5)
    img = torch.from_numpy(rng.random((3, H, W), dtype=np.float32))
    return orbit_cameras(1, W, H, seed=1, images=[img])[0]


def _model(cam, seed=0, P=P, SH=SH):
    gen = torch.Generator().manual_seed(100 + seed)
    m = synthetic_gaussians(P, SH, seed=seed, s0=0.03)
    # a tenth of the Gaussians behind the camera (culled by the near plane): Pa < P
    c = cam.camera_center.float().cpu()
    f = -c / c.norm()  # the camera looks at the origin
    out = torch.randperm(P, generator=gen)[:P // 10 + 1]  # (301: the list then has an odd length, 2683)
    n = len(out)
    m._xyz.data[out] = c - f * (0.5 + torch.rand(n, 1, generator=gen)) + 0.3 * (torch.rand(n, 3, generator=gen) - 0.5)
    return m


def _problem(model, cam, sh_projection="auto"):
    from gslm.lm import LMProblem
    prob = LMProblem(model, [cam], torch.zeros(3), device=DEV, sh_projection=sh_projection)
    prob.evaluate()
    g = prob.rhs(prob.zeros())  # builds the row map
    return prob, g


class Scene:
    def __init__(self):
        self.cam = _camera().to(DEV)
        self.model = _model(_camera()).to(DEV)
        self.prob, self.g = _problem(self.model, self.cam)
        self.ids, self.Pa = self.prob.views[0].active_list(P, self.prob.stream)
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def scene():
    return Scene()


def _solve(prob, g, monkeypatch, active=True, lean=True, **kw):
    from gslm import lm
    monkeypatch.setenv("GSLM_CG_ACTIVE", "1" if active else "0")
    monkeypatch.setenv("GSLM_CG_LEAN", "1" if lean else "0")
    prob._lean_state = None
    x, info = lm.cgls_fused(prob, g, **kw)
    torch.cuda.synchronize()
    return x, info


_REF = {}


def _reference(case, monkeypatch):
    """x of the full-layout loop, once per case."""
    if case not in _REF:
        s = scene()
        x, _ = _solve(s.prob, s.g, monkeypatch, active=False, max_iter=case[0], restart_iter=case[1], check_every=False)
        _REF[case] = x.clone()
    return _REF[case]


def test_scene_shapes():
    s = scene()
    n_full = s.prob.layout.numel
    n_act = s.prob.active_view().layout.numel
    print(f"P {P}  Pa {s.Pa}  N {s.prob.views[0].N}  projected layout {n_full}  active layout {n_act}")
    assert s.prob.layout.rest_projected
    assert 0 < s.Pa < P
    for n in (n_full, n_act):
        assert n % 4 != 0 and n % 256 != 0, n
    assert s.Pa > 256  # more than one block of every per-Gaussian kernel


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"iter{c[0]}_restart{c[1]}")
def test_x_is_bitwise_the_full_layout_loops(case, monkeypatch):
    s = scene()
    ref = _reference(case, monkeypatch)
    kw = dict(max_iter=case[0], restart_iter=case[1], check_every=False)
    x, info = _solve(s.prob, s.g, monkeypatch, **kw)
    assert s.prob._lean_state is not None, "the lean loop was not taken"
    assert info["iters"] == case[0]
    d = float((x.double() - ref.double()).abs().max())
    print(f"{case}: max |x| {float(ref.abs().max()):.4e}  max |x - full-layout x| {d:.3e}")
    assert x.shape == ref.shape and torch.equal(x.view(torch.int32), ref.view(torch.int32))
    # the active loop without the lean path: the same groupings of every sum, so the same bits by construction
    xa, _ = _solve(s.prob, s.g, monkeypatch, lean=False, **kw)
    assert s.prob._lean_state is None
    assert torch.equal(x.view(torch.int32), xa.view(torch.int32))


@pytest.mark.parametrize("case", [(1, 1), (2, 2), (3, 2), (10, 10)], ids=lambda c: f"iter{c[0]}_restart{c[1]}")
def test_scalar_slots_hold_the_finalised_partials(case, monkeypatch):
    from gslm import _lib
    s = scene()
    _solve(s.prob, s.g, monkeypatch, max_iter=case[0], restart_iter=case[1], check_every=False)
    st = s.prob._lean_state
    sc = st["sc"]
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    for k, name in enumerate(("gamma", "delta")):
        part = st[name + "_partials"]
        _lib.check(_lib.lib.gslm_dot_finalize(part.data_ptr(), part.numel(), out.data_ptr() + 8 * k, s.prob.stream))
    torch.cuda.synchronize()
    lo = st["lo"]
    sv, pv, qv = (st[k][lo:].cpu().numpy().astype(np.float64) for k in ("s", "p", "q"))
    want = {"gamma": float(np.dot(sv, sv)), "delta": float(np.dot(pv, qv))}
    for k, name in enumerate(("gamma", "delta")):
        slot, fin = float(sc[st[name]]), float(out[k])
        print(f"{case} {name}: slot {slot!r} finalised {fin!r} float64 dot {want[name]!r} "
              f"rel {abs(slot - want[name]) / abs(want[name]):.2e}")
        assert np.float64(slot).view(np.int64) == np.float64(fin).view(np.int64)
        assert math.isfinite(slot) and slot > 0.0
        assert abs(slot - want[name]) <= 1e-12 * abs(want[name])
        assert abs(fin - want[name]) <= 1e-12 * abs(want[name])


def _block_arrays(prob, block, na):
    """The block's arrays (xyz, scale, rotation, opacity as float32; the clamp word as int32), carved as the library
    lays them out: each array starts at a multiple of 256 bytes."""
    out, o = [], 0
    for width, dt in ((3, torch.float32), (3, torch.float32), (4, torch.float32), (1, torch.float32), (1, torch.int32)):
        nbytes = 4 * width * na
        out.append(block[o:o + nbytes].view(dt).reshape(na, width))
        o = (o + nbytes + 255) // 256 * 256
    return out


def _check_block(prob, model):
    from gslm import _lib
    vr = prob.views[0]
    ids, na = vr.active_list(P, prob.stream)
    block, pos = vr.active_params(model, P, prob.stream)
    torch.cuda.synchronize()
    assert block.numel() >= _lib.lib.gslm_active_params_bytes(na)
    xyz, sc, rot, op, cw = _block_arrays(prob, block, na)
    idx = ids.long()
    for got, leaf in ((xyz, model._xyz), (sc, model._scaling), (rot, model._rotation), (op, model._opacity)):
        assert torch.equal(got.view(torch.int32), leaf.detach()[idx].reshape(na, -1).view(torch.int32))
    # the clamp word is the geometry's: gslm_view_flags reports it (bit 31: touches a tile, as every listed one does)
    flags = torch.zeros(P, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.gslm_view_flags(vr.geom.data_ptr(), P, flags.data_ptr(), prob.stream))
    torch.cuda.synchronize()
    assert bool((flags[idx] < 0).all())
    assert torch.equal(cw.reshape(-1), flags[idx] & 7)
    want = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    want[idx] = torch.arange(na, dtype=torch.int32, device=DEV)
    assert torch.equal(pos[:P], want)
    return block


def test_parameter_block_is_the_scene_indexed_by_the_list():
    s = scene()
    _check_block(s.prob, s.model)


def test_changed_parameters_rebuild_the_block(monkeypatch):
    s = scene()
    kw = dict(max_iter=3, restart_iter=3, check_every=False)
    model = _model(_camera()).to(DEV)
    prob, g = _problem(model, s.cam)
    x0, _ = _solve(prob, g, monkeypatch, **kw)
    b0 = _check_block(prob, model).clone()
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        model._opacity += 0.2 * torch.randn(P, 1, generator=gen).to(DEV)
        model._scaling += 0.05 * torch.randn(P, 3, generator=gen).to(DEV)
        model._rotation += 0.05 * torch.randn(P, 4, generator=gen).to(DEV)
    # written in place, before any forward: a block asked for now is already the new parameters'
    b1 = _check_block(prob, model)
    assert not torch.equal(b0, b1[:b0.numel()]) or b0.numel() != b1.numel()
    prob.evaluate()
    g = prob.rhs(g)
    x1, _ = _solve(prob, g, monkeypatch, **kw)
    assert prob._lean_state is not None
    _check_block(prob, model)
    fresh, gf = _problem(model, s.cam)
    xf, _ = _solve(fresh, gf, monkeypatch, **kw)
    assert torch.equal(g.view(torch.int32), gf.view(torch.int32))
    assert torch.equal(x1.view(torch.int32), xf.view(torch.int32))
    assert not torch.equal(x1, x0)
    xr, _ = _solve(fresh, gf, monkeypatch, active=False, **kw)
    assert torch.equal(x1.view(torch.int32), xr.view(torch.int32))


@pytest.mark.parametrize("host_checks", [False, True])
def test_checked_loop_is_unchanged(host_checks, monkeypatch):
    """check_every=True keeps its own loop (finalising launches, monitor): the active and the full-layout solve stop at
    the same iteration with the same code and the same x.  Their residual histories are float64 sums of the same
    exact products grouped differently (list order against scene order): n u = 51029 x 1.1e-16 = 5.7e-12 < 1e-11 of
    the summed magnitudes, which b^2 + 2 |x| |g| bounds (Cauchy-Schwarz, |s_k| <= |g|)."""
    s = scene()
    kw = dict(max_iter=10, restart_iter=10, check_every=True, host_checks=host_checks)
    xf, inf = _solve(s.prob, s.g, monkeypatch, active=False, **kw)
    xa, ina = _solve(s.prob, s.g, monkeypatch, **kw)
    assert s.prob._lean_state is None  # not the lean loop
    print(f"host_checks={host_checks}: iters {ina['iters']} stop {ina.get('stop')} residuals {ina['residuals']}")
    assert ina["iters"] == inf["iters"] and ina.get("stop") == inf.get("stop")
    assert torch.equal(xa.view(torch.int32), xf.view(torch.int32))
    assert len(ina["residuals"]) == len(inf["residuals"]) > 0
    b2 = float(s.prob.loss)
    tol = 1e-11 * (b2 + 2.0 * float(xf.double().norm()) * float(s.g.double().norm()))
    np.testing.assert_allclose(ina["residuals"], inf["residuals"], rtol=0, atol=tol)


# ------------------------------------------------------------------------------------------------ the other layouts
# name -> (P, SH degree, sh_projection, kind).  "tenth_behind": _model's scene (a tenth of the Gaussians culled by the
# near plane); "all_listed": a few translucent Gaussians in the middle of the frustum, each a pixel or more wide, so
# every one of them blends somewhere and no pixel saturates.
LAYOUT_SCENES = {
    "sh3_full": (3001, 3, False, "tenth_behind"),        # rest group 45 wide: the generic-width paths
    "sh1_full": (3001, 1, False, "tenth_behind"),        # 9 wide
    "sh0": (3001, 0, "auto", "tenth_behind"),            # 0 wide: two groups start at the same offset
    "all_listed_sh2_full": (300, 2, False, "all_listed"),  # Pa = P: the inverse map has no -1; 24 wide
    "short_list_sh3": (200, 3, "auto", "tenth_behind"),  # Pa < 256: one block, one delta partial
}
LAYOUT_CASES = [(1, 1), (3, 2), (10, 10)]


def _model_all_listed(P, sh, seed=0):
    from gslm.model import inverse_sigmoid
    gen = torch.Generator().manual_seed(200 + seed)
    m = synthetic_gaussians(P, sh, seed=seed, s0=0.05)
    m._xyz.data[:] = torch.rand(P, 3, generator=gen) - 0.5
    m._opacity.data[:] = inverse_sigmoid(0.1 + 0.2 * torch.rand(P, 1, generator=gen))
    return m


class LayoutScene:
    def __init__(self, name):
        self.P, self.sh, proj, kind = LAYOUT_SCENES[name]
        self.cam = _camera().to(DEV)
        if kind == "tenth_behind":
            model = _model(_camera(), P=self.P, SH=self.sh)
        else:
            model = _model_all_listed(self.P, self.sh)
        self.model = model.to(DEV)
        self.prob, self.g = _problem(self.model, self.cam, sh_projection=proj)
        self.ids, self.Pa = self.prob.views[0].active_list(self.P, self.prob.stream)
        self.ref = {}
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def layout_scene(name):
    return LayoutScene(name)


@pytest.mark.parametrize("name", list(LAYOUT_SCENES))
def test_layout_scene_shapes(name):
    s = layout_scene(name)
    lay = s.prob.layout
    act = s.prob.active_view()
    w, ng, tail = act._pack_args()
    print(f"{name}: P {s.P}  Pa {s.Pa}  N {s.prob.views[0].N}  layout {lay.numel}  active layout {act.layout.numel}  "
          f"widths {list(w)}")
    K = (s.sh + 1) ** 2
    assert list(w) == [3, 3, {"sh0": 0, "short_list_sh3": 3}.get(name, 3 * (K - 1)), 3, 4, 1] and tail == 12
    assert lay.rest_projected == (name == "short_list_sh3")
    if name == "all_listed_sh2_full":
        assert s.Pa == s.P and torch.equal(s.ids.cpu(), torch.arange(s.P, dtype=torch.int32))
    elif name == "short_list_sh3":
        assert 0 < s.Pa < min(s.P, 256)
    else:
        assert 256 < s.Pa < s.P


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda c: f"iter{c[0]}_restart{c[1]}")
@pytest.mark.parametrize("name", list(LAYOUT_SCENES))
def test_x_is_bitwise_the_full_layout_loops_on_every_layout(name, case, monkeypatch):
    """test_x_is_bitwise_the_full_layout_loops and the bitwise half of test_scalar_slots_hold_the_finalised_partials
    on LAYOUT_SCENES."""
    from gslm import _lib
    s = layout_scene(name)
    kw = dict(max_iter=case[0], restart_iter=case[1], check_every=False)
    if case not in s.ref:
        s.ref[case] = _solve(s.prob, s.g, monkeypatch, active=False, **kw)[0].clone()
        assert s.prob._lean_state is None
    ref = s.ref[case]
    x, info = _solve(s.prob, s.g, monkeypatch, **kw)
    st = s.prob._lean_state
    assert st is not None, "the lean loop was not taken"
    assert info["iters"] == case[0]
    d = float((x.double() - ref.double()).abs().max())
    print(f"{name} {case}: max |x| {float(ref.abs().max()):.4e}  max |x - full-layout x| {d:.3e}")
    assert x.shape == ref.shape and torch.equal(x.view(torch.int32), ref.view(torch.int32))
    # the gamma and delta slots: what gslm_dot_finalize makes of the partials behind them
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    for k, slot_name in enumerate(("gamma", "delta")):
        part = st[slot_name + "_partials"]
        _lib.check(_lib.lib.gslm_dot_finalize(part.data_ptr(), part.numel(), out.data_ptr() + 8 * k, s.prob.stream))
    torch.cuda.synchronize()
    assert st["delta_partials"].numel() == (s.Pa + 255) // 256
    for k, slot_name in enumerate(("gamma", "delta")):
        slot, fin = float(st["sc"][st[slot_name]]), float(out[k])
        print(f"{name} {case} {slot_name}: slot {slot!r} finalised {fin!r}")
        assert np.float64(slot).view(np.int64) == np.float64(fin).view(np.int64)
    xa, _ = _solve(s.prob, s.g, monkeypatch, lean=False, **kw)
    assert s.prob._lean_state is None
    assert torch.equal(x.view(torch.int32), xa.view(torch.int32))
