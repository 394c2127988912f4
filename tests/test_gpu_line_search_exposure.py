"""GPU: the trained exposure inside the loss blends (gslm_rasterize_loss_exposure / _slot_exposure / _sets_exposure)
and the line search that runs on them (LossEvaluator(fused_exposure=True), lm_step(val_exposure="fused")).

The exposure forms apply the camera's 3x4 map to the pixel's final colour in the blend's loss epilogue with
k_lm_residual_exposure's arithmetic, so their per-pixel residuals are the floats gslm_rasterize followed by
gslm_lm_residual_exposure gives; only the grouping of the double sum differs (per tile against per block).  Hence:
  a. X = [I | 0]: bitwise the plain forms;
  b. generic X: the forward + residual path's loss to 1e-12 of the loss (the bound test_loss_evaluator_agrees_with_problem
     holds the two groupings to);
  c. the shared binning: slot a bitwise the set's own exact render under its own X, the sets form bitwise the slot form;
  d. LossEvaluator: fused evaluate() against the forward path to 1e-12, evaluate_points bitwise fused evaluate();
  e. lm_step: union bitwise exact under val_exposure="fused", and the default path's losses to 1e-12.
Every X used is unsymmetric (a transposed read fails), the sets' X differ (a set reading another's fails), and the
exposed colour of the reference image has pixels below 0 and above 1 (both sides of the clamp) -- asserted below."""
import ctypes
import functools
import math

import pytest
import torch

from lm_exposure_ref import SCENES, exposure_scene
from scenes import BG_GENERIC, BG_ZERO, stack_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
BGS = {"zero": BG_ZERO, "generic": BG_GENERIC}
IDENT = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
# rows [i][j]: C_j = sum_i R_i X[i][j] + X[j][3].  XA sends dark red / bright blue below 0 in channel 0 and raises
# channel 2; the others are further unsymmetric maps around the identity
XA = [[1.20, 0.05, -0.03, -0.05], [-0.06, 0.90, 0.10, 0.02], [-0.50, -0.04, 1.30, 0.05]]
XB = [[0.85, -0.07, 0.04, 0.03], [0.09, 1.25, -0.45, -0.04], [-0.02, 0.06, 1.10, -0.06]]
XC = [[1.10, 0.30, -0.02, 0.06], [-0.40, 1.05, 0.03, -0.07], [0.05, -0.35, 0.95, 0.02]]
XD = [[0.95, 0.02, 0.25, -0.03], [0.04, 1.15, -0.30, 0.05], [-0.45, 0.03, 1.20, -0.02]]
XE = [[1.30, -0.05, 0.06, -0.08], [-0.35, 0.80, 0.02, 0.07], [0.03, 0.20, 1.00, 0.04]]
ROWS = (XA, XB, XC, XD, XE)
# the stack scene's image is nearly flat (0.42, 0.43, 0.54): channel 0 below 0, channel 1 inside, channel 2 above 1
XS = [[3.00, 0.05, -0.03, -1.20], [-0.06, 0.90, 0.10, 0.02], [-0.50, -0.04, 3.00, -0.60]]
TOL = 1e-12


def _unsymmetric(X):
    X = torch.as_tensor(X)
    return bool((X[:, :3] != X[:, :3].t()).any())


def _exposed(R, X):
    """The exposed colour before the clamp (k_lm_residual_exposure's order; only its sign and size are used here)."""
    X = torch.as_tensor(X, dtype=R.dtype, device=R.device)
    return torch.stack([((R[0] * X[0][j] + R[1] * X[1][j]) + R[2] * X[2][j]) + X[j][3] for j in range(3)])


def _assert_clamp_live(R, X, what):
    C = _exposed(R, X)
    assert bool((C < 0).any()) and bool((C > 1).any()), (what, float(C.min()), float(C.max()))


class Render:
    """One view of one parameter set: the evaluator's preprocess (depth order sorted), its pair count, and the
    workspaces of the loss blends.  The reference image (gslm_rasterize) is rendered on demand."""

    def __init__(self, model, cam, bg, gt=None, mask=None):
        from gslm import _lib
        from gslm._lib import check, lib
        from gslm.params import raw_gaussians
        self.model, self.g = model, raw_gaussians(model)
        self.vw = _lib.view_from_camera(cam, torch.tensor(bg), model.active_sh_degree)
        self.H, self.W, self.P = self.vw.image_height, self.vw.image_width, self.g.P
        self.gt = (cam.original_image if gt is None else gt).to(DEV).contiguous()
        self.mask = None if mask is None else mask.to(device=DEV, dtype=torch.float32).contiguous()
        self.h = _lib.stream_handle()
        self.geom = _lib.u8(lib.gslm_geom_bytes(self.P), DEV)
        self.order = torch.empty(max(self.P, 1), dtype=torch.int32, device=DEV)
        check(lib.gslm_preprocess_ordered(ctypes.byref(self.vw), ctypes.byref(self.g), self.geom.data_ptr(),
                                          self.geom.numel(), None, self.order.data_ptr(), 1, self.h),
              "gslm_preprocess_ordered")
        n = ctypes.c_int64(0)
        check(lib.gslm_num_rendered(self.geom.data_ptr(), self.P, ctypes.byref(n), self.h), "gslm_num_rendered")
        self.N = int(n.value)
        self.binning = _lib.u8(lib.gslm_binning_bytes(self.N, self.H, self.W), DEV)
        self.scr = torch.empty(lib.gslm_loss_scratch_bytes(self.H, self.W) // 8 + 1, dtype=torch.float64, device=DEV)
        self._image = None
        self.xa = XA  # the case's first exposure: both sides of the clamp live on its image

    def _mp(self):
        return None if self.mask is None else self.mask.data_ptr()

    def loss(self, X=None, start=0.0, accumulate=0):
        """gslm_rasterize_loss (X None) or gslm_rasterize_loss_exposure into a double holding `start`."""
        from gslm._lib import check, lib
        out = torch.full((1,), start, dtype=torch.float64, device=DEV)
        a = (ctypes.byref(self.vw), self.P, self.geom.data_ptr(), self.binning.data_ptr(), self.binning.numel(), self.N,
             self.gt.data_ptr(), self._mp())
        b = (self.scr.data_ptr(), self.scr.numel() * 8, out.data_ptr(), accumulate, self.h)
        if X is None:
            check(lib.gslm_rasterize_loss(*a, *b), "gslm_rasterize_loss")
        else:
            Xd = torch.tensor(X, dtype=torch.float32, device=DEV).contiguous()
            check(lib.gslm_rasterize_loss_exposure(*a, Xd.data_ptr(), *b), "gslm_rasterize_loss_exposure")
        return float(out)

    def image(self):
        from gslm import _lib
        from gslm._lib import check, lib
        if self._image is None:
            ws = _lib.u8(lib.gslm_image_bytes(self.H, self.W), DEV)
            R = torch.empty(3, self.H, self.W, device=DEV)
            check(lib.gslm_rasterize(ctypes.byref(self.vw), self.P, self.geom.data_ptr(), self.binning.data_ptr(),
                                     self.binning.numel(), self.N, ws.data_ptr(), ws.numel(), R.data_ptr(), None, self.h),
                  "gslm_rasterize")
            self._image = R
        return self._image

    def reference(self, X, start=0.0, accumulate=0):
        """The forward's image through gslm_lm_residual_exposure in its loss-only mode."""
        from gslm._lib import check, lib
        R = self.image()
        Xd = torch.tensor(X, dtype=torch.float32, device=DEV).contiguous()
        out = torch.full((1,), start, dtype=torch.float64, device=DEV)
        scr = torch.empty(lib.gslm_exposure_scratch_bytes(self.H, self.W) // 8, dtype=torch.float64, device=DEV)
        check(lib.gslm_lm_residual_exposure(self.H, self.W, R.data_ptr(), self.gt.data_ptr(), self._mp(), Xd.data_ptr(),
                                            None, None, None, None, scr.data_ptr(), scr.numel() * 8, out.data_ptr(),
                                            accumulate, self.h), "gslm_lm_residual_exposure")
        return float(out)


def _gt(H, W, seed=31):
    return torch.rand(3, H, W, generator=torch.Generator().manual_seed(seed))


def _nothing_scene():
    """sh1_33x17 with every Gaussian moved behind the camera: the view renders nothing (N = 0)."""
    model, cams = exposure_scene("sh1_33x17", masked=False)
    c = cams[0].camera_center.float()
    with torch.no_grad():
        model._xyz.copy_(2.0 * c + 0.05 * model._xyz)  # the camera looks at the origin from c
    return model, cams[0]


@functools.lru_cache(maxsize=None)
def _renders():
    """name -> Render: both scenes masked and unmasked under both backgrounds, one 16x16 tile, a view of nothing."""
    out = {}
    for name in SCENES:
        for masked in (False, True):
            for bgname, bg in BGS.items():
                model, cams = exposure_scene(name, masked=masked)
                v = 1 if masked else 0  # the second view too
                out[f"{name}-{'masked' if masked else 'plain'}-{bgname}"] = Render(
                    model.to(DEV), cams[v].to(DEV), bg, mask=cams[v].alpha_mask if masked else None)
    model, cam = stack_scene(129, 16, 16)
    out["stack129_16x16"] = Render(model.to(DEV), cam.to(DEV), BG_GENERIC, gt=_gt(16, 16))
    out["stack129_16x16"].xa = XS
    model, cam = _nothing_scene()
    out["nothing_33x17"] = Render(model.to(DEV), cam.to(DEV), BG_GENERIC)
    return out


RENDERS = [f"{n}-{m}-{b}" for n in SCENES for m in ("plain", "masked") for b in BGS] + ["stack129_16x16", "nothing_33x17"]


def test_the_exposures_are_unsymmetric_and_distinct():
    for X in ROWS + (XS,):
        assert _unsymmetric(X)
    for a in range(len(ROWS)):
        for b in range(a):
            assert ROWS[a] != ROWS[b]


def test_the_cases_cover_their_edges():
    r = _renders()
    assert r["nothing_33x17"].N == 0 and r["nothing_33x17"].P > 0
    assert (r["stack129_16x16"].H, r["stack129_16x16"].W) == (16, 16)
    assert all(r[k].N > 0 for k in RENDERS if k != "nothing_33x17")
    assert any(r[k].mask is not None and bool((r[k].mask == 0).any()) for k in RENDERS)


# ---------------------------------------------------------------- a. identity
@pytest.mark.parametrize("name", RENDERS)
def test_identity_exposure_is_the_plain_loss(name):
    r = _renders()[name]
    plain = r.loss()
    assert r.loss(IDENT) == plain and plain > 0
    assert r.loss(IDENT, start=3.5, accumulate=1) == r.loss(start=3.5, accumulate=1)


# ---------------------------------------------------------------- b. generic X
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name", RENDERS)
def test_generic_exposure_matches_forward_plus_residual(name, accumulate):
    r = _renders()[name]
    _assert_clamp_live(r.image(), r.xa, name)
    for X in (r.xa, XB):
        scale = r.reference(X)  # the loss itself: the bound's unit with and without a start value
        ref = r.reference(X, start=2.25, accumulate=accumulate)
        got = r.loss(X, start=2.25, accumulate=accumulate)
        print(f"{name} accumulate={accumulate}: blend {got!r} forward+residual {ref!r} of the loss "
              f"{abs(got - ref) / scale:.2e}")
        assert abs(got - ref) <= TOL * scale, (name, got, ref)
        # the exposure matters to the loss, and so does its orientation
        assert abs(got - r.loss(start=2.25, accumulate=accumulate)) > 1e-3 * scale
        Xt = [[X[j][i] for j in range(3)] + [X[i][3]] for i in range(3)]
        assert abs(r.reference(Xt) - scale) > 1e-6 * scale
    if accumulate == 0:
        assert r.loss(r.xa, start=7.0) == r.loss(r.xa)  # the start value is overwritten


# ---------------------------------------------------------------- c. the shared binning
def _walk(model, n=6, keep_row=None, seed=5, after=None):
    """n parameter sets along a random walk of every leaf the step moves and of the exposure rows (row keep_row left
    alone): snapshots with their exposure.  after(a): called with the model at set a."""
    from gslm.lm import param_snapshot
    gen = torch.Generator().manual_seed(seed)
    sets = []
    for a in range(n):
        with torch.no_grad():
            for leaf, sd in (("_features_dc", 0.1), ("_features_rest", 0.02), ("_scaling", 0.15), ("_rotation", 0.2),
                             ("_opacity", 0.5)):
                t = getattr(model, leaf)
                t.add_((sd * torch.randn(t.shape, generator=gen)).to(t.device))
            d = (0.02 * torch.randn(model._exposure.shape, generator=gen)).to(model._exposure.device)
            if keep_row is not None:
                d[keep_row] = 0
            model._exposure.add_(d)
        sets.append(param_snapshot(model, exposure=True))
        if after is not None:
            after(a)
    return sets


def _assert_sets_differ(sets, rows):
    for a in range(len(sets)):
        for b in range(a):
            for leaf in ("_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
                assert not torch.equal(getattr(sets[a], leaf), getattr(sets[b], leaf))
            for r in rows:
                assert not torch.equal(sets[a]._exposure[r], sets[b]._exposure[r])
    for s in sets:
        for r in rows:
            assert _unsymmetric(s._exposure[r].cpu())


@pytest.mark.parametrize("name,bgname,masked", [("sh1_33x17", "generic", True), ("sh3_40x33", "zero", False)])
def test_union_slots_equal_the_sets_own_renders(name, bgname, masked):
    """One view, six sets: slot a of the union binning under set a's X is that set's exact render under its X; the sets
    form is the slot form for every group size and start; a slot past the binning's set count gives NaN."""
    from gslm import _lib
    from gslm._lib import check, lib
    from gslm.lm import LossEvaluator
    model, cams = exposure_scene(name, masked=masked, rows=(XA, XB))
    model, cam, bg = model.to(DEV), cams[0].to(DEV), BGS[bgname]
    ev = LossEvaluator(model, [cam], torch.tensor(bg), device=DEV, batch=1, streams=1, train_exposure=True,
                       fused_exposure=True)
    sets = _walk(model)
    _assert_sets_differ(sets, [0])
    mask = cam.alpha_mask if masked else None
    exact = []
    for a, st in enumerate(sets):
        r = Render(st, cam, bg, mask=mask)
        _assert_clamp_live(r.image(), st._exposure[0], (name, a))
        exact.append(r.loss(st._exposure[0].tolist()))
    got = [float(x) for x in ev.evaluate_points(sets)]
    assert got == exact
    assert len(set(exact)) == 6
    # the evaluator's union binning of the view (built for 6 sets), through the entry points directly
    sl, binning, vw = ev.uslots[0][0], ev.ubins[0], ev.views[0]
    P, N, sb = model._xyz.shape[0], ev.union_counts[0], sl["geoms"][0].numel()
    H, W = vw.image_height, vw.image_width
    assert N > 0
    mp = None if ev.masks[0] is None else ev.masks[0].data_ptr()
    scr = ev.loss_scratch[0]
    h = _lib.stream_handle()
    one = torch.zeros(1, dtype=torch.float64, device=DEV)

    def slot(a, X, n_sets=6, geom=None):
        check(lib.gslm_rasterize_loss_slot_exposure(
            ctypes.byref(vw), P, sl["geoms"][a if geom is None else geom].data_ptr(), sb, binning.data_ptr(),
            binning.numel(), N, a, n_sets, ev.gts[0].data_ptr(), mp, X.data_ptr(), scr.data_ptr(), scr.numel() * 8,
            one.data_ptr(), 0, h), "gslm_rasterize_loss_slot_exposure")
        return float(one)

    xs = [st._exposure[0].contiguous() for st in sets]
    assert [slot(a, xs[a]) for a in range(6)] == exact
    assert slot(2, xs[3]) != exact[2]  # another set's X is another loss
    ident = torch.tensor(IDENT, device=DEV)
    for a in (0, 5):  # X = [I | 0]: the plain slot form, bitwise
        check(lib.gslm_rasterize_loss_slot(ctypes.byref(vw), P, sl["geoms"][a].data_ptr(), sb, binning.data_ptr(),
                                           binning.numel(), N, a, 6, ev.gts[0].data_ptr(), mp, scr.data_ptr(),
                                           scr.numel() * 8, one.data_ptr(), 0, h), "gslm_rasterize_loss_slot")
        assert slot(a, ident) == float(one)
    for a in (6, 7):  # past the six sets the masks were built for
        assert math.isnan(slot(a, xs[0], n_sets=8, geom=0))

    def group(first, n, exposure=True):
        sscr = torch.empty(lib.gslm_loss_sets_scratch_bytes(n, H, W) // 8 + 1, dtype=torch.float64, device=DEV)
        out = torch.full((n,), 1.5, dtype=torch.float64, device=DEV)
        gg = (ctypes.c_void_p * n)(*[sl["geoms"][min(first + a, 5)].data_ptr() for a in range(n)])
        lp = (ctypes.c_void_p * n)(*[out.data_ptr() + 8 * a for a in range(n)])
        a0 = (ctypes.byref(vw), P, gg, n, first, sb, binning.data_ptr(), binning.numel(), N, ev.gts[0].data_ptr(), mp)
        a1 = (sscr.data_ptr(), sscr.numel() * 8, lp, 0, h)
        if exposure is True:
            xp = (ctypes.c_void_p * n)(*[xs[min(first + a, 5)].data_ptr() for a in range(n)])
            check(lib.gslm_rasterize_loss_sets_exposure(*a0, xp, *a1), "gslm_rasterize_loss_sets_exposure")
        elif exposure == "identity":
            xp = (ctypes.c_void_p * n)(*[ident.data_ptr()] * n)
            check(lib.gslm_rasterize_loss_sets_exposure(*a0, xp, *a1), "gslm_rasterize_loss_sets_exposure")
        else:
            check(lib.gslm_rasterize_loss_sets(*a0, *a1), "gslm_rasterize_loss_sets")
        return [float(x) for x in out.cpu()]

    for first, n in ((0, 1), (0, 2), (0, 6), (3, 1), (4, 2), (1, 5), (2, 3)):
        assert group(first, n) == exact[first:first + n], (first, n)
    for first, n in ((0, 8), (5, 3)):  # groups reaching past the recorded six sets: NaN there, the slot form's before
        got = group(first, n)
        assert got[:6 - first] == exact[first:6] and all(math.isnan(x) for x in got[6 - first:]), (first, n, got)
    for first, n in ((0, 6), (2, 2), (0, 8)):  # X = [I | 0]: the plain sets form, bitwise (NaN slots included)
        a, b = group(first, n, "identity"), group(first, n, False)
        assert all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(a, b)), (first, n, a, b)


# ---------------------------------------------------------------- d. LossEvaluator
def _five_views(name, bgname, masked):
    """Five views; views 1 and 4 share camera row 1, row 3 is the camera the walk leaves alone."""
    model, cams = exposure_scene(name, masked=False, n_views=5, rows=ROWS)
    if masked:
        from scenes import lm_bg_mask
        for i in (0, 2, 4):  # masked and unmasked views in one evaluator
            cams[i].alpha_mask = lm_bg_mask(name, seed=i)
    model.exposure_mapping[cams[4].image_name] = 1
    return model.to(DEV), [c.to(DEV) for c in cams], torch.tensor(BGS[bgname])


@pytest.mark.parametrize("name,bgname,masked", [("sh1_33x17", "zero", True), ("sh3_40x33", "generic", True),
                                                ("sh3_40x33", "zero", False)])
def test_fused_evaluate_matches_the_forward_path(name, bgname, masked):
    from gslm.lm import LossEvaluator
    model, cams, bg = _five_views(name, bgname, masked)
    fwd = LossEvaluator(model, cams, bg, device=DEV, train_exposure=True)
    fused = LossEvaluator(model, cams, bg, device=DEV, batch=2, train_exposure=True, fused_exposure=True)
    assert fused.exp_idx == [0, 1, 2, 3, 1]
    C = torch.cat([_exposed(Render(model, c, tuple(bg.tolist())).image(), model._exposure[fused.exp_idx[i]]).flatten()
                   for i, c in enumerate(cams)])
    assert bool((C < 0).any()) and bool((C > 1).any())  # both sides of the clamp among the evaluator's views
    a, b = float(fwd.evaluate()), float(fused.evaluate())
    print(f"{name} {bgname}: forward {a!r} fused {b!r} rel {abs(a - b) / a:.2e}")
    assert abs(a - b) <= TOL * a
    assert float(fused.evaluate()) == b  # cached depth orders: the same loss
    assert abs(float(LossEvaluator(model, cams, bg, device=DEV).evaluate()) - a) > 1e-3 * a
    with torch.no_grad():  # a row moves: the next evaluation reads it on the device
        model._exposure[1, 0, 3] += 0.05
    a2, b2 = float(fwd.evaluate()), float(fused.evaluate())
    assert b2 != b and abs(a2 - b2) <= TOL * a2


@pytest.mark.parametrize("group", [1, 8])
@pytest.mark.parametrize("name,bgname,masked", [("sh1_33x17", "generic", True), ("sh3_40x33", "zero", False)])
def test_evaluate_points_equal_fused_evaluate(name, bgname, masked, group, monkeypatch):
    """5 views at batch 2 (both slot sets and a short last batch), per-set and all-sets blends."""
    from gslm.lm import LossEvaluator
    monkeypatch.setenv("GSLM_LOSS_SET_GROUP", str(group))
    model, cams, bg = _five_views(name, bgname, masked)
    kw = dict(device=DEV, batch=2, streams=2, train_exposure=True, fused_exposure=True)
    ev_x, ev_u = LossEvaluator(model, cams, bg, **kw), LossEvaluator(model, cams, bg, **kw)
    assert ev_u.loss_sets == group
    exact = []
    sets = _walk(model, keep_row=3, after=lambda a: exact.append(float(ev_x.evaluate())))
    _assert_sets_differ(sets, [0, 1, 2, 4])
    assert all(torch.equal(s._exposure[3], sets[0]._exposure[3]) for s in sets)  # the row no point moves
    got = [float(x) for x in ev_u.evaluate_points(sets)]
    assert got == exact and len(set(exact)) == 6
    assert [float(x) for x in ev_u.evaluate_points(sets[1:4])] == exact[1:4]
    # two views of one camera row: moving that row in one set alone moves that set's loss alone
    with torch.no_grad():
        sets[2]._exposure[1, 2, 0] += 0.1
    moved = [float(x) for x in ev_u.evaluate_points(sets)]
    assert moved[2] != exact[2] and moved[:2] + moved[3:] == exact[:2] + exact[3:]


def test_eight_sets_in_one_pass(monkeypatch):
    """All eight slots of a binning live (k_render_loss_sets<8>): the one-pass blend equals the per-set blends and the
    fused evaluate() at each set."""
    from gslm.lm import LossEvaluator
    model, cams, bg = _five_views("sh1_33x17", "generic", True)
    kw = dict(device=DEV, batch=2, streams=2, train_exposure=True, fused_exposure=True)
    ev_x = LossEvaluator(model, cams, bg, **kw)
    exact = []
    sets = _walk(model, n=8, seed=6, after=lambda a: exact.append(float(ev_x.evaluate())))
    _assert_sets_differ(sets, [0, 1, 2, 3])
    monkeypatch.setenv("GSLM_LOSS_SET_GROUP", "8")
    ev8 = LossEvaluator(model, cams, bg, **kw)
    assert ev8.loss_sets == 8
    assert [float(x) for x in ev8.evaluate_points(sets)] == exact
    assert [float(x) for x in ev_x.evaluate_points(sets)] == exact and len(set(exact)) == 8


def test_evaluator_option_errors():
    from gslm.lm import LossEvaluator, param_snapshot
    model, cams, bg = _five_views("sh1_33x17", "generic", False)
    with pytest.raises(ValueError):
        LossEvaluator(model, cams, bg, device=DEV, fused_exposure=True)
    with pytest.raises(ValueError):
        LossEvaluator(model, cams, bg, device=DEV, train_exposure=True, fused_exposure=True, device_count=True)
    with pytest.raises(ValueError):  # as before: no exposure in the union evaluator without fused_exposure
        LossEvaluator(model, cams, bg, device=DEV, train_exposure=True).evaluate_points([param_snapshot(model, exposure=True)])
    ev = LossEvaluator(model, cams, bg, device=DEV, batch=2, train_exposure=True, fused_exposure=True)
    with pytest.raises(ValueError):
        ev.evaluate_points([])
    with pytest.raises(ValueError):
        ev.evaluate_points([param_snapshot(model)])  # no _exposure
    good = param_snapshot(model, exposure=True)
    for bad in (good._exposure.double(), good._exposure[:2].clone(), good._exposure.cpu(),
                good._exposure.transpose(1, 2).contiguous().transpose(1, 2), good._exposure.tolist()):
        st = param_snapshot(model, exposure=True)
        st._exposure = bad
        with pytest.raises(ValueError):
            ev.evaluate_points([good, st])
    assert float(ev.evaluate_points([good])[0]) == float(ev.evaluate())


# ---------------------------------------------------------------- e. lm_step
def _run_step(**kw):
    from test_gpu_lm_exposure import _step_scene
    from gslm.lm import clear_val_cache, lm_step
    model, cams = _step_scene()
    out = lm_step(model, cams[:2], cams, torch.tensor(BG_GENERIC), max_iter=5, restart_iter=5, train_exposure=True,
                  val_at_start=True, cache_val=False, val_batch=2, **kw)
    clear_val_cache()
    leaves = [getattr(model, k).detach().clone() for k in ("_exposure", "_features_dc", "_features_rest", "_scaling",
                                                           "_rotation", "_opacity", "_xyz")]
    return out, leaves


def test_lm_step_fused_union_equals_fused_exact_and_the_default():
    """The batch is cameras 0 and 1; the validation set adds camera 2, whose row the step does not move."""
    (u, pu), (x, px), (d, pd) = (_run_step(val_exposure="fused", line_search="union"),
                                 _run_step(val_exposure="fused", line_search="exact"), _run_step())
    assert u["line_search"] == "union" and x["line_search"] == "exact" and d["line_search"] == "exact"
    assert u["union_pairs"] > 0
    assert u["trace"] == x["trace"] and len(u["trace"]) == 6
    assert u["best_alpha"] == x["best_alpha"]
    assert u["final_val_loss"] == x["final_val_loss"] and u["val_start_loss"] == x["val_start_loss"]
    for a, b in zip(pu, px):
        assert torch.equal(a, b)
    # against the forward + residual validation: the same losses up to the grouping of the sum
    for (a0, l0), (a1, l1) in zip(u["trace"], d["trace"]):
        print(f"alpha {a0}: fused {l0!r} forward {l1!r} rel {abs(l0 - l1) / l1:.2e}")
        assert a0 == a1 and abs(l0 - l1) <= TOL * l1
    assert abs(u["final_val_loss"] - d["final_val_loss"]) <= TOL * d["final_val_loss"]
    assert abs(u["val_start_loss"] - d["val_start_loss"]) <= TOL * d["val_start_loss"]
    best, second = sorted(v for _, v in d["trace"])[:2]
    assert second - best > 1e-9 * best, (best, second)  # the scene separates the two best points
    assert u["best_alpha"] == d["best_alpha"]
    for a, b in zip(pu, pd):
        assert torch.equal(a, b)
    assert u["final_val_loss"] < u["val_start_loss"]


def test_lm_step_option_errors():
    from gslm.lm import lm_step
    model, cams = exposure_scene("sh1_33x17")
    model, cams, bg = model.to(DEV), [c.to(DEV) for c in cams], torch.tensor(BG_GENERIC)
    kw = dict(max_iter=1, restart_iter=1, cache_val=False)
    with pytest.raises(ValueError):
        lm_step(model, cams, cams, bg, val_exposure="fused", **kw)
    with pytest.raises(ValueError):
        lm_step(model, cams, cams, bg, train_exposure=False, val_exposure="fused", **kw)
    for bad in ("union", "Fused", "", None):
        with pytest.raises(ValueError):
            lm_step(model, cams, cams, bg, train_exposure=True, val_exposure=bad, **kw)
        with pytest.raises(ValueError):
            lm_step(model, cams, cams, bg, val_exposure=bad, **kw)
