"""GPU: the LM row map refines the list's quadrant masks to the visits some pixel blends (k_quad_live, forward.hip;
GSLM_LIVE_MASKS, default on).

Scenes (tests/live_mask_scene.py): 16x16, 17x9 (partial tiles, quadrants wholly outside the image) and 48x40, with
per-tile list lengths 1, 63, 64, 65, 127, 128, 129, 300 (and 20), Gaussians that touch one tile each, a nonzero
background and fractional alpha masks with a block of zeros.  Checked:
  * the refined masks equal, bit for bit, a numpy replay of the definition from the library's own records, list and
    n_contrib (gslm_inspect, gslm_inspect_list).  Share of (entry, pixel) pairs excluded because their alpha lies
    within 2e-6 (relative) of 1/255 or their power within 1e-6 of zero, where the replay's float64 exp could decide
    differently from the kernels' hardware exp2: ZERO for every committed seed (asserted);
  * the switch on against off: J^T b, A v, J v alone, the exposure product and the SSIM product on the projected,
    the full SH 3 and the SH 0 layouts -- `==` element for element on the full vectors, and `==` after scattering
    to the full layout on the active list;
  * head counts: on <= off, on == the replay's exact count, and the active list == the Gaussians that are some
    pixel's contributor;
  * planted cases: an entry below 1/255 at every pixel owns no row and leaves the list; behind pixels that stopped
    early, entries that reach only those pixels lose their visits while the entries at or past a quadrant's bound
    keep their bits; an image with nothing visible;
  * the row map rebuilt on the same binning: the same masks, hscan and slots;
  * three CG iterations and one LM step, on against off: `==` on the full path (GSLM_CG_ACTIVE=0) and `==` on the
    active list, whose Pa differs; one batched two-view problem and its union list likewise.
alpha == 1/255 exactly: test_alpha_on_the_threshold.  power > 0: the case 48x40_pow writes indefinite conics into
the render records between the preprocess and the binning (live_mask_scene.planted_conics); it runs through the replay,
the head counts, the products and the solves.  The forward's blend reads the masks only of a list it has just rebuilt
(every forward entry point runs the binning first), so there is no
forward on a refined list to compare."""
import contextlib
import copy
import functools
import os

import numpy as np
import pytest
import torch

import live_mask_scene as lms
import multiview_scene as ms
from gslm import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BG = (0.2, 0.5, 0.9)


@contextlib.contextmanager
def switch(on, **extra):
    env = {"GSLM_LIVE_MASKS": "1" if on else "0", **extra}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def same(a, b):
    """Element for element `==` (-0.0 against +0.0 is equal)."""
    return a.shape == b.shape and bool((a == b).all())


class Built:
    """One geometry under one switch state: a forward, J^T b (which builds the row map) and copies of the list."""

    def __init__(self, model, cam, on, layout="auto", ssim=False, exposure=False, antialiasing=False, conics=None):
        from gslm.lm import LMProblem
        self.on = on
        self.model = copy.deepcopy(model).to(DEV)
        self.cam = copy.deepcopy(cam).to(DEV)
        if exposure:
            from lm_exposure_ref import X0, set_exposures
            set_exposures(self.model, [self.cam], rows=(X0,))
        self.P = self.model._xyz.shape[0]
        with switch(on):
            self.prob = LMProblem(self.model, [self.cam], torch.tensor(BG), device=DEV, sh_projection=layout,
                                  ssim=ssim, train_exposure=exposure)
            self.prob.views[0].view.antialiasing = int(antialiasing)
            self.evaluate(conics)
            self.g = self.prob.rhs(self.prob.zeros())
            self.vr = self.prob.views[0]
            ids, self.Pa = self.vr.active_list(self.P, self.prob.stream)
            self.active = ids.clone().cpu().long().numpy()
            self.read()
        torch.cuda.synchronize()

    def evaluate(self, conics):
        """prob.evaluate(); conics = (ids, abc): those Gaussians' conics are written over their render records between
        the preprocess and the binning (the geometry workspace is the caller's: 16 floats per Gaussian, x y a b | c
        opacity ...), so the binning, the forward's n_contrib and the row map all see them."""
        from gslm import lm
        if conics is None:
            self.prob.evaluate()
            return
        ids, abc = conics
        orig = lm.lib.gslm_rasterize

        def rasterize(*args):
            rec = self.prob.views[0].geom[:self.P * 64].view(torch.float32).view(self.P, 16)
            rec[ids.to(DEV), 2:5] = abc.to(DEV)
            return orig(*args)

        lm.lib.gslm_rasterize = rasterize
        try:
            self.prob.evaluate()
        finally:
            lm.lib.gslm_rasterize = orig

    def read(self):
        vr, P, st = self.vr, self.P, self.prob.stream
        H, W, N = vr.H, vr.W, vr.N
        self.N = N
        ntiles = ((W + 15) // 16) * ((H + 15) // 16)
        i32 = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device=DEV)
        pl, rg, tiles, nc, goff, hscan = i32(N), i32(2 * ntiles), i32(P), i32(H * W), i32(P), i32(N + 1)
        rec = torch.zeros(max(P, 1) * 12, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib.gslm_inspect(vr.geom.data_ptr(), P, vr.binning.data_ptr(), N, H, W, vr.image.data_ptr(),
                                         pl.data_ptr(), rg.data_ptr(), tiles.data_ptr(), None, nc.data_ptr(),
                                         rec.data_ptr(), st))
        _lib.check(_lib.lib.gslm_inspect_rowmap(vr.geom.data_ptr(), P, N, vr.scratch.data_ptr(), vr.scratch.numel(),
                                                goff.data_ptr(), hscan.data_ptr(), st))
        words, slots = vr.list_words(st)
        torch.cuda.synchronize()
        u32 = lambda t, n: t[:n].cpu().numpy().view(np.uint32)
        self.words, self.slots = u32(words, N), u32(slots, N)
        self.ids, self.ranges = u32(pl, N).astype(np.int64), u32(rg, 2 * ntiles).astype(np.int64).reshape(-1, 2)
        self.tiles, self.n_contrib = u32(tiles, P), u32(nc, H * W).astype(np.int64).reshape(H, W)
        self.hscan = u32(hscan, N + 1).astype(np.int64)
        self.records = rec[:P * 12].cpu().numpy().reshape(P, 12)
        assert np.array_equal(self.words & 0x0FFFFFFF, self.ids)
        self.masks = (self.words >> 28).astype(np.uint8)
        self.heads = int(self.hscan[N]) if N else 0  # (nothing rendered: no row map is built, hscan is not written)

    def random_v(self, seed):
        lay = self.prob.layout
        v = torch.randn(lay.numel, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        a, b = lay.offsets["xyz"]
        v[a:b] = 0
        if not self.prob.train_exposure:
            a, b = lay.offsets["exposure"]
            v[a:b] = 0
        return v

    def matvec(self, v):
        with switch(self.on):
            return self.prob.matvec(v.clone(), self.prob.zeros())

    def active_matvec(self, v):
        """A v through the active list, scattered back to the full layout (v zeroed off the list first)."""
        with switch(self.on):
            act = self.prob.active_view()
            y = act.matvec(act.pack(v), act.zeros())
            return act.unpack(y), act.unpack(act.pack(v))


@functools.lru_cache(maxsize=None)
def built(case, on, layout="auto", ssim=False, exposure=False):
    m, cam, kinds = lms.tile_scene(case)
    return Built(m, cam, on, layout, ssim, exposure, conics=lms.planted_conics(kinds) if case == "48x40_pow" else None)


@functools.lru_cache(maxsize=None)
def replayed(case):
    b = built(case, True)
    W, H = lms.CASES[case][:2]
    return lms.replay(b.records, b.ids, b.ranges, b.n_contrib, W, H)


@pytest.mark.parametrize("case", list(lms.CASES))
def test_masks_equal_the_replay(case):
    on, off = built(case, True), built(case, False)
    W, H, lengths = lms.CASES[case][:3]
    # the scene is what the case names, on the library's own binning; the geometry does not depend on the switch
    assert tuple(int(b - a) for a, b in on.ranges) == tuple(lengths)
    assert int((on.tiles != 1).sum()) == 0
    for k in ("ids", "ranges", "n_contrib", "records"):
        assert np.array_equal(getattr(on, k), getattr(off, k)), k
    r = replayed(case)
    print(f"{case}: pairs {r['pairs']}  excluded (within the margins) {r['near']} = "
          f"{r['near'] / max(r['pairs'], 1):.1e}  power > 0 pairs {r['power_pos']}  pairs past n_contrib that pass "
          f"power and alpha {r['stopped']}")
    assert r["near"] == 0
    if case == "48x40_pow":  # the planted conics: pairs the passes skip for `power > 0`, in the written records
        ids, abc = lms.planted_conics(lms.tile_scene(case)[2])
        assert np.array_equal(on.records[ids.numpy(), 2:5], abc.numpy()) and r["power_pos"] > 1000
    live, below = r["live"], r["below"]
    # the binning's mask is a reach test: it holds every live quadrant
    assert np.array_equal(off.masks & live & below, live & below)
    want = off.masks & (live | (~below & 0xF))  # bits at or past the quadrant's bound stay as they were
    bad = np.nonzero(on.masks != want)[0]
    assert bad.size == 0, [(int(k), int(on.masks[k]), int(want[k]), int(off.masks[k])) for k in bad[:8]]
    visits_off = int(np.unpackbits(off.masks & below).sum())
    visits_on = int(np.unpackbits(on.masks & below).sum())
    print(f"{case}: wave-visits below the bounds {visits_off} -> {visits_on}")
    assert visits_on <= visits_off


@pytest.mark.parametrize("case", list(lms.CASES))
def test_head_counts(case):
    on, off = built(case, True), built(case, False)
    r = replayed(case)
    head = (r["live"] & r["below"]) != 0
    print(f"{case}: N {on.N}  heads off {off.heads}  on {on.heads}  replay {int(head.sum())}  Pa off {off.Pa} on {on.Pa}")
    assert on.heads <= off.heads
    assert on.heads == int(head.sum())
    assert np.array_equal(on.active, np.unique(on.ids[head]))
    assert set(on.active.tolist()) <= set(off.active.tolist())


@pytest.mark.parametrize("case", ["48x40", "48x40_sh0", "16x16_len129"])
def test_planted_cases(case):
    on, off = built(case, True), built(case, False)
    r = replayed(case)
    kinds = np.array(lms.tile_scene(case)[2])
    act_on, act_off = set(on.active.tolist()), set(off.active.tolist())
    faint, hidden, wall = (np.nonzero(kinds == k)[0] for k in ("faint", "hidden", "wall"))
    assert faint.size and hidden.size and wall.size
    # below 1/255 at every pixel: no row, off the list (the binning's reach test had given them quadrants)
    assert not (set(faint.tolist()) & act_on)
    print(f"{case}: faint entries on the list with the switch off {len(set(faint.tolist()) & act_off)} of {faint.size}")
    # behind the wall: alpha and power pass at the stopped pixels only.  (Where the wall's spot lies below the image --
    # the 48x40 scenes' last tile row -- the entries behind it reach no pixel at all and were no heads before either.)
    assert r["stopped"] > 0
    H = lms.CASES[case][1]
    seen = hidden[on.records[hidden, 1] < H - 1]
    assert seen.size >= 10
    assert not (set(hidden.tolist()) & act_on) and set(seen.tolist()) <= act_off
    assert set(wall.tolist()) <= act_on
    # entries at or past every quadrant's bound are untouched
    past = r["below"] == 0
    assert np.array_equal(on.words[past], off.words[past])
    if "tail" in kinds:
        tail = np.isin(on.ids, np.nonzero(kinds == "tail")[0])
        assert tail.any() and past[tail].all()
        print(f"{case}: tail entries {int(tail.sum())}, with quadrant bits {int((off.masks[tail] != 0).sum())}")
    assert on.heads < off.heads and on.Pa < off.Pa


def test_alpha_on_the_threshold():
    """alpha >= 1/255 holds with equality (tests/live_mask_scene.py threshold_scene: one entry per pixel, tuned so that
    its alpha at that pixel lands within a few ulp of 1/255, a tenth of them exactly on it).  Whatever the GPU's
    rounding gives, the forward names every pixel's last contributor by the same test, and that entry's visit of the
    pixel's quadrant is live by the definition: its bit must survive the refinement."""
    m, cam = lms.threshold_scene()
    W, H = 48, 48
    on, off = Built(m, cam, True), Built(m, cam, False)
    assert np.array_equal(on.records, off.records) and np.array_equal(on.n_contrib, off.n_contrib)
    blended = on.n_contrib > 0
    share = float(blended.mean())
    print(f"threshold scene: {int(blended.sum())} of {W * H} pixels blend their entry ({share:.2f})")
    assert 0.2 <= share <= 0.8  # the alphas straddle the threshold
    ys, xs = np.nonzero(blended)
    tile = (ys // 16) * ((W + 15) // 16) + xs // 16
    k = on.ranges[tile, 0] + on.n_contrib[ys, xs] - 1  # the last contributor's list entry
    q = (2 * ((ys % 16) >= 8) + ((xs % 16) >= 8)).astype(np.uint8)
    assert (on.ids[k] == ys * W + xs).all()  # it is the pixel's own entry: nothing else reaches the pixel
    assert (((off.masks[k] >> q) & 1) == 1).all()
    kept = ((on.masks[k] >> q) & 1) == 1
    assert kept.all(), f"{int((~kept).sum())} last contributors lost their visit"
    assert on.heads == int(blended.sum()) <= off.heads
    assert same(on.g, off.g)
    v = on.random_v(5)
    assert same(on.matvec(v), off.matvec(v))


def test_nothing_visible():
    m, cam = lms.empty_scene()
    on, off = Built(m, cam, True), Built(m, cam, False)
    assert on.N == 0 and on.Pa == 0 and on.heads == 0 and off.heads == 0
    with switch(True):
        assert on.prob.active_view() is None
    assert same(on.g, off.g) and not bool(on.g.any())
    v = on.random_v(3)
    assert same(on.matvec(v), off.matvec(v))


@pytest.mark.parametrize("case", ["48x40", "17x9"])
def test_rebuilt_row_map_is_the_same(case):
    m, cam, _ = lms.tile_scene(case)
    b = Built(m, cam, True)
    words, slots, hscan, g = b.words.copy(), b.slots.copy(), b.hscan.copy(), b.g.clone()
    with switch(True):
        b.vr.tail_clean = False  # as after a backward: the next product builds the row map again, on this binning
        g2 = b.prob.rhs(b.prob.zeros())
        b.read()
    assert np.array_equal(b.words, words) and np.array_equal(b.slots, slots) and np.array_equal(b.hscan, hscan)
    assert same(g2, g)


LAYOUTS = {"projected": ("48x40", True), "full_sh3": ("48x40", False), "sh0": ("48x40_sh0", False),
           "planted_power": ("48x40_pow", True)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_products_on_against_off(layout):
    case, proj = LAYOUTS[layout]
    on, off = built(case, True, proj), built(case, False, proj)
    assert on.prob.layout.rest_projected == proj
    assert same(on.g, off.g)  # J^T b
    assert bool(on.g.any())
    for seed in (1, 2):
        v = on.random_v(seed)
        y_on, y_off = on.matvec(v), off.matvec(v)
        assert same(y_on, y_off) and bool(torch.isfinite(y_on).all())
        # J v alone
        jv = []
        for b in (on, off):
            with switch(b.on):
                out = [torch.empty_like(b.vr.color)]
                jv.append(b.prob.jv_residual(v, b.prob.residual_masks(), out)[0].clone())
        assert same(jv[0], jv[1]) and bool(jv[0].any())
        # the active list: each side packs to its own list; equal after scattering back.  v restricted to the
        # shorter list (the switch on) is a vector of both lists' subspaces
        _, v_on = on.active_matvec(v)
        ya_on, _ = on.active_matvec(v_on)
        ya_off, v_back = off.active_matvec(v_on)
        assert same(v_back, v_on)
        assert same(ya_on, ya_off)
        # ... and it is the full path's product of that vector, on the listed rows
        yf = on.matvec(v_on)
        lay = on.prob.layout
        listed = torch.zeros(on.P, dtype=torch.bool, device=DEV)
        listed[torch.from_numpy(on.active).to(DEV)] = True
        for name, t in lay.views(yf).items():
            if name != "exposure" and t.numel():
                assert same(t.reshape(on.P, -1)[listed], lay.views(ya_on)[name].reshape(on.P, -1)[listed]), name


def test_exposure_product_on_against_off():
    on, off = built("48x40", True, "auto", False, True), built("48x40", False, "auto", False, True)
    assert on.prob.train_exposure
    assert same(on.g, off.g)
    e0, e1 = on.prob.layout.offsets["exposure"]
    assert bool(on.g[e0:e1].any())
    for seed in (1, 2):
        v = on.random_v(seed)
        assert bool(v[e0:e1].any())
        assert same(on.matvec(v), off.matvec(v))


def test_ssim_product_on_against_off():
    on, off = built("48x40", True, "auto", True), built("48x40", False, "auto", True)
    assert on.prob.ssim
    assert same(on.g, off.g)
    for seed in (1, 2):
        v = on.random_v(seed)
        assert same(on.matvec(v), off.matvec(v))


def _cg(b, active, iters=3):
    from gslm.lm import cgls_fused
    with switch(b.on, GSLM_CG_ACTIVE="1" if active else "0"):
        x, info = cgls_fused(b.prob, b.g, max_iter=iters, restart_iter=iters, check_every=False)
    torch.cuda.synchronize()
    return x.clone(), info


def _rel(a, b):
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), 1e-300)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_cg_on_against_off(layout):
    case, proj = LAYOUTS[layout]
    on, off = built(case, True, proj), built(case, False, proj)
    xf_on, _ = _cg(on, False)
    xf_off, _ = _cg(off, False)
    assert same(xf_on, xf_off) and bool(xf_on.any())
    xa_on, _ = _cg(on, True)
    xa_off, _ = _cg(off, True)
    print(f"{layout}: three CG iterations on the active list (Pa {on.Pa} against {off.Pa}); against the full path "
          f"rel {_rel(xa_on, xf_on):.2e}")
    assert same(xa_on, xa_off) and bool(xa_on.any())


def _lm_step(on, active, **kw):
    from gslm.lm import lm_step
    model, cams = ms.scene(600, 4, 3)
    m = copy.deepcopy(model).to(DEV)
    cams = [copy.deepcopy(c).to(DEV) for c in cams]
    nt = kw.pop("n_train", 1)
    with switch(on, GSLM_CG_ACTIVE="1" if active else "0"):
        out = lm_step(m, cams[:nt], cams[nt:], torch.zeros(3), max_iter=3, restart_iter=3, check_every=False,
                      cache_val=False, **kw)
    torch.cuda.synchronize()
    return out["step"].clone(), out["final_val_loss"], out["best_alpha"]


def test_lm_step_on_against_off():
    s_on, l_on, a_on = _lm_step(True, False)
    s_off, l_off, a_off = _lm_step(False, False)
    assert same(s_on, s_off) and l_on == l_off and a_on == a_off and bool(s_on.any())
    sa_on, la_on, aa_on = _lm_step(True, True)
    sa_off, la_off, aa_off = _lm_step(False, True)
    assert same(sa_on, sa_off) and la_on == la_off and aa_on == aa_off and bool(sa_on.any())


@pytest.mark.parametrize("union", [False, True])
def test_batched_two_views_on_against_off(union):
    from gslm.lm import BatchedLMProblem, cgls_fused
    model, cams = ms.scene(600, 2, 3)
    xs, pas = [], []
    for on in (True, False):
        with switch(on):
            prob = BatchedLMProblem(copy.deepcopy(model).to(DEV), [copy.deepcopy(c).to(DEV) for c in cams],
                                    torch.zeros(3), union_active=union)
            prob.evaluate()
            g = prob.rhs(prob.zeros())
            v = torch.randn(prob.layout.numel, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
            for grp in ("xyz", "exposure"):
                a, b = prob.layout.offsets[grp]
                v[a:b] = 0
            y = prob.matvec(v, prob.zeros()).clone()
            if union:
                pas.append(prob.active_view()._active[1])
            x, _ = cgls_fused(prob, g, max_iter=3, restart_iter=3, check_every=False)
            torch.cuda.synchronize()
            xs.append((g.clone(), y, x.clone()))
    assert same(xs[0][0], xs[1][0]) and same(xs[0][1], xs[1][1])  # J^T b and A v on the full vectors
    print(f"batched two views union={union}: union Pa {pas}")
    assert same(xs[0][2], xs[1][2]) and bool(xs[0][2].any())
    if union:
        assert pas[0] <= pas[1]
