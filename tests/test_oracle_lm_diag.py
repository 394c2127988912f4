"""CPU: the yardsticks of diag(J^T W J + D) and of Jacobi-preconditioned CG (tests/lm_diag_ref.py), pinned on the
oracle, and the host-side argument checks of the new entry points.

The GPU tests (tests/test_gpu_lm_diag.py) compare gslm_lm_diag_view with lm_diag_ref.jacobian_diag -- the diagonal
from the float64 dense Jacobian of the oracle's residual.  Here that yardstick is pinned twice: against e_j^T (A e_j)
of OracleLMProblem.matvec on sampled columns of every group (measured 9e-16 relative at worst, asserted 1e-8), and
against the closed form the kernels implement, evaluated in float64 torch from the oracle's per-pixel quantities
(measured 7e-16 of the group's max, asserted 1e-10).  test_float32_floor measures the float32 oracle's own distance
from the float64 diagonal, in the GPU tests' measure; the GPU bounds are 8 x the recorded floors.

Scene: lm_bg_scene("sh1_33x17") -- 600 Gaussians, SH 1, 33x17 (one tile plus one pixel on each axis), generic
background, a fractional alpha mask with a block of zeros, brightened so that the clamp zeroes weights.  The PCG
restatement runs on the same scene and background without the brightening and the mask (float64, one view, default
damping): the quadratic model phi(x) = x^T A x / 2 - g^T x after k iterations,

  k          1       2       3       5       8       10
  plain CG  -32.42  -43.94  -50.05  -57.14  -60.36  -60.92
  Jacobi    -39.83  -51.38  -56.60  -59.70  -60.86  -61.06"""
import ctypes
import functools

import pytest
import torch

import lm_diag_ref as R
from scenes import BG_GENERIC, lm_bg_mask, lm_bg_scene, to_float64

SCENE = "sh1_33x17"
FAKE = 16  # a non-NULL pointer nothing may dereference


@functools.lru_cache(maxsize=None)
def _case():
    """(model32, cams32, model64, cams64, float64 diagonal without D): computed once, not modified."""
    model, cams = lm_bg_scene(SCENE)
    cams[0].alpha_mask = lm_bg_mask(SCENE, seed=0)
    m64, c64 = to_float64(model, cams)
    d64 = R.jacobian_diag(m64, c64, torch.tensor(BG_GENERIC, dtype=torch.float64), damp=False)
    return model, cams, m64, c64, d64


def test_yardstick_is_the_operators_diagonal():
    """diag + D against e_j^T (A e_j) of OracleLMProblem.matvec: the three largest and two seeded random columns of
    every group the solve moves (the oracle masks the xyz and exposure columns out of v, D included)."""
    from oracle.lm_ref import OracleLMProblem
    _, _, m64, c64, d64 = _case()
    lay = R.layout_of(m64)
    diag = d64 + R.damp_vector(lay)
    op = OracleLMProblem(m64, c64, torch.tensor(BG_GENERIC, dtype=torch.float64))
    op.evaluate()
    gen = torch.Generator().manual_seed(3)
    worst = 0.0
    for name in R.DIAG_GROUPS:
        a, b = lay.offsets[name]
        cols = torch.argsort(d64[a:b], descending=True)[:3].tolist()
        cols += torch.randint(0, b - a, (2,), generator=gen).tolist()
        for j in cols:
            e = torch.zeros(lay.numel, dtype=torch.float64)
            e[a + j] = 1.0
            y = op.matvec(e, torch.zeros(lay.numel, dtype=torch.float64))
            err = abs(float(y[a + j]) - float(diag[a + j])) / float(diag[a + j])
            worst = max(worst, err)
            assert err <= 1e-8, (name, j, float(y[a + j]), float(diag[a + j]))
    print(f"yardstick vs e_j^T A e_j: worst relative error {worst:.2e}")
    assert float(d64[lay.offsets["scaling"][0]:lay.offsets["scaling"][1]].max()) > 0.1  # (J^T J is not hidden by D)


def test_closed_form_is_the_yardstick():
    """The per-visit formula (float64 torch) against the dense Jacobian: on tile 0 alone and on the whole image."""
    _, _, m64, c64, d64 = _case()
    lay = R.layout_of(m64)
    bg = torch.tensor(BG_GENERIC, dtype=torch.float64)
    tile = R.jacobian_diag(m64, c64, bg, damp=False, tiles={0})
    for what, cf, ref in (("tile 0", R.closed_form(m64, c64[0], bg, tiles={0}), tile),
                          ("image", R.closed_form(m64, c64[0], bg), d64)):
        err = R.group_errors(cf, ref, lay)
        print(f"closed form vs yardstick ({what}):", {k: f"{v:.2e}" for k, v in err.items()})
        assert max(err.values()) <= 1e-10, (what, err)
    # the other tiles contribute: tile 0 alone is a different number
    assert max(R.group_errors(tile, d64, lay).values()) > 1e-3


def test_float32_floor():
    """The float32 oracle's distance from the float64 diagonal, per group, relative to the group's max: the floors
    lm_diag_ref.F32_FLOOR records (the GPU bounds are 8 x them)."""
    model, cams, m64, _, d64 = _case()
    d32 = R.jacobian_diag(model, cams, torch.tensor(BG_GENERIC), damp=False)
    err = R.group_errors(d32, d64, R.layout_of(m64))
    print("float32 floor:", {k: f"{v:.2e}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= R.F32_FLOOR[k], (k, v)
        assert R.GPU_TOL[k] == min(8.0 * R.F32_FLOOR[k], R.MAX_TOL)


@functools.lru_cache(maxsize=None)
def _pcg_case():
    from oracle.lm_ref import OracleLMProblem
    model, cams = lm_bg_scene(SCENE, brighten=False)
    m64, c64 = to_float64(model, cams)
    bg = torch.tensor(BG_GENERIC, dtype=torch.float64)
    op = OracleLMProblem(m64, c64, bg)
    op.evaluate()
    g = op.rhs()
    diag = R.jacobian_diag(m64, c64, bg, damp=True)
    return op, g, diag


def test_pcg_with_unit_preconditioner_is_cgls_ref():
    from oracle.lm_ref import cgls_ref
    op, g, _ = _pcg_case()
    ones = torch.ones_like(g)
    for max_iter, restart in ((2, 1), (3, 3)):
        assert torch.equal(R.pcg_ref(op, g, ones, max_iter, restart), cgls_ref(op, g, max_iter, restart))


def test_jacobi_lowers_the_model_at_every_iteration():
    """phi(x_k) of Jacobi PCG is below plain CG's at each of the first 10 iterations, and both reproduce the
    module docstring's table."""
    op, g, diag = _pcg_case()
    minv = torch.where(diag > 0, 1.0 / diag, torch.zeros_like(diag))
    plain, jac = [], []
    R.pcg_ref(op, g, torch.ones_like(g), 10, 10, history=plain)
    R.pcg_ref(op, g, minv, 10, 10, history=jac)
    print("plain :", [f"{v:.2f}" for v in plain])
    print("jacobi:", [f"{v:.2f}" for v in jac])
    assert len(plain) == 10 and len(jac) == 10
    for k in range(10):
        assert jac[k] < plain[k], (k, jac[k], plain[k])
    table = {1: (-32.42, -39.83), 2: (-43.94, -51.38), 3: (-50.05, -56.60), 5: (-57.14, -59.70),
             8: (-60.36, -60.86), 10: (-60.92, -61.06)}
    for k, (p_ref, j_ref) in table.items():
        assert abs(plain[k - 1] - p_ref) <= 0.006 and abs(jac[k - 1] - j_ref) <= 0.006, (k, plain[k - 1], jac[k - 1])
    assert jac[1] < plain[2] and jac[2] < plain[3]  # Jacobi at 2 is past plain CG at 3, at 3 past plain CG at 4


# ---------------------------------------------------------------- argument checks (no device call: fake pointers)
def _view(lib_mod, sh_degree=0):
    return lib_mod.make_view(64, 64, 0.5, 0.5, [0, 0, 0], 1.0, [0.0] * 16, [0.0] * 16, sh_degree, [0, 0, 0])


def _gaussians(lib_mod, P, raw=1, K=1):
    g = lib_mod.make_gaussians(P, max_coeffs=K, raw=bool(raw))
    g.means3D = g.opacities = g.scales = g.rotations = g.sh_dc = FAKE
    g.sh_dc_stride = 3
    if K > 1:
        g.sh_rest, g.sh_rest_stride = FAKE, 3 * (K - 1)
    return g


def _grads(K=1, rest_stride=None):
    from gslm import _lib
    v = _lib.GslmGrads()
    v.means3D = v.opacities = v.scales = v.rotations = v.sh_dc = FAKE
    v.sh_dc_stride = 3
    if K > 1:
        v.sh_rest, v.sh_rest_stride = FAKE, 3 * (K - 1) if rest_stride is None else rest_stride
    return v


def test_lm_diag_view_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    INV, CAP = _lib.GSLM_ERR_INVALID, _lib.GSLM_ERR_CAPACITY
    P, N = 10, 100
    view, g, y = _view(_lib), _gaussians(_lib, P), _grads()
    sbytes = lib.gslm_scratch_bytes(P, N)

    def call(view=view, g=g, w=FAKE, mask=1, geom=FAKE, binning=FAKE, N=N, image=FAKE, scratch=FAKE, sbytes=sbytes,
             y=y, damp=None, flags=0):
        return lib.gslm_lm_diag_view(None if view is None else ctypes.byref(view),
                                     None if g is None else ctypes.byref(g), w, mask, geom, binning, N, image, scratch,
                                     sbytes, None if y is None else ctypes.byref(y), damp, flags, None)

    assert call(mask=0) == INV
    assert b"mask_xyz" in lib.gslm_last_error()
    assert call(w=None) == INV and call(y=None) == INV
    assert b"NULL pixel_weight or destination" in lib.gslm_last_error()
    assert call(flags=8) == INV
    assert b"flag" in lib.gslm_last_error()
    assert call(view=None) == INV and call(g=None) == INV and call(geom=None) == INV and call(image=None) == INV
    assert call(scratch=None) == INV and call(binning=None) == INV and call(N=-1) == INV
    assert call(sbytes=sbytes - 1) == CAP
    assert b"scratch" in lib.gslm_last_error()
    assert call(g=_gaussians(_lib, P, raw=0)) == INV
    assert b"raw" in lib.gslm_last_error()
    ybad = _grads()
    ybad.sh_dc_stride = 4
    assert call(y=ybad) == INV
    assert b"flat param-space" in lib.gslm_last_error()
    # the SH-rest stride follows the layout flag: 3(M-1) in the full layout, 3 projected
    g4 = _gaussians(_lib, P, K=4)
    assert call(g=g4, y=_grads(K=4, rest_stride=3)) == INV
    assert call(g=g4, y=_grads(K=4), flags=4) == INV


def test_pcg_entry_points_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    INV = _lib.GSLM_ERR_INVALID
    ok = dict(n=8, gam=FAKE, dele=FAKE, p=FAKE, q=FAKE, x=FAKE, s=FAKE, minv=FAKE, z=FAKE, scratch=FAKE, out=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gslm_pcg_update(a["n"], a["gam"], a["dele"], a["p"], a["q"], a["x"], a["s"], a["minv"], a["z"],
                                   a["scratch"], a["out"], None)

    for k in ("gam", "dele", "q", "s", "minv", "z", "scratch", "out"):
        assert call(**{k: None}) == INV, k
    assert call(n=-1) == INV
    assert call(p=None) == INV  # x without p
    assert b"gslm_pcg_update" in lib.gslm_last_error()
    for k in ("p", "q", "x", "s", "minv", "z"):
        assert call(**{k: FAKE + 4}) == INV, k
        assert b"16-byte aligned" in lib.gslm_last_error()
    assert lib.gslm_precond_invert(-1, FAKE, FAKE, None) == INV
    assert lib.gslm_precond_invert(4, None, FAKE, None) == INV and lib.gslm_precond_invert(4, FAKE, None, None) == INV
    assert lib.gslm_precond_invert(0, None, None, None) == _lib.GSLM_OK


def test_lm_step_refuses_the_excluded_combinations():
    """precond='jacobi' with anything it does not cover, and any other string: ValueError before anything runs."""
    from gslm.lm import lm_step
    for kw in (dict(precond="ssor"), dict(precond="jacobi", recursion="cgls"),
               dict(precond="jacobi", train_exposure=True), dict(precond="jacobi", multiview="batched"),
               dict(precond="jacobi", mask_xyz=False), dict(precond="jacobi", backend=(None, None, None))):
        with pytest.raises(ValueError):
            lm_step(None, [], [], None, **kw)
