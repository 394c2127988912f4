"""The depth residual's public surface, checked without a GPU: the library exports gslm_lm_residual_depth, include/gslm.h
declares it and GSLM_MV_DEPTH, the flag is a bit of its own and needs no extension struct, the ABI version is unchanged,
the host-side argument checks of the epilogue return before any launch, the product entry points refuse the flag's
excluded combinations from the flags, stages and pointers alone, and the Python side has the keywords."""
import ctypes
import inspect
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "gslm.h")) as f:
        return f.read()


def test_library_exports_the_epilogue():
    from gslm import _lib
    assert hasattr(_lib.lib, "gslm_lm_residual_depth")
    restype, args = _lib.EXPORTS["gslm_lm_residual_depth"]
    assert restype is ctypes.c_int and len(args) == 14
    assert args[5] is ctypes.c_double  # depth_weight, by value
    # the plain epilogue with invdepth / invdepth_gt / depth_mask for color / gt / alpha_mask, plus the weight
    assert len(args) == len(_lib.EXPORTS["gslm_lm_residual"][1]) + 1


def test_library_exports_the_loss_blends():
    from gslm import _lib
    for name, plain in (("gslm_rasterize_loss_depth", "gslm_rasterize_loss"),
                        ("gslm_rasterize_loss_slot_depth", "gslm_rasterize_loss_slot")):
        assert hasattr(_lib.lib, name), name
        assert len(_lib.EXPORTS[name][1]) == len(_lib.EXPORTS[plain][1]) + 3  # invdepth_gt, depth_mask, depth_weight
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", _header(), re.S)
        assert m and "const float* invdepth_gt" in m.group(1) and "double depth_weight" in m.group(1), name
    h = _header()
    for absent in ("gslm_rasterize_loss_sets_depth", "gslm_rasterize_loss_dev_depth"):
        assert absent not in h


def test_loss_blend_argument_checks():
    """The depth blends' own checks and the plain forms' return before any launch (dummy pointers, no GPU)."""
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)
    view = _lib.make_view(17, 33, 0.5, 0.5, [0, 0, 0], 1.0, [0.0] * 16, [0.0] * 16, 1, [0, 0, 0])
    vp = ctypes.byref(view)
    H, W, N, P = view.image_height, view.image_width, 10, 5
    nbin, nscr = lib.gslm_binning_bytes(N, H, W), lib.gslm_loss_scratch_bytes(H, W)
    ubin, nset = lib.gslm_union_binning_bytes(N, H, W), lib.gslm_depth_records_bytes(P)

    def plain(gt=a, gtd=a, lam=4.0, nbytes=nscr, loss=a, binning_bytes=nbin):
        return lib.gslm_rasterize_loss_depth(vp, P, a, a, binning_bytes, N, gt, None, gtd, None, lam, a, nbytes, loss,
                                             0, None)

    def slot(gt=a, gtd=a, lam=4.0, slot=0, n_sets=6, nbytes=nscr, set_bytes=nset, binning_bytes=ubin):
        return lib.gslm_rasterize_loss_slot_depth(vp, P, a, set_bytes, a, binning_bytes, N, slot, n_sets, gt, None,
                                                  gtd, None, lam, a, nbytes, a, 0, None)

    for fn in (plain, slot):
        for lam in (-1.0, math.nan, math.inf):
            assert fn(lam=lam) == _lib.GSLM_ERR_INVALID, (fn.__name__, lam)
            assert b"depth_weight" in lib.gslm_last_error()
        assert fn(gtd=None) == _lib.GSLM_ERR_INVALID
        assert b"invdepth_gt" in lib.gslm_last_error()
        assert fn(gt=None) == _lib.GSLM_ERR_INVALID
        assert fn(nbytes=nscr - 1) == _lib.GSLM_ERR_CAPACITY
    assert plain(loss=None) == _lib.GSLM_ERR_INVALID
    assert plain(binning_bytes=nbin - 1) == _lib.GSLM_ERR_CAPACITY
    assert slot(slot=6) == _lib.GSLM_ERR_INVALID and slot(slot=-1) == _lib.GSLM_ERR_INVALID
    assert slot(set_bytes=nset - 1) == _lib.GSLM_ERR_CAPACITY
    assert slot(binning_bytes=ubin - 1) == _lib.GSLM_ERR_CAPACITY


def test_header_declares_the_flag_and_the_entry_point():
    h = _header()
    assert re.search(r"#define\s+GSLM_MV_DEPTH\s+32\b", h)
    m = re.search(r"\bint\s+gslm_lm_residual_depth\s*\((.*?)\)\s*;", h, re.S)
    assert m
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["H", "W", "invdepth", "invdepth_gt", "depth_mask", "depth_weight", "residual", "weight", "seed",
                      "scratch", "scratch_bytes", "loss_dev", "accumulate", "stream"]
    assert "double depth_weight" in m.group(1)
    assert "gslm_matvec_opts_depth" not in h  # no extension struct: the flag composes with LEAN and the projection


def test_the_flag_is_a_bit_of_its_own():
    from gslm import lm
    flags = [int(v) for v in re.findall(r"#define\s+GSLM_MV_\w+\s+(\d+)", _header())]
    assert len(flags) == 6 and len(set(flags)) == 6 and all(f & (f - 1) == 0 for f in flags)
    assert lm.MV_DEPTH == 32
    assert len({lm.MV_TAIL_CLEAN, lm.MV_SH_REST_PROJECTED, lm.MV_LEAN, lm.MV_EXPOSURE, lm.MV_DAMP_VEC,
                lm.MV_DEPTH}) == 6


def test_abi_version_is_still_9():
    from gslm import _lib
    assert _lib.lib.gslm_abi_version() == 9
    assert re.search(r"#define\s+GSLM_ABI_VERSION\s+9\b", _header())


def test_residual_depth_argument_checks():
    """Every check returns before a launch (no GPU is touched: the pointers are never dereferenced on the host)."""
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)  # stands for any non-NULL pointer
    big = lib.gslm_residual_scratch_bytes(4, 4)

    def call(H=4, W=4, D=a, gt=a, lam=4.0, scratch=a, nbytes=big, loss=a):
        return lib.gslm_lm_residual_depth(H, W, D, gt, None, lam, a, a, a, scratch, nbytes, loss, 0, None)

    assert call(H=-1) == _lib.GSLM_ERR_INVALID
    assert b"negative" in lib.gslm_last_error()
    assert call(W=-1) == _lib.GSLM_ERR_INVALID
    assert call(D=None) == _lib.GSLM_ERR_INVALID
    assert call(gt=None) == _lib.GSLM_ERR_INVALID
    for lam in (-1.0, -1e-30, math.nan, math.inf, -math.inf):
        assert call(lam=lam) == _lib.GSLM_ERR_INVALID, lam
        assert b"depth_weight" in lib.gslm_last_error()
    assert call(scratch=None) == _lib.GSLM_ERR_INVALID
    assert call(loss=None) == _lib.GSLM_ERR_INVALID
    assert call(nbytes=big - 1) == _lib.GSLM_ERR_CAPACITY
    assert b"scratch" in lib.gslm_last_error()


def test_the_flag_is_refused_before_any_device_work():
    """GSLM_MV_DEPTH with mask_xyz = 0, GSLM_MV_EXPOSURE, GSLM_MV_DAMP_VEC, jv_out or the SCREEN stage, and from the
    multi-view entry points: GSLM_ERR_INVALID from the flags, the stages and the pointers alone (P = 0: no device
    memory stands behind the call, and a call that got as far as a launch would return GSLM_ERR_HIP)."""
    from gslm import _lib
    lib = _lib.lib
    INV = _lib.GSLM_ERR_INVALID
    FAKE = 4096  # a non-NULL pointer that is never followed
    view = _lib.make_view(64, 64, 0.5, 0.5, [0, 0, 0], 1.0, [0.0] * 16, [0.0] * 16, 0, [0, 0, 0])
    g = _lib.make_gaussians(0)
    g.raw = 1
    v = _lib.GslmGrads()
    v.sh_dc_stride = 3

    def opts(**fields):
        o = _lib.GslmMatvecOpts()
        for k, val in fields.items():
            setattr(o, k, val)
        return o

    def ex(mask_xyz=1, **fields):
        o = opts(**fields)
        return lib.gslm_matvec_view_ex(ctypes.byref(view), ctypes.byref(g), ctypes.byref(v), FAKE, mask_xyz, None,
                                       None, 0, None, None, 1 << 20, ctypes.byref(v), ctypes.byref(o), None)

    def active(mask_xyz=1, **fields):
        o = opts(**fields)
        return lib.gslm_matvec_view_active(ctypes.byref(view), ctypes.byref(g), ctypes.byref(v), FAKE, mask_xyz, None,
                                           None, 0, None, None, 1 << 20, ctypes.byref(v), ctypes.byref(o), None, None,
                                           0, None)

    cases = [("mask_xyz = 0", dict(flags=32, mask_xyz=0)),
             ("GSLM_MV_EXPOSURE", dict(flags=32 | 8)),
             ("GSLM_MV_DAMP_VEC", dict(flags=32 | 16)),
             ("jv_out", dict(flags=32, stages=1 | 2, jv_out=FAKE)),
             ("the SCREEN stage", dict(flags=32, stages=1 | 2 | 16, screen_out=FAKE))]
    for what, kw in cases:
        for fn in (ex, active):
            assert fn(**kw) == INV, (what, fn.__name__)
            assert b"GSLM_MV_DEPTH" in lib.gslm_last_error(), (what, fn.__name__, lib.gslm_last_error())
    views = (_lib.GslmView * 2)(view, view)
    o = opts(flags=32)
    assert lib.gslm_gather_screen(views, 2, ctypes.byref(g), FAKE, ctypes.byref(v), ctypes.byref(v), ctypes.byref(o),
                                  None) == INV
    assert b"GSLM_MV_DEPTH" in lib.gslm_last_error()
    ws = (_lib.GslmViewWs * 2)()
    assert lib.gslm_gather_views(views, ws, 2, ctypes.byref(g), ctypes.byref(v), ctypes.byref(v), ctypes.byref(o),
                                 None) == INV
    assert b"GSLM_MV_DEPTH" in lib.gslm_last_error()
    assert lib.gslm_tangent_views(views, 2, ctypes.byref(g), ctypes.byref(v), 1, None, 0, None, 0, ctypes.byref(o),
                                  None) == INV
    assert b"GSLM_MV_DEPTH" in lib.gslm_last_error()


def test_python_keywords_exist_and_default_off():
    from gslm import lm
    from gslm.cameras import Camera
    for fn in (lm.LMProblem.__init__, lm.LossEvaluator.__init__):
        p = inspect.signature(fn).parameters
        for k in ("depth_weight", "invdepths", "depth_masks"):
            assert k in p and p[k].default is None, (fn, k)
    p = inspect.signature(lm.lm_step).parameters
    assert "depth_weight" in p and p["depth_weight"].default is None
    assert "depth_mask" in inspect.getsource(Camera.__init__)
