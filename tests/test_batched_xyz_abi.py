"""GSLM_MV_XYZ (the unmasked form of gslm_gather_views), checked without a GPU: the header defines the flag as a bit of
its own and the ABI version is unchanged; every entry point but gslm_gather_views refuses it, and gslm_gather_views
refuses it with the options it excludes and with a NULL xyz group of v or y -- all from the flags and the pointers
alone (FAKE pointers are never followed: a call that got as far as a launch would return GSLM_ERR_HIP or crash)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096  # a non-NULL pointer that is never followed
XYZ = 64


def _header():
    with open(os.path.join(ROOT, "include", "gslm.h")) as f:
        return f.read()


def test_header_defines_the_flag_as_a_new_bit():
    h = _header()
    m = re.search(r"#define\s+GSLM_MV_XYZ\s+\(1 << (\d+)\)", h)
    assert m and 1 << int(m.group(1)) == XYZ
    others = [int(v) for v in re.findall(r"#define\s+GSLM_MV_\w+\s+(\d+)", h)]
    assert XYZ not in others and all(f & (f - 1) == 0 for f in others) and len(set(others)) == len(others)
    assert "xyz-masked form only" not in h
    assert re.search(r"#define\s+GSLM_ABI_VERSION\s+9\b", h)
    from gslm import _lib, lm
    assert _lib.lib.gslm_abi_version() == 9
    assert lm.MV_XYZ == XYZ
    assert lm.MV_XYZ not in (lm.MV_TAIL_CLEAN, lm.MV_SH_REST_PROJECTED, lm.MV_LEAN, lm.MV_EXPOSURE, lm.MV_DAMP_VEC,
                             lm.MV_DEPTH)


def _setup(P=0):
    from gslm import _lib
    view = _lib.make_view(64, 64, 0.5, 0.5, [0, 0, 0], 1.0, [0.0] * 16, [0.0] * 16, 0, [0, 0, 0])
    g = _lib.make_gaussians(P)
    g.raw = 1
    if P:
        g.means3D = g.opacities = g.scales = g.rotations = g.sh_dc = FAKE
        g.sh_dc_stride = 3
    v = _lib.GslmGrads()
    v.sh_dc_stride = 3
    return _lib, view, g, v


def _opts(_lib, **fields):
    o = _lib.GslmMatvecOpts()
    for k, val in fields.items():
        setattr(o, k, val)
    return o


def test_the_other_entry_points_refuse_the_flag():
    _lib, view, g, v = _setup()
    lib, INV = _lib.lib, _lib.GSLM_ERR_INVALID
    views = (_lib.GslmView * 2)(view, view)
    ws = (_lib.GslmViewWs * 2)()
    bg, bv = ctypes.byref(g), ctypes.byref(v)

    def refused(rc, who):
        assert rc == INV, who
        assert b"GSLM_MV_XYZ" in lib.gslm_last_error(), (who, lib.gslm_last_error())

    for mask_xyz in (1, 0):
        o = _opts(_lib, flags=XYZ)
        refused(lib.gslm_matvec_view_ex(ctypes.byref(view), bg, bv, FAKE, mask_xyz, None, None, 0, None, None, 1 << 20,
                                        bv, ctypes.byref(o), None), "matvec_view_ex")
        o = _opts(_lib, flags=XYZ | 1)  # (with GSLM_MV_TAIL_CLEAN, which the list form needs)
        refused(lib.gslm_matvec_view_active(ctypes.byref(view), bg, bv, FAKE, mask_xyz, None, None, 0, None, None,
                                            1 << 20, bv, ctypes.byref(o), None, None, 0, None), "matvec_view_active")
        o = _opts(_lib, flags=XYZ)
        refused(lib.gslm_tangent_views(views, 2, bg, bv, mask_xyz, None, 0, None, 0, ctypes.byref(o), None),
                "tangent_views")
    o = _opts(_lib, flags=XYZ)
    refused(lib.gslm_tangent_views_active(views, 2, bg, bv, 1, None, 0, None, 0, None, 0, ctypes.byref(o), None),
            "tangent_views_active")
    refused(lib.gslm_gather_screen(views, 2, bg, FAKE, bv, bv, ctypes.byref(o), None), "gather_screen")
    refused(lib.gslm_gather_views_active(views, ws, 2, bg, bv, bv, None, 0, FAKE, 1, None, 0, ctypes.byref(o), None),
            "gather_views_active")


def test_gather_views_refuses_the_excluded_options():
    _lib, view, g, v = _setup()
    lib, INV = _lib.lib, _lib.GSLM_ERR_INVALID
    views = (_lib.GslmView * 2)(view, view)
    ws = (_lib.GslmViewWs * 2)()
    for what, bit in (("GSLM_MV_DAMP_VEC", 16), ("GSLM_MV_DEPTH", 32), ("GSLM_MV_EXPOSURE", 8)):
        o = _opts(_lib, flags=XYZ | bit)
        rc = lib.gslm_gather_views(views, ws, 2, ctypes.byref(g), ctypes.byref(v), ctypes.byref(v), ctypes.byref(o), None)
        assert rc == INV, what
        err = lib.gslm_last_error()
        assert b"GSLM_MV_XYZ" in err and what.encode() in err, (what, err)
    # without the flag GSLM_MV_EXPOSURE is ignored by this entry point as it always was (P = 0: an empty call)
    o = _opts(_lib, flags=8)
    assert lib.gslm_gather_views(views, ws, 2, ctypes.byref(g), ctypes.byref(v), ctypes.byref(v), ctypes.byref(o),
                                 None) == _lib.GSLM_OK


def test_gather_views_demands_the_xyz_groups():
    """P = 5, two views that rendered nothing: the plan is built up to the flat vectors, and the NULL xyz group of v or
    of y is refused there (with both given the call would launch: not called here)."""
    _lib, view, g, v = _setup(P=5)
    lib, INV = _lib.lib, _lib.GSLM_ERR_INVALID
    views = (_lib.GslmView * 2)(view, view)
    ws = (_lib.GslmViewWs * 2)()

    def grads(xyz):
        s = _lib.GslmGrads()
        s.means3D = xyz
        s.sh_dc = s.scales = s.rotations = s.opacities = FAKE
        s.sh_dc_stride = 3
        return s

    o = _opts(_lib, flags=XYZ)
    for vin, y in ((grads(None), grads(FAKE)), (grads(FAKE), grads(None)), (grads(None), grads(None))):
        rc = lib.gslm_gather_views(views, ws, 2, ctypes.byref(g), ctypes.byref(vin), ctypes.byref(y), ctypes.byref(o),
                                   None)
        assert rc == INV
        err = lib.gslm_last_error()
        assert b"GSLM_MV_XYZ" in err and b"xyz groups" in err, err


def test_python_accepts_the_mode():
    from gslm import lm
    src = inspect.getsource(lm.BatchedLMProblem)
    assert "MV_XYZ" in src and "_trec_w" in src
    assert issubclass(lm.BatchedXyzLMProblem, lm.BatchedLMProblem) and lm.BatchedXyzLMProblem.XYZ_FREE
    assert inspect.signature(lm.BatchedXyzLMProblem.__init__).parameters["mask_xyz"].default is False
    assert "batched_xyz" in inspect.getsource(lm.lm_step)
