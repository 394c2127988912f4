"""The trained-exposure mode's public surface, checked without a GPU: the library exports its entry points,
include/gslm.h declares them and the extension structs, the bindings mirror the structs, the ABI version is unchanged
(the entry points are additive), the host-side argument checks of gslm_lm_residual_exposure return before any launch,
and the Python side has the `train_exposure` keywords."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "gslm.h")) as f:
        return f.read()


def test_library_exports_exposure_entry_points():
    from gslm import _lib
    for name, nargs in (("gslm_lm_residual_exposure", 15), ("gslm_exposure_scratch_bytes", 2)):
        assert hasattr(_lib.lib, name), name
        assert len(_lib.EXPORTS[name][1]) == nargs, name
    assert _lib.EXPORTS["gslm_lm_residual_exposure"][0] is ctypes.c_int
    assert _lib.EXPORTS["gslm_exposure_scratch_bytes"][0] is ctypes.c_size_t


def test_header_declares_the_flag_the_structs_and_the_entry_points():
    h = _header()
    assert re.search(r"#define\s+GSLM_MV_EXPOSURE\s+8\b", h)
    assert re.search(r"\bint\s+gslm_lm_residual_exposure\s*\(\s*int32_t\s+H\s*,\s*int32_t\s+W\s*,", h)
    assert re.search(r"\bsize_t\s+gslm_exposure_scratch_bytes\s*\(", h)
    m = re.search(r"typedef\s+struct\s+gslm_exposure_opts\s*\{(.*?)\}\s*gslm_exposure_opts\s*;", h, re.S)
    assert m, "gslm_exposure_opts is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == ["exposure", "v_rows", "y_rows", "color", "u_image", "scratch", "scratch_bytes", "damp",
                      "overwrite", "_pad"]
    m = re.search(r"typedef\s+struct\s+gslm_matvec_opts_exposure\s*\{(.*?)\}\s*gslm_matvec_opts_exposure\s*;", h, re.S)
    assert m and re.findall(r"(\w+)\s*;", m.group(1)) == ["base", "exposure"]


def test_bindings_match_the_header():
    from gslm import _lib
    from gslm import lm
    names = [n for n, _ in _lib.GslmExposureOpts._fields_]
    assert names == ["exposure", "v_rows", "y_rows", "color", "u_image", "scratch", "scratch_bytes", "damp",
                     "overwrite", "_pad"]
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.GslmExposureOpts) == 6 * p + ctypes.sizeof(ctypes.c_size_t) + 8 + 4 + 4
    assert [n for n, _ in _lib.GslmMatvecOptsExposure._fields_] == ["base", "exposure"]
    assert _lib.GslmMatvecOptsExposure.exposure.offset == ctypes.sizeof(_lib.GslmMatvecOpts)
    assert lm.MV_EXPOSURE == 8
    # the flag is a bit of its own
    assert len({lm.MV_TAIL_CLEAN, lm.MV_SH_REST_PROJECTED, lm.MV_LEAN, lm.MV_EXPOSURE}) == 4


def test_abi_version_is_still_9():
    from gslm import _lib
    assert _lib.lib.gslm_abi_version() == 9
    assert re.search(r"#define\s+GSLM_ABI_VERSION\s+9\b", _header())


def test_scratch_size():
    from gslm import _lib
    n = _lib.lib.gslm_exposure_scratch_bytes(1080, 1920)
    assert n == 13 * 1024 * 8 == _lib.lib.gslm_exposure_scratch_bytes(1, 1)
    assert n >= _lib.lib.gslm_residual_scratch_bytes(1080, 1920)


def test_residual_exposure_argument_checks():
    """Every check returns before a launch (no GPU is touched: the pointers are never dereferenced on the host)."""
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)  # stands for any non-NULL pointer
    big = lib.gslm_exposure_scratch_bytes(4, 4)

    def call(H=4, W=4, color=a, gt=a, exposure=a, scratch=a, nbytes=big, loss=a):
        return lib.gslm_lm_residual_exposure(H, W, color, gt, None, exposure, None, None, None, None, scratch, nbytes,
                                             loss, 0, None)

    assert call(H=-1) == _lib.GSLM_ERR_INVALID
    assert b"negative" in lib.gslm_last_error()
    assert call(W=-1) == _lib.GSLM_ERR_INVALID
    assert call(color=None) == _lib.GSLM_ERR_INVALID
    assert call(gt=None) == _lib.GSLM_ERR_INVALID
    assert call(exposure=None) == _lib.GSLM_ERR_INVALID
    assert b"exposure" in lib.gslm_last_error()
    assert call(scratch=None) == _lib.GSLM_ERR_INVALID
    assert call(loss=None) == _lib.GSLM_ERR_INVALID
    assert call(nbytes=big - 1) == _lib.GSLM_ERR_CAPACITY
    assert b"scratch" in lib.gslm_last_error()
    # the plain epilogue's scratch is too small for this one
    assert call(nbytes=lib.gslm_residual_scratch_bytes(4, 4)) == _lib.GSLM_ERR_CAPACITY


def test_python_keywords_exist_and_default_off():
    from gslm import lm
    for fn in (lm.LMProblem.__init__, lm.LossEvaluator.__init__, lm.lm_step):
        p = inspect.signature(fn).parameters
        assert "train_exposure" in p and p["train_exposure"].default is False, fn
