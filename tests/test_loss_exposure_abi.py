"""The exposure forms of the loss blends (gslm_rasterize_loss_exposure / _slot_exposure / _sets_exposure) and the
line search's `fused_exposure` / `val_exposure` options, checked without a GPU: the library exports the entry points
with their argument counts, include/gslm.h declares them, the ABI version is unchanged (they are additive), every
host-side argument check returns before any launch, and the Python keywords exist with their defaults."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gslm_rasterize_loss_exposure": "gslm_rasterize_loss", "gslm_rasterize_loss_slot_exposure": "gslm_rasterize_loss_slot",
       "gslm_rasterize_loss_sets_exposure": "gslm_rasterize_loss_sets"}


def _header():
    with open(os.path.join(ROOT, "include", "gslm.h")) as f:
        return f.read()


def test_library_exports_the_entry_points():
    """Each form is its plain form with one more pointer, placed right after alpha_mask."""
    from gslm import _lib
    for name, nargs in (("gslm_rasterize_loss_exposure", 14), ("gslm_rasterize_loss_slot_exposure", 17),
                        ("gslm_rasterize_loss_sets_exposure", 17)):
        assert hasattr(_lib.lib, name), name
        res, args = _lib.EXPORTS[name]
        pres, pargs = _lib.EXPORTS[NEW[name]]
        assert res is ctypes.c_int and len(args) == nargs == len(pargs) + 1, name
        k = len(pargs) - 6  # alpha_mask: followed by scratch, scratch_bytes, loss_dev, accumulate, stream
        assert args[:k + 1] == pargs[:k + 1] and args[k + 2:] == pargs[k + 1:], name
    assert _lib.EXPORTS["gslm_rasterize_loss_exposure"][1][8] is ctypes.c_void_p
    assert _lib.EXPORTS["gslm_rasterize_loss_slot_exposure"][1][11] is ctypes.c_void_p
    assert _lib.EXPORTS["gslm_rasterize_loss_sets_exposure"][1][11] == ctypes.POINTER(ctypes.c_void_p)


def test_header_declares_the_entry_points():
    h = _header()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", h, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        k = [i for i, a in enumerate(args) if a.endswith("alpha_mask")]
        assert k and args[k[0] + 1].endswith("exposure"), (name, args)
        want = "const float* const* exposure" if "sets" in name else "const float* exposure"
        assert args[k[0] + 1] == want, (name, args[k[0] + 1])
        assert args[k[0] + 2] == "void* scratch", name
    assert "gslm_rasterize_loss_dev_exposure" not in h  # the device-count form has no exposure variant


def test_abi_version_is_still_9():
    from gslm import _lib
    assert _lib.lib.gslm_abi_version() == 9
    assert re.search(r"#define\s+GSLM_ABI_VERSION\s+9\b", _header())


def _view(W=33, H=17):
    import torch
    from gslm import _lib
    from gslm.cameras import orbit_cameras
    return _lib.view_from_camera(orbit_cameras(1, W, H, seed=1)[0], torch.zeros(3), 1)


def test_rasterize_loss_exposure_argument_checks():
    """Every check returns before a launch (no GPU is touched: the pointers are never dereferenced on the host)."""
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)  # stands for any non-NULL pointer
    vw = _view()
    H, W, N = vw.image_height, vw.image_width, 10
    nbin, nscr = lib.gslm_binning_bytes(N, H, W), lib.gslm_loss_scratch_bytes(H, W)

    def call(exposure=a, gt=a, scratch=a, nbytes=nscr, loss=a, binning_bytes=nbin):
        return lib.gslm_rasterize_loss_exposure(ctypes.byref(vw), 5, a, a, binning_bytes, N, gt, None, exposure,
                                                scratch, nbytes, loss, 0, None)

    assert call(exposure=None) == _lib.GSLM_ERR_INVALID
    assert b"exposure" in lib.gslm_last_error()
    assert call(gt=None) == _lib.GSLM_ERR_INVALID
    assert call(scratch=None) == _lib.GSLM_ERR_INVALID
    assert call(loss=None) == _lib.GSLM_ERR_INVALID
    assert call(nbytes=nscr - 1) == _lib.GSLM_ERR_CAPACITY
    assert b"scratch" in lib.gslm_last_error()
    assert call(binning_bytes=nbin - 1) == _lib.GSLM_ERR_CAPACITY


def test_rasterize_loss_slot_exposure_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)
    vw = _view()
    H, W, N, P = vw.image_height, vw.image_width, 10, 5
    nbin, nscr, nset = lib.gslm_union_binning_bytes(N, H, W), lib.gslm_loss_scratch_bytes(H, W), lib.gslm_depth_records_bytes(P)

    def call(exposure=a, slot=0, n_sets=6, nbytes=nscr, set_bytes=nset, gt=a, binning_bytes=nbin):
        return lib.gslm_rasterize_loss_slot_exposure(ctypes.byref(vw), P, a, set_bytes, a, binning_bytes, N, slot, n_sets,
                                                     gt, None, exposure, a, nbytes, a, 0, None)

    assert call(exposure=None) == _lib.GSLM_ERR_INVALID
    assert b"exposure" in lib.gslm_last_error()
    assert call(slot=6) == _lib.GSLM_ERR_INVALID
    assert call(slot=-1) == _lib.GSLM_ERR_INVALID
    assert call(n_sets=9, slot=8) == _lib.GSLM_ERR_INVALID
    assert call(n_sets=0) == _lib.GSLM_ERR_INVALID
    assert call(gt=None) == _lib.GSLM_ERR_INVALID
    assert call(nbytes=nscr - 1) == _lib.GSLM_ERR_CAPACITY
    assert b"scratch" in lib.gslm_last_error()
    assert call(set_bytes=nset - 1) == _lib.GSLM_ERR_CAPACITY
    assert call(binning_bytes=nbin - 1) == _lib.GSLM_ERR_CAPACITY


def test_rasterize_loss_sets_exposure_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)
    vw = _view()
    H, W, N, P = vw.image_height, vw.image_width, 10, 5
    nbin, nset = lib.gslm_union_binning_bytes(N, H, W), lib.gslm_depth_records_bytes(P)

    def ptrs(n, hole=None):
        return (ctypes.c_void_p * max(n, 1))(*[None if k == hole else a for k in range(max(n, 1))])

    def call(n=3, first=0, exposure="all", hole=None, nbytes=None, geoms=None):
        nbytes = lib.gslm_loss_sets_scratch_bytes(n, H, W) if nbytes is None else nbytes
        xp = ptrs(n, hole) if exposure == "all" else exposure
        return lib.gslm_rasterize_loss_sets_exposure(ctypes.byref(vw), P, ptrs(n) if geoms is None else geoms, n, first,
                                                     nset, a, nbin, N, a, None, xp, a, nbytes, ptrs(n), 0, None)

    assert call(exposure=None) == _lib.GSLM_ERR_INVALID
    assert b"exposure" in lib.gslm_last_error()
    for hole in (0, 2):  # a NULL entry of the array, first or last
        assert call(hole=hole) == _lib.GSLM_ERR_INVALID
        assert b"exposure" in lib.gslm_last_error()
    assert call(n=8, hole=7) == _lib.GSLM_ERR_INVALID
    assert b"exposure" in lib.gslm_last_error()
    for n in (0, 9, -1):  # n outside 1..8
        assert call(n=n) == _lib.GSLM_ERR_INVALID, n
    assert call(n=3, first=6) == _lib.GSLM_ERR_INVALID  # slots 6..8 reach past the binning's 8
    assert call(n=1, first=-1) == _lib.GSLM_ERR_INVALID
    assert call(nbytes=lib.gslm_loss_sets_scratch_bytes(3, H, W) - 1) == _lib.GSLM_ERR_CAPACITY
    assert b"scratch" in lib.gslm_last_error()
    # one set's scratch is too small for three
    assert call(nbytes=lib.gslm_loss_scratch_bytes(H, W)) == _lib.GSLM_ERR_CAPACITY
    assert call(geoms=ptrs(3, hole=1)) == _lib.GSLM_ERR_INVALID


def test_plain_forms_take_no_exposure():
    """The plain entry points keep their signatures (the exposure forms are separate symbols)."""
    from gslm import _lib
    assert len(_lib.EXPORTS["gslm_rasterize_loss"][1]) == 13
    assert len(_lib.EXPORTS["gslm_rasterize_loss_slot"][1]) == 16
    assert len(_lib.EXPORTS["gslm_rasterize_loss_sets"][1]) == 16
    assert len(_lib.EXPORTS["gslm_rasterize_loss_dev"][1]) == 13


def test_python_keywords_exist_with_their_defaults():
    from gslm import lm
    p = inspect.signature(lm.LossEvaluator.__init__).parameters
    assert p["fused_exposure"].default is False and p["train_exposure"].default is False
    p = inspect.signature(lm.lm_step).parameters
    assert p["val_exposure"].default == "forward" and p["train_exposure"].default is False
    p = inspect.signature(lm.param_snapshot).parameters
    assert p["exposure"].default is False
