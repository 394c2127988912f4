"""The batched multi-view operator's public surface, checked without a GPU: the library exports gslm_gather_views,
include/gslm.h declares it and gslm_view_ws, the ABI version is unchanged (the entry point is additive), and the
Python side has BatchedLMProblem and lm_step's `multiview` option."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "gslm.h")) as f:
        return f.read()


def test_library_exports_gather_views():
    from gslm import _lib
    assert hasattr(_lib.lib, "gslm_gather_views")
    restype, argtypes = _lib.EXPORTS["gslm_gather_views"]
    assert restype is ctypes.c_int and len(argtypes) == 8
    assert argtypes[1] == ctypes.POINTER(_lib.GslmViewWs)


def test_header_declares_gather_views_and_view_ws():
    h = _header()
    assert re.search(r"\bint\s+gslm_gather_views\s*\(\s*const\s+gslm_view\s*\*\s*views\s*,\s*const\s+gslm_view_ws\s*\*", h)
    m = re.search(r"typedef\s+struct\s+gslm_view_ws\s*\{(.*?)\}\s*gslm_view_ws\s*;", h, re.S)
    assert m, "gslm_view_ws is not declared"
    fields = re.findall(r"(\w+)\s*;", m.group(1))
    assert fields == ["geom", "scratch", "scratch_bytes", "num_rendered"]


def test_view_ws_binding_matches_header():
    from gslm import _lib
    names = [n for n, _ in _lib.GslmViewWs._fields_]
    assert names == ["geom", "scratch", "scratch_bytes", "num_rendered"]
    assert ctypes.sizeof(_lib.GslmViewWs) == 2 * ctypes.sizeof(ctypes.c_void_p) + ctypes.sizeof(ctypes.c_size_t) + 8


def test_abi_version_is_still_9():
    from gslm import _lib
    assert _lib.lib.gslm_abi_version() == 9
    assert re.search(r"#define\s+GSLM_ABI_VERSION\s+9\b", _header())


def test_batched_problem_and_lm_step_option_exist():
    from gslm import lm
    assert issubclass(lm.BatchedLMProblem, lm.LMProblem)
    p = inspect.signature(lm.lm_step).parameters
    assert "multiview" in p and p["multiview"].default == "loop"
