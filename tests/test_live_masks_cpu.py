"""CPU: the live-mask refinement's host side -- the ABI stays 9 with gslm_inspect_list added, the entry point's
argument checks, and the GSLM_LIVE_MASKS switch's validation (no kernel is launched)."""
import pytest


def test_abi_is_still_9_and_inspect_list_is_bound():
    from gslm import _lib
    assert _lib.lib.gslm_abi_version() == _lib.ABI_VERSION == 9
    assert "gslm_inspect_list" in _lib.EXPORTS and hasattr(_lib.lib, "gslm_inspect_list")


def test_inspect_list_argument_errors():
    from gslm import _lib
    lib = _lib.lib
    INV, CAP = _lib.GSLM_ERR_INVALID, _lib.GSLM_ERR_CAPACITY
    H, W, N = 40, 48, 1000
    nb = lib.gslm_binning_bytes(N, H, W)
    fake = 4096  # never dereferenced: every call below is refused before a copy is queued
    assert lib.gslm_inspect_list(None, nb, N, H, W, None, None, None) == INV
    assert lib.gslm_inspect_list(fake, nb, -1, H, W, None, None, None) == INV
    assert lib.gslm_inspect_list(fake, nb, N, 0, W, None, None, None) == INV
    assert lib.gslm_inspect_list(fake, nb, N, H, 0, None, None, None) == INV
    assert lib.gslm_inspect_list(fake, nb - 1, N, H, W, None, None, None) == CAP
    assert lib.gslm_inspect_list(fake, 0, N, H, W, None, None, None) == CAP
    # both outputs NULL: nothing to copy
    assert lib.gslm_inspect_list(fake, nb, N, H, W, None, None, None) == _lib.GSLM_OK
    assert lib.gslm_inspect_list(fake, lib.gslm_binning_bytes(0, H, W), 0, H, W, None, None, None) == _lib.GSLM_OK


def test_live_masks_env_is_validated(monkeypatch):
    from gslm.lm import live_masks
    monkeypatch.delenv("GSLM_LIVE_MASKS", raising=False)
    assert live_masks() is True
    monkeypatch.setenv("GSLM_LIVE_MASKS", "1")
    assert live_masks() is True
    monkeypatch.setenv("GSLM_LIVE_MASKS", "0")
    assert live_masks() is False
    for bad in ("", "2", "-1", "on", "off", "true", " 0", "00"):
        monkeypatch.setenv("GSLM_LIVE_MASKS", bad)
        with pytest.raises(ValueError, match="GSLM_LIVE_MASKS"):
            live_masks()
