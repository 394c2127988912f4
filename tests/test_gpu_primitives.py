"""Device self-tests of the wave primitives and the scan building blocks (through the C ABI).  The radix sort, the tile
ranges and the tile launch order have theirs in tests/test_gpu_binning_primitives.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _selftest(which, x):
    from gslm import _lib
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib.gslm_selftest(which, x.data_ptr(), out.data_ptr(), _lib.stream_handle()))
    torch.cuda.synchronize()
    return out.cpu()


def test_transposed_wave_reduction():
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-1000, 1000, (64, 8), generator=g).float()  # integers: exact sums
    got = _selftest(0, x.cuda().contiguous())
    ref = x.sum(dim=0)
    for lane in range(64):
        assert got[lane].item() == ref[(lane >> 3) & 7].item(), lane


def test_dpp_wave_sum():
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-1000, 1000, (64, 8), generator=g).float()
    got = _selftest(1, x.cuda().contiguous())
    assert got[63].item() == x[:, 0].sum().item()


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 300_000, 9_000_001])
@pytest.mark.parametrize("force_top", [0, 1])
def test_exclusive_scan_both_forms(n, force_top):
    """the scan's apply pass sums its own prefix of block sums (O(nb^2) loads over the grid) only up to
    4096 blocks of 2048; longer scans (the LM row map at 5M Gaussians / 4K: nb ~ 12k-49k) scan the block sums in a
    launch of their own.  Both forms against torch's cumsum, exact (9M elements: nb = 4395 takes the long form
    unforced)."""
    from gslm import _lib
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 64, (n,), generator=g, dtype=torch.int64)
    xin = x.to(torch.int32).cuda()
    out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    tmp = torch.empty((8 * ((n + 2047) // 2048) + 64 + 255) // 256 * 256, dtype=torch.uint8, device="cuda")
    tot = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.gslm_selftest_scan(xin.data_ptr(), out.data_ptr(), n, force_top, tmp.data_ptr(), tmp.numel(),
                                           tot.data_ptr(), _lib.stream_handle()))
    torch.cuda.synchronize()
    ref = torch.cumsum(x, 0) - x
    assert torch.equal(out.cpu().to(torch.int64), ref)
    assert int(tot.item()) == int(x.sum())
    # in place (out = in, the LM row map's head-flag scan: k_scan_apply_inplace, both forms)
    tot.fill_(-1)
    _lib.check(_lib.lib.gslm_selftest_scan(xin.data_ptr(), xin.data_ptr(), n, force_top, tmp.data_ptr(), tmp.numel(),
                                           tot.data_ptr(), _lib.stream_handle()))
    torch.cuda.synchronize()
    assert torch.equal(xin.cpu().to(torch.int64), ref)
    assert int(tot.item()) == int(x.sum())


def _scan_dual(x, idx, xb, force_top):
    """gslm_selftest_scan_dual on host int64 tensors -> (out_a, out_b, total_a, total_b), outputs prefilled with -1."""
    from gslm import _lib
    n = x.numel()
    dev = lambda t: None if t is None else t.to(torch.int32).cuda()
    xin, idxd, xbd = dev(x), dev(idx), dev(xb)
    out_a = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    out_b = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    tmp = torch.empty((8 * ((n + 2047) // 2048) + 64 + 255) // 256 * 256, dtype=torch.uint8, device="cuda")
    tot = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.gslm_selftest_scan_dual(xin.data_ptr(), _lib.ptr(idxd), _lib.ptr(xbd), out_a.data_ptr(),
                                                out_b.data_ptr(), n, force_top, tmp.data_ptr(), tmp.numel(),
                                                tot.data_ptr(), tot.data_ptr() + 4, _lib.stream_handle()))
    torch.cuda.synchronize()
    return out_a.cpu().to(torch.int64), out_b.cpu().to(torch.int64), int(tot[0].item()), int(tot[1].item())


def _check_scan_dual(n, form, force_top):
    g = torch.Generator().manual_seed(n + 17)
    x = torch.randint(0, 64, (n,), generator=g, dtype=torch.int64)
    if form == "idx":  # the second sequence is the first gathered through a permutation (the binning's depth order)
        idx, xb = torch.randperm(n, generator=g), None
        b = x[idx]
    else:
        idx, xb = None, torch.randint(0, 64, (n,), generator=g, dtype=torch.int64)
        b = xb
    out_a, out_b, tot_a, tot_b = _scan_dual(x, idx, xb, force_top)
    assert torch.equal(out_a, torch.cumsum(x, 0) - x)
    assert torch.equal(out_b, torch.cumsum(b, 0) - b)
    assert tot_a == int(x.sum()) and tot_b == int(b.sum())


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 18437, 4_198_403])
@pytest.mark.parametrize("force_top", [0, 1])
@pytest.mark.parametrize("form", ["idx", "in_b"])
def test_exclusive_scan_dual_both_forms(n, force_top, form):
    """The binning's dual scan (two sequences' block sums side by side in tmp): the inline form and, forced, the long
    form (k_scan_top with one block per sequence, then k_scan2_apply<true>), which the library takes by itself only
    above 4096 blocks of 2048.  4,198,403 elements are 2051 blocks: k_scan_top's second chunk of 2048, in both of its
    blocks.  Exact against torch's cumsum."""
    _check_scan_dual(n, form, force_top)


def test_exclusive_scan_dual_long_form_unforced():
    """8,390,657 elements = 4098 blocks > 4096: the long form by the library's own threshold."""
    _check_scan_dual(8_390_657, "idx", 0)


def test_exclusive_scan_dual_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    p, h = t.data_ptr(), _lib.stream_handle()
    assert lib.gslm_selftest_scan_dual(p, p, p, p, p, 8, 0, p, 256, p, p, h) == _lib.GSLM_ERR_INVALID  # idx and in_b
    assert lib.gslm_selftest_scan_dual(p, None, None, p, p, 8, 0, p, 256, p, p, h) == _lib.GSLM_ERR_INVALID
    assert lib.gslm_selftest_scan_dual(p, p, None, p, p, -1, 0, p, 256, p, p, h) == _lib.GSLM_ERR_INVALID
    assert lib.gslm_selftest_scan_dual(p, p, None, p, p, 8, 0, p, 255, p, p, h) == _lib.GSLM_ERR_CAPACITY
