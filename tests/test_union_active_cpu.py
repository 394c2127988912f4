"""CPU: the host-side argument checks of the union-list entry points (gslm_active_union, gslm_tangent_views_active,
gslm_gather_views_active).  Every check below returns before any device call, so the pointers are fakes (16): a
check that let a call through would launch on them.  The valid calls and the outputs of a refused call run in
tests/test_gpu_union_active.py."""
import ctypes

FAKE = 16  # a non-NULL pointer nothing may dereference


def _view(lib_mod, sh_degree=0):
    return lib_mod.make_view(64, 64, 0.5, 0.5, [0, 0, 0], 1.0, [0.0] * 16, [0.0] * 16, sh_degree, [0, 0, 0])


def _gaussians(lib_mod, P, raw=1):
    g = lib_mod.make_gaussians(P, max_coeffs=1, raw=bool(raw))
    g.means3D = g.opacities = g.scales = g.rotations = g.sh_dc = FAKE
    g.sh_dc_stride = 3
    return g


def _grads():
    from gslm import _lib
    v = _lib.GslmGrads()
    v.means3D = v.opacities = v.scales = v.rotations = v.sh_dc = FAKE
    v.sh_dc_stride = 3
    return v


def _ws(n, P, N=100):
    from gslm import _lib
    ws = (_lib.GslmViewWs * n)()
    for k in range(n):
        ws[k].geom, ws[k].scratch = FAKE, FAKE
        ws[k].scratch_bytes, ws[k].num_rendered = _lib.lib.gslm_scratch_bytes(P, N), N
    return ws


def test_active_union_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    P = 10
    wb = lib.gslm_active_union_bytes(P)
    assert wb >= 4 * P and wb == lib.gslm_active_list_bytes(P)
    ok = lambda ws=None, n=2, P=P, work=FAKE, wbytes=wb, ids=FAKE, hrow=FAKE, afl=FAKE, cnt=FAKE: \
        lib.gslm_active_union(_ws(2, P) if ws is None else ws, n, P, work, wbytes, ids, hrow, afl, cnt, None)
    INV, CAP = _lib.GSLM_ERR_INVALID, _lib.GSLM_ERR_CAPACITY
    assert lib.gslm_active_union(None, 2, P, FAKE, wb, FAKE, FAKE, FAKE, FAKE, None) == INV
    assert b"active_union" in lib.gslm_last_error()
    for n in (0, -1):
        assert ok(n=n) == INV
    assert ok(P=-1) == INV
    assert ok(P=1 << 28) == INV
    assert ok(work=None) == INV and ok(cnt=None) == INV and ok(hrow=None) == INV
    assert ok(ids=None) == INV and ok(afl=None) == INV
    ws = _ws(2, P)
    ws[1].num_rendered = -1
    assert ok(ws=ws) == INV
    ws = _ws(2, P)
    ws[1].geom = None
    assert ok(ws=ws) == INV
    ws = _ws(2, P)
    ws[0].scratch = None
    assert ok(ws=ws) == INV
    assert b"NULL workspace" in lib.gslm_last_error()
    assert ok(wbytes=wb - 1) == CAP
    assert b"gslm_active_union_bytes" in lib.gslm_last_error()
    ws = _ws(2, P)
    ws[1].scratch_bytes -= 1
    assert ok(ws=ws) == CAP
    assert b"scratch" in lib.gslm_last_error()
    # V is any count >= 1: 17 views pass the count check and fail on the next one
    ws = _ws(17, P)
    ws[16].scratch_bytes -= 1
    assert ok(ws=ws, n=17) == CAP


def test_tangent_views_active_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    INV = _lib.GSLM_ERR_INVALID
    P, na = 10, 4
    view = _view(_lib)
    views = (_lib.GslmView * 17)(*([view] * 17))
    g, v = _gaussians(_lib, P), _grads()

    def call(views=views, n=2, g=g, v=v, mask=1, ids=FAKE, na=na, afl=FAKE, fs=P, trec=FAKE, ts=P, opts=None):
        return lib.gslm_tangent_views_active(views, n, None if g is None else ctypes.byref(g),
                                             None if v is None else ctypes.byref(v), mask, ids, na, afl, fs, trec, ts,
                                             None if opts is None else ctypes.byref(opts), None)

    assert call(views=None) == INV and call(g=None) == INV and call(v=None) == INV
    for n in (0, 17):
        assert call(n=n) == INV
        assert b"nviews" in lib.gslm_last_error()
    assert call(na=-1) == INV
    assert b"negative n_active" in lib.gslm_last_error()
    assert call(mask=0) == INV
    assert b"mask_xyz" in lib.gslm_last_error()
    assert call(na=P + 1) == INV
    assert call(ids=None) == INV
    assert call(g=_gaussians(_lib, P, raw=0)) == INV
    assert b"raw" in lib.gslm_last_error()
    assert call(afl=None) == INV and call(trec=None) == INV
    assert call(fs=na - 1) == INV and call(ts=P - 1) == INV
    assert b"stride" in lib.gslm_last_error()
    opts = _lib.GslmMatvecOpts()
    opts.rest_basis, opts.rest_views, opts.view_base = FAKE, 2, 1  # views past the last column
    assert call(opts=opts) == INV
    assert b"rest_views" in lib.gslm_last_error()


def test_gather_views_active_argument_checks():
    from gslm import _lib
    lib = _lib.lib
    INV, CAP = _lib.GSLM_ERR_INVALID, _lib.GSLM_ERR_CAPACITY
    P, na = 10, 4
    view = _view(_lib)
    views = (_lib.GslmView * 17)(*([view] * 17))
    g, v, y = _gaussians(_lib, P), _grads(), _grads()
    plain = _lib.GslmMatvecOpts()
    plain.stages = 7 | 8

    def call(views=views, ws=None, n=2, g=g, v=v, y=y, ids=FAKE, na=na, hrow=FAKE, hs=P + 1, afl=FAKE, fs=P, opts=plain):
        return lib.gslm_gather_views_active(views, _ws(17, P) if ws is None else ws, n,
                                            None if g is None else ctypes.byref(g),
                                            None if v is None else ctypes.byref(v),
                                            None if y is None else ctypes.byref(y), ids, na, hrow, hs, afl, fs,
                                            None if opts is None else ctypes.byref(opts), None)

    assert call(views=None) == INV and call(g=None) == INV and call(v=None) == INV and call(y=None) == INV
    assert lib.gslm_gather_views_active(views, None, 2, ctypes.byref(g), ctypes.byref(v), ctypes.byref(y), FAKE, na, FAKE,
                                        P + 1, FAKE, P, ctypes.byref(plain), None) == INV
    for n in (0, 17):
        assert call(n=n) == INV
        assert b"nviews" in lib.gslm_last_error()
    assert call(na=-1) == INV
    assert b"negative n_active" in lib.gslm_last_error()
    assert call(na=P + 1, hs=P + 2, fs=P + 1) == INV
    assert call(ids=None) == INV and call(hrow=None) == INV and call(afl=None) == INV
    assert call(hs=na) == INV and call(fs=na - 1) == INV
    assert b"stride" in lib.gslm_last_error()
    assert call(g=_gaussians(_lib, P, raw=0)) == INV
    assert b"raw" in lib.gslm_last_error()
    ws = _ws(2, P)
    ws[1].num_rendered = -1
    assert call(ws=ws) == INV
    ws = _ws(2, P)
    ws[0].geom = None
    assert call(ws=ws) == INV
    ws = _ws(2, P)
    ws[1].scratch_bytes -= 1
    assert call(ws=ws) == CAP
    assert b"scratch" in lib.gslm_last_error()
    # the dot's partials are the list's: (n_active + 255) / 256 of them
    od = _lib.GslmMatvecOpts()
    od.stages = 7 | 8
    od.dot_vy, od.dot_scratch = FAKE, FAKE
    od.dot_scratch_bytes = lib.gslm_dot_scratch_bytes(na) - 1
    assert call(opts=od) == CAP
    assert b"dot scratch" in lib.gslm_last_error()
    od.dot_scratch, od.dot_scratch_bytes = None, 1 << 20
    assert call(opts=od) == CAP
    o9 = _lib.GslmMatvecOpts()
    o9.stages = 7 | 8
    o9.rest_basis, o9.rest_views = FAKE, 9
    assert call(opts=o9) == INV
    assert b"rest_views" in lib.gslm_last_error()
    # group strides that do not match the layout (the launcher's check, before its launch)
    ybad = _grads()
    ybad.sh_dc_stride = 4
    assert call(y=ybad) == INV
    assert b"flat param-space" in lib.gslm_last_error()
