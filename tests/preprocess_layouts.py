"""Helper of tests/test_gpu_preprocess_records.py and tests/test_oracle_preprocess_records.py (no tests here).

  * the SH layouts a caller can hand to gslm_preprocess / gslm_preprocess_views, each holding the same float values, and
    stage_lead() (csrc/gslm_kernels.hpp) restated on their pointers and strides;
  * the geometry workspace (geom_layout, csrc/api.hip) parsed into named arrays -- the 256-B aligned offsets are stated
    here once (_al / _off, which tests/test_gpu_line_search.py imports);
  * the cases, sizes, oracle records, error measure and boundary exclusion shared by the CPU floor test and the GPU test.

Layouts (M = stored SH coefficients; every layout is built with raw=True, the GaussianModel leaves, and raw=False, the
torch-activated tensors of scenes.activated):
  leaf              dc [P,1,3] stride 3; rest [P,M-1,3] stride 3(M-1), 16-B aligned              stage_lead  0
  features          one [P,M,3] tensor; rest = dc + 3 floats; both strides 3M                     stage_lead  3
  leaf_shifted      as leaf, the rest copied to a flat buffer one float past a 16-B boundary      stage_lead -1
  features_shifted  as features, one float past a 16-B boundary                                   stage_lead -1
  padded            rest rows at stride 3(M-1) + 1, the pad floats NaN                            stage_lead -1
  colors            colors_precomp = the float32 oracle's rgb, no SH                              stage_lead -1
At M = 1 (degree 0) there is no rest and nothing is staged in any layout.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

LAYOUTS = ("leaf", "features", "leaf_shifted", "features_shifted", "padded", "colors")
EXPECTED_LEAD = {"leaf": 0, "features": 3, "leaf_shifted": -1, "features_shifted": -1, "padded": -1, "colors": -1}

SIZES = (1, 2, 3, 255, 256, 258, 515, 768)
DEGREE_PAIRS = [(3, 3), (3, 1), (3, 0), (2, 2), (1, 1), (0, 0)]       # (allocated, active) SH degree
# (allocated, active, antialiasing, scale_modifier): plain settings everywhere, the other two on (3, 3) only
CASES = [(a, b, False, 1.0) for a, b in DEGREE_PAIRS] + [(3, 3, True, 0.7)]
GUARD = 64                     # guard entries behind radii_out
SENTINEL = -123456789
EXCLUDE_REL = 1e-5             # the boundary exclusion of the discrete outputs
EXCLUDE_CAP = 0.005            # of P * views
OUT_NAMES = ("x", "y", "conic_a", "conic_b", "conic_c", "opacity", "r", "g", "b", "invdepth", "depth")
TOL_FACTOR = 8.0               # the project's margin over a float32 floor (chain_jacobian.TOL_FACTOR)


def case_id(case):
    return f"sh{case[0]}_{case[1]}" + ("_aa_s0.7" if case[2] else "")


# ------------------------------------------------------------------ the geometry workspace
def _al(x):
    return (x + 255) // 256 * 256


def _off(rec, keys):
    """Byte offset of the tile counts in the geometry layout (rec, depth_key, tiles, ...; 256-B aligned, api.hip)."""
    return _al(rec) + _al(keys)


def parse_geom(buf, P):
    """A geometry workspace of exactly gslm_geom_bytes(P) bytes (uint8 tensor) as numpy arrays: rec [P,16] float32, keys
    [P] uint32 (the depth sort of gslm_preprocess reuses this buffer: raw keys only after gslm_preprocess_views), tiles
    [P] int32, rect [P,2] uint32 (min | max, x in the low and y in the high 16 bits) and clampw [P] uint32 -- geom_layout's
    last region, so its offset is the workspace's size minus its own aligned size."""
    b = buf.detach().cpu().numpy()
    rec, keys = 64 * P, 4 * P
    t0 = _off(rec, keys)
    r0 = t0 + _al(keys)
    c0 = b.size - _al(keys)
    assert c0 >= r0 + _al(8 * P)
    return dict(rec=b[:rec].view(np.float32).reshape(P, 16).copy(),
                keys=b[_al(rec):_al(rec) + keys].view(np.uint32).copy(),
                tiles=b[t0:t0 + keys].view(np.int32).copy(),
                rect=b[r0:r0 + 8 * P].view(np.uint32).reshape(P, 2).copy(),
                clampw=b[c0:c0 + keys].view(np.uint32).copy())


def unpack_rect(words):
    """[n, 2] uint32 rect words -> [n, 4] int64 (xmin, ymin, xmax, ymax), the order of the oracle's `rect`."""
    w = words.astype(np.int64)
    return np.stack([w[:, 0] & 0xFFFF, w[:, 0] >> 16, w[:, 1] & 0xFFFF, w[:, 1] >> 16], axis=1)


# ------------------------------------------------------------------ layouts
def model_values(model, P):
    """The float32 values of the model's first P Gaussians, on the CPU: the raw leaves and their torch activations."""
    with torch.no_grad():
        t = lambda x: x.detach()[:P].cpu().float().contiguous()
        xyz, dc, rest = t(model._xyz), t(model._features_dc), t(model._features_rest)
        sc, rot, op = t(model._scaling), t(model._rotation), t(model._opacity)
        return dict(P=P, M=1 + rest.shape[1], xyz=xyz, dc=dc, rest=rest,
                    raw=dict(opacities=op.reshape(-1), scales=sc, rotations=rot),
                    act=dict(opacities=torch.sigmoid(op).reshape(-1).contiguous(), scales=torch.exp(sc),
                             rotations=F.normalize(rot)))


def _place(values, shift, device):
    """The values in a flat buffer, starting `shift` floats past a 16-B boundary.  Returns (buffer, view)."""
    flat = values.reshape(-1)
    n = flat.numel()
    buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device=device)
    start = (-(buf.data_ptr() // 4)) % 4 + shift
    view = buf[start:start + n]
    view.copy_(flat)
    assert (view.data_ptr() - 4 * shift) % 16 == 0
    return buf, view


class Layout:
    """One layout's tensors (kept alive here) and the fields of its gslm_gaussians."""

    def __init__(self, name, vals, raw, device, colors=None):
        P, M = vals["P"], vals["M"]
        self.name, self.P, self.raw, self.keep = name, P, bool(raw), []
        g = vals["raw" if raw else "act"]
        self.means3D = vals["xyz"].to(device)
        self.opacities, self.scales, self.rotations = (g[k].to(device) for k in ("opacities", "scales", "rotations"))
        self.colors, self.dc_ptr, self.dc_stride, self.rest_ptr, self.rest_stride, self.M = None, None, 0, None, 0, M
        dc, rest = vals["dc"].reshape(P, 3), vals["rest"].reshape(P, 3 * (M - 1))
        if name == "colors":
            assert colors is not None and colors.shape == (P, 3)
            self.colors = colors.float().contiguous().to(device)
            self.M = 1
        elif name in ("leaf", "leaf_shifted", "padded"):
            _, d = _place(dc, 0, device)
            self.keep.append(d)
            self.dc_ptr, self.dc_stride = d.data_ptr(), 3
            if M > 1:
                if name == "padded":
                    rows = torch.full((P, 3 * (M - 1) + 1), float("nan"))
                    rows[:, :3 * (M - 1)] = rest
                    self.rest_stride = 3 * (M - 1) + 1
                else:
                    rows = rest
                    self.rest_stride = 3 * (M - 1)
                _, r = _place(rows, 1 if name == "leaf_shifted" else 0, device)
                self.keep.append(r)
                self.rest_ptr = r.data_ptr()
        elif name in ("features", "features_shifted"):
            _, f = _place(torch.cat([dc, rest], dim=1), 1 if name == "features_shifted" else 0, device)
            self.keep.append(f)
            self.dc_ptr, self.dc_stride = f.data_ptr(), 3 * M
            if M > 1:
                self.rest_ptr, self.rest_stride = f.data_ptr() + 12, 3 * M
        else:
            raise KeyError(name)

    def stage_lead(self):
        """stage_lead() of csrc/gslm_kernels.hpp on this layout's pointers and strides."""
        if self.colors is not None or self.rest_ptr is None or self.M <= 1:
            return -1
        lead = -1
        if self.rest_stride == 3 * (self.M - 1):
            lead = 0
        elif (self.dc_ptr and self.rest_ptr == self.dc_ptr + 12 and self.dc_stride == self.rest_stride
              and self.rest_stride == 3 * self.M):
            lead = 3
        if lead < 0 or (self.rest_ptr - 4 * lead) % 16 != 0:
            return -1
        return lead

    def expected_lead(self):
        return EXPECTED_LEAD[self.name] if (self.M > 1 and self.colors is None) else -1

    def gaussians(self):
        from gslm import _lib
        return _lib.make_gaussians(self.P, self.means3D, self.opacities, self.scales, self.rotations, None, self.dc_ptr,
                                   self.dc_stride, self.rest_ptr, self.rest_stride, self.M, self.colors, raw=self.raw)


# ------------------------------------------------------------------ GPU calls
def view_of(cam, case):
    from gslm import _lib
    return _lib.view_from_camera(cam, torch.zeros(3), case[1], case[3], case[2])


def run_preprocess(layout, view):
    """gslm_preprocess of one layout and view: parse_geom's arrays plus radii [P] int32 (the guard entries behind it
    are asserted untouched)."""
    import ctypes
    from gslm import _lib
    lib, P = _lib.lib, layout.P
    nb = lib.gslm_geom_bytes(P)
    geom = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    radii = torch.full((P + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    g = layout.gaussians()
    _lib.check(lib.gslm_preprocess(ctypes.byref(view), ctypes.byref(g), geom.data_ptr(), nb, radii.data_ptr(),
                                   _lib.stream_handle("cuda")), "gslm_preprocess")
    torch.cuda.synchronize()
    out = parse_geom(geom, P)
    r = radii.cpu().numpy()
    assert (r[P:] == SENTINEL).all(), "a guard entry behind radii_out was written"
    out["radii"] = r[:P].copy()
    return out


def run_preprocess_views(layout, views, pos=None):
    """gslm_preprocess_views of one layout for the listed GslmViews: parse_geom's arrays per view (raw depth keys).
    pos: per-view depth positions (int32 tensors) -- the records then lie at pos[i] and nothing else is written."""
    import ctypes
    from gslm import _lib
    lib, P, n = _lib.lib, layout.P, len(views)
    nb = lib.gslm_geom_bytes(P)
    arr = (_lib.GslmView * n)(*views)
    geoms = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(n)]
    ge = (ctypes.c_void_p * n)(*[t.data_ptr() for t in geoms])
    pp = None if pos is None else (ctypes.c_void_p * n)(*[t.data_ptr() for t in pos])
    g = layout.gaussians()
    _lib.check(lib.gslm_preprocess_views(arr, n, ctypes.byref(g), ge, nb, pp, _lib.stream_handle("cuda")),
               "gslm_preprocess_views")
    torch.cuda.synchronize()
    return [parse_geom(t, P) for t in geoms]


def depth_positions(layout, view):
    """The depth position of every Gaussian in one view (gslm_preprocess_ordered + gslm_depth_positions): int32 [P]."""
    import ctypes
    from gslm import _lib
    lib, P = _lib.lib, layout.P
    nb = lib.gslm_geom_bytes(P)
    geom = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    order = torch.empty(P, dtype=torch.int32, device="cuda")
    g = layout.gaussians()
    _lib.check(lib.gslm_preprocess_ordered(ctypes.byref(view), ctypes.byref(g), geom.data_ptr(), nb, None,
                                           order.data_ptr(), 1, _lib.stream_handle("cuda")), "gslm_preprocess_ordered")
    pos = torch.empty(P, dtype=torch.int32, device="cuda")
    _lib.check(lib.gslm_depth_positions(order.data_ptr(), P, pos.data_ptr(), _lib.stream_handle("cuda")))
    torch.cuda.synchronize()
    assert torch.equal(pos.long()[order.long()], torch.arange(P, device="cuda"))
    return pos


FIELDS = ("tiles", "rect", "clampw", "radii")


def same_bits(a, b, vis, fields=FIELDS, rec_cols=16):
    """The names of the fields in which two parsed results differ bitwise (records: of the visible Gaussians only)."""
    bad = []
    ra, rb = a["rec"][vis][:, :rec_cols].view(np.uint32), b["rec"][vis][:, :rec_cols].view(np.uint32)
    if not np.array_equal(ra, rb):
        rows = np.nonzero((ra != rb).any(axis=1))[0]
        err = np.abs(a["rec"][vis][rows][:, :12].astype(np.float64) - b["rec"][vis][rows][:, :12])
        bad.append(f"rec ({len(rows)} of {int(vis.sum())} Gaussians, first {np.nonzero(vis)[0][rows[0]]}, "
                   f"max |diff| {np.nanmax(err):.3e})")
    for f in fields:
        if f in a and f in b:
            x, y = (a[f][vis], b[f][vis]) if f in ("rect", "clampw") else (a[f], b[f])
            if not np.array_equal(x, y):
                bad.append(f)
    return bad


# ------------------------------------------------------------------ the oracle's records (CPU)
def _oracle(model, cam, case, dtype):
    """oracle.torch_raster.preprocess as chain_jacobian.record_fn calls it (sigmoid, exp and normalize in torch, in the
    dtype of the leaves): its dict, plus `record` [P, 11] = record_fn's ten outputs and the depth."""
    import chain_jacobian as cj
    from oracle import torch_raster as tr
    from scenes import to_float64
    if dtype == torch.float64:
        model, (cam,) = to_float64(model, [cam])
    st = cj.settings(cam, case[1], case[2], case[3], dtype)
    xyz, dc, rest, scaling, rotation, opacity = cj.leaves_of(model)
    n = xyz.shape[0]
    with torch.no_grad():
        shs = torch.cat([dc.reshape(n, 1, 3), rest.reshape(n, -1, 3)], dim=1)
        pre = tr.preprocess(xyz, torch.zeros_like(xyz), torch.sigmoid(opacity), shs, None, torch.exp(scaling),
                            F.normalize(rotation), None, st)
        rec = cj.record_fn([xyz, dc, rest, scaling, rotation, opacity], st)
        pre = dict(pre)
        pre["record"] = torch.cat([rec, pre["depth"][:, None]], dim=1)
        # what the exclusion looks at (float64 only makes sense): the radius before its ceil, the rect edges in tile
        # units before their truncation, and the colour before its clamp
        a, b, c = pre["cov2d"].unbind(1)
        mid = 0.5 * (a + c)
        pre["r0"] = 3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp_min(mid * mid - (a * c - b * b), 0.1)))
        radius = torch.ceil(pre["r0"])
        pre["edges"] = torch.stack([(pre["xy"][:, k] + s * radius + o) / 16.0 for k in (0, 1)
                                    for s, o in ((-1.0, 0.0), (1.0, 15.0))], dim=1)
        d = xyz - cam.camera_center.to(dtype)[None]
        pre["res"] = tr.eval_sh(st.sh_degree, shs, d / d.norm(dim=1, keepdim=True)) + 0.5
    return pre


def lowered_opacity_model(model):
    """A copy whose every 16th Gaussian's opacity is sigmoid(-6.5) = 0.0015, under the 1 / 255 of the alpha threshold."""
    import copy
    m = copy.deepcopy(model)
    with torch.no_grad():
        m._opacity[::16] = -6.5
    return m


def mirrored_model(model, cam):
    """A copy whose every 8th Gaussian is reflected through the camera's centre, so that it lies behind the near plane
    (its view depth changes sign)."""
    import copy
    m = copy.deepcopy(model)
    with torch.no_grad():
        c = cam.camera_center.detach().cpu().float()
        m._xyz[::8] = 2.0 * c[None] - m._xyz[::8]
    return m


@functools.lru_cache(maxsize=None)
def oracle_case(case, lowered=False):
    """(model, cams, [float32 dict per view], [float64 dict per view]) of the branch scene for one case, all 768
    Gaussians; computed once, never modified.  The preprocess is elementwise per Gaussian, so the oracle of a prefix is
    the prefix of these.  The scene's conditions are asserted by chain_jacobian.branch_case."""
    import chain_jacobian as cj
    sub, cams, _, _ = cj.branch_case(case[0], case[1], case[2], case[3])
    if lowered:
        sub = lowered_opacity_model(sub)
    return sub, cams, [_oracle(sub, c, case, torch.float32) for c in cams], \
        [_oracle(sub, c, case, torch.float64) for c in cams]


def excluded(o64):
    """bool [P]: the Gaussians of one view whose discrete outputs float32 rounding may flip -- in the float64 oracle the
    pre-rounding radius, a rect edge in tile units, t.z - 0.2 or a colour channel before the clamp lies within
    EXCLUDE_REL (relative; for the colour, whose boundary is 0, of its O(1) scale) of its boundary."""
    def near_int(t):
        return (t - torch.round(t)).abs() <= EXCLUDE_REL * t.abs().clamp_min(1.0)
    ex = near_int(o64["r0"]) | ((o64["depth"] - 0.2).abs() <= EXCLUDE_REL * 0.2)
    ex |= near_int(o64["edges"]).any(dim=1)
    ex |= (o64["res"].abs() <= EXCLUDE_REL).any(dim=1)
    return ex


def medians(o32, o64):
    """m_o [11]: the median of |ref_o| over the Gaussians the float32 oracle calls visible (the case's whole scene; the
    prefixes share it, so a bound measured on the whole scene covers every prefix)."""
    vis = o32["visible"]
    return o64["record"][vis].abs().median(dim=0).values


def record_measure(got, o32, o64, rows):
    """[11] float64: max over `rows` (bool, within the float32 oracle's visible set) of |got - ref| / max(|ref|, m_o).
    got [n, 11] (any float dtype, the first n Gaussians); NaN in got counts as infinite."""
    n = got.shape[0]
    ref = o64["record"][:n]
    m = medians(o32, o64)
    err = (torch.as_tensor(got).double() - ref).abs() / torch.maximum(ref.abs(), m[None, :])
    err = torch.nan_to_num(err, nan=float("inf"))
    rows = torch.as_tensor(rows)[:n] & o32["visible"][:n]
    if not bool(rows.any()):
        return torch.zeros(ref.shape[1], dtype=torch.float64)
    return err[rows].max(dim=0).values


# The float32 oracle's own value of record_measure against the float64 record, the largest over every case and both
# views, as tests/test_oracle_preprocess_records.py::test_float32_floor prints and asserts it (rounded up).  The GPU
# bounds are TOL_FACTOR x these.
FLOORS = {                  # measured maximum (the same in every degree pair unless noted), rounded up
    "x": 2.2e-7,            # 1.99e-7
    "y": 6.4e-7,            # 5.74e-7
    "conic_a": 8.2e-7,      # 7.27e-7 (7.41e-7 with antialiasing and scale_modifier 0.7)
    "conic_b": 5.8e-6,      # 5.18e-6: the off-diagonal term cancels where the footprint is nearly axis-aligned
    "conic_c": 9.6e-7,      # 7.80e-7 (8.69e-7 with antialiasing and scale_modifier 0.7)
    "opacity": 1.1e-7,      # 9.45e-8: the sigmoid alone
    "opacity_aa": 7.5e-7,   # 6.72e-7: times h = sqrt(det0 / det)
    "r": 4.0e-7,            # 3.61e-7 at SH 3; 2.4e-7 at SH 2, 1.6e-7 at SH 1, 9.4e-8 at SH 0
    "g": 4.0e-7,            # 3.43e-7
    "b": 4.0e-7,            # 3.37e-7
    "invdepth": 2.7e-7,     # 2.43e-7
    "depth": 9.0e-8,        # 8.02e-8
}


def floor_key(name, aa):
    return "opacity_aa" if (name == "opacity" and aa) else name


def record_tol(name, aa):
    return TOL_FACTOR * FLOORS[floor_key(name, aa)]


def gpu_record(parsed):
    """[P, 11] float32 of a parsed result: the record's ten continuous outputs; column 10 (the depth) is NaN -- the
    depth lives in the key, tested apart."""
    rec = parsed["rec"]
    out = np.full((rec.shape[0], 11), np.nan, dtype=np.float32)
    out[:, :10] = rec[:, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)]
    return out


# ------------------------------------------------------------------ every path of one case (GPU)
def run_case(case, layouts=LAYOUTS, sizes=SIZES, raws=(True, False)):
    """{(P, view, raw, layout): run_preprocess's arrays} of one case of the branch scene, through gslm_preprocess."""
    model, cams, o32s, _ = oracle_case(case)
    out = {}
    for P in sizes:
        vals = model_values(model, P)
        for b, cam in enumerate(cams):
            view = view_of(cam, case)
            for raw in raws:
                for name in layouts:
                    L = Layout(name, vals, raw, "cuda", colors=o32s[b]["rgb"][:P] if name == "colors" else None)
                    assert L.stage_lead() == L.expected_lead(), (name, P, L.stage_lead())
                    out[(P, b, raw, name)] = run_preprocess(L, view)
    return out
