"""The float64 per-Gaussian Jacobian of the render record, and the two error measures the chain-rule tests use.

F_b(raw leaves of Gaussian i) = (xy_pix[2], conic[3], opacity_eff, rgb[3], 1 / depth) of view b, taken from
oracle.torch_raster.preprocess in float64 with sigmoid, exp and normalize applied in torch -- the oracle carries the
reference's linearisation quirks (tan-FoV clamp, SH clamp mask, antialiasing clamp), so nothing is restated here.
jacobian() differentiates it by forward-mode AD, one unit tangent per input column (the 59 passes at SH 3 batched
along the Gaussian axis: preprocess is elementwise per Gaussian): J[P, 10, C], C = 3 + 3 + 3 (K - 1) + 3 + 4 + 1 in
the flat layout's group order xyz, features_dc, features_rest, scaling, rotation, opacity.

Record conventions, read off chain_jvp (csrc/gslm_chain.hpp), which F's output order follows:
  T2[0..1]  the pixel-space xy tangent (d xy_pix = 0.5 W d ndc_x, 0.5 H d ndc_y);
  T2[2..4]  the conic tangent in the order (a, b, c) = the columns of pre["conic"] = (c11, -c01, c00) / det;
  T2[5]     the effective opacity's (sigmoid(o) h, h the antialiasing factor);
  T2[6..8]  rgb's (zero on a clamped channel);
  T2[9]     d(1 / t.z).
gslm_tangent_views stores T2[2..8] and a zero (8 floats, mask_xyz) or T2[0..9] and two zeros (12 floats);
gslm_gather_screen's rows are the cotangents of T2[2..8] and the flags word.

Measures (no blow-up under cancellation: a plain per-Gaussian relative error reaches 9e-4 for the float32 oracle itself):
  forward   per (Gaussian, output o):  |T - (J v)[o]| / sum_k |J[o, k]| |v[k]|
  reverse   per (Gaussian, group g):   max_k |y - ref| / max_k (|J|^T |s| + |d v|),  k over the group's columns
"""
import functools

import torch
import torch.autograd.forward_ad as fwAD
import torch.nn.functional as F

from oracle import torch_raster as tr
from scenes import to_float64

N_OUT = 10
GROUP_NAMES = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity")
OUT_NAMES = ("x", "y", "conic_a", "conic_b", "conic_c", "opacity", "r", "g", "b", "invdepth")


def group_slices(K):
    """name -> slice of the Jacobian's columns."""
    widths = (3, 3, 3 * (K - 1), 3, 4, 1)
    out, off = {}, 0
    for n, w in zip(GROUP_NAMES, widths):
        out[n] = slice(off, off + w)
        off += w
    return out


def n_columns(K):
    return 14 + 3 * (K - 1)


def leaves_of(model):
    m = model
    P = m._xyz.shape[0]
    return [m._xyz.detach(), m._features_dc.detach().reshape(P, 3), m._features_rest.detach().reshape(P, -1),
            m._scaling.detach(), m._rotation.detach(), m._opacity.detach()]


def record_fn(leaves, st):
    """The render record [n, 10] of every Gaussian from its raw leaves (the dtype of the leaves)."""
    xyz, dc, rest, scaling, rotation, opacity = leaves
    n = xyz.shape[0]
    shs = torch.cat([dc.reshape(n, 1, 3), rest.reshape(n, -1, 3)], dim=1)
    pre = tr.preprocess(xyz, torch.zeros_like(xyz), torch.sigmoid(opacity), shs, None, torch.exp(scaling),
                        F.normalize(rotation), None, st)
    return torch.cat([pre["xy"], pre["conic"], pre["opacity"][:, None], pre["rgb"], (1.0 / pre["depth"])[:, None]],
                     dim=1)


def settings(cam, D, aa, scale_modifier, dtype):
    return tr.settings_from_camera(cam, torch.zeros(3, dtype=dtype), D, scale_modifier=scale_modifier,
                                   antialiasing=aa)


def jacobian(model, cam, aa=False, scale_modifier=1.0):
    """J[P, 10, C] (float64) of F at the model's leaves for one camera, by forward-mode AD."""
    mc, (cc,) = to_float64(model, [cam])
    st = settings(cc, mc.active_sh_degree, aa, scale_modifier, torch.float64)
    lv = leaves_of(mc)
    P = lv[0].shape[0]
    C = sum(t.shape[1] for t in lv)
    eye = torch.eye(C, dtype=torch.float64)
    prim, tang, off = [], [], 0
    for t in lv:
        w = t.shape[1]
        prim.append(t.repeat(C, 1))
        # block c of the batch carries the unit tangent of column c
        tang.append(eye[:, off:off + w].repeat_interleave(P, dim=0))
        off += w
    with torch.no_grad(), fwAD.dual_level():
        out = record_fn([fwAD.make_dual(p, t) for p, t in zip(prim, tang)], st)
        jt = fwAD.unpack_dual(out).tangent
    return jt.reshape(C, P, N_OUT).permute(1, 2, 0).contiguous()


def per_gaussian(layout, flat):
    """[P, C] rows (float64, on the CPU) of a flat param-space vector of the full layout, exposure dropped."""
    views = layout.views(flat.detach().cpu().double())
    return torch.cat([views[n].reshape(layout.P, -1) for n in GROUP_NAMES], dim=1)


def forward_measure(T, J, v, visible):
    """max over the visible Gaussians of |T - J v| / (|J| |v|) per output: [10].  T [P, 10], v [P, C]."""
    ref = torch.einsum("poc,pc->po", J, v)
    den = torch.einsum("poc,pc->po", J.abs(), v.abs())
    err = (T.double() - ref).abs()
    ok = err <= 1e-30
    ratio = torch.where(ok, torch.zeros_like(err), err / den.clamp_min(1e-300))
    return ratio[visible].max(dim=0).values if bool(visible.any()) else torch.zeros(N_OUT, dtype=torch.float64)


def reverse_reference(Js, ss, viss):
    """(sum_b J_b^T s_b, sum_b |J_b|^T |s_b|) per Gaussian: [P, C] each.  ss[b]: [P, 10] cotangents; viss[b]: [P]."""
    ref = torch.zeros(Js[0].shape[0], Js[0].shape[2], dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for J, s, vis in zip(Js, ss, viss):
        m = vis.double()[:, None]
        ref += m * torch.einsum("poc,po->pc", J, s.double())
        mag += m * torch.einsum("poc,po->pc", J.abs(), s.double().abs())
    return ref, mag


def reverse_measure(y, ref, mag, K, rows=None):
    """name -> max over Gaussians (rows: a mask) of max_k |y - ref| / max_k mag over the group's columns."""
    out = {}
    for n, sl in group_slices(K).items():
        if sl.stop == sl.start:
            continue
        err = (y[:, sl].double() - ref[:, sl]).abs().max(dim=1).values
        den = mag[:, sl].max(dim=1).values
        ratio = torch.where(err <= 1e-30, torch.zeros_like(err), err / den.clamp_min(1e-300))
        if rows is not None:
            ratio = ratio[rows]
        out[n] = float(ratio.max()) if ratio.numel() else 0.0
    return out


def flags_word(visible, clamped):
    """The flags word of gslm_view_flags / the SCREEN rows from the oracle: bit 31 visible, bits 0-2 the SH clamp mask
    (0 for an invisible Gaussian), int64 [P]."""
    bits = (clamped[:, 0].long() | (clamped[:, 1].long() << 1) | (clamped[:, 2].long() << 2))
    return torch.where(visible, bits | (1 << 31), torch.zeros_like(bits))


# ---- the branch scene's cases, shared by the CPU floor test and the GPU tests
DEGREES = [(0, 0), (1, 1), (2, 1), (3, 3), (3, 0)]   # (stored, active) SH degree


@functools.lru_cache(maxsize=None)
def branch_case(max_degree=3, active_degree=3, aa=False, scale_modifier=1.0):
    """(model, cams, [J per view], [stats per view]) of the branch scene for one case; computed once, never modified."""
    from scenes import assert_chain_branch_scene, chain_branch_scene, sh_subset
    model, cams = chain_branch_scene()
    stats = [assert_chain_branch_scene(model, c, aa, scale_modifier) for c in cams]
    sub = sh_subset(model, max_degree, active_degree)
    if (max_degree, active_degree) != (3, 3):
        # the clamp bits and colours of the case's own degree
        from scenes import chain_branch_stats
        stats = [chain_branch_stats(sub, c, aa, scale_modifier) for c in cams]
    Js = [jacobian(sub, c, aa, scale_modifier) for c in cams]
    return sub, cams, Js, stats


def direction(layout, seed, only=None):
    """A random flat direction (exposure zero); only: the one group that is nonzero."""
    v = torch.randn(layout.numel, generator=torch.Generator().manual_seed(seed))
    for n, (a, b) in layout.offsets.items():
        if n == "exposure" or (only is not None and n != only):
            v[a:b] = 0
    return v


def cotangents(P, n_views, seed):
    """Random cotangents [n_views, P, 10] with the xy and inverse-depth entries zero (the screen rows carry conic,
    opacity and rgb only)."""
    s = torch.randn(n_views, P, N_OUT, generator=torch.Generator().manual_seed(seed))
    s[..., 0:2] = 0
    s[..., 9] = 0
    return s


def float32_forward(model, cam, aa, scale_modifier, vrows):
    """The float32 oracle's own J v by forward-mode AD: [P, 10].  vrows [P, C] (float32)."""
    st = settings(cam, model.active_sh_degree, aa, scale_modifier, torch.float32)
    lv = leaves_of(model)
    tang, off = [], 0
    for t in lv:
        tang.append(vrows[:, off:off + t.shape[1]].to(torch.float32).contiguous())
        off += t.shape[1]
    with torch.no_grad(), fwAD.dual_level():
        out = record_fn([fwAD.make_dual(p.clone(), t) for p, t in zip(lv, tang)], st)
        return fwAD.unpack_dual(out).tangent.clone()


def float32_reverse(model, cam, aa, scale_modifier, s, visible):
    """The float32 oracle's own J^T s by reverse-mode AD: [P, C].  s [P, 10]; rows of invisible Gaussians masked."""
    st = settings(cam, model.active_sh_degree, aa, scale_modifier, torch.float32)
    lv = [t.clone().requires_grad_(True) for t in leaves_of(model)]
    out = record_fn(lv, st)
    w = s.to(torch.float32) * visible[:, None].to(torch.float32)
    grads = torch.autograd.grad((out * w).sum(), lv, allow_unused=True)
    return torch.cat([g if g is not None else torch.zeros_like(t) for g, t in zip(grads, lv)], dim=1).detach()


# ---- float32 floors and the GPU tolerances built from them.
# Floors: the float32 oracle's own forward-mode J v / reverse-mode J^T s against the float64 J on the branch scene, the
# largest over both views, the five degree cases, scale_modifier 1.0 / 0.7 and (where not split) antialiasing off / on,
# as tests/test_oracle_chain_jacobian.py::test_float32_floor measures and asserts them.  The GPU bounds are 8 x the
# floor of the same measure (the factor covers the kernels' other operation order and their local FMA contraction); a
# wrong branch shows as O(1).
FLOORS = {                         # measured maximum, rounded up
    "forward": 7.5e-6,             # 6.9e-6 (rgb with v in xyz alone; conic 6.5e-6, x 4.0e-6): any output, any case, except
    "forward_opacity_aa": 4.5e-5,  # 4.01e-5: the effective opacity with antialiasing (det0 = c00 c11 - c01^2 cancels
                                   # in float32 for the thin Gaussians just above the clamp; 1.7e-5 .. 4.0e-5 by case)
    "forward_single_group": 6.5e-5,  # 6.07e-5: the conic with v in xyz, scaling or rotation alone
    "reverse": 1.2e-6,             # 1.05e-6: dc / rest / opacity, antialiasing off or on
    "reverse_scaling": 3.0e-6,     # 2.78e-6: scaling without antialiasing
    "reverse_scaling_aa": 1.2e-5,  # 1.13e-5: scaling with antialiasing
    "reverse_rotation": 1.1e-5,    # 1.03e-5 (4.1e-6 without antialiasing): rotation
}
MAX_TOL = 2e-4                     # no bound exceeds it: 8 x forward_opacity_aa and 8 x forward_single_group are cut to it
TOL_FACTOR = 8.0


SINGLE_GROUP_CASE = (False, 0.7)   # (antialiasing, scale_modifier) of the single-group cases
SINGLE_GROUPS = [("features_dc", 1), ("features_rest", 1), ("scaling", 1), ("rotation", 1), ("opacity", 1), ("xyz", 0),
                 ("features_rest", 0)]   # (the one group that carries v, mask_xyz)


def forward_floor_of(output, aa, only=None):
    """only: v lives in that one group.  The conic and opacity outputs of a geometry group on its own lose the other
    groups' terms of sum_k |J| |v| that otherwise cover the cancellation inside the conic's derivative."""
    if only in ("xyz", "scaling", "rotation") and output in ("conic_a", "conic_b", "conic_c", "opacity"):
        return FLOORS["forward_single_group"]
    return FLOORS["forward_opacity_aa" if (output == "opacity" and aa) else "forward"]


def reverse_floor_of(group, aa):
    if group == "rotation":
        return FLOORS["reverse_rotation"]
    if group == "scaling":
        return FLOORS["reverse_scaling_aa" if aa else "reverse_scaling"]
    return FLOORS["reverse"]


def forward_tol(output, aa, only=None):
    return min(TOL_FACTOR * forward_floor_of(output, aa, only), MAX_TOL)


def reverse_tol(group, aa):
    return min(TOL_FACTOR * reverse_floor_of(group, aa), MAX_TOL)
