"""Yardsticks of diag(J^T W J + D) and of Jacobi-preconditioned CG on the CPU oracle (tests/test_oracle_lm_diag.py,
tests/test_gpu_lm_diag.py).

jacobian_diag   the diagonal from the dense Jacobian of the [r; r] residual: one reverse pass per residual element
                (retain_graph), diag = 2 sum_rows J^2 (+ D), xyz and exposure masked as OracleLMProblem._mask does.
                The residual is built per tile (torch_raster's own preprocess, binning and _blend_tile), so a reverse
                pass walks one tile's blend, not the image's.
closed_form     the same number from the formula the kernels implement, in torch from the oracle's per-pixel
                quantities: per (entry, pixel) visit g_c = (col_c - acc_c) T - T_final bg_c / (1 - alpha),
                w = 2 sum_c w_c g_c^2, d alpha / d(a, b, c, o) = G (-o dx^2 / 2, -o dx dy, -o dy^2 / 2, 1) (the 0.99
                clamp ignored), S = sum w G^2 d d^T, diag_j = c_j^T S c_j with c_j from autograd of the preprocess,
                and (d rgb_c / d sh_k)^2 sum 2 w_c (alpha T)^2 for the SH groups.
pcg_ref         cgls_ref with a diagonal preconditioner, float64 scalars; with minv = 1 its iterates are cgls_ref's.

Bounds of the GPU comparison (tests/test_gpu_lm_diag.py): 8 x the float32 oracle's own distance from the float64
diagonal, per group, relative to the group's max (tests/test_oracle_lm_diag.py::test_float32_floor measures it and
asserts it stays below the recorded floors), capped at MAX_TOL: a row read from the wrong slot is an O(1) error."""
import math

import torch

from gslm.params import GROUPS, ParamLayout
from oracle import torch_raster as tr
from oracle.lm_ref import DEFAULT_DAMP

DIAG_GROUPS = ("features_dc", "features_rest", "scaling", "rotation", "opacity")
# float32 oracle vs float64 yardstick (jacobian_diag in both), max |d32 - d64| / max |d64| per group, measured on
#   sh1_33x17 / sh3_40x33 (generic background, masked, brightened), the chain-branch scene (64x48, antialiasing,
#   scale_modifier 0.7) and stack_scene(129, 16, 16):
#   features_dc   5.3e-7  9.5e-7  2.7e-7  1.7e-7      features_rest 4.7e-7  7.9e-7  2.4e-7  2.5e-7
#   scaling       6.7e-7  5.4e-7  6.8e-7  1.6e-6      rotation      8.5e-7  1.4e-6  5.7e-7  5.9e-7
#   opacity       4.8e-7  7.8e-7  2.4e-7  1.3e-7
# (the float32 closed form sits at the same distance: 3.6e-7, 3.4e-7, 2.6e-6, 9.8e-7, 2.4e-7 on the chain-branch scene)
F32_FLOOR = {"features_dc": 1.0e-6, "features_rest": 8.5e-7, "scaling": 2.6e-6, "rotation": 1.5e-6, "opacity": 8.5e-7}
MAX_TOL = 1e-3
CHUNK = 128  # rows of J per batched reverse pass
GPU_TOL = {k: min(8.0 * v, MAX_TOL) for k, v in F32_FLOOR.items()}


def _leaves(m):
    return [m._xyz, m._features_dc, m._features_rest, m._scaling, m._rotation, m._opacity, m._exposure]


def layout_of(model):
    return ParamLayout(model._xyz.shape[0], 1 + model._features_rest.shape[1], model._exposure.shape[0])


def damp_vector(layout, damp=None, dtype=torch.float64):
    damp = DEFAULT_DAMP if damp is None else damp
    d = torch.zeros(layout.numel, dtype=dtype)
    for g in GROUPS:
        a, b = layout.offsets[g]
        d[a:b] = damp[g]
    return d


def _pre(model, cam, bg, scale_modifier, antialiasing):
    st = tr.settings_from_camera(cam, bg, model.active_sh_degree, scale_modifier=scale_modifier,
                                 antialiasing=antialiasing)
    xyz = model.get_xyz
    pre = tr.preprocess(xyz, torch.zeros_like(xyz), model.get_opacity, model.get_features, None, model.get_scaling,
                        model.get_rotation, None, st)
    point_list, _, ranges = tr.binning(pre)
    return st, pre, point_list, ranges


def tile_residuals(model, cam, bg, scale_modifier=1.0, antialiasing=False, tiles=None):
    """[(tile, residual [npx, 3], raw colour, py, px)] of one view: r = m clamp01(R) - gt, tile by tile."""
    st, pre, point_list, ranges = _pre(model, cam, bg, scale_modifier, antialiasing)
    H, W = int(st.image_height), int(st.image_width)
    gx, gy = pre["grid"]
    dtype = pre["xy"].dtype
    bgt = torch.as_tensor(bg).to(dtype).reshape(3)
    invd = 1.0 / pre["depth"]
    out = []
    for t in range(gx * gy):
        if tiles is not None and t not in tiles:
            continue
        s, e = int(ranges[t, 0]), int(ranges[t, 1])
        if e <= s:
            continue  # background only: no dependence on the parameters
        py, px = tr._tile_pixels(t, gx, H, W)
        col = tr._blend_tile(pre["xy"], pre["conic"], pre["opacity"], pre["rgb"], invd, point_list[s:e], px, py, bgt)[0]
        m = cam.alpha_mask.to(dtype).reshape(H, W)[py, px][:, None]
        gt = cam.original_image.to(dtype)[:, py, px].t()
        out.append((t, col.clamp(0, 1) * m - gt, col, py, px))
    return out


def jacobian_diag(model, cams, bg, damp=True, scale_modifier=1.0, antialiasing=False, tiles=None, damp_values=None):
    """diag(2 sum_views J^T J) (+ D) from the dense Jacobian, in the model's dtype and the reference's layout."""
    leaves = _leaves(model)
    acc = [torch.zeros_like(t) for t in leaves]
    for cam in cams:
        for _, r, _, _, _ in tile_residuals(model, cam, bg, scale_modifier, antialiasing, tiles):
            flat = r.reshape(-1)
            eye = torch.eye(flat.numel(), dtype=flat.dtype)
            for k0 in range(0, flat.numel(), CHUNK):
                # the reverse passes of CHUNK residual elements, batched (one row of J each)
                grads = torch.autograd.grad(flat, leaves, grad_outputs=eye[k0:k0 + CHUNK], retain_graph=True,
                                            allow_unused=True, is_grads_batched=True)
                for a, gr in zip(acc, grads):
                    if gr is not None:
                        a += (gr * gr).sum(dim=0)
    lay = layout_of(model)
    d = 2.0 * torch.cat([a.reshape(-1) for a in acc]).detach()
    for name in ("xyz", "exposure"):
        a, b = lay.offsets[name]
        d[a:b] = 0
    if damp:
        d = d + damp_vector(lay, damp_values, d.dtype)
    return d


def closed_form(model, cam, bg, scale_modifier=1.0, antialiasing=False, tiles=None):
    """diag(2 J^T J) of one view (no D) from the per-visit formula; the model's dtype, the reference's layout."""
    leaves = _leaves(model)
    st, pre, point_list, ranges = _pre(model, cam, bg, scale_modifier, antialiasing)
    H, W = int(st.image_height), int(st.image_width)
    gx, gy = pre["grid"]
    P = model._xyz.shape[0]
    dtype = pre["xy"].dtype
    bgt = torch.as_tensor(bg).to(dtype).reshape(3)
    S = torch.zeros(P, 4, 4, dtype=dtype)
    Scol = torch.zeros(P, 3, dtype=dtype)
    with torch.no_grad():
        xy, conic, opac, rgb = pre["xy"], pre["conic"], pre["opacity"], pre["rgb"]
        for t in range(gx * gy):
            if tiles is not None and t not in tiles:
                continue
            s, e = int(ranges[t, 0]), int(ranges[t, 1])
            if e <= s:
                continue
            L = point_list[s:e]
            py, px = tr._tile_pixels(t, gx, H, W)
            power, araw = tr._power_alpha(xy, conic, opac, L, px, py)
            contrib = tr._decisions(power, araw)[0]
            m = contrib.to(dtype)
            alpha = m * torch.clamp_max(araw, 0.99)
            G = m * torch.exp(power)
            Tin = torch.cumprod(1 - alpha, dim=1)
            Tex = torch.cat([torch.ones(len(py), 1, dtype=dtype), Tin[:, :-1]], dim=1)  # T in front of the entry
            Tfin = Tin[:, -1]
            col = rgb[L]  # [n, 3]
            R = (alpha * Tex) @ col + Tfin[:, None] * bgt[None]
            mk = cam.alpha_mask.to(dtype).reshape(H, W)[py, px]
            w = (mk * mk)[:, None] * ((R >= 0) & (R <= 1)).to(dtype)  # [npx, 3]
            # the colour accumulated behind entry i: acc_i = sum_{j > i} col_j alpha_j T_j / T_{i+1}
            n = len(L)
            acc = torch.zeros(len(py), 3, dtype=dtype)
            om = torch.zeros(len(py), n, dtype=dtype)
            for i in range(n - 1, -1, -1):
                g = (col[i][None] - acc) * Tex[:, i:i + 1] - Tfin[:, None] * bgt[None] / (1 - alpha[:, i:i + 1])
                om[:, i] = 2.0 * (w * g * g).sum(dim=1)
                acc = alpha[:, i:i + 1] * col[i][None] + (1 - alpha[:, i:i + 1]) * acc
            dx = xy[L, 0][None] - px.to(dtype)[:, None]
            dy = xy[L, 1][None] - py.to(dtype)[:, None]
            o = opac[L][None]
            d = torch.stack([-0.5 * o * dx * dx, -o * dx * dy, -0.5 * o * dy * dy, torch.ones_like(dx)], dim=2)
            wg = om * G * G  # zero where the pixel does not blend the entry
            S.index_add_(0, L, torch.einsum("pn,pni,pnj->nij", wg, d, d))
            aT = alpha * Tex
            Scol.index_add_(0, L, 2.0 * torch.einsum("pc,pn->nc", w, aT * aT))
    # c_j = d(conic a, b, c, effective opacity) / d parameter j, per Gaussian (each depends on its own Gaussian only)
    outs = [pre["conic"][:, 0], pre["conic"][:, 1], pre["conic"][:, 2], pre["opacity"]]
    geo = [model._scaling, model._rotation, model._opacity]
    C = []
    for y in outs:
        gr = torch.autograd.grad(y.sum(), geo, retain_graph=True, allow_unused=True)
        C.append(torch.cat([(g if g is not None else torch.zeros_like(t)).reshape(P, -1) for g, t in zip(gr, geo)],
                           dim=1))
    C = torch.stack(C, dim=1)  # [P, 4, 8]
    dgeo = torch.einsum("pij,pik,pkj->pj", C, S, C)  # [P, 8]
    sh = [model._features_dc, model._features_rest]
    dsh = [torch.zeros_like(t) for t in sh]
    for c in range(3):
        gr = torch.autograd.grad(pre["rgb"][:, c].sum(), sh, retain_graph=True, allow_unused=True)
        for acc_t, g in zip(dsh, gr):
            if g is not None:
                acc_t += g * g * Scol[:, c][:, None, None]
    lay = layout_of(model)
    out = torch.zeros(lay.numel, dtype=dtype)
    v = lay.views(out)
    v["features_dc"].copy_(dsh[0].detach())
    v["features_rest"].copy_(dsh[1].detach())
    v["scaling"].copy_(dgeo[:, 0:3].detach())
    v["rotation"].copy_(dgeo[:, 3:7].detach())
    v["opacity"].copy_(dgeo[:, 7:8].detach())
    return out


def group_errors(got, ref, layout, groups=DIAG_GROUPS):
    """{group: max |got - ref| / max |ref|} in float64."""
    out = {}
    gv, rv = layout.views(got.double()), layout.views(ref.double())
    for k in groups:
        if rv[k].numel():
            out[k] = float((gv[k] - rv[k]).abs().max() / rv[k].abs().max().clamp_min(1e-300))
    return out


def pcg_ref(op, g, minv, max_iter, restart_iter, tol=1e-10, atol=0.0, history=None):
    """cgls_ref (oracle/lm_ref.py) with z = minv (.) s, gamma = <s, z>, p = z + beta p; float64 scalars.  history (a
    list, optional) receives phi(x_k) = x^T A x / 2 - g^T x after every iteration, from the monitor
    b^2 - <x, g> - <x, s> = b^2 + 2 phi (s = g - A x)."""
    vdot = lambda a, b: float((a.double() * b.double()).sum())
    x = torch.zeros_like(g)
    b2 = float(op.loss)
    iter_total, last_res, first = 0, math.inf, True
    q = torch.zeros_like(x)
    while iter_total < max_iter:
        if first:
            s = g.clone()
            first = False
        else:
            s = g - op.matvec(x, q)
        z = minv * s
        p = z.clone()
        gamma = vdot(s, z)
        stop = False
        for _ in range(restart_iter):
            op.matvec(p, q)
            delta = vdot(p, q)
            if delta < 1e-20:
                stop = True
                break
            alpha = gamma / delta
            x = x + alpha * p
            s = s - alpha * q
            z = minv * s
            gamma_new = vdot(s, z)
            p = z + (gamma_new / gamma) * p
            res = b2 - vdot(x, g) - vdot(x, s)
            if history is not None:
                history.append(0.5 * (res - b2))
            if res > last_res:
                stop = True
                break
            last_res = res
            if gamma_new < max(tol * math.sqrt(max(gamma, 0.0)), atol):
                stop = True
                break
            gamma = gamma_new
            iter_total += 1
            if iter_total >= max_iter:
                stop = True
                break
        if stop:
            break
    return x
