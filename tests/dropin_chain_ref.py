"""Float64 references and cancellation-free error measures for the drop-in rasterizer's VJP and JVP, per Gaussian and
per pixel (tests/test_oracle_dropin_chain.py, tests/test_gpu_dropin_chain.py).

Everything comes from oracle/torch_raster.py in float64, split at the render record rec[i] = (xy[2], conic[3],
effective opacity, rgb[3], 1 / depth) of Gaussian i, as tests/test_cpu_baseline.py::test_split_backward_equals_unsplit
splits it:
  J[i]  [10, C]      the Jacobian of rec[i] with respect to the call's own inputs of Gaussian i (forward-mode AD through
                     tr.preprocess, batched along the Gaussian axis; preprocess is elementwise per Gaussian);
  D     [px, 4, i, 10] the Jacobian of a pixel's (r, g, b, inverse depth) with respect to the records of its tile's
                     list (torch.func.jacrev through tr._blend_tile, one pixel at a time under vmap, tile by tile).
The decisions (skip, clamp, stop, list order) are frozen at the float64 primal, as the oracle freezes them.

Reverse, per (Gaussian i, input tensor g):   max_k |y - ref| / max_k mag,   k over the tensor's columns of Gaussian i,
  ref = J_i^T s_i,  s_i[o] = sum_p u_p . D[p, :, i, o],   mag = |J_i|^T S_i,  S_i[o] = sum_p |u_p . D[p, :, i, o]|
  (S is the size of the screen cotangent without the cancellation between pixels; a Gaussian with mag == 0 in every
  column has radius 0 or is blended by no pixel and must get exactly 0).
Forward, per (pixel p, channel c):           |T - ref| / den,
  ref = sum_{i,o} D[p, c, i, o] (J_i v_i)[o],   den = sum_{i,o} |D[p, c, i, o]| (|J_i| |v_i|)[o]
  (a pixel-channel with den == 0 must get exactly 0).
No Gaussian and no pixel is left out of a maximum.

Bounds: min(8 x FLOORS[...], chain_jacobian.MAX_TOL), FLOORS the float32 oracle's own value of the same measure against
float64, measured on the CPU by tests/test_oracle_dropin_chain.py::test_float32_floors over every case below.
"""
import functools
from collections import namedtuple

import torch
import torch.autograd.forward_ad as fwAD
import torch.nn.functional as F

import chain_jacobian as cj
from oracle import torch_raster as tr
from scenes import chain_branch_scene, chain_branch_stats, sh_subset

N_REC = 10
BG = (0.25, 0.5, 0.75)

# One configuration of one call: view of the branch scene, antialiasing, scale_modifier, input form, (stored, active) SH
# degree, number of Gaussians (a prefix of the scene).  Forms: "plain" (scales, rotations, shs), "cov" (cov3D_precomp),
# "col" (colors_precomp), "cov_col", "split" (dc= and the SH rest), "raw" (the model's leaves, activations inside).
Cfg = namedtuple("Cfg", "view aa smod form degrees P opaque_thin",
                 defaults=(0, False, 1.0, "plain", (3, 3), 768, True))
# opaque_thin: the copy of the scene these tests run on gives the thin Gaussians (every 8th, offset 1: the ones under the
# antialiasing clamp) an opacity of 0.97.  Under the clamp the antialiasing factor is sqrt(2.5e-5) = 0.005, so with the
# scene's own opacities (below 0.78) their alpha stays under 1 / 255 at every pixel and nothing blends them: the clamp's
# branch of aa_grad would carry no gradient at all.  False: scenes.chain_branch_scene() as it is.
THIN_OPACITY = 0.97

CONFIGS = [(False, 1.0), (True, 0.7)]      # (antialiasing, scale_modifier): plain, and both options on
PREFIXES = (255, 256, 257, 513)


def reverse_cases():
    """Every configuration the reverse tests run (GaussianRasterizer and the raw C ABI)."""
    out = [Cfg(b, aa, sm) for aa, sm in CONFIGS for b in (0, 1)]
    out += [Cfg(0, True, 0.7, f) for f in ("cov", "col", "cov_col", "split")]
    out += [Cfg(0, True, 0.7, "plain", d) for d in cj.DEGREES if d != (3, 3)]
    out += [Cfg(0, True, 0.7, "plain", (3, 3), P) for P in PREFIXES]
    out += [Cfg(b, aa, sm, "raw") for aa, sm in CONFIGS for b in (0, 1)]
    return out


FORWARD_CFG = [Cfg(0, False, 0.7), Cfg(0, True, 0.7)]
FORWARD_SPLIT = Cfg(0, False, 0.7, "split")   # dc and rest as tangents of their own


def cfg_id(c):
    return f"v{c.view}-aa{int(c.aa)}-s{c.smod}-{c.form}-sh{c.degrees[0]}{c.degrees[1]}-P{c.P}"


# ---------------------------------------------------------------- inputs
def _columns(form, K):
    """Ordered (name, width) of the call's input tensors, each flattened to [P, width]."""
    if form == "raw":
        return [("xyz", 3), ("features_dc", 3), ("features_rest", 3 * (K - 1)), ("scaling", 3), ("rotation", 4),
                ("opacity", 1)]
    cols = [("means3D", 3), ("means2D", 3), ("opacities", 1)]
    cols += [("cov3D_precomp", 6)] if form in ("cov", "cov_col") else [("scales", 3), ("rotations", 4)]
    if form in ("col", "cov_col"):
        cols += [("colors_precomp", 3)]
    elif form == "split":
        cols += [("dc", 3), ("shs", 3 * (K - 1))]
    else:
        cols += [("shs", 3 * K)]
    return cols


def _shape(name, t, form):
    """A flat [P, w] column block in the shape the rasterizer takes."""
    P = t.shape[0]
    if name in ("shs", "dc"):
        return t.reshape(P, -1, 3)
    return t


def oracle_kwargs(form, x):
    """tr.rasterize / tr.preprocess keyword arguments from the flat inputs x (any dtype, plain or dual tensors)."""
    if form == "raw":
        n = x["xyz"].shape[0]
        shs = torch.cat([x["features_dc"].reshape(n, 1, 3), x["features_rest"].reshape(n, -1, 3)], dim=1)
        return dict(means3D=x["xyz"], means2D=torch.zeros_like(x["xyz"]), opacities=torch.sigmoid(x["opacity"]),
                    shs=shs, colors_precomp=None, scales=torch.exp(x["scaling"]),
                    rotations=F.normalize(x["rotation"]), cov3D_precomp=None)
    P = x["means3D"].shape[0]
    shs = None
    if "shs" in x:
        shs = x["shs"].reshape(P, -1, 3)
        if "dc" in x:
            shs = torch.cat([x["dc"].reshape(P, 1, 3), shs], dim=1)
    return dict(means3D=x["means3D"], means2D=x["means2D"], opacities=x["opacities"], shs=shs,
                colors_precomp=x.get("colors_precomp"), scales=x.get("scales"), rotations=x.get("rotations"),
                cov3D_precomp=x.get("cov3D_precomp"))


def gpu_kwargs(form, x):
    """GaussianRasterizer keyword arguments from the flat inputs x (form != "raw")."""
    return {n: _shape(n, t, form) for n, t in x.items()}


@functools.lru_cache(maxsize=None)
def _scene(degrees, P, opaque_thin=True):
    import copy
    from gslm.model import inverse_sigmoid
    model, cams = chain_branch_scene()
    sub = sh_subset(model, degrees[0], degrees[1])
    m = copy.deepcopy(sub)
    if opaque_thin:
        with torch.no_grad():
            m._opacity[1::8] = inverse_sigmoid(torch.tensor(THIN_OPACITY))
    m.set_params(m._xyz[:P], m._features_dc[:P], m._features_rest[:P], m._scaling[:P], m._rotation[:P],
                 m._opacity[:P], m._exposure, requires_grad=False)
    m.max_sh_degree, m.active_sh_degree = degrees
    return m, cams


def flat_inputs(cfg):
    """name -> float32 [P, w] CPU tensors of the call (fresh each time; the same values the GPU call gets)."""
    m, _ = _scene(cfg.degrees, cfg.P, cfg.opaque_thin)
    P = cfg.P
    with torch.no_grad():
        if cfg.form == "raw":
            return {"xyz": m._xyz.detach().clone(), "features_dc": m._features_dc.detach().reshape(P, 3).clone(),
                    "features_rest": m._features_rest.detach().reshape(P, -1).clone(),
                    "scaling": m._scaling.detach().clone(), "rotation": m._rotation.detach().clone(),
                    "opacity": m._opacity.detach().clone()}
        x = {"means3D": m.get_xyz.detach().clone(), "means2D": torch.zeros(P, 3),
             "opacities": m.get_opacity.detach().clone()}
        if cfg.form in ("cov", "cov_col"):
            # pc.get_covariance(scaling_modifier): the modifier is inside the covariance
            x["cov3D_precomp"] = tr.compute_cov3d(m.get_scaling.detach(), cfg.smod, m.get_rotation.detach()).contiguous()
        else:
            x["scales"], x["rotations"] = m.get_scaling.detach().clone(), m.get_rotation.detach().clone()
        shs = m.get_features.detach()
        if cfg.form in ("col", "cov_col"):
            # colours of both signs around the clamp's corner are plain inputs here: nothing clamps a precomputed colour
            x["colors_precomp"] = torch.rand(P, 3, generator=torch.Generator().manual_seed(21))
        elif cfg.form == "split":
            x["dc"], x["shs"] = shs[:, 0].reshape(P, 3).clone(), shs[:, 1:].reshape(P, -1).clone()
        else:
            x["shs"] = shs.reshape(P, -1).clone()
    return x


def oracle_settings(cfg, dtype):
    _, cams = _scene(cfg.degrees, cfg.P, cfg.opaque_thin)
    cam = cams[cfg.view]
    if dtype == torch.float64:
        import copy
        cam = copy.deepcopy(cam)
        for k in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
            setattr(cam, k, getattr(cam, k).double())
    return tr.settings_from_camera(cam, torch.tensor(BG, dtype=dtype), cfg.degrees[1], scale_modifier=cfg.smod,
                                   antialiasing=cfg.aa)


def camera(cfg):
    return _scene(cfg.degrees, cfg.P, cfg.opaque_thin)[1][cfg.view]


def _record(pre):
    return torch.cat([pre["xy"], pre["conic"], pre["opacity"][:, None], pre["rgb"], (1.0 / pre["depth"])[:, None]],
                     dim=1)


def _preprocess(cfg, x, st):
    kw = oracle_kwargs(cfg.form, x)
    return tr.preprocess(kw["means3D"], kw["means2D"], kw["opacities"], kw["shs"], kw["colors_precomp"], kw["scales"],
                         kw["rotations"], kw["cov3D_precomp"], st)


# ---------------------------------------------------------------- the float64 case
class Case:
    """The float64 reference of one configuration; computed once (case()), never modified."""

    def __init__(self, cfg):
        self.cfg = cfg
        m, _ = _scene(cfg.degrees, cfg.P, cfg.opaque_thin)
        self.K = 1 + m._features_rest.shape[1]
        self.cols = [(n, w) for n, w in _columns(cfg.form, self.K)]
        self.slices, off = {}, 0
        for n, w in self.cols:
            self.slices[n] = slice(off, off + w)
            off += w
        self.C = off
        self.x32 = flat_inputs(cfg)
        self.x64 = {n: t.double() for n, t in self.x32.items()}
        self.st = oracle_settings(cfg, torch.float64)
        self.H, self.W = int(self.st.image_height), int(self.st.image_width)
        with torch.no_grad():
            self.pre = _preprocess(cfg, self.x64, self.st)
            self.rec = _record(self.pre)
            self.point_list, _, self.ranges = tr.binning(self.pre)
            color, invd, _, self.n_contrib = tr.blend(self.pre, self.point_list, self.ranges, self.H, self.W, self.st.bg)
            self.image = torch.cat([color, invd], dim=0)   # [4, H, W]
        self.radii = self.pre["radii"]
        self.J = self._jacobian()

    def _jacobian(self):
        """J[P, 10, C] by forward-mode AD: block c of the batch carries the unit tangent of column c."""
        P, C = self.cfg.P, self.C
        eye = torch.eye(C, dtype=torch.float64)
        with torch.no_grad(), fwAD.dual_level():
            x = {}
            for n, w in self.cols:
                sl = self.slices[n]
                x[n] = fwAD.make_dual(self.x64[n].repeat(C, 1), eye[:, sl].repeat_interleave(P, dim=0))
            jt = fwAD.unpack_dual(_record(_preprocess(self.cfg, x, self.st))).tangent
        return jt.reshape(C, P, N_REC).permute(1, 2, 0).contiguous()

    def rows(self, tensors):
        """[P, C] float64 rows from a name -> tensor mapping (any shape with P leading); a missing name is zero."""
        out = torch.zeros(self.cfg.P, self.C, dtype=torch.float64)
        for n, _ in self.cols:
            if tensors.get(n) is not None:
                out[:, self.slices[n]] = tensors[n].detach().cpu().double().reshape(self.cfg.P, -1)
        return out

    def tiles(self):
        """Yields (flat pixel indices [npx], list L [n], D [npx, 4, n, 10]) of every nonempty tile."""
        gx, gy = self.pre["grid"]
        bg = self.st.bg

        for t in range(gx * gy):
            s, e = int(self.ranges[t, 0]), int(self.ranges[t, 1])
            if e <= s:
                continue
            py, px = tr._tile_pixels(t, gx, self.H, self.W)
            L = self.point_list[s:e]
            local = torch.arange(e - s)

            def one(r, x, y):
                col, dep, _, _ = tr._blend_tile(r[:, 0:2], r[:, 2:5], r[:, 5], r[:, 6:9], r[:, 9], local, x[None],
                                                y[None], bg)
                return torch.cat([col[0], dep])

            D = torch.func.vmap(torch.func.jacrev(one), in_dims=(None, 0, 0))(self.rec[L], px, py)
            yield py * self.W + px, L, D


@functools.lru_cache(maxsize=None)
def case(cfg):
    return Case(cfg)


def cotangent(cfg, seed=4):
    """Random colour and inverse-depth cotangents u [4, H, W] (float32 values)."""
    c = camera(cfg)
    return torch.randn(4, int(c.image_height), int(c.image_width), generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def reverse_reference(cfg, seed=4):
    """(ref [P, C], mag [P, C], S [P, 10]) for the cotangent of `seed`; computed once, never modified."""
    cs = case(cfg)
    u = cotangent(cfg, seed).double().reshape(4, -1)
    s = torch.zeros(cfg.P, N_REC, dtype=torch.float64)
    S = torch.zeros_like(s)
    for pix, L, D in cs.tiles():
        g = torch.einsum("pc,pcio->pio", u[:, pix].t(), D)
        s.index_add_(0, L, g.sum(dim=0))
        S.index_add_(0, L, g.abs().sum(dim=0))
    ref = torch.einsum("poc,po->pc", cs.J, s)
    mag = torch.einsum("poc,po->pc", cs.J.abs(), S)
    return ref, mag, S


def forward_reference(cfg, vs):
    """[(ref [4, H, W], den [4, H, W])] for each tangent v [P, C] (float64 rows) of vs, in one pass over the tiles."""
    cs = case(cfg)
    Jv = [torch.einsum("poc,pc->po", cs.J, v) for v in vs]
    Av = [torch.einsum("poc,pc->po", cs.J.abs(), v.abs()) for v in vs]
    out = [(torch.zeros(4, cs.H * cs.W, dtype=torch.float64), torch.zeros(4, cs.H * cs.W, dtype=torch.float64))
           for _ in vs]
    for pix, L, D in cs.tiles():
        Da = D.abs()
        for k in range(len(vs)):
            out[k][0][:, pix] = torch.einsum("pcio,io->cp", D, Jv[k][L])
            out[k][1][:, pix] = torch.einsum("pcio,io->cp", Da, Av[k][L])
    return [(r.reshape(4, cs.H, cs.W), d.reshape(4, cs.H, cs.W)) for r, d in out]


# ---------------------------------------------------------------- measures
def _ratio(err, den):
    return torch.where(err <= 1e-30, torch.zeros_like(err), err / den.clamp_min(1e-300))


def reverse_measure(cs, yrows, ref, mag, names=None):
    """(name, thin) -> max over the Gaussians of that class (the two classes cover ALL Gaussians) of
    max_k |y - ref| / max_k mag over the input tensor's columns.  names: the tensors to measure (default: all)."""
    is_thin = thin(cs.cfg)
    out = {}
    for n, w in cs.cols:
        if w == 0 or (names is not None and n not in names):
            continue
        sl = cs.slices[n]
        err = (yrows[:, sl] - ref[:, sl]).abs().max(dim=1).values
        r = _ratio(err, mag[:, sl].max(dim=1).values)
        for t, rows in ((False, ~is_thin), (True, is_thin)):
            out[(n, t)] = float(r[rows].max()) if bool(rows.any()) else 0.0
    return out


def forward_measure(T, ref, den):
    """[4]: max over ALL pixels of |T - ref| / den per channel (r, g, b, inverse depth).  T [4, H, W]."""
    err = (T.detach().cpu().double() - ref).abs()
    return _ratio(err, den).reshape(4, -1).max(dim=1).values


# ---------------------------------------------------------------- the oracle end to end, either precision
def oracle_reverse(cfg, u, dtype):
    """The oracle's own reverse-mode gradient rows [P, C] (float64 container) of <u, (colour, inverse depth)>, and its
    (radii, n_contrib)."""
    cs = case(cfg)
    x = {n: t.to(dtype).clone().requires_grad_(True) for n, t in cs.x32.items()}
    st = oracle_settings(cfg, dtype)
    color, radii, invd, I = tr.rasterize(st=st, return_internals=True, **oracle_kwargs(cfg.form, x))
    loss = (color * u[:3].to(dtype)).sum() + (invd * u[3:].to(dtype)).sum()
    names = [n for n, w in cs.cols if w > 0]
    grads = torch.autograd.grad(loss, [x[n] for n in names], allow_unused=True)
    return cs.rows(dict(zip(names, grads))), radii, I["n_contrib"]


def oracle_forward(cfg, vrows, dtype):
    """The oracle's own forward-mode tangent [4, H, W] for the tangent rows [P, C]."""
    cs = case(cfg)
    st = oracle_settings(cfg, dtype)
    with torch.no_grad(), fwAD.dual_level():
        x = {n: fwAD.make_dual(t.to(dtype).clone(), vrows[:, cs.slices[n]].to(dtype).contiguous())
             for n, t in cs.x32.items()}
        color, _, invd = tr.rasterize(st=st, **oracle_kwargs(cfg.form, x))
        return torch.cat([fwAD.unpack_dual(color).tangent, fwAD.unpack_dual(invd).tangent], dim=0).clone()


# ---------------------------------------------------------------- decisions
def decision_margins(cfg, dtype=torch.float64):
    """The blend's decisions of every tile in `dtype`: (smallest relative distance of a seen entry's alpha from 1/255
    and from 0.99 and of a blended entry's transmittance from 1e-4, [(skip, clamp, stop masks)] per tile)."""
    cs = case(cfg)
    x = {n: t.to(dtype) for n, t in cs.x32.items()}
    st = oracle_settings(cfg, dtype)
    with torch.no_grad():
        pre = _preprocess(cfg, x, st)
        pl, _, ranges = tr.binning(pre)
    gx, gy = pre["grid"]
    margin = dict(skip=float("inf"), clamp=float("inf"), stop=float("inf"))
    masks = []
    for t in range(gx * gy):
        d = tr.tile_decisions(pre, pl, ranges, t, cs.H, cs.W)
        if d is None:
            continue
        seen = d["seen"] & (d["power"] <= 0)
        a = d["alpha_raw"].double()
        margin["skip"] = min(margin["skip"], float((a * 255.0 - 1).abs()[seen].min()))
        margin["clamp"] = min(margin["clamp"], float((a / 0.99 - 1).abs()[seen].min()))
        blended = d["seen"] & d["valid"]
        if bool(blended.any()):
            margin["stop"] = min(margin["stop"], float((d["test_T"].double() / 1e-4 - 1).abs()[blended].min()))
        masks.append((d["seen"], d["seen"] & d["valid"], seen & (a > 0.99), blended & (d["test_T"] < 1e-4)))
    return margin, masks, pl, pre["radii"]


# ---------------------------------------------------------------- branch classes and tangent supports
def branch_classes(cfg):
    """name -> bool [P]: the Gaussians of each branch class (float64 oracle data of the configuration's own view)."""
    m, cams = _scene(cfg.degrees, cfg.P, cfg.opaque_thin)
    s = chain_branch_stats(m, cams[cfg.view], cfg.aa, cfg.smod)
    return {"outside_fov": s["outx"] | s["outy"], "under_aa": s["under_aa"], "sh_clamped": s["clamped"].any(dim=1)}


def tangent_rows(cfg, seed=3, only=None, rows=None):
    """Random tangent rows [P, C] of float32 values (float64 container); only: the one input tensor that is nonzero;
    rows: a bool [P] mask of the Gaussians that are."""
    cs = case(cfg)
    v = torch.randn(cfg.P, cs.C, generator=torch.Generator().manual_seed(seed)).double()
    if cfg.form != "raw":
        v[:, cs.slices["means2D"].start + 2] = 0   # the third means2D column is unused
    if only is not None:
        keep = torch.zeros(cs.C, dtype=torch.bool)
        keep[cs.slices[only]] = True
        v[:, ~keep] = 0
    if rows is not None:
        v[~rows] = 0
    return v


def forward_supports(cfg):
    """[(name, tangent rows [P, C])]: every input at once, each input tensor alone, each branch class alone (every other
    Gaussian's tangent zero, so that den holds that class only)."""
    cs = case(cfg)
    sup = [("all", tangent_rows(cfg))]
    sup += [(n, tangent_rows(cfg, only=n)) for n, w in cs.cols if w]
    sup += [(k, tangent_rows(cfg, rows=m)) for k, m in branch_classes(cfg).items()]
    return sup


@functools.lru_cache(maxsize=None)
def forward_references(cfg):
    """name -> (tangent rows, ref [4, H, W], den [4, H, W]) of forward_supports(cfg); computed once, never modified."""
    sup = forward_supports(cfg)
    refs = forward_reference(cfg, [v for _, v in sup])
    return {n: (v, r, d) for (n, v), (r, d) in zip(sup, refs)}


def thin(cfg):
    """bool [P]: the Gaussians whose det0 / det lies under the antialiasing clamp's 2.5e-5 (whatever the setting)."""
    return branch_classes(cfg)["under_aa"]


# ---------------------------------------------------------------- float32 floors and the bounds built from them
# The float32 oracle's own reverse-mode gradient / forward-mode tangent against the float64 reference in the measures
# above, the largest over the cases named, as tests/test_oracle_dropin_chain.py::test_float32_floors measures and
# asserts them.  The bounds are 8 x the floor (the kernels' other operation order and their local FMA contraction), cut
# to chain_jacobian.MAX_TOL.
#
# Reverse floors are kept per kind of input tensor, per antialiasing setting and per class of Gaussian.  The thin
# Gaussians (thin(): a screen footprint that is the 0.3 low-pass alone) are blended only by a pixel or two next to
# their centre, above all with antialiasing, where their factor h = 0.005 leaves alpha >= 1 / 255 within 0.34 pixels
# of the centre.  There d = xy - pixel is a difference of two numbers of size 30 .. 60 that float32 holds to 4e-6, a
# relative error of 1e-5 .. 1e-4 in d and twice that in the conic's cotangent (which is quadratic in d) -- in the
# oracle's float32 as in any float32 rasterizer, and the only route by which the scales, rotations and covariances
# of these Gaussians are reached.  S cannot see a cancellation inside one pixel's own derivative, so these Gaussians
# carry a floor of their own rather than lifting everyone's.
KINDS = {"means3D": "geometry", "means2D": "geometry", "scales": "geometry", "rotations": "geometry",
         "cov3D_precomp": "geometry", "xyz": "geometry", "scaling": "geometry", "rotation": "geometry",
         "opacities": "opacity", "opacity": "opacity",
         "shs": "colour", "dc": "colour", "colors_precomp": "colour", "features_dc": "colour",
         "features_rest": "colour"}
FLOORS = {                               # measured maximum, rounded up; x 8 -> the bound
    "reverse_geometry": 8.0e-6,           # 6.76e-6
    "reverse_geometry_aa": 1.6e-5,        # 1.35e-5
    "reverse_geometry_thin": 3.0e-5,      # 2.52e-5  (cut to 2e-4)
    "reverse_geometry_aa_thin": 1.5e-4,   # 1.27e-4  cov3D_precomp; scales 9.9e-5, rotations 7.1e-5 (cut to 2e-4)
    "reverse_opacity": 1.0e-5,            # 8.39e-6
    "reverse_opacity_aa": 1.8e-5,         # 1.53e-5
    "reverse_opacity_thin": 3.3e-5,       # 2.85e-5  (cut to 2e-4)
    "reverse_opacity_aa_thin": 2.4e-5,    # 2.01e-5
    "reverse_colour": 9.0e-6,             # 7.41e-6
    "reverse_colour_aa": 1.5e-5,          # 1.29e-5
    "reverse_colour_thin": 3.0e-5,        # 2.60e-5  (cut to 2e-4)
    "reverse_colour_aa_thin": 4.0e-6,     # 3.26e-6
    "forward": 1.2e-5,                    # 9.77e-6  every input at once, each input but means2D, the other classes
    "forward_means2D": 3.2e-5,            # 2.76e-5  (cut to 2e-4)
    "forward_thin": 3.2e-5,               # 2.77e-5  (cut to 2e-4)
}
# Forward floors by tangent support: a means2D tangent alone moves xy only (the same d = xy - pixel differences, with
# no other term in den to cover them), and the thin Gaussians alone are the class above.
FORWARD_KEYS = {"means2D": "forward_means2D", "under_aa": "forward_thin"}


def reverse_floor_key(name, aa, is_thin):
    return f"reverse_{KINDS[name]}" + ("_aa" if aa else "") + ("_thin" if is_thin else "")


def reverse_tol(name, aa, is_thin):
    return min(cj.TOL_FACTOR * FLOORS[reverse_floor_key(name, aa, is_thin)], cj.MAX_TOL)


def forward_floor_key(support):
    return FORWARD_KEYS.get(support, "forward")


def forward_tol(support):
    return min(cj.TOL_FACTOR * FLOORS[forward_floor_key(support)], cj.MAX_TOL)
