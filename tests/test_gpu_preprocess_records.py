"""GPU: the render records of k_preprocess<RAW> (SH rows read from global memory), k_preprocess_dma<RAW> (staged by
LDS-DMA) and k_preprocess_views<RAW, STAGE> (csrc/forward.hip) on every layout, against the float64 record and bitwise
against each other.

Scene: chain_jacobian.branch_case's model (P = 768, 64x48, two views; tan-FoV clamp, antialiasing clamp, SH clamps on
every channel, 14 % culled), cut to the (allocated, active) degree pairs (3,3) (3,1) (3,0) (2,2) (1,1) (0,0) with plain
settings, (3,3) also with antialiasing and scale_modifier 0.7, and to the prefixes P = 1, 2, 3, 255, 256, 258, 515, 768
(every float4 residue of the last block's staged span at the strides 9, 45 and 27; tests/test_oracle_preprocess_records.py
asserts that arithmetic).  The layouts are those of tests/preprocess_layouts.py, each with raw=True and raw=False.

a. The ten continuous outputs of every visible Gaussian (layout `leaf`) against chain_jacobian.record_fn in float64, in
   the measure max |got - ref| / max(|ref|, median |ref|) per output.  Bounds: 8 x the float32 oracle's own value of the
   measure (preprocess_layouts.FLOORS, asserted on the CPU by test_oracle_preprocess_records.py::test_float32_floor):
       x 1.8e-6   y 5.1e-6   conic_a 6.6e-6   conic_b 4.6e-5   conic_c 7.7e-6   opacity 8.8e-7 (antialiasing 6.0e-6)
       r, g, b 3.2e-6   invdepth 2.2e-6   depth (the key of d.) 7.2e-7
b. Tile count, rect (both copies), radii_out, clamp word (both copies) and visibility equal the float32 oracle's
   exactly, outside the boundary exclusion (<= 0.5 % of P x views; 0 Gaussians on this scene).
c. tq, the alpha threshold, from each record's own opacity: negative exactly when 255 o <= 1 in float32, else within
   [t - 1 ulp, t + 2 ulp] of t = 2 ln(255 o) 1.02 + 1e-4.
d. The depth keys gslm_preprocess_views leaves: the float32 depth's bits for every Gaussian in front of the near plane,
   culled by its footprint or not, 0xFFFFFFFF otherwise.
e. Every layout writes the bits of layout `leaf`: the LDS-DMA records (leaf, features) equal those of the layouts that
   read global memory unstaged (leaf_shifted, features_shifted, padded).
f. gslm_preprocess_views (staged and unstaged instantiations, index space and depth space) writes gslm_preprocess's bits.
h. The drop-in rasterizer's outputs, gradients and tangents do not depend on how the caller lays out the SH tensor.
"""
import functools

import numpy as np
import pytest
import torch

import preprocess_layouts as pl
from margins import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
case_param = pytest.mark.parametrize("case", pl.CASES, ids=pl.case_id)


@functools.lru_cache(maxsize=None)
def _results(case):
    return pl.run_case(case)


def _vis(r):
    return r["tiles"] > 0


def _keep(case, b, P):
    """The Gaussians of view b outside the boundary exclusion; the exclusion's share is capped."""
    _, cams, _, o64s = pl.oracle_case(case)
    n = sum(int(pl.excluded(o)[:P].sum()) for o in o64s)
    assert n <= pl.EXCLUDE_CAP * P * len(cams), (P, n)
    return ~pl.excluded(o64s[b])[:P].numpy()


# ------------------------------------------------------------------ a. records against float64
@pytest.mark.parametrize("raw", [True, False])
@case_param
def test_records_against_float64(case, raw):
    _, cams, o32s, o64s = pl.oracle_case(case)
    res = _results(case)
    worst = torch.zeros(len(pl.OUT_NAMES), dtype=torch.float64)
    for P in pl.SIZES:
        for b in range(len(cams)):
            r = res[(P, b, raw, "leaf")]
            vis32 = o32s[b]["visible"][:P].numpy()
            rows = vis32 & _vis(r) & _keep(case, b, P)
            assert np.isfinite(r["rec"][_vis(r)][:, :12]).all()
            worst = torch.maximum(worst, pl.record_measure(pl.gpu_record(r), o32s[b], o64s[b], rows))
    bad = []
    for o, name in enumerate(pl.OUT_NAMES[:10]):
        tol = pl.record_tol(name, case[2])
        e = record("test_records_against_float64", f"{pl.case_id(case)} raw={int(raw)}: {name}", float(worst[o]), tol)
        if not e <= tol:
            bad.append((name, e, tol))
    assert not bad, bad


# ------------------------------------------------------------------ b. discrete outputs
@pytest.mark.parametrize("raw", [True, False])
@case_param
def test_discrete_outputs_equal_the_float32_oracle(case, raw):
    _, cams, o32s, _ = pl.oracle_case(case)
    res = _results(case)
    for P in pl.SIZES:
        for b in range(len(cams)):
            r, o = res[(P, b, raw, "leaf")], o32s[b]
            keep = _keep(case, b, P)
            tag = (pl.case_id(case), raw, P, b)
            vis = o["visible"][:P].numpy()
            assert np.array_equal(_vis(r)[keep], vis[keep]), tag
            gone = ~_vis(r)
            assert (r["tiles"][gone] == 0).all() and (r["radii"][gone] == 0).all(), tag
            v = vis & _vis(r) & keep
            assert np.array_equal(r["tiles"][v], o["tiles_touched"][:P].numpy()[v]), tag
            assert np.array_equal(r["radii"][v], o["radii"][:P].numpy()[v]), tag
            want = o["rect"][:P].numpy()[v]
            assert np.array_equal(pl.unpack_rect(r["rect"][v]), want), tag
            assert np.array_equal(pl.unpack_rect(r["rec"][v][:, 12:14].copy().view(np.uint32)), want), tag
            assert (r["rec"][v][:, 14:16].view(np.uint32) == 0).all(), tag
            c = o["clamped"][:P].numpy()[v].astype(np.uint32)
            bits = c[:, 0] | (c[:, 1] << 1) | (c[:, 2] << 2)
            assert np.array_equal(r["clampw"][v], bits), tag
            assert np.array_equal(r["rec"][v][:, 10].copy().view(np.uint32), bits), tag


# ------------------------------------------------------------------ c. the alpha threshold
def _tq_check(r, tag):
    """(Gaussians with tq < 0, with tq >= 0, the lowest and highest (tq - t) / ulp) of one result's visible records."""
    v = _vis(r)
    o, tq = r["rec"][v][:, 5], r["rec"][v][:, 11]
    above = (o * np.float32(255.0)) > np.float32(1.0)          # float32 product, as alpha_threshold
    assert np.array_equal(tq >= 0, above), (tag, "tq must be negative exactly when 255 o <= 1 in float32")
    assert (tq[~above] < 0).all(), tag
    if not above.any():
        return int((~above).sum()), 0, 0.0, 0.0
    t = 2.0 * np.log(255.0 * o[above].astype(np.float64)) * 1.02 + 1e-4
    ulp = np.spacing(t.astype(np.float32)).astype(np.float64)
    d = (tq[above].astype(np.float64) - t) / ulp
    assert d.min() >= -1.0, (tag, f"tq is {-d.min():.2f} ulp BELOW t: the dangerous direction -- the quadrant cull, "
                             f"which promises to be exact, would drop blends the tile pass accepts")
    assert d.max() <= 2.0, (tag, f"tq is {d.max():.2f} ulp above t")
    return int((~above).sum()), int(above.sum()), float(d.min()), float(d.max())


@case_param
def test_alpha_threshold(case):
    lo, hi, nb, na = 0.0, 0.0, 0, 0
    for key, r in _results(case).items():
        b_, a_, dlo, dhi = _tq_check(r, (pl.case_id(case),) + key)
        lo, hi, nb, na = min(lo, dlo), max(hi, dhi), nb + b_, na + a_
    print(f"[tq] {pl.case_id(case)}: {nb} records below 255 o = 1, {na} above; (tq - t) / ulp in [{lo:.3f}, {hi:.3f}]")
    assert na > 0


@pytest.mark.parametrize("case,lowered", [(pl.CASES[-1], False), (pl.CASES[0], True)],
                         ids=["antialiasing", "lowered_opacity"])
def test_alpha_threshold_both_sides_populated(case, lowered):
    """At least 5 visible Gaussians on each side of 255 o = 1 in each view (asserted on the oracle, then seen on the
    GPU): under antialiasing the scene has them as it is; without, a copy with every 16th opacity lowered."""
    model, cams, o32s, _ = pl.oracle_case(case, lowered)
    vals = pl.model_values(model, 768)
    for b, cam in enumerate(cams):
        o = o32s[b]["opacity"][o32s[b]["visible"]]
        assert int((o * 255.0 <= 1.0).sum()) >= 5 and int((o * 255.0 > 1.0).sum()) >= 5
        for raw in (True, False):
            r = pl.run_preprocess(pl.Layout("leaf", vals, raw, DEV), pl.view_of(cam, case))
            nb, na, lo, hi = _tq_check(r, (pl.case_id(case), lowered, b, raw))
            print(f"[tq] {pl.case_id(case)} lowered={lowered} view {b} raw={int(raw)}: {nb} below, {na} above; "
                  f"(tq - t) / ulp in [{lo:.3f}, {hi:.3f}]")
            assert nb >= 5 and na >= 5


# ------------------------------------------------------------------ d. depth keys
def _check_keys(r, o32, o64, keep, tag):
    P = r["keys"].shape[0]
    depth = o32["depth"][:P].numpy()
    want = np.where(depth > np.float32(0.2), depth.view(np.uint32), np.uint32(0xFFFFFFFF))
    assert np.array_equal(r["keys"][keep], want[keep]), tag
    keyed = (r["keys"] != 0xFFFFFFFF) & keep
    got = np.full((P, 11), np.nan, dtype=np.float32)
    got[:, 10] = r["keys"].view(np.float32)
    # the measure of a. over every keyed Gaussian (the footprint-culled ones included: the float64 depth exists for all)
    ref = o64["record"][:P, 10]
    m = pl.medians(o32, o64)[10]
    err = (torch.from_numpy(got[:, 10]).double() - ref).abs() / torch.maximum(ref.abs(), m)
    return float(err[torch.from_numpy(keyed)].max()) if keyed.any() else 0.0


@pytest.mark.parametrize("raw", [True, False])
@case_param
def test_depth_keys(case, raw):
    model, cams, o32s, o64s = pl.oracle_case(case)
    worst = 0.0
    for b, cam in enumerate(cams):
        assert int(((o32s[b]["depth"] > 0.2) & ~o32s[b]["visible"]).sum()) >= 20   # culled by footprint yet keyed
        for P in pl.SIZES:
            L = pl.Layout("leaf", pl.model_values(model, P), raw, DEV)
            (r,) = pl.run_preprocess_views(L, [pl.view_of(cam, case)])
            worst = max(worst, _check_keys(r, o32s[b], o64s[b], _keep(case, b, P), (pl.case_id(case), raw, b, P)))
            culled_keyed = (r["keys"] != 0xFFFFFFFF) & ~_vis(r)
            if P == 768:
                assert int(culled_keyed.sum()) >= 20
    tol = pl.record_tol("depth", case[2])
    assert record("test_depth_keys", f"{pl.case_id(case)} raw={int(raw)}: depth", worst, tol) <= tol
    # Gaussians behind the near plane (the scene has none): every 8th reflected through the first camera's centre
    mm = pl.mirrored_model(model, cams[0])
    o32, o64 = pl._oracle(mm, cams[0], case, torch.float32), pl._oracle(mm, cams[0], case, torch.float64)
    assert int((~(o32["depth"] > 0.2)).sum()) >= 20
    keep = ~pl.excluded(o64).numpy()
    (r,) = pl.run_preprocess_views(pl.Layout("leaf", pl.model_values(mm, 768), raw, DEV), [pl.view_of(cams[0], case)])
    _check_keys(r, o32, o64, keep, (pl.case_id(case), raw, "mirrored"))
    assert int((r["keys"] == 0xFFFFFFFF).sum()) >= 20
    assert np.array_equal(_vis(r)[keep], o32["visible"].numpy()[keep])


# ------------------------------------------------------------------ e. every path writes the same bits
@case_param
def test_every_layout_writes_the_bits_of_leaf(case):
    res = _results(case)
    bad = []
    for (P, b, raw, name), r in res.items():
        if name == "leaf":
            continue
        ref = res[(P, b, raw, "leaf")]
        v = _vis(ref)
        tag = f"{name} raw={int(raw)} P={P} view {b}"
        if not np.array_equal(_vis(r), v):
            bad.append(f"{tag}: visibility")
            continue
        assert np.isfinite(r["rec"][v][:, :10]).all(), (tag, "a pad float was read")
        if name == "colors":
            # given colours are never clamped: the clamp word is 0 in both copies, everything else is leaf's
            if (r["clampw"][v] != 0).any() or (r["rec"][v][:, 10].copy().view(np.uint32) != 0).any():
                bad.append(f"{tag}: clamp word not 0")
            a, c = dict(r), dict(ref)
            a["rec"], c["rec"] = np.delete(r["rec"], 10, axis=1), np.delete(ref["rec"], 10, axis=1)
            d = pl.same_bits(a, c, v, fields=("tiles", "rect", "radii"), rec_cols=15)
        else:
            d = pl.same_bits(r, ref, v)
        bad += [f"{tag}: {x}" for x in d]
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ f. gslm_preprocess_views
VIEWS_LAYOUTS = [("leaf_shifted", True), ("features", True), ("padded", True), ("leaf", False), ("leaf", True)]


def _other_size_camera():
    from gslm.cameras import orbit_cameras
    return orbit_cameras(2, 130, 57, seed=9)[1]


@pytest.mark.parametrize("nviews", [1, 3])
@case_param
def test_preprocess_views_writes_the_bits_of_preprocess(case, nviews):
    """leaf / raw=True runs k_preprocess_views<true, true> (staged); the other four layouts its unstaged instantiations
    <true, false> and <false, false>.  Index space: records, tile counts, rects and clamp words bitwise those of
    gslm_preprocess.  Depth space: the same records at pos[i], the rect slot zero when culled."""
    model, cams, _, _ = pl.oracle_case(case)
    cam_list = [cams[0]] if nviews == 1 else [cams[0], _other_size_camera(), cams[1]]
    views = [pl.view_of(c, case) for c in cam_list]
    bad = []
    for P in (3, 258, 515):
        vals = pl.model_values(model, P)
        for name, raw in VIEWS_LAYOUTS:
            L = pl.Layout(name, vals, raw, DEV)
            staged = L.raw and L.stage_lead() == 0   # views_pass_ok
            assert staged == (name == "leaf" and raw and case[0] > 0)
            single = [pl.run_preprocess(L, v) for v in views]
            many = pl.run_preprocess_views(L, views)
            pos = [pl.depth_positions(L, v) for v in views]
            deep = pl.run_preprocess_views(L, views, pos)
            for k in range(nviews):
                tag = f"{name} raw={int(raw)} P={P} view {k} of {nviews}"
                v = _vis(single[k])
                bad += [f"{tag}: {x}" for x in pl.same_bits(many[k], single[k], v, fields=("tiles", "rect", "clampw"))]
                p = pos[k].cpu().numpy().astype(np.int64)
                rc = deep[k]["rec"][p]                      # back in index order
                if not np.array_equal(rc[v][:, :12].view(np.uint32), single[k]["rec"][v][:, :12].view(np.uint32)):
                    bad.append(f"{tag}: depth-space records")
                if not np.array_equal(rc[v][:, 12:14].copy().view(np.uint32), single[k]["rect"][v]):
                    bad.append(f"{tag}: depth-space rect slot")
                if not (rc[~v][:, 12:14].view(np.uint32) == 0).all():
                    bad.append(f"{tag}: depth-space rect slot of a culled Gaussian not zero")
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ h. the drop-in's SH layouts
def _dropin_calls(case, P, cam):
    """(outputs, gradients, tangents) of the three calls, each a list of CPU tensors in one order."""
    import torch.autograd.forward_ad as fwAD
    from diff_gaussian_rasterization import GaussianRasterizer
    from scenes import gpu_settings
    model, _, _, _ = pl.oracle_case(case)
    vals = pl.model_values(model, P)
    M = vals["M"]
    st = gpu_settings(cam, case[1], torch.tensor([0.25, 0.5, 0.75]), scale_modifier=case[3], antialiasing=case[2])
    H, W = int(cam.image_height), int(cam.image_width)
    gen = torch.Generator().manual_seed(40 + P)
    dcol, ddep = torch.randn(3, H, W, generator=gen).to(DEV), torch.randn(1, H, W, generator=gen).to(DEV)
    shs0 = torch.cat([vals["dc"], vals["rest"]], dim=1)                       # [P, M, 3]
    base = dict(means3D=vals["xyz"], opacities=vals["act"]["opacities"][:, None].contiguous(),
                scales=vals["act"]["scales"], rotations=vals["act"]["rotations"])
    tang = {k: torch.randn(v.shape, generator=gen) for k, v in base.items()}
    t_shs, t_m2 = torch.randn(shs0.shape, generator=gen), torch.randn(P, 3, generator=gen)

    def sh_args(which, values):
        if which == "features":
            return dict(shs=values.to(DEV))
        if which == "split":
            return dict(dc=values[:, :1].contiguous().to(DEV), shs=values[:, 1:].contiguous().to(DEV))
        buf, view = pl._place(values, 1, DEV)                                  # one float past a 16-B boundary
        view = view.view(P, M, 3)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return dict(shs=view)

    outs = {}
    for which in ("features", "split", "shifted"):
        inp = {k: v.to(DEV).requires_grad_(True) for k, v in base.items()}
        sh = {k: v.requires_grad_(True) for k, v in sh_args(which, shs0).items()}
        m2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
        c, radii, d = GaussianRasterizer(st)(means2D=m2, **inp, **sh)
        ((c * dcol).sum() + (d * ddep).sum()).backward()
        g_sh = torch.cat([sh["dc"].grad, sh["shs"].grad], dim=1) if which == "split" else sh["shs"].grad
        grads = [inp[k].grad for k in sorted(inp)] + [m2.grad, g_sh]
        with torch.no_grad(), fwAD.dual_level():
            dinp = {k: fwAD.make_dual(v.to(DEV), tang[k].to(DEV)) for k, v in base.items()}
            p, t = sh_args(which, shs0), sh_args(which, t_shs)
            dsh = {k: fwAD.make_dual(p[k], t[k]) for k in p}
            dm2 = fwAD.make_dual(torch.zeros(P, 3, device=DEV), t_m2.to(DEV))
            tc, _, td = GaussianRasterizer(st)(means2D=dm2, **dinp, **dsh)
            tans = [fwAD.unpack_dual(tc).tangent, fwAD.unpack_dual(td).tangent]
        outs[which] = ([c.detach().cpu(), d.detach().cpu(), radii.cpu()], [g.detach().cpu() for g in grads],
                       [x.detach().cpu() for x in tans])
    return outs


@pytest.mark.parametrize("P", [515, 258])
@pytest.mark.parametrize("case", [pl.CASES[0], pl.CASES[3]], ids=pl.case_id)
def test_dropin_does_not_depend_on_the_sh_layout(case, P):
    """shs [P, M, 3] (k_preprocess_dma<false> and stage_sh_rows at lead 3), the dc= / shs= split (lead 0) and shs one
    float past a 16-B boundary (unstaged): colour, inverse depth, radii, every input gradient (k_preprocess_bwd's
    strided SH stores) and the forward-mode tangents (k_preprocess_jvp) are bitwise equal."""
    _, cams, _, _ = pl.oracle_case(case)
    bad = []
    for b, cam in enumerate(cams):
        outs = _dropin_calls(case, P, cam)
        ref = outs["features"]
        assert int((ref[0][2] > 0).sum()) > 0.5 * P
        for which in ("split", "shifted"):
            for kind, xs, ys in zip(("output", "gradient", "tangent"), outs[which], ref):
                for i, (x, y) in enumerate(zip(xs, ys)):
                    assert x.shape == y.shape and bool(torch.isfinite(y.float()).all())
                    if not torch.equal(x, y):
                        bad.append(f"view {b} {which}: {kind} {i}, max |diff| {float((x.float() - y.float()).abs().max()):.3e}")
    assert not bad, bad
