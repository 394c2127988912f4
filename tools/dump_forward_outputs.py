#!/usr/bin/env python3
"""Every output of the front-to-back tile passes (csrc/render_fwd.hip), of the residual epilogues that share
block_sum4 (csrc/residual.hip) and of k_quad_live, as .npy files, for a bitwise comparison of two builds of libgslm.so
(run it once per build, GSLM_LIB selecting the build, then --compare).  The sibling of dump_tile_outputs.py, which does
the same for the back-to-front passes.

Per case: the drop-in forward (colour, inverse depth, final_T, n_contrib); LMProblem.evaluate plain, masked, Huber,
Cauchy and under exposure (colour, final_T, n_contrib, residual, weight, seed, loss, the exposure rows of J^T b); the
point list's words after the row map (k_quad_live); gslm_rasterize_loss, _robust (Huber, Cauchy) and _exposure, with
and without an alpha mask, overwriting and accumulating onto a seeded double; and on a union binning of 8 perturbed
parameter sets, in the plain, Huber, Cauchy and exposure forms, every slot 0..7 (gslm_rasterize_loss_slot*), the sets
form at n = 1..8 from set 0 and at n = 3 from set 5 (gslm_rasterize_loss_sets*), and a slot past a binning built for
2 sets (the NaN loss).  Cases (tests/blend_reference.CASES): one 16x16 tile at list depths 1, 63, 64, 65, 127, 128,
129 and 257 -- on and next to the wave passes' 64-entry round -- the wall and blob cases that stop on a round's last
entry, and the two several-tile cases.  Inputs are seeded.

  GSLM_LIB=<parent libgslm.so> GSLM_ABI_ANY=1 python tools/dump_forward_outputs.py --out DIR_A
  python tools/dump_forward_outputs.py --out DIR_B
  python tools/dump_forward_outputs.py --compare DIR_A DIR_B      # exit status 1 unless every array is equal
Arrays are compared by bit pattern (a NaN loss equals itself).  There is no fallback: without a GPU the dump fails."""
import argparse
import copy
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f"stack{n}_16x16" for n in (1, 63, 64, 65, 127, 128, 129, 257)] + \
    ["wall64_of200_16x16", "blobs_q0_stop64_of128", "blobs_q0_stop65_of128", "stack64_33x17", "stack97_40x33"]
ROBUST = {"huber": ("huber", 0.1), "cauchy": ("cauchy", 0.1)}  # residuals lie in [-1, 1]: both branches are taken


def compare(a, b):
    import numpy as np
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb or not fa:
        print(json.dumps({"equal": False, "error": "different or empty file sets", "only_a": sorted(set(fa) - set(fb)),
                          "only_b": sorted(set(fb) - set(fa))}))
        return 1
    differing, elems, nans = [], 0, 0
    for f in fa:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        elems += x.size
        if x.dtype.kind == "f":
            nans += int(np.isnan(x).sum())
        bits = np.dtype(f"u{x.dtype.itemsize}")
        if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(np.ascontiguousarray(x).view(bits),
                                                                          np.ascontiguousarray(y).view(bits)):
            differing.append(f)
    print(json.dumps({"equal": not differing, "arrays": len(fa), "elements": elems, "nan_elements": nans,
                      "differing": differing}))
    return 1 if differing else 0


def line_search_step(model, seed=3):
    """A step on every group but xyz (the LM mask), large enough that radii, rects and quadrant masks differ from one
    parameter set to the next."""
    import torch
    from gslm.params import ParamLayout
    P, K = model._xyz.shape[0], 1 + model._features_rest.shape[1]
    lay = ParamLayout(P, K, model._exposure.shape[0])
    s = torch.zeros(lay.numel, device=model._xyz.device)
    v = lay.views(s)
    gen = torch.Generator().manual_seed(seed)
    for name, sd in (("features_dc", 0.1), ("features_rest", 0.02), ("scaling", 0.25), ("rotation", 0.2),
                     ("opacity", 0.8), ("exposure", 0.05)):
        v[name].copy_(sd * torch.randn(v[name].shape, generator=gen))
    return lay, s


def eight_sets(model, exposure):
    """Eight snapshots of a copy of `model` along the step, at scales 2, 1, 1/2, ... as the line search halves them."""
    from gslm.lm import param_snapshot, update_params
    m = copy.deepcopy(model)
    lay, s = line_search_step(m)
    sets, alpha, at = [], 2.0, 0.0
    for _ in range(8):
        update_params(m, lay, s, alpha - at, skip_xyz=True)
        at = alpha
        sets.append(param_snapshot(m, exposure=exposure))
        alpha *= 0.5
    return m, sets


def dump(out_dir):
    sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting-lm_amd"), os.path.join(ROOT, "tests"), ROOT]
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dump_forward_outputs.py needs the GPU")
    import blend_reference as br
    from diff_gaussian_rasterization import _gaussians, forward_buffers
    from gslm import _lib
    from gslm.lm import LMProblem, LossEvaluator, _robust_struct, robust_option
    from lm_exposure_ref import X0, set_exposures
    from scenes import activated, gpu_settings
    lib, check = _lib.lib, _lib.check
    dev = "cuda"
    os.makedirs(out_dir, exist_ok=True)

    def save(case, what, t):
        np.save(os.path.join(out_dir, f"{case}.{what}.npy"), t.detach().cpu().numpy())

    def internals(case, what, P, geom, binning, N, image, H, W):
        fT = torch.zeros(H * W, dtype=torch.float32, device=dev)
        nc = torch.zeros(H * W, dtype=torch.int32, device=dev)
        check(lib.gslm_inspect(geom.data_ptr(), P, binning.data_ptr(), N, H, W, image.data_ptr(), None, None, None,
                               fT.data_ptr(), nc.data_ptr(), None, _lib.stream_handle()), "gslm_inspect")
        save(case, what + ".final_T", fT)
        save(case, what + ".n_contrib", nc)

    for name in NAMES:
        c = br.CASES[name]
        bg = torch.tensor(c.bg)
        model, cam = br.build(name)
        H, W = cam.image_height, cam.image_width
        P = model._xyz.shape[0]
        # ---- the drop-in forward: k_render_fwd_wave<FWD_FULL>
        a = {k: v.to(dev) for k, v in activated(model).items()}
        g = _gaussians(P, a["means3D"], a["opacities"].reshape(-1).contiguous(), a["scales"], a["rotations"], None,
                       a["shs"], None, None)
        view = _lib.view_from_settings(gpu_settings(cam, 1, bg))
        color, radii, invd, geom, binning, image, N = forward_buffers(view, g, dev)
        save(name, "dropin.colour", color)
        save(name, "dropin.invdepth", invd)
        internals(name, "dropin", P, geom, binning, N, image, H, W)
        # ---- LMProblem.evaluate: k_render_fwd_wave<FWD_NO_INV>, k_lm_residual<*>, k_lm_residual_exposure, k_quad_live
        model.to(dev)
        cam.to(dev)
        mask = torch.rand(1, H, W, generator=torch.Generator().manual_seed(11)).to(dev)
        cam_m = copy.copy(cam)
        cam_m.alpha_mask = mask
        mexp = set_exposures(copy.deepcopy(model), [cam], rows=(X0,))
        for tag, mdl, cm, kw in (("lm", model, cam, {}), ("lm_mask", model, cam_m, {}),
                                 ("lm_huber", model, cam, dict(robust=ROBUST["huber"])),
                                 ("lm_cauchy", model, cam_m, dict(robust=ROBUST["cauchy"])),
                                 ("lm_exposure", mexp, cam_m, dict(train_exposure=True))):
            prob = LMProblem(mdl, [cm], bg, device=dev, **kw)
            loss = prob.evaluate()
            vr = prob.views[0]
            save(name, tag + ".colour", vr.color)
            internals(name, tag, P, vr.geom, vr.binning, vr.N, vr.image, H, W)
            save(name, tag + ".residual", prob.residuals[0])
            save(name, tag + ".weight", prob.weights[0])
            save(name, tag + ".seed", prob.seeds[0])
            save(name, tag + ".loss", loss.reshape(1))
            if kw.get("train_exposure"):
                save(name, tag + ".rhs_rows", prob._exp_rhs)
            if tag == "lm":  # the row map refines the list's quadrant masks
                prob.rhs(prob.zeros())
                words, _ = vr.list_words(prob.stream)
                save(name, "lm.list_words_live", words)
        # ---- gslm_rasterize_loss and its forms on the view's own binning: k_render_fwd_wave<FWD_LOSS, false, *, *>
        sh = _lib.stream_handle()
        ev = LossEvaluator(model, [cam], bg, device=dev, batch=1, streams=1)
        ev.evaluate()
        sl, vw, N = ev.slots[0], ev.views[0], ev.num_rendered[0]
        scr = ev.loss_scratch[0]
        xrow = mexp._exposure.data_ptr()
        for mtag, mp in (("", None), ("_mask", mask.data_ptr())):
            for acc in (0, 1):
                def out():
                    return torch.full((1,), 0.37 if acc else 0.0, dtype=torch.float64, device=dev)
                head = (ctypes.byref(vw), P, sl["geom"].data_ptr(), sl["binning"].data_ptr(), sl["binning"].numel(), N,
                        ev.gts[0].data_ptr(), mp)
                tail = (scr.data_ptr(), scr.numel() * 8)
                o = out()
                check(lib.gslm_rasterize_loss(*head, *tail, o.data_ptr(), acc, sh), "gslm_rasterize_loss")
                save(name, f"loss{mtag}.acc{acc}", o)
                o = out()
                check(lib.gslm_rasterize_loss_exposure(*head, xrow, *tail, o.data_ptr(), acc, sh),
                      "gslm_rasterize_loss_exposure")
                save(name, f"loss_exposure{mtag}.acc{acc}", o)
                for kind, opt in ROBUST.items():
                    rb = _robust_struct(robust_option(opt))
                    o = out()
                    check(lib.gslm_rasterize_loss_robust(*head, ctypes.byref(rb), *tail, o.data_ptr(), acc, sh),
                          "gslm_rasterize_loss_robust")
                    save(name, f"loss_{kind}{mtag}.acc{acc}", o)
        # ---- the union binning of 8 parameter sets: k_render_fwd_wave<FWD_LOSS, true, *, *>, k_render_loss_sets<*>
        for tag, mdl, kw in (("plain", model, {}), ("huber", model, dict(robust=ROBUST["huber"])),
                             ("cauchy", model, dict(robust=ROBUST["cauchy"])),
                             ("exposure", mexp, dict(train_exposure=True, fused_exposure=True))):
            m8, sets = eight_sets(mdl, exposure=tag == "exposure")
            ev = LossEvaluator(m8, [cam], bg, device=dev, batch=1, streams=1, alpha_masks=[mask], **kw)
            ev.loss_sets = 1  # per set: gslm_rasterize_loss_slot*, slots 0..7
            save(name, f"union_{tag}.slots", torch.stack(ev.evaluate_points(sets)))
            ev.loss_sets = 8  # one pass: gslm_rasterize_loss_sets* at n sets from set 0
            for n in range(1, 9):
                save(name, f"union_{tag}.sets_n{n}", torch.stack(ev.evaluate_points(sets[:n])))
            ev.loss_sets = 5  # groups of 5: sets 0..4, then n = 3 at first_set = 5
            save(name, f"union_{tag}.sets_5_3", torch.stack(ev.evaluate_points(sets)))
        # a slot past the set count its binning was built for: the NaN loss (tests/test_gpu_line_search.py)
        _, sets = eight_sets(model, exposure=False)
        ev = LossEvaluator(model, [cam], bg, device=dev, batch=1, streams=1)
        ev.evaluate_points(sets[:2])
        usl, ubin = ev.uslots[0][0], ev.ubins[0]
        o = torch.zeros(3, dtype=torch.float64, device=dev)
        for k, slot in enumerate((1, 2, 5)):
            check(lib.gslm_rasterize_loss_slot(ctypes.byref(ev.views[0]), P, usl["geoms"][min(slot, 1)].data_ptr(),
                                               usl["geoms"][0].numel(), ubin.data_ptr(), ubin.numel(),
                                               ev.union_counts[0], slot, 6, ev.gts[0].data_ptr(), None,
                                               ev.loss_scratch[0].data_ptr(), ev.loss_scratch[0].numel() * 8,
                                               o.data_ptr() + 8 * k, 0, sh), "gslm_rasterize_loss_slot")
        save(name, "union_plain.slot_1_2_5_of_2", o)
        torch.cuda.synchronize()
        print(f"{name}: dumped", flush=True)
    print(json.dumps({"dir": out_dir, "arrays": len(os.listdir(out_dir))}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write this build's arrays here")
    ap.add_argument("--compare", nargs=2, metavar="DIR", default=None)
    args = ap.parse_args()
    if (args.out is None) == (args.compare is None):
        ap.error("one of --out DIR and --compare DIR_A DIR_B")
    return compare(*args.compare) if args.compare else dump(args.out)


if __name__ == "__main__":
    sys.exit(main())
