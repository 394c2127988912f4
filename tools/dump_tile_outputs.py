#!/usr/bin/env python3
"""Every output of the tile passes that share gslm_tile.hpp's back-to-front parts, as .npy files, for a bitwise
comparison of two builds of libgslm.so (run it once per build, GSLM_LIB selecting the build, then --compare).

Per case: the drop-in backward with and without the depth cotangent, the LM gradient J^T b, the product
(J^T J + D) v with mask_xyz on and off, the exposure product, the drop-in JVP with and without position tangents, and
LMProblem.diagonal in the full and the projected layout, overwriting (one view) and accumulating (the view twice).
Cases (tests/blend_reference.CASES): one 16x16 tile at list depths 95, 96, 97, 127, 128, 129 and 257 -- on and next
to the 96- and 128-entry batches -- a wall case, a blob case and the six-tile 33x17 case.  Inputs are seeded.

  GSLM_LIB=<parent libgslm.so> GSLM_ABI_ANY=1 python tools/dump_tile_outputs.py --out DIR_A
  python tools/dump_tile_outputs.py --out DIR_B
  python tools/dump_tile_outputs.py --compare DIR_A DIR_B      # exit status 1 unless every array is equal
There is no fallback: without a GPU the dump fails."""
import argparse
import copy
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f"stack{n}_16x16" for n in (95, 96, 97, 127, 128, 129, 257)] + \
    ["wall129_of300_16x16", "blobs_q1_stop128_of192", "stack128_33x17"]


def compare(a, b):
    import numpy as np
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb or not fa:
        print(json.dumps({"equal": False, "error": "different or empty file sets", "only_a": sorted(set(fa) - set(fb)),
                          "only_b": sorted(set(fb) - set(fa))}))
        return 1
    differing, elems = [], 0
    for f in fa:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        elems += x.size
        if not np.array_equal(x, y):  # (a NaN is unequal to itself: none is expected)
            differing.append(f)
    print(json.dumps({"equal": not differing, "arrays": len(fa), "elements": elems, "differing": differing}))
    return 1 if differing else 0


def dump(out_dir):
    sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting-lm_amd"), os.path.join(ROOT, "tests"), ROOT]
    import numpy as np
    import torch
    import torch.autograd.forward_ad as fwAD
    if not torch.cuda.is_available():
        raise SystemExit("dump_tile_outputs.py needs the GPU")
    import blend_reference as br
    from diff_gaussian_rasterization import GaussianRasterizer
    from gslm._lib import check, lib
    from gslm.lm import DIAG_ACCUMULATE, DIAG_SH_REST_PROJECTED, DIAG_TAIL_CLEAN, LMProblem
    from gslm.params import raw_gaussians
    from lm_exposure_ref import X0, direction, set_exposures
    from scenes import gpu_settings
    dev = "cuda"
    os.makedirs(out_dir, exist_ok=True)

    def save(case, what, t):
        np.save(os.path.join(out_dir, f"{case}.{what}.npy"), t.detach().float().cpu().numpy())

    for name in NAMES:
        c = br.CASES[name]
        bg = torch.tensor(c.bg)
        # ---- the drop-in rasterizer: k_render_bwd<true, *, 3>, k_render_jvp<*>
        model, cam, a, cot, tang = br.dropin_inputs(name)
        rast = GaussianRasterizer(gpu_settings(cam, 1, bg))
        for with_depth in (False, True):
            leaves = {k: v.to(dev).requires_grad_(True) for k, v in a.items()}
            m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
            col, _, dep = rast(means3D=leaves["means3D"], means2D=m2, shs=leaves["shs"],
                               opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"])
            obj = (col * cot["color"].to(dev)).sum()
            if with_depth:
                obj = obj + (dep * cot["depth"].to(dev)).sum()
            obj.backward()
            for k, v in leaves.items():
                save(name, f"bwd_depth{int(with_depth)}.{k}", v.grad)
            save(name, f"bwd_depth{int(with_depth)}.means2D", m2.grad)
        for with_xy in (True, False):
            with torch.no_grad(), fwAD.dual_level():
                dual = {k: (fwAD.make_dual(v.to(dev), tang[k].to(dev)) if (with_xy or k != "means3D") else v.to(dev))
                        for k, v in a.items()}
                z = torch.zeros_like(a["means3D"]).to(dev)
                m2 = fwAD.make_dual(z, tang["means2D"].to(dev)) if with_xy else z
                col, _, dep = rast(means3D=dual["means3D"], means2D=m2, shs=dual["shs"], opacities=dual["opacities"],
                                   scales=dual["scales"], rotations=dual["rotations"])
                save(name, f"jvp_xy{int(with_xy)}.colour", fwAD.unpack_dual(col).tangent)
                save(name, f"jvp_xy{int(with_xy)}.invdepth", fwAD.unpack_dual(dep).tangent)
        # ---- the LM path: k_render_bwd<false, false, 2>, k_render_matvec<*>, k_render_matvec_exposure, k_render_diag
        model, cam = br.build(name)
        model.to(dev)
        cam.to(dev)
        for mask_xyz in (True, False):
            prob = LMProblem(model, [cam], bg, device=dev, sh_projection=False, mask_xyz=mask_xyz)
            prob.evaluate()
            v = br.lm_direction(prob.layout, mask_xyz).to(dev)
            save(name, f"lm_xyz{int(not mask_xyz)}.product", prob.matvec(v, prob.zeros()))
            save(name, f"lm_xyz{int(not mask_xyz)}.gradient", prob.rhs(prob.zeros()))
        for projected in (False, True):
            prob = LMProblem(model, [cam], bg, device=dev, sh_projection=projected)
            prob.evaluate()
            save(name, f"diag_proj{int(projected)}.overwrite", prob.diagonal())
            save(name, f"diag_proj{int(projected)}.overwrite_nodamp", prob.diagonal(damp=False))
            # the accumulating form (a second view's call of LMProblem.diagonal) on top of a seeded vector
            acc = torch.rand(prob.layout.numel, device=dev, generator=torch.Generator(dev).manual_seed(5))
            vr = prob.views[0]
            flags = DIAG_TAIL_CLEAN | DIAG_ACCUMULATE | (DIAG_SH_REST_PROJECTED if projected else 0)
            g, ys = raw_gaussians(prob.model), prob.layout.grads_struct(acc)
            check(lib.gslm_lm_diag_view(ctypes.byref(vr.view), ctypes.byref(g), prob.weights[0].data_ptr(), 1,
                                        vr.geom.data_ptr(), vr.binning.data_ptr(), vr.N, vr.image.data_ptr(),
                                        vr.scratch.data_ptr(), vr.scratch.numel(), ctypes.byref(ys), None, flags,
                                        prob.stream), "gslm_lm_diag_view")
            save(name, f"diag_proj{int(projected)}.accumulate", acc)
        mexp = set_exposures(copy.deepcopy(model), [cam], rows=(X0,))
        prob = LMProblem(mexp, [cam], bg, device=dev, train_exposure=True)
        prob.evaluate()
        save(name, "exposure.product", prob.matvec(direction(prob.layout).to(dev), prob.zeros()))
        save(name, "exposure.gradient", prob.rhs(prob.zeros()))
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
