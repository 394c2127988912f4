#!/usr/bin/env python3
"""Every output of the preprocess kernels (k_preprocess, k_preprocess_dma, k_preprocess_views) that
tests/preprocess_layouts.py produces, as .npz files, for a bitwise comparison of two builds of libgslm.so (run it once
per build, GSLM_LIB selecting the build, then --compare).

Per case of preprocess_layouts.CASES:
  run_case.<case>.npz   run_case: gslm_preprocess on every layout, both raw values, every size in SIZES, both views --
                        rec, keys, tiles, rect, clampw, radii (run_preprocess asserts the guard entries behind radii_out
                        untouched, so a dump that finishes has them equal too);
  views.<case>.npz      the gslm_preprocess_views results of tests/test_gpu_preprocess_records.py (f): 1 and 3 views
                        (one of another size), P = 3, 258, 515, its five (layout, raw) pairs, in index space and at depth
                        positions (the positions are dumped too);
  keys.<case>.npz       the results of its test (d): gslm_preprocess_views on layout leaf, one view at a time, every
                        size, both raw values, and the model with every 8th Gaussian behind the near plane.
The workspaces are zero-filled, so what a kernel does not write compares equal as well.

  GSLM_LIB=<parent libgslm.so> GSLM_ABI_ANY=1 python tools/dump_preprocess_records.py --out DIR_A
  python tools/dump_preprocess_records.py --out DIR_B
  python tools/dump_preprocess_records.py --compare DIR_A DIR_B      # exit status 1 unless every array is equal
There is no fallback: without a GPU the dump fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS_SIZES = (3, 258, 515)
VIEWS_LAYOUTS = [("leaf_shifted", True), ("features", True), ("padded", True), ("leaf", False), ("leaf", True)]


def compare(a, b):
    import numpy as np
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb or not fa:
        print(json.dumps({"equal": False, "error": "different or empty file sets", "only_a": sorted(set(fa) - set(fb)),
                          "only_b": sorted(set(fb) - set(fa))}))
        return 1
    differing, arrays, elems = [], 0, 0
    for f in fa:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        if sorted(x.files) != sorted(y.files):
            differing.append(f"{f}: different array names")
            continue
        for k in x.files:
            arrays += 1
            elems += x[k].size
            # the 32-bit words, not the floats: neither a NaN nor a signed zero may fake or hide a difference
            u, w = x[k], y[k]
            if u.shape != w.shape or u.dtype != w.dtype or not np.array_equal(u.view(np.uint32), w.view(np.uint32)):
                differing.append(f"{f}: {k}")
    print(json.dumps({"equal": not differing, "files": len(fa), "arrays": arrays, "elements": elems,
                      "differing": differing[:40], "n_differing": len(differing)}))
    return 1 if differing else 0


def dump(out_dir):
    sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting-lm_amd"), os.path.join(ROOT, "tests"), ROOT]
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dump_preprocess_records.py needs the GPU")
    import preprocess_layouts as pl
    from gslm.cameras import orbit_cameras
    os.makedirs(out_dir, exist_ok=True)
    other = orbit_cameras(2, 130, 57, seed=9)[1]                      # test (f)'s view of another size
    total = 0

    def put(store, tag, r):
        for field, a in r.items():
            store[f"{tag}/{field}"] = a

    for case in pl.CASES:
        cid = pl.case_id(case)
        model, cams, _, _ = pl.oracle_case(case)
        store = {}
        for (P, b, raw, name), r in pl.run_case(case).items():
            put(store, f"{P}/{b}/{int(raw)}/{name}", r)
        np.savez(os.path.join(out_dir, f"run_case.{cid}.npz"), **store)
        total += len(store)

        store = {}
        for nviews, cam_list in ((1, [cams[0]]), (3, [cams[0], other, cams[1]])):
            views = [pl.view_of(c, case) for c in cam_list]
            for P in VIEWS_SIZES:
                vals = pl.model_values(model, P)
                for name, raw in VIEWS_LAYOUTS:
                    L = pl.Layout(name, vals, raw, "cuda")
                    pos = [pl.depth_positions(L, v) for v in views]
                    many, deep = pl.run_preprocess_views(L, views), pl.run_preprocess_views(L, views, pos)
                    for k in range(nviews):
                        tag = f"{nviews}/{P}/{name}/{int(raw)}/{k}"
                        put(store, f"{tag}/index", many[k])
                        put(store, f"{tag}/depth", deep[k])
                        store[f"{tag}/pos"] = pos[k].cpu().numpy()
        np.savez(os.path.join(out_dir, f"views.{cid}.npz"), **store)
        total += len(store)

        store = {}
        mirrored = pl.mirrored_model(model, cams[0])
        for raw in (True, False):
            for b, cam in enumerate(cams):
                for P in pl.SIZES:
                    L = pl.Layout("leaf", pl.model_values(model, P), raw, "cuda")
                    put(store, f"{int(raw)}/{b}/{P}", pl.run_preprocess_views(L, [pl.view_of(cam, case)])[0])
            L = pl.Layout("leaf", pl.model_values(mirrored, 768), raw, "cuda")
            put(store, f"{int(raw)}/mirrored", pl.run_preprocess_views(L, [pl.view_of(cams[0], case)])[0])
        np.savez(os.path.join(out_dir, f"keys.{cid}.npz"), **store)
        total += len(store)
        print(f"{cid}: dumped", flush=True)
    print(json.dumps({"dir": out_dir, "files": len(os.listdir(out_dir)), "arrays": total}))
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
