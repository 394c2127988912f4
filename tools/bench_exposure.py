#!/usr/bin/env python3
"""The single-view LM solve with and without trained exposure.

By default 1M Gaussians, SH 3, one 1080p view, 10 CG iterations, check_every=False (no host synchronisation inside the
solve).  Three modes, timed one after the other in every run of one process:
  default    cgls_fused on gslm.lm.LMProblem: the benchmark's solve (active list, lean loop);
  exposure   cgls_fused on LMProblem(train_exposure=True): the fused tile pass with the 3x4 affine map between its two
             halves (GSLM_MV_EXPOSURE), the exposure rows' streaming reduction, a separate <p, A p> (active list, no
             lean loop);
  split      the exposure PRODUCT as the split composition: J v (jv_out) -> the affine step, weight and transpose in
             torch -> the seeded back-to-front pass + gather, the 12 rows as torch sums -- two tile passes.
`cg` lines give ms per CG iteration of a solve (default, exposure); `product` lines ms per (J^T J + D) v on the full
vectors (all three: for default the plain product).  The exposure and split products are compared once (`agreement`).
Each mode is settled first (untimed work >= 200 ms, the clock settle of bench.py).  One JSON line per measurement to
stdout and, with --out, to a file.  There is no fallback: without a GPU the tool fails.

  python tools/bench_exposure.py --runs 5 --out profiles/lm_exposure/runs.jsonl
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--s0", type=float, default=0.005)
    ap.add_argument("--iters", type=int, default=10, help="CG iterations per timed solve")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--product-reps", type=int, default=10)
    ap.add_argument("--label", default="", help="copied into every line (e.g. the commit)")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


# the exposure the ground truth is rendered under and the one the model starts from (row-major [i][k])
X_GT = [[0.90, 0.05, -0.03, 0.04], [-0.06, 1.10, 0.02, -0.02], [0.03, -0.04, 0.80, 0.03]]


def split_product(prob, v, y):
    """(J^T J + D) v of LMProblem(train_exposure=True) as the split composition, one view (full layout)."""
    import torch
    from gslm import _lib
    from gslm.lm import MV_TAIL_CLEAN, STAGE_OVERWRITE
    from gslm.params import raw_gaussians
    lib, check = _lib.lib, _lib.check
    vr = prob.views[0]
    g = raw_gaussians(prob.model)
    vs, ys = prob.layout.grads_struct(v), prob.layout.grads_struct(y)
    e0, e1 = prob.layout.offsets["exposure"]
    k = prob.exp_idx[0]
    X = prob.model._exposure[k].detach()
    V = v[e0 + 12 * k:e0 + 12 * k + 12].view(3, 4)
    jv, w, R = prob._split_jv, prob.weights[0], vr.color

    def call(opts, weight):
        check(lib.gslm_matvec_view_ex(ctypes.byref(vr.view), ctypes.byref(g), ctypes.byref(vs), weight.data_ptr(), 1,
                                      vr.geom.data_ptr(), vr.binning.data_ptr(), vr.N, vr.image.data_ptr(),
                                      vr.scratch.data_ptr(), vr.scratch.numel(), ctypes.byref(ys), ctypes.byref(opts),
                                      prob.stream), "gslm_matvec_view_ex")

    o1 = _lib.GslmMatvecOpts()
    o1.stages = 1 | 2  # TANGENT | RENDER: J v
    o1.flags = prob.mv_flags
    o1.jv_out = jv.data_ptr()
    call(o1, jv)
    dC = torch.einsum("ihw,ij->jhw", jv, X[:, :3]) + torch.einsum("ihw,ij->jhw", R, V[:, :3]) + V[:, 3, None, None]
    u = 2.0 * w * dC
    ub = torch.einsum("jhw,ij->ihw", u, X[:, :3]).contiguous()
    o2 = _lib.GslmMatvecOpts()
    o2.stages = 2 | 4 | STAGE_OVERWRITE  # RENDER | GATHER, seeded
    o2.flags = (MV_TAIL_CLEAN if vr.tail_clean else 0) | prob.mv_flags
    o2.pixel_seed = ub.data_ptr()
    o2.damp7 = prob._damps
    call(o2, ub)
    vr.tail_clean = True
    yt = y[e0:e1].view(-1, 3, 4)
    torch.mul(v[e0:e1].view(-1, 3, 4), float(prob._damps[6]), out=yt)
    yt[k, :, :3] += torch.einsum("ihw,jhw->ij", R, u)
    yt[k, :, 3] += u.sum((1, 2))
    return y


def main():
    args = parse()
    sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-lm_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_exposure.py needs the GPU: a CPU run has no timing to report")
    from gslm.cameras import orbit_cameras
    from gslm.lm import LMProblem, cgls_fused
    from gslm.model import synthetic_gaussians
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None

    def emit(line):
        line = dict(line, label=args.label, P=args.P, sh=args.sh, width=args.width, height=args.height,
                    iters=args.iters)
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    W, H = args.width, args.height
    cams = [c.to(dev) for c in orbit_cameras(1, W, H, seed=1)]
    bg = torch.zeros(3)
    # ground truth as in bench.py (the render of the model with f_dc / opacity / scaling perturbed by N(0, 0.01^2)),
    # here under the exposure X_GT; the model starts from the identity exposure
    pert = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=1)
    g2 = torch.Generator().manual_seed(2)
    with torch.no_grad():
        pert._features_dc += 0.01 * torch.randn(pert._features_dc.shape, generator=g2)
        pert._opacity += 0.01 * torch.randn(pert._opacity.shape, generator=g2)
        pert._scaling += 0.01 * torch.randn(pert._scaling.shape, generator=g2)
    pert.to(dev)
    gt = LMProblem(pert, cams, bg, device=dev)
    gt.evaluate()
    X = torch.tensor(X_GT, device=dev)
    R = gt.views[0].color
    cams[0].original_image = (torch.matmul(R.permute(1, 2, 0), X[:, :3]).permute(2, 0, 1) +
                              X[:, 3, None, None]).clamp(0, 1).contiguous()
    del gt, pert, R
    torch.cuda.empty_cache()
    model = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=1).to(dev)
    model.exposure_mapping = {cams[0].image_name: 0}

    probs = {}
    for m, kw in (("default", {}), ("exposure", {"train_exposure": True})):
        p = LMProblem(model, cams, bg, device=dev, sh_projection="auto", **kw)
        p.evaluate()
        probs[m] = (p, p.rhs(p.zeros()))
    pe = probs["exposure"][0]
    pe._split_jv = torch.empty_like(pe.views[0].color)
    torch.cuda.synchronize()
    emit({"kind": "scene", "num_rendered": [int(n) for n in pe.num_rendered()],
          "loss": {m: float(p.loss) for m, (p, _) in probs.items()}})

    def solve(m, iters):
        p, g = probs[m]
        return cgls_fused(p, g, max_iter=iters, restart_iter=iters, check_every=False)

    vecs = {m: (g.clone(), p.zeros()) for m, (p, g) in probs.items()}
    vecs["split"] = (vecs["exposure"][0], pe.zeros())

    def product(m):
        v, y = vecs[m]
        if m == "split":
            return split_product(pe, v, y)
        return probs[m][0].matvec(v, y)

    # the two forms of the exposure product agree
    ye = product("exposure").clone()
    ys = product("split").clone()
    e0, e1 = pe.layout.offsets["exposure"]
    emit({"kind": "agreement", "gaussian_rows_of_max": float((ye[:e0] - ys[:e0]).abs().max() / ys[:e0].abs().max()),
          "exposure_rows_of_max": float((ye[e0:e1] - ys[e0:e1]).abs().max() / ys[e0:e1].abs().max())})

    for m in ("default", "exposure", "split"):
        t0 = time.perf_counter()
        n = 0
        while n < 2 or time.perf_counter() - t0 < 0.2:
            if m == "split":
                product(m)
            else:
                solve(m, args.iters)
            torch.cuda.synchronize()
            n += 1
        emit({"kind": "settle", "mode": m, "calls": n, "ms": 1e3 * (time.perf_counter() - t0)})

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for r in range(args.runs):
        for m in ("default", "exposure"):
            solve(m, 3)  # warm-up of this mode's kernels right before its window
            torch.cuda.synchronize()
            a, b = events()
            a.record()
            solve(m, args.iters)
            b.record()
            torch.cuda.synchronize()
            emit({"kind": "cg", "run": r, "mode": m, "ms_per_iter": a.elapsed_time(b) / args.iters})
        for m in ("default", "exposure", "split"):
            product(m)
            torch.cuda.synchronize()
            a, b = events()
            a.record()
            for _ in range(args.product_reps):
                product(m)
            b.record()
            torch.cuda.synchronize()
            emit({"kind": "product", "run": r, "mode": m, "ms": a.elapsed_time(b) / args.product_reps})
    if out:
        out.close()


if __name__ == "__main__":
    main()
