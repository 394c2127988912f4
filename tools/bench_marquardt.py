#!/usr/bin/env python3
"""Fixed damping against Marquardt-scaled damping on the LM normal equations.

By default bench.py's scene: 1M Gaussians, SH 3, one 1080p view (--views 5: the five-view loop problem), the ground
truth rendered from the perturbed model.  Same scene, same g; per run the modes alternate in one process:
  fixed         LMProblem(damp=DEFAULT_DAMP); plain = cgls_fused(check_every=False) -- one view: the active list and
                the lean loop, as the benchmark -- and jacobi = cgls_jacobi(check_every=False)
  fixed_general the same plain solve with GSLM_CG_LEAN=0: the loop the damping vector runs (one view only)
  marquardt     LMProblem(damping="marquardt", damp=lambda, marquardt_floor=floor): the same two solvers, the
                damping vector built once before the timed solves (its cost is the `vector` line)
`product` lines: ms of one (J^T J + D) v; `solve` lines: ms per --iters-iteration solve; `vector` lines: ms of the
once-per-step diagonal(damp=False) + gslm_marquardt_scale; `diag_stats`: the undamped diagonal's medians of nonzero
entries, maxima and smallest nonzero entries per group.  `lm_step` lines (--val validation views; 0 skips them): the
line search's alpha and the validation loss for fixed damping and for lambda in --lambdas at floor 0 and --floor,
precond None and "jacobi".  Each mode is settled first.  One JSON line per measurement to stdout and, with --out, to a
file.  There is no fallback: without a GPU the tool fails.

  python tools/bench_marquardt.py --runs 5 --out profiles/lm_marquardt/runs_1view.jsonl
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "exposure")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--s0", type=float, default=0.005)
    ap.add_argument("--views", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10, help="max_iter of the timed solves")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lam", type=float, default=1e-2, help="lambda of the timed Marquardt problem")
    ap.add_argument("--floor", type=float, default=1e-3, help="the nonzero floor")
    ap.add_argument("--lambdas", type=float, nargs="+", default=[1e-4, 1e-3, 1e-2, 1e-1, 1.0])
    ap.add_argument("--step-iters", type=int, default=2, help="max_iter of the lm_step sweep")
    ap.add_argument("--val", type=int, default=4, help="validation views of the lm_step sweep (0: skip it)")
    ap.add_argument("--label", default="", help="copied into every line (e.g. the commit)")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main():
    args = parse()
    sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-lm_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_marquardt.py needs the GPU: a CPU run has no timing to report")
    from gslm.cameras import orbit_cameras
    from gslm.lm import LMProblem, cgls_fused, cgls_jacobi, clear_val_cache, lm_step
    from gslm.model import synthetic_gaussians
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None

    def emit(line):
        line = dict(line, label=args.label, P=args.P, sh=args.sh, width=args.width, height=args.height,
                    views=args.views)
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    W, H = args.width, args.height
    nv = args.views + args.val
    cams = [c.to(dev) for c in orbit_cameras(nv, W, H, seed=1)]
    bg = torch.zeros(3)
    # ground truth as in bench.py: the render of the model with f_dc / opacity / scaling perturbed by N(0, 0.01^2)
    pert = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=nv)
    g2 = torch.Generator().manual_seed(2)
    with torch.no_grad():
        pert._features_dc += 0.01 * torch.randn(pert._features_dc.shape, generator=g2)
        pert._opacity += 0.01 * torch.randn(pert._opacity.shape, generator=g2)
        pert._scaling += 0.01 * torch.randn(pert._scaling.shape, generator=g2)
    pert.to(dev)
    for c in cams:
        gt = LMProblem(pert, [c], bg, device=dev)
        gt.evaluate()
        c.original_image = gt.views[0].color.clamp(0, 1).clone()
        del gt
    del pert
    torch.cuda.empty_cache()
    model = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu", n_cams=nv).to(dev)
    train, val = cams[:args.views], cams[args.views:]
    lam = {k: args.lam for k in GROUPS}

    probs = {"fixed": LMProblem(model, train, bg, device=dev, sh_projection="auto"),
             "marquardt": LMProblem(model, train, bg, device=dev, sh_projection="auto", damping="marquardt", damp=lam,
                                    marquardt_floor=args.floor)}
    rhs = {}
    for name, prob in probs.items():
        prob.evaluate()
        rhs[name] = prob.rhs(prob.zeros())
    torch.cuda.synchronize()
    prob = probs["marquardt"]
    emit({"kind": "scene", "num_rendered": [int(n) for n in prob.num_rendered()], "loss": float(prob.loss),
          "projected": bool(prob.layout.rest_projected), "lam": args.lam, "floor": args.floor})
    d0 = prob.diagonal(damp=False)
    stats = {}
    for name, t in prob.layout.views(d0).items():
        if name in ("xyz", "exposure") or not t.numel():
            continue
        nz = t[t > 0]
        stats[name] = {"median_nonzero": float(nz.median()), "max": float(t.max()), "min_nonzero": float(nz.min()),
                       "share_nonzero": nz.numel() / t.numel(), "share_below_floor": float((t < args.floor).float().mean())}
    emit({"kind": "diag_stats", **stats})
    del d0

    modes = [("fixed", "plain"), ("marquardt", "plain"), ("fixed", "jacobi"), ("marquardt", "jacobi")]
    if args.views == 1:
        modes.insert(1, ("fixed_general", "plain"))

    def solve(damping, solver, k):
        name = "fixed" if damping == "fixed_general" else damping
        os.environ["GSLM_CG_LEAN"] = "0" if damping == "fixed_general" else "1"
        fn = cgls_fused if solver == "plain" else cgls_jacobi
        return fn(probs[name], rhs[name], max_iter=k, restart_iter=k, check_every=False)[0]

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for damping, solver in modes:
        t0 = time.perf_counter()
        n = 0
        while n < 2 or time.perf_counter() - t0 < 0.2:
            solve(damping, solver, args.iters)
            torch.cuda.synchronize()
            n += 1
        emit({"kind": "settle", "damping": damping, "solver": solver, "calls": n, "ms": 1e3 * (time.perf_counter() - t0)})

    y = prob.zeros()
    for r in range(args.runs):
        for damping, solver in modes:
            solve(damping, solver, 2)  # warm-up of this mode's kernels right before its window
            torch.cuda.synchronize()
            a, b = events()
            a.record()
            solve(damping, solver, args.iters)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            emit({"kind": "solve", "run": r, "damping": damping, "solver": solver, "max_iter": args.iters, "ms": ms,
                  "ms_per_iter": ms / args.iters})
        for name in ("fixed", "marquardt"):
            p = probs[name]
            p.matvec(rhs[name], y)
            torch.cuda.synchronize()
            a, b = events()
            a.record()
            for _ in range(10):
                p.matvec(rhs[name], y)
            b.record()
            torch.cuda.synchronize()
            emit({"kind": "product", "run": r, "damping": name, "ms": a.elapsed_time(b) / 10})
        torch.cuda.synchronize()
        a, b = events()
        a.record()
        for _ in range(10):
            prob.set_damping_vector(None)  # (forget the vector: the next use builds it, as after an evaluate())
            prob.damping_vector()
        b.record()
        torch.cuda.synchronize()
        emit({"kind": "vector", "run": r, "ms": a.elapsed_time(b) / 10})
    os.environ.pop("GSLM_CG_LEAN", None)

    if args.val > 0:
        k = args.step_iters
        cases = [("fixed", None, 0.0)] + [("marquardt", lv, f) for f in (0.0, args.floor) for lv in args.lambdas]
        for damping, lv, f in cases:
            for precond in (None, "jacobi"):
                m = copy.deepcopy(model)
                clear_val_cache()
                kw = {} if damping == "fixed" else dict(damping="marquardt", damp={g: lv for g in GROUPS},
                                                        marquardt_floor=f)
                try:
                    res = lm_step(m, train, val, bg, max_iter=k, restart_iter=k, check_every=False, device=dev,
                                  val_at_start=True, cache_val=False, precond=precond, **kw)
                    emit({"kind": "lm_step", "damping": damping, "lam": lv, "floor": f,
                          "solver": "plain" if precond is None else "jacobi", "max_iter": k, "alpha": res["best_alpha"],
                          "val_start": res["val_start_loss"], "val_final": res["final_val_loss"],
                          "train_start": res["start_loss"], "step_norm": float(res["step"].double().norm())})
                except AssertionError as e:  # (NonFiniteError: reported, not hidden)
                    emit({"kind": "lm_step", "damping": damping, "lam": lv, "floor": f,
                          "solver": "plain" if precond is None else "jacobi", "max_iter": k, "error": str(e)})
                del m
        clear_val_cache()


if __name__ == "__main__":
    main()
