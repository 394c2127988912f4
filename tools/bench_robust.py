#!/usr/bin/env python3
"""The LM step under a robust loss: what it costs and what it buys.

The scene and validation set of bench.py's `lm_step` measurement: 1M Gaussians, SH 3, one 1080p training view, 50
validation views (orbit seed 5), ground truth = the render of the perturbed model.  Three measurements:

  cost (default)   lm_step(max_iter=10, restart_iter=10, timing=True) and LMProblem.evaluate() in the modes
                   plain / huber / cauchy, alternating in one process over --rounds rounds, the model restored after
                   every step; every mode keeps its own validation evaluator from step to step (lm_step's cache holds
                   one: the tool swaps the entry around each call).  --delta is chosen inside the residuals' range so
                   that both branches of |r| <= delta are taken.
  --transient      a constant-colour block painted into the ground truth of the training view only; --steps LM steps
                   in plain, huber and cauchy from the same start, the line search on the training view (the step has no
                   clean data), and after each step the PLAIN loss 2 sum r^2 of the clean validation views and of
                   the training view against its ground truth without the block.
  --oracle         the same experiment in float64 on the CPU oracle at sh3_40x33 (two training views with the block,
                   two clean views; cgls_ref 5 x 5, line_search_ref); needs no GPU.
One JSON line per measurement to stdout and, with --out, to a file.  There is no fallback: without a GPU the GPU modes
fail.

  python tools/bench_robust.py --rounds 5 --out profiles/lm_robust/cost.jsonl
  python tools/bench_robust.py --transient --out profiles/lm_robust/transient_gpu.jsonl
  python tools/bench_robust.py --oracle --out profiles/lm_robust/transient_oracle.jsonl
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_COLOUR = (0.9, 0.1, 0.6)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sh", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--s0", type=float, default=0.005)
    ap.add_argument("--val-views", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--delta", type=float, default=None, help="default 0.002 (cost), 0.1 (--transient, --oracle)")
    ap.add_argument("--modes", default="plain,huber,cauchy")
    ap.add_argument("--transient", action="store_true")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def paint_block(img, frac=(0.30, 0.35, 0.60, 0.70)):
    """A constant-colour block over the given fractions (x0, y0, x1, y1) of a [3, H, W] image, in place."""
    _, H, W = img.shape
    x0, y0, x1, y1 = int(frac[0] * W), int(frac[1] * H), int(frac[2] * W), int(frac[3] * H)
    for c in range(3):
        img[c, y0:y1, x0:x1] = BLOCK_COLOUR[c]
    return (x1 - x0) * (y1 - y0) / float(H * W)


def oracle_transient(args, emit):
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import torch
    import lm_robust_ref as RR
    from gslm.lm import update_params
    from oracle import torch_raster as tr
    from oracle.lm_ref import OracleLMProblem, OracleLossEvaluator, cgls_ref, line_search_ref
    from scenes import BG_GENERIC, lm_bg_scene, to_float64
    delta = 0.1 if args.delta is None else args.delta
    model, cams = lm_bg_scene("sh3_40x33", n_views=4, brighten=False)
    model, cams = to_float64(model, cams)
    bg = torch.tensor(BG_GENERIC, dtype=torch.float64)
    true = copy.deepcopy(model)
    gen = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for t, sd in ((true._features_dc, 0.3), (true._opacity, 0.5), (true._scaling, 0.1)):
            t += sd * torch.randn(t.shape, generator=gen, dtype=torch.float64)
        for c in cams:
            c.original_image = tr.render_model(true, c, bg)[0].clamp(0, 1).detach()
    train, clean = cams[:2], cams[2:]
    train_clean = [copy.deepcopy(c) for c in train]  # the training views without the block
    share = [paint_block(c.original_image) for c in train]
    for mode in ("plain", "huber", "cauchy"):
        m = copy.deepcopy(model)
        rob = (mode, delta)
        held = OracleLossEvaluator(m, clean, bg)
        held_train = OracleLossEvaluator(m, train_clean, bg)
        emit({"kind": "oracle_transient", "mode": mode, "step": 0, "clean_val_l2": float(held.evaluate()),
              "clean_train_l2": float(held_train.evaluate()), "delta": delta, "block_share": share[0]})
        for k in range(1, args.steps + 1):
            prob = OracleLMProblem(m, train, bg) if mode == "plain" else RR.RobustOracleLMProblem(m, train, bg, rob)
            start = float(prob.evaluate())
            s = cgls_ref(prob, prob.rhs(), 5, 5)
            ls = OracleLossEvaluator(m, train, bg) if mode == "plain" else RR.RobustOracleLossEvaluator(m, train, bg, rob)
            alpha, final, _ = line_search_ref(lambda a: update_params(m, prob.layout, s, a), ls.evaluate)
            emit({"kind": "oracle_transient", "mode": mode, "step": k, "train_loss_start": start, "train_loss_end": final,
                  "best_alpha": alpha, "clean_val_l2": float(held.evaluate()),
                  "clean_train_l2": float(held_train.evaluate()), "delta": delta})


def main():
    args = parse()
    out = open(args.out, "a") if args.out else None

    def emit(line):
        s = json.dumps(dict(line, label=args.label))
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-lm_amd"))
    if args.oracle:
        oracle_transient(args, emit)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust.py needs the GPU: a CPU run has no timing to report (--oracle runs on the CPU)")
    from gslm import lm
    from gslm.cameras import orbit_cameras
    from gslm.model import synthetic_gaussians
    dev = torch.device("cuda", 0)
    W, H = args.width, args.height
    bg = torch.zeros(3)
    cams = [c.to(dev) for c in orbit_cameras(1, W, H, seed=1)]
    val = [c.to(dev) for c in orbit_cameras(args.val_views, W, H, seed=5)]
    pert = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu")
    g2 = torch.Generator().manual_seed(2)
    with torch.no_grad():
        pert._features_dc += 0.01 * torch.randn(pert._features_dc.shape, generator=g2)
        pert._opacity += 0.01 * torch.randn(pert._opacity.shape, generator=g2)
        pert._scaling += 0.01 * torch.randn(pert._scaling.shape, generator=g2)
    pert.to(dev)
    every = cams + val
    for c0 in range(0, len(every), 8):
        chunk = every[c0:c0 + 8]
        p = lm.LMProblem(pert, chunk, bg, device=dev)
        p.evaluate()
        for c, vr in zip(chunk, p.views):
            c.original_image = vr.color.clamp(0, 1).clone()
        del p
    del pert
    torch.cuda.empty_cache()
    model = synthetic_gaussians(args.P, args.sh, seed=0, s0=args.s0, device="cpu").to(dev)
    leaves = [t for t in model.params() if t is not model._xyz]  # xyz is masked: its version keeps the depth orders
    saved = [t.detach().clone() for t in leaves]

    def restore():
        with torch.no_grad():
            for t, s0 in zip(leaves, saved):
                t.copy_(s0)

    if args.transient:
        delta = 0.1 if args.delta is None else args.delta
        clean_gt = cams[0].original_image.clone()  # the training view without the block
        share = paint_block(cams[0].original_image)
        held = lm.LossEvaluator(model, val, bg, device=dev)
        held_train = lm.LossEvaluator(model, cams, bg, device=dev, gts=[clean_gt])
        for mode in ("plain", "huber", "cauchy"):
            restore()
            lm.clear_val_cache()
            kw = {} if mode == "plain" else {"robust": (mode, delta)}
            emit({"kind": "transient", "mode": mode, "step": 0, "clean_val_l2": float(held.evaluate()),
                  "clean_train_l2": float(held_train.evaluate()), "delta": delta, "block_share": share, "P": args.P})
            for k in range(1, args.steps + 1):
                o = lm.lm_step(model, cams, cams, bg, max_iter=args.iters, restart_iter=args.iters, **kw)
                emit({"kind": "transient", "mode": mode, "step": k, "train_loss_start": o["start_loss"],
                      "train_loss_end": o["final_val_loss"], "best_alpha": o["best_alpha"],
                      "clean_val_l2": float(held.evaluate()), "clean_train_l2": float(held_train.evaluate()),
                      "delta": delta})
        lm.clear_val_cache()
        return

    delta = 0.002 if args.delta is None else args.delta  # (the residuals' rms is 0.0018: both branches busy)
    MODES = {"plain": {}, "huber": {"robust": ("huber", delta)}, "cauchy": {"robust": ("cauchy", delta)}}
    modes = [m for m in args.modes.split(",") if m]
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode {m!r}")
    caches = {}
    probs = {m: lm.LMProblem(model, cams, bg, device=dev, sh_projection="auto", **MODES[m]) for m in modes}

    def step(m):
        lm._VAL_CACHE.clear()
        if m in caches:
            lm._VAL_CACHE["last"] = caches[m]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = lm.lm_step(model, cams, val, bg, max_iter=args.iters, restart_iter=args.iters, timing=True, **MODES[m])
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        caches[m] = lm._VAL_CACHE.get("last")
        restore()
        return ms, o

    def evaluate_ms(m, reps=10):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        probs[m].evaluate()
        ev[0].record()
        for k in range(reps):
            probs[m].evaluate()
            ev[k + 1].record()
        torch.cuda.synchronize()
        return sorted(ev[k].elapsed_time(ev[k + 1]) for k in range(reps))[reps // 2]

    for m in modes:  # workspaces, depth orders, clocks
        for _ in range(2):
            ms, o = step(m)
        emit({"kind": "warmup", "mode": m, "ms": ms, "line_search": o["line_search"], "delta": delta})
    probs[modes[0]].evaluate()
    r = probs[modes[0]].residuals[0]
    emit({"kind": "residuals", "share_outside_delta": float((r.abs() > delta).float().mean()), "delta": delta,
          "rms": float(r.double().pow(2).mean().sqrt())})
    for rnd in range(args.rounds):
        for m in modes:
            ms, o = step(m)
            emit({"kind": "lm_step", "round": rnd, "mode": m, "ms": ms, "phases_ms": o["timing"],
                  "evaluate_ms": evaluate_ms(m), "line_search": o["line_search"], "best_alpha": o["best_alpha"],
                  "final_val_loss": o["final_val_loss"], "P": args.P, "val_views": args.val_views, "iters": args.iters})
    if out:
        out.close()


if __name__ == "__main__":
    main()
