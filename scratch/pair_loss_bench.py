"""The fused pairwise ranking losses against the torch form of criterion.py on one MI355X: time and peak memory of one
forward + backward of `pairwise_distillation_loss` and `lambda_loss` at the training batch (B = 32, N = 500) and at the reference's
all-dataset corpus (B = 32, N = 6 847), switch off (torch) and on (one HIP launch), same process, same inputs; and the largest errors of
both paths against the float64 statement of the rules over the input kinds of tests/pair_loss_cases.py.

Times are HIP-event times around one call (loss = f(s, t); loss.backward()) that ends in a device synchronise, >= 20 calls per leg after
warm-up, the two paths alternating; memory is torch.cuda.max_memory_allocated over one call minus what was allocated just before it.

    python scratch/pair_loss_bench.py --out profiles/pair_losses.json [--reps 20] [--small]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import evdr_amd  # noqa: E402,F401
from evdr_amd import criterion as crit, ops  # noqa: E402
import pair_loss_cases as PC  # noqa: E402

ALPHA, EPS = 1.0, 1e-6
LOSSES = {"pairwise_distillation_loss": lambda s, t: crit.pairwise_distillation_loss(s, t),
          "lambda_loss": lambda s, t: crit.lambda_loss(s, t, alpha=ALPHA, eps=EPS)}


def step(fn, s, t, fused):
    """One forward + backward on a fresh leaf; returns (loss, grad, ms, peak bytes over the baseline)."""
    (crit.enable_fused_pair_losses if fused else crit.disable_fused_pair_losses)()
    try:
        sg = s.detach().clone().requires_grad_(True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        a.record()
        loss = fn(sg, t)
        loss.backward()
        b.record()
        torch.cuda.synchronize()
        return loss.detach(), sg.grad, a.elapsed_time(b), torch.cuda.max_memory_allocated() - base
    finally:
        crit.disable_fused_pair_losses()


def summary(ms):
    return {"mean_ms": statistics.fmean(ms), "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def timing(b, n, reps, warmup, dev):
    s, t = (x.to(dev) for x in PC.scores("normal", b, n, seed=11))
    out = {"B": b, "N": n, "one_BNN_fp32_bytes": b * n * n * 4}
    for name, fn in LOSSES.items():
        legs = {"fused": True, "torch": False}
        rec = {}
        try:
            for _ in range(warmup):
                step(fn, s, t, False)
        except torch.OutOfMemoryError as e:
            legs.pop("torch")
            rec["torch"] = {"out_of_memory": str(e)[:200]}
            torch.cuda.empty_cache()
        for _ in range(warmup):
            step(fn, s, t, True)
        ms = {k: [] for k in legs}
        peak = {k: 0 for k in legs}
        last = {}
        for _ in range(reps):
            for k, fused in legs.items():
                loss, grad, dt, pk = step(fn, s, t, fused)
                ms[k].append(dt)
                peak[k] = max(peak[k], pk)
                last[k] = (float(loss), grad)
        for k in legs:
            rec[k] = dict(summary(ms[k]), peak_bytes_over_baseline=peak[k], loss=last[k][0])
        if "torch" in legs:
            rec["torch_over_fused_time"] = rec["torch"]["mean_ms"] / rec["fused"]["mean_ms"]
            rec["torch_over_fused_peak"] = rec["torch"]["peak_bytes_over_baseline"] / max(rec["fused"]["peak_bytes_over_baseline"], 1)
            rec["loss_rel_diff"] = abs(last["fused"][0] - last["torch"][0]) / abs(last["torch"][0])
            rec["grad_max_abs_diff_over_max"] = float((last["fused"][1] - last["torch"][1]).abs().max() / last["torch"][1].abs().max())
        del last
        torch.cuda.empty_cache()
        out[name] = rec
        print(b, n, name, json.dumps(rec), flush=True)
    return out


def errors(dev, shapes):
    """Per input kind, the largest error of each path against the float64 rule: loss relative; RankNet gradient |g - g64| in units of
    G = 2 / (B N); LambdaLoss gradient |g - g64| in units of max|g64|."""
    out = {}
    for kind in PC.KINDS:
        w = {p: {"ranknet_loss_rel": 0.0, "ranknet_grad_over_G": 0.0, "lambda_loss_rel": 0.0, "lambda_grad_over_max": 0.0} for p in ("fused", "torch")}
        for b, n in shapes:
            s, t = (x.to(dev) for x in PC.scores(kind, b, n))
            l64, g64 = ops.pairwise_distill_reference(s, t)
            s_sorted, gain, disc, order = PC.lambda_inputs(s, t)
            ll64, lg64 = ops.lambda_reference(s_sorted, gain, disc, ALPHA, EPS)
            lg64 = torch.zeros_like(lg64).scatter_(1, order, lg64)
            for p in ("fused", "torch"):
                loss, grad, _, _ = step(LOSSES["pairwise_distillation_loss"], s, t, p == "fused")
                w[p]["ranknet_loss_rel"] = max(w[p]["ranknet_loss_rel"], abs(float(loss) - float(l64)) / abs(float(l64)))
                w[p]["ranknet_grad_over_G"] = max(w[p]["ranknet_grad_over_G"], float((grad.double() - g64).abs().max()) / (2.0 / (b * n)))
                loss, grad, _, _ = step(LOSSES["lambda_loss"], s, t, p == "fused")
                if float(ll64) != 0.0:
                    w[p]["lambda_loss_rel"] = max(w[p]["lambda_loss_rel"], abs(float(loss) - float(ll64)) / abs(float(ll64)))
                if float(lg64.abs().max()) > 0.0:
                    w[p]["lambda_grad_over_max"] = max(w[p]["lambda_grad_over_max"], float((grad.double() - lg64).abs().max() / lg64.abs().max()))
        out[kind] = w
        print("errors", kind, json.dumps(w), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_losses.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a rehearsal size (B = 4, N = 200 / 600): overheads only, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_loss_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    reps = max(args.reps, 20)
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "small": args.small, "alpha": ALPHA, "eps": EPS,
           "timing": "HIP events around loss = f(s, t); loss.backward() on a fresh leaf, device synchronise before and after, paths alternating",
           "memory": "torch.cuda.max_memory_allocated over one call minus memory_allocated just before it"}
    sizes = [(4, 200), (4, 600)] if args.small else [(32, 500), (32, 6847)]
    res["shapes"] = [timing(b, n, reps, 3, dev) for b, n in sizes]
    err_shapes = [(1, 64), (3, 257), (33, 1000)]
    res["errors_vs_float64"] = {"shapes": err_shapes, "kinds": errors(dev, err_shapes)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
