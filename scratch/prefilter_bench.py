"""Exhaustive vs prefiltered fp32 top-k (PageCorpus.topk(..., prefilter=True)) in ONE process, alternating launches.

Shapes: 1024 x 100 000 x 1030 (52.7 GB of fp16 hi/lo planes; genuinely fp32 unit-norm Gaussian pages, not bf16-representable) and
500 x 6 847 (the configs2 shape), k = 100; seeded random unit-norm queries and planted queries (query i on page (i * 7919) mod N,
token n = normalise(P[t_i, pi_i(n)] + 0.5 eps), as bench.py plants them).  Per case: device-event times of >= 3 launches of each
form after one warm-up, bit-equality asserted on every launch, and the candidate-count distribution / fallback rows.

    python scratch/prefilter_bench.py --out profiles/prefilter_fp32.json [--reps 3] [--small]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scratch/prefilter_bench.py --reps 1 --trace   (per-kernel split)
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LP, D, LQ, K = 1030, 128, 32, 100
SEED = 20261016


def gen_pages(n, dev):
    P = torch.empty((n, LP, D), dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev)
    for lo in range(0, n, 1000):
        hi = min(lo + 1000, n)
        g.manual_seed(SEED + lo)
        P[lo:hi] = F.normalize(torch.randn((hi - lo, LP, D), generator=g, device=dev), dim=-1)
    return P


def queries(kind, nq, P, dev):
    g = torch.Generator(device=dev).manual_seed(SEED - 1)
    eps = F.normalize(torch.randn((nq, LQ, D), generator=g, device=dev), dim=-1)
    if kind == "random":
        return eps
    n = P.shape[0]
    t = (torch.arange(nq, device=dev) * 7919) % n
    rows = torch.stack([torch.randperm(LP, generator=g, device=dev)[:LQ] for _ in range(nq)])
    return F.normalize(P[t[:, None], rows] + 0.5 * eps, dim=-1)


def same(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def run_case(corpus, Q, reps):
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1)
    ex = lambda: corpus.topk(Q, None, K)                         # noqa: E731
    pf = lambda: corpus.topk(Q, None, K, prefilter=True)          # noqa: E731
    (es, ei), _ = timed(ex)                                      # warm-up (the first prefiltered call also computes the corpus bound)
    (ps, pi), _ = timed(pf)
    assert torch.equal(pi, ei) and same(ps, es)
    t_ex, t_pf = [], []
    for _ in range(reps):
        (es, ei), t = timed(ex)
        t_ex.append(t)
        (ps, pi), t = timed(pf)
        t_pf.append(t)
        assert torch.equal(pi, ei) and same(ps, es), "prefiltered top-k differs from the exhaustive one"
    st = corpus.prefilter_stats()
    cnt = None
    if corpus._pf_stats is not None:
        c = corpus._pf_stats[0][:-1].float()
        c = c[c >= 0]
        cnt = {f"p{p}": float(torch.quantile(c, p / 100).item()) for p in (0, 10, 50, 90, 99, 100)}
    return {"exhaustive_ms": t_ex, "prefilter_ms": t_pf, "exhaustive_ms_mean": sum(t_ex) / len(t_ex),
            "prefilter_ms_mean": sum(t_pf) / len(t_pf), "speedup": (sum(t_ex) / len(t_ex)) / (sum(t_pf) / len(t_pf)),
            "bit_equal_launches": reps + 1, "stats": st, "candidate_quantiles": cnt,
            "candidate_fraction_mean": st["candidates_mean"] / corpus.n_pages if st["candidates_mean"] is not None else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="only the configs2 shape")
    ap.add_argument("--trace", action="store_true", help="large shape, random queries only (under rocprofv3)")
    a = ap.parse_args()
    import evdr_amd  # noqa: F401
    from evdr_amd.corpus import PageCorpus
    dev = torch.device("cuda:0")
    shapes = [(500, 6847)] if a.small else ([(1024, 100000)] if a.trace else [(500, 6847), (1024, 100000)])
    rec = {"workload": "PageCorpus.topk, k = 100, fp32 unit-norm Gaussian pages (fp16 hi/lo planes), lq = 32, all-valid masks",
           "method": f"one process, exhaustive and prefiltered calls alternating, {a.reps} timed launches each after one warm-up, HIP events "
                     "around the whole call on the current stream; bit-equality of scores and indices asserted on every launch",
           "device": torch.cuda.get_device_name(dev), "cases": []}
    for nq, n in shapes:
        t0 = time.time()
        P = gen_pages(n, dev)
        Qs = {kind: queries(kind, nq, P, dev) for kind in (("random",) if a.trace else ("random", "planted"))}
        corpus = PageCorpus.from_tensor(P)
        del P
        torch.cuda.empty_cache()
        for kind, Q in Qs.items():
            r = run_case(corpus, Q, a.reps)
            r.update({"queries": nq, "pages": n, "query_kind": kind})
            rec["cases"].append(r)
            print(json.dumps(r), flush=True)
        print(f"shape {nq} x {n}: {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        del corpus, Qs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
