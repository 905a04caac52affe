"""Filtered two-stage search (TwoStageRetriever.search(..., subset=): fp8 page-list first stage, exact bf16 rerank) against the
exhaustive bf16 subset top-k, ONE process, alternating launches.

At 1024 x 100 000 x 1030, k = 100, candidates = 512, for random subsets of 10 % and 50 % of the pages: HIP-event times of >= 3
launches of each form after one warm-up.  Two comparisons, each against a path that exists without the page-list kernel:
  1. the fp8 list pass `coarse.score_pages(Q, None, subset.pages)` against `coarse.shard(0, m).score(Q)`: the same number of
     CONTIGUOUS fp8 pages, same query batch, same kernel instance (ratio = list / contiguous);
  2. the whole filtered search and its three parts (coarse, select, rerank) against `exact.topk(Q, None, 100, subset=s)`.
Quality: recall@{1,10,100} of the filtered two-stage result against the exhaustive subset top-k and the share of complete top-100
lists, on planted queries (planted as bench.py plants them; top-1 is reported over the queries whose target the subset holds) and on
random queries.

    python scratch/two_stage_subset_bench.py --out profiles/two_stage_subset.json [--reps 3] [--small]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fp8_bench import D, K, LQ, SEED, build, planted, recall, timed      # noqa: E402

LP = 1030
CANDIDATES = 512


def mean(x):
    return sum(x) / len(x)


def list_vs_contiguous(c8, Q, s, block, reps, kernel_name):
    """The fp8 pass over the subset's list against the pass over the first m pages of the corpus, alternating."""
    head = c8.shard(0, s.m)
    f_list = lambda: c8.score_pages(Q, None, s.pages, out=block)      # noqa: E731
    f_cont = lambda: head.score(Q, None, out=block)                   # noqa: E731
    timed(f_list)
    k_list = kernel_name()
    timed(f_cont)
    k_cont = kernel_name()
    tl, tc = [], []
    for _ in range(reps):
        tc.append(timed(f_cont)[1])
        tl.append(timed(f_list)[1])
    pairs = Q.shape[0] * s.m
    return {"list_ms": tl, "contiguous_ms": tc, "list_ms_mean": mean(tl), "contiguous_ms_mean": mean(tc),
            "list_over_contiguous": mean(tl) / mean(tc), "list_pairs_per_s": pairs / (mean(tl) * 1e-3),
            "contiguous_pairs_per_s": pairs / (mean(tc) * 1e-3), "list_kernel": k_list, "contiguous_kernel": k_cont}


def search_vs_exhaustive(ts, exact, Qe, Qc, s, reps):
    """Alternating launches of exact.topk(subset=) and the filtered two-stage search, the parts of the latter, both results."""
    search = lambda: ts.search(Qe, None, k=K, candidates=CANDIDATES, Q_coarse=Qc, subset=s)      # noqa: E731
    exhaustive = lambda: exact.topk(Qe, None, K, subset=s)                                       # noqa: E731
    (es, ei), _ = timed(exhaustive)
    ts.part_events = None
    (s0, i0), _ = timed(search)
    t_ex, t_ts, parts = [], [], []
    for _ in range(reps):
        (xs, xi), t = timed(exhaustive)
        t_ex.append(t)
        assert torch.equal(xi, ei)
        ts.part_events = []
        (gs, gi), t = timed(search)
        t_ts.append(t)
        ev = ts.part_events[0]
        parts.append([ev[j].elapsed_time(ev[j + 1]) for j in range(3)])
        ts.part_events = None
        assert torch.equal(gi, i0) and torch.equal(gs, s0), "two-stage result changed between launches"
    out = {"exhaustive_subset_ms": t_ex, "two_stage_ms": t_ts, "exhaustive_subset_ms_mean": mean(t_ex), "two_stage_ms_mean": mean(t_ts),
           "speedup": mean(t_ex) / mean(t_ts), "coarse_ms": mean([p[0] for p in parts]), "select_ms": mean([p[1] for p in parts]),
           "rerank_ms": mean([p[2] for p in parts])}
    return out, (es, ei), (s0, i0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import evdr_amd  # noqa: F401
    from evdr_amd import _lib
    from evdr_amd.corpus import TwoStageRetriever
    kernel_name = lambda: _lib.load().evdr_last_fwd_kernel().decode()      # noqa: E731
    dev = torch.device("cuda:0")
    n = 4000 if a.small else 100_000
    nq = 1024
    res = {"device": torch.cuda.get_device_name(0), "shape": f"{nq}x{n}x{LP}", "k": K, "candidates": CANDIDATES, "reps": a.reps,
           "compared_with": {"list_pass": "coarse.shard(0, m).score(Q): evdr_maxsim_fwd_fp8 over m contiguous pages",
                             "search": "exact.topk(Q, None, 100, subset=s): evdr_maxsim_fwd_pages (bf16) + evdr_topk"}}
    cb, c8 = build(n, LP, dev)
    g = torch.Generator(device=dev).manual_seed(SEED + 5)
    Qr = F.normalize(torch.randn((nq, LQ, D), generator=g, device=dev), dim=-1)
    Qp, target = planted(nq, cb, LP, dev)
    ts = TwoStageRetriever(c8, cb)
    block = torch.empty((nq, n), dtype=torch.float32, device=dev)
    for frac in (0.1, 0.5):
        gs = torch.Generator(device=dev).manual_seed(SEED + int(frac * 100))
        allow = torch.rand(n, generator=gs, device=dev) < frac
        s = cb.subset(allow=allow)
        sect = {"m": s.m}
        sect["fp8_list_pass"] = list_vs_contiguous(c8, Qp, s, block[:, :s.m], a.reps, kernel_name)
        for qname, Q in (("planted", Qp), ("random", Qr)):
            timing, (es, ei), (s2, i2) = search_vs_exhaustive(ts, cb, Q.bfloat16(), Q, s, a.reps if qname == "planted" else 1)
            timing["recall_vs_exhaustive_subset"] = recall(ei, i2)
            timing["top100_complete_share"] = float(((i2[:, :, None] == ei[:, None, :]).any(-1).all(1)).float().mean())
            timing["indices_inside_subset"] = bool(allow[i2.clamp_min(0).long()][i2 >= 0].all())
            if qname == "planted":
                inside = allow[target]
                timing["planted_targets_inside"] = int(inside.sum())
                timing["planted_top1_of_allowed_targets"] = float((i2[inside, 0].long() == target[inside]).float().mean())
            sect[qname] = timing
        res[f"subset_{int(frac * 100)}pct"] = sect
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
