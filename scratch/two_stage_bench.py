"""Two-stage search (TwoStageRetriever: fp8 first stage, exact bf16 rerank) against the exhaustive bf16 top-k, ONE process,
alternating launches.

At 1024 x 100 000 x 1030, k = 100, for candidates in {128, 256, 512, 1024}: HIP-event times of >= 3 launches of each form after one
warm-up -- the exhaustive `exact.topk`, `TwoStageRetriever.search` and its three parts (coarse pass, selection, rerank) -- recall@{1,
10,100} of the two-stage result against the exhaustive one on planted queries (planted as bench.py plants them) and on random
queries, and the rerank alone as pairs/s and bytes of corpus per second.  With --pooled the same with a first stage of the pages
mean-pooled to 41 patches (bf16; on pages without structure its recall says nothing about a trained student).

    python scratch/two_stage_bench.py --out profiles/two_stage_topk.json [--reps 3] [--small] [--pooled]
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
PAGE_BYTES = LP * D * 2
STREAM_TBPS = 7.1                 # README: 1-query streaming rate of the exhaustive bf16 kernel, the ceiling of a one-query-per-page pass


def mean(x):
    return sum(x) / len(x)


def pooled_corpus(cb, nout, dev):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    n, g = cb.n_pages, LP // nout
    out = torch.empty((n, nout, D), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, 2000):
        x = cb.planes[0, lo:lo + 2000, :g * nout].float()
        out[lo:lo + 2000] = F.normalize(x.view(x.shape[0], nout, g, D).mean(2), dim=-1).bfloat16()
    tm, pf = ops.pack_pmask(None, n, nout, dev)
    return PageCorpus(out[None], tm, pf)


def run(ts, exact, Qe, Qc, cands, reps):
    """Per candidate count: alternating exhaustive / two-stage launches, the parts of the latter, its result."""
    out, last = {}, {}
    es, ei = exact.topk(Qe, None, K)                                  # warm-up of the exhaustive form (and its result)
    for c in cands:
        search = lambda: ts.search(Qe, None, k=K, candidates=c, Q_coarse=Qc)      # noqa: E731
        ts.part_events = None
        (s0, i0), _ = timed(search)                                   # warm-up (workspaces, first launches)
        t_ex, t_ts, parts = [], [], []
        for _ in range(reps):
            (xs, xi), t = timed(lambda: exact.topk(Qe, None, K))
            t_ex.append(t)
            assert torch.equal(xi, ei)
            ts.part_events = []
            (s, i), t = timed(search)
            t_ts.append(t)
            ev = ts.part_events[0]
            parts.append([ev[j].elapsed_time(ev[j + 1]) for j in range(3)])
            ts.part_events = None
            assert torch.equal(i, i0) and torch.equal(s, s0), "two-stage result changed between launches"
        pairs = Qe.shape[0] * c
        rr = mean([p[2] for p in parts])
        out[str(c)] = {"exhaustive_ms": t_ex, "two_stage_ms": t_ts, "exhaustive_ms_mean": mean(t_ex), "two_stage_ms_mean": mean(t_ts),
                       "speedup": mean(t_ex) / mean(t_ts), "coarse_ms": mean([p[0] for p in parts]), "select_ms": mean([p[1] for p in parts]),
                       "rerank_ms": rr, "rerank_pairs_per_s": pairs / (rr * 1e-3), "rerank_corpus_TBps": pairs * PAGE_BYTES / (rr * 1e-3) / 1e12,
                       "rerank_frac_of_streaming": pairs * PAGE_BYTES / (rr * 1e-3) / 1e12 / STREAM_TBPS}
        last[c] = (s0, i0)
    return out, (es, ei), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--pooled", action="store_true")
    a = ap.parse_args()
    import evdr_amd  # noqa: F401
    from evdr_amd import _lib
    from evdr_amd.corpus import TwoStageRetriever
    dev = torch.device("cuda:0")
    n = 4000 if a.small else 100_000
    nq = 1024
    cands = (128, 256, 512, 1024)
    res = {"device": torch.cuda.get_device_name(0), "shape": f"{nq}x{n}x{LP}", "k": K, "reps": a.reps, "streaming_TBps_readme": STREAM_TBPS}
    cb, c8 = build(n, LP, dev)
    g = torch.Generator(device=dev).manual_seed(SEED + 5)
    Qr = F.normalize(torch.randn((nq, LQ, D), generator=g, device=dev), dim=-1)
    Qp, target = planted(nq, cb, LP, dev)
    stages = {"fp8": c8}
    if a.pooled:
        stages["pooled41_bf16"] = pooled_corpus(cb, 41, dev)
    for name, coarse in stages.items():
        ts = TwoStageRetriever(coarse, cb)
        sect = {}
        for qname, Q in (("planted", Qp), ("random", Qr)):
            Qe = Q.bfloat16()
            Qc = Q if coarse.fp8 else Qe
            timing, (es, ei), last = run(ts, cb, Qe, Qc, cands, a.reps if qname == "planted" else 1)
            for c in cands:
                s, i = last[c]
                timing[str(c)]["recall_vs_exhaustive"] = recall(ei, i)
                timing[str(c)]["top100_complete_share"] = float(((i[:, :, None] == ei[:, None, :]).any(-1).all(1)).float().mean())
                if qname == "planted":
                    timing[str(c)]["planted_top1"] = float((i[:, 0].long() == target).float().mean())
            sect[qname] = timing
        sect["coarse_kernel"] = None
        coarse.score(Qp if coarse.fp8 else Qp.bfloat16(), None, out=ts._ws[:nq * n].view(nq, n))
        sect["coarse_kernel"] = _lib.load().evdr_last_fwd_kernel().decode()
        cb.score_candidates(Qp.bfloat16(), None, torch.zeros((nq, 8), dtype=torch.int32, device=dev))
        sect["rerank_kernel"] = _lib.load().evdr_last_fwd_kernel().decode()
        res[name] = sect
        del ts
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
