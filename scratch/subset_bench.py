"""Page-subset top-k (PageCorpus.topk(..., subset=s)) against the same number of CONTIGUOUS pages (corpus.shard(0, m).topk, the
exhaustive kernel over a view) and against scoring everything, ONE process, alternating launches.

bf16, 100 000 x 1030, k = 100: 1024 queries and 8 queries x random subsets of m = 1 000, 10 000 and 50 000 pages; fp32, 500 x 6 847 x
1030 with a 10 % and a 50 % subset.  Per case: HIP-event times of >= 3 launches of each form after one warm-up (mean, with the minimum
beside it), subset / shard ratio, speed-up over the full search, the kernel instance, and whether the subset scores are the full
search's bits (checked on the 8-query batch).

    python scratch/subset_bench.py --out profiles/subset_topk.json [--reps 5] [--small]
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

from fp8_bench import D, K, LQ, SEED, gen_chunk, timed      # noqa: E402

LP = 1030


def stats(ts):
    return {"ms": ts, "mean_ms": sum(ts) / len(ts), "min_ms": min(ts)}


def bf16_corpus(n, dev):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    bf = torch.empty((n, LP, D), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, 1000):
        hi = min(lo + 1000, n)
        bf[lo:hi] = gen_chunk(lo, hi, LP, dev).bfloat16()
    tm, pf = ops.pack_pmask(None, n, LP, dev)
    return PageCorpus(bf[None], tm, pf)


def run_case(corpus, Q, m, reps, gen, full_ms=None):
    """Alternating launches: contiguous shard of m pages / random subset of m pages (/ the whole corpus when full_ms is None)."""
    from evdr_amd import _lib
    n = corpus.n_pages
    sub = corpus.subset(pages=torch.randperm(n, generator=gen, device=Q.device)[:m])
    assert sub.m == m
    view = corpus.shard(0, m)
    f_sub = lambda: corpus.topk(Q, None, K, subset=sub)       # noqa: E731
    f_shard = lambda: view.topk(Q, None, K)                   # noqa: E731
    f_full = lambda: corpus.topk(Q, None, K)                  # noqa: E731
    (s0, i0), _ = timed(f_sub)                                # warm-up of each form (score blocks, first launches)
    kern = _lib.load().evdr_last_fwd_kernel().decode()
    timed(f_shard)
    shard_kern = _lib.load().evdr_last_fwd_kernel().decode()
    if full_ms is None:
        timed(f_full)
    t_sub, t_shard, t_full = [], [], []
    for _ in range(reps):
        _, t = timed(f_shard)
        t_shard.append(t)
        (s, i), t = timed(f_sub)
        t_sub.append(t)
        assert torch.equal(i, i0) and torch.equal(s, s0), "subset top-k changed between launches"
        if full_ms is None:
            _, t = timed(f_full)
            t_full.append(t)
    out = {"nq": Q.shape[0], "n_pages": n, "m": m, "subset": stats(t_sub), "shard": stats(t_shard), "subset_kernel": kern,
           "shard_kernel": shard_kern}
    if t_full:
        out["full"] = stats(t_full)
        full_ms = out["full"]["mean_ms"]
    out["full_mean_ms"] = full_ms
    out["subset_over_shard"] = out["subset"]["mean_ms"] / out["shard"]["mean_ms"]
    out["subset_over_shard_min"] = out["subset"]["min_ms"] / out["shard"]["min_ms"]
    out["speedup_over_full"] = full_ms / out["subset"]["mean_ms"]
    return out, sub


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 3
    import evdr_amd  # noqa: F401
    from evdr_amd.corpus import PageCorpus
    dev = torch.device("cuda:0")
    n = 4000 if a.small else 100_000
    sizes = (40, 400, 2000) if a.small else (1000, 10_000, 50_000)
    res = {"device": torch.cuda.get_device_name(0), "k": K, "reps": a.reps, "lp": LP, "gate": "subset <= 1.05 x shard at m = 10 000 and 50 000 (1024 queries)"}
    g = torch.Generator(device=dev).manual_seed(SEED + 9)
    cb = bf16_corpus(n, dev)
    for nq in (1024, 8):
        Q = F.normalize(torch.randn((nq, LQ, D), generator=g, device=dev), dim=-1).bfloat16()
        sect, full_ms = {}, None
        for m in sizes:
            sect[str(m)], sub = run_case(cb, Q, m, a.reps, g, full_ms)
            full_ms = sect[str(m)]["full_mean_ms"]
            if nq == 8:                                      # the subset's scores are the full search's bits for those columns
                want = cb.score(Q, None)[:, sub.pages.long()]
                sect[str(m)]["bits_equal_full_search"] = bool(torch.equal(cb.score(Q, None, subset=sub), want))
        res[f"bf16_{nq}x{n}"] = sect
    del cb
    torch.cuda.empty_cache()
    n32 = 400 if a.small else 6847
    P = torch.cat([gen_chunk(lo, min(lo + 1000, n32), LP, dev) for lo in range(0, n32, 1000)])
    c32 = PageCorpus.from_tensor(P)
    del P
    Q = F.normalize(torch.randn((500, LQ, D), generator=g, device=dev), dim=-1)
    sect, full_ms = {}, None
    for frac in (0.1, 0.5):
        m = int(n32 * frac)
        sect[f"{int(frac * 100)}%"], sub = run_case(c32, Q, m, a.reps, g, full_ms)
        full_ms = sect[f"{int(frac * 100)}%"]["full_mean_ms"]
        want = c32.score(Q, None)[:, sub.pages.long()]
        sect[f"{int(frac * 100)}%"]["bits_equal_full_search"] = bool(torch.equal(c32.score(Q, None, subset=sub), want))
    res[f"fp32_500x{n32}"] = sect
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
