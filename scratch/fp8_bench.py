"""bf16 vs fp8 (e4m3fn) corpora built from the SAME fp32 pages, top-k in ONE process with alternating launches.

Shapes (k = 100): 1024 x 100 000 x 1030 (the headline), 8 x 100 000 (streaming: GB/s of corpus bytes), 500 x 6 847 (the configs2
shape: the first 6 847 pages as a shard view) and 1024 x 100 000 x 41-patch pages (student-sized).  Per case: HIP-event times of
>= 3 launches of each form after one warm-up, pairs/s, executed TFLOP/s (padded to 16-patch granules, 32 tokens x 128 x 2) and the
fp8 / bf16 ratio.  Quality: recall@{1,10,100} of the fp8 top-k against the bf16 top-k on random and on planted queries (planted
as bench.py plants them), and max / mean |s_fp8 - s_bf16| and |s_fp8 - s_fp32| on the first 2 000 pages.

    python scratch/fp8_bench.py --out profiles/fp8_topk.json [--reps 3] [--small]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, LQ, K = 128, 32, 100
SEED = 20261016
FP8_PEAK_TFLOPS = 5000.0
BF16_PEAK_TFLOPS = 2500.0


def gen_chunk(lo, hi, lp, dev):
    g = torch.Generator(device=dev).manual_seed(SEED + lo + 7 * lp)
    return F.normalize(torch.randn((hi - lo, lp, D), generator=g, device=dev), dim=-1)


def build(n, lp, dev):
    """bf16 and fp8 corpora of the same fp32 pages (generated chunk by chunk, never held whole in fp32)."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    bf = torch.empty((n, lp, D), dtype=torch.bfloat16, device=dev)
    f8 = torch.empty((n, lp, D), dtype=ops.FP8, device=dev)
    sh = torch.empty((n,), dtype=torch.int32, device=dev)
    for lo in range(0, n, 1000):
        hi = min(lo + 1000, n)
        x = gen_chunk(lo, hi, lp, dev)
        bf[lo:hi] = x.bfloat16()
        f8[lo:hi], sh[lo:hi] = ops.quantize_fp8(x, lp)
    tm, pf = ops.pack_pmask(None, n, lp, dev)
    return PageCorpus(bf[None], tm, pf), PageCorpus(f8[None], tm.clone(), pf.clone(), shift=sh)


def planted(nq, corpus_bf, lp, dev):
    g = torch.Generator(device=dev).manual_seed(SEED - 1)
    eps = F.normalize(torch.randn((nq, LQ, D), generator=g, device=dev), dim=-1)
    n = corpus_bf.n_pages
    t = (torch.arange(nq, device=dev) * 7919) % n
    rows = torch.stack([torch.randperm(lp, generator=g, device=dev)[:LQ] for _ in range(nq)])
    P = corpus_bf.planes[0]
    return F.normalize(P[t[:, None], rows].float() + 0.5 * eps, dim=-1), t


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def run_case(cb, c8, Q, reps, lp):
    nq = Q.shape[0]
    Qb = Q.bfloat16()
    fb = lambda: cb.topk(Qb, None, K)             # noqa: E731
    f8 = lambda: c8.topk(Q, None, K)              # noqa: E731
    (bs, bi), _ = timed(fb)
    (s8, i8), _ = timed(f8)
    tb, t8 = [], []
    for _ in range(reps):
        (bs, bi), t = timed(fb)
        tb.append(t)
        (x, y), t = timed(f8)
        t8.append(t)
        assert torch.equal(y, i8) and torch.equal(x, s8), "fp8 top-k changed between launches"
    mb, m8 = sum(tb) / len(tb), sum(t8) / len(t8)
    pairs = nq * cb.n_pages
    flops = pairs * (-(-lp // 16) * 16) * LQ * D * 2
    return {"nq": nq, "n_pages": cb.n_pages, "lp": lp, "bf16_ms": tb, "fp8_ms": t8, "bf16_ms_mean": mb, "fp8_ms_mean": m8,
            "bf16_pairs_per_s": pairs / (mb * 1e-3), "fp8_pairs_per_s": pairs / (m8 * 1e-3), "fp8_over_bf16": mb / m8,
            "fp8_tflops": flops / (m8 * 1e-3) / 1e12, "fp8_frac_of_5pf": flops / (m8 * 1e-3) / 1e12 / FP8_PEAK_TFLOPS,
            "bf16_tflops": flops / (mb * 1e-3) / 1e12, "bf16_frac_of_2_5pf": flops / (mb * 1e-3) / 1e12 / BF16_PEAK_TFLOPS,
            "fp8_corpus_GBps": c8.n_pages * lp * D / (m8 * 1e-3) / 1e9,
            "bf16_corpus_GBps": cb.n_pages * lp * D * 2 / (mb * 1e-3) / 1e9}, (bs, bi, s8, i8)


def recall(ib, i8):
    out = {}
    for r in (1, 10, 100):
        a, b = ib[:, :r].long(), i8[:, :r].long()
        hit = (b[:, :, None] == a[:, None, :]).any(-1).float().sum(1) / r
        out[f"recall@{r}"] = float(hit.mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import evdr_amd  # noqa: F401
    from evdr_amd import _lib
    from evdr_amd.corpus import PageCorpus
    dev = torch.device("cuda:0")
    n = 4000 if a.small else 100_000
    res = {"device": torch.cuda.get_device_name(0), "k": K, "reps": a.reps, "cases": {}}
    cb, c8 = build(n, 1030, dev)
    g = torch.Generator(device=dev).manual_seed(SEED + 5)
    Qr = F.normalize(torch.randn((1024, LQ, D), generator=g, device=dev), dim=-1)
    r, (bs, bi, s8, i8) = run_case(cb, c8, Qr, a.reps, 1030)
    r["kernel"] = _lib.load().evdr_last_fwd_kernel().decode()
    r["random_vs_bf16"] = recall(bi, i8)
    Qp, t = planted(1024, cb, 1030, dev)
    (pbs, pbi), _ = timed(lambda: cb.topk(Qp.bfloat16(), None, K))
    (p8s, p8i), _ = timed(lambda: c8.topk(Qp, None, K))
    r["planted_vs_bf16"] = recall(pbi, p8i)
    r["planted_top1_fp8"] = float((p8i[:, 0].long() == t).float().mean())
    r["planted_top1_bf16"] = float((pbi[:, 0].long() == t).float().mean())
    res["cases"]["1024x100000x1030"] = r
    # score differences on the first 2 000 pages (fp32 corpus of the same pages)
    m = min(2000, n)
    P32 = torch.cat([gen_chunk(lo, min(lo + 1000, m), 1030, dev) for lo in range(0, m, 1000)])
    c32 = PageCorpus.from_tensor(P32)
    Qs = Qr[:256]
    s32 = c32.score(Qs).double()
    sbf = cb.shard(0, m).score(Qs.bfloat16()).double()
    sf8 = c8.shard(0, m).score(Qs).double()
    res["score_diff_256x2000"] = {"fp8_vs_bf16_max": float((sf8 - sbf).abs().max()), "fp8_vs_bf16_mean": float((sf8 - sbf).abs().mean()),
                                  "fp8_vs_fp32_max": float((sf8 - s32).abs().max()), "fp8_vs_fp32_mean": float((sf8 - s32).abs().mean()),
                                  "bf16_vs_fp32_max": float((sbf - s32).abs().max())}
    del P32, c32
    r8, _ = run_case(cb, c8, Qr[:8], a.reps, 1030)
    res["cases"]["8x100000x1030"] = r8
    nc = min(6847, n)
    r5, _ = run_case(cb.shard(0, nc), c8.shard(0, nc), Qr[:500], a.reps, 1030)
    res["cases"][f"500x{nc}x1030"] = r5
    del cb, c8
    torch.cuda.empty_cache()
    cb, c8 = build(n, 41, dev)
    r41, _ = run_case(cb, c8, Qr, a.reps, 41)
    res["cases"]["1024x100000x41"] = r41
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
