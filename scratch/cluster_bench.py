"""Clustered corpora, ONE process, alternating legs, median and spread of >= 5 runs; writes
profiles/clustered_two_stage.json.

1. Building, on 4096 x 1030 x 128 bf16 pages at factor 4 and 9, iters 8: `ops.cluster_pages` alone, `PageCorpus.from_clustered` whole,
   `PageCorpus.from_pooled` with windows of the same factor (what clustering adds to a pooled build) and `ops.cluster_reference` on the
   same GPU tensors (the plain-torch statement of the rule, which takes its pages a few at a time; timed once on a slice of the pages
   and scaled -- it is hundreds of launches per slice).  The kernel's lists are compared with the reference's on that slice.
2. Searching: first-stage time and recall@10 / @100 of `TwoStageRetriever(coarse, exact bf16)` with the clustered against the
   window-pooled coarse corpus, against the exhaustive `exact.topk`, on structured pages (patches are noisy copies of K prototypes per
   page in shuffled order; queries are noisy patches of their page) and on random unit pages with planted queries as bench.py plants
   them.  Random pages have no groups to find: their recall stays poor for either grouping and says nothing about real documents.

    python scratch/cluster_bench.py --out profiles/clustered_two_stage.json [--reps 5] [--small]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fp8_bench import D, LQ, SEED, gen_chunk, recall  # noqa: E402

LP, ITERS = 1030, 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def summary(ms):
    return {"ms": ms, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def structured(n, lp, K, sigma, dev, seed):
    """proto = l2norm(randn(n, K, d)), z = randint(K, (n, lp)), P = l2norm(proto[z] + sigma * randn(n, lp, d) / sqrt(d)), by chunks."""
    out = torch.empty((n, lp, D), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, 1000):
        hi = min(lo + 1000, n)
        g = torch.Generator(device=dev).manual_seed(seed + lo)
        proto = F.normalize(torch.randn((hi - lo, K, D), generator=g, device=dev), dim=-1)
        z = torch.randint(K, (hi - lo, lp), generator=g, device=dev)
        noise = torch.randn((hi - lo, lp, D), generator=g, device=dev)
        out[lo:hi] = F.normalize(proto.gather(1, z[:, :, None].expand(-1, -1, D)) + sigma * noise / D ** 0.5, dim=-1).bfloat16()
    return out


def build_legs(n, lp, reps, ref_pages, dev):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    P = torch.cat([gen_chunk(lo, min(lo + 1000, n), lp, dev).bfloat16() for lo in range(0, n, 1000)])
    g = torch.Generator(device=dev).manual_seed(SEED + 3)
    pm = torch.arange(lp, device=dev)[None, :] < torch.randint(lp // 2, lp + 1, (n, 1), generator=g, device=dev)
    out = {}
    for f in (4, 9):
        ls = (lp + f - 1) // f
        win = ops.pool_groups_windows(lp, f)
        forms = {"cluster_pages": lambda: ops.cluster_pages(P, pm, factor=f, iters=ITERS),
                 "from_clustered": lambda: PageCorpus.from_clustered(P, pm, factor=f, iters=ITERS),
                 "from_pooled_windows": lambda: PageCorpus.from_pooled(P, pm, *win)}
        for fn in forms.values():
            timed(fn)
        ms = {k: [] for k in forms}
        for _ in range(reps):
            for k, fn in forms.items():
                ms[k].append(timed(fn)[1])
        res = {k: summary(v) for k, v in ms.items()}
        got = ops.cluster_pages(P[:ref_pages], pm[:ref_pages], factor=f, iters=ITERS, return_labels=True)
        want, t_ref = timed(lambda: ops.cluster_reference(P[:ref_pages], pm[:ref_pages], ls, ITERS))
        nv = int(pm.sum())
        lane_ops = 2.0 * nv * ls * D * ITERS                          # the pinned assign: one multiply and one add per column
        t = res["cluster_pages"]["median_ms"] * 1e-3
        res.update({"pages": n, "lp_src": lp, "ls": ls, "iters": ITERS, "valid_patches": nv,
                    "reference_pages": ref_pages, "reference_ms_once": t_ref, "reference_ms_scaled_to_all_pages": t_ref * n / ref_pages,
                    "reference_over_cluster_pages": t_ref * n / ref_pages / res["cluster_pages"]["median_ms"],
                    "kernel_equals_reference_on_those_pages": all(bool(torch.equal(a, b)) for a, b in zip(got, want)),
                    "assign_lane_ops": lane_ops, "assign_Tlane_ops_per_s": lane_ops / t / 1e12,
                    "pages_per_s": n / t,
                    "from_clustered_over_from_pooled_windows": res["from_clustered"]["median_ms"] / res["from_pooled_windows"]["median_ms"]})
        out[f"f{f}"] = res
        print("build", f"f{f}", json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}), flush=True)
    return out


def search_legs(name, P, pm, Q, target, ls, k, cands, reps):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    lp = P.shape[1]
    exact = PageCorpus.from_tensor(P, pm)
    f = (lp + ls - 1) // ls
    stages = {"windows": PageCorpus.from_pooled(P, pm, *ops.pool_groups_windows(lp, f)),
              "clustered": PageCorpus.from_clustered(P, pm, ls=ls, iters=ITERS)}
    retr = {s: TwoStageRetriever(c, exact) for s, c in stages.items()}
    truth = exact.topk(Q, None, k)
    for s in stages:
        retr[s].search(Q, None, k=k, candidates=cands)
    t_ex, ms, parts = [], {s: [] for s in stages}, {s: [] for s in stages}
    for _ in range(reps):
        t_ex.append(timed(lambda: exact.topk(Q, None, k))[1])
        for s in stages:
            retr[s].part_events = []
            _, t = timed(lambda: retr[s].search(Q, None, k=k, candidates=cands))
            ev = retr[s].part_events[0]
            retr[s].part_events = None
            ms[s].append(t)
            parts[s].append(ev[0].elapsed_time(ev[1]))
    res = {"shape": f"{Q.shape[0]}x{P.shape[0]}x{lp}x{D}", "k": k, "candidates": cands, "exhaustive_bf16_topk": summary(t_ex), "legs": {}}
    for s, c in stages.items():
        leg = summary(ms[s])
        _, idx = retr[s].search(Q, None, k=k, candidates=cands)
        r = recall(truth[1], idx)
        leg.update({"first_stage_tokens": c.lp, "first_stage_ms": statistics.median(parts[s]), "recall@10": r["recall@10"],
                    "recall@100": r["recall@100"], "planted_top1": float((idx[:, 0].long() == target).float().mean())})
        res["legs"][s] = leg
        print("search", name, s, json.dumps({a: b for a, b in leg.items() if a != "ms"}), flush=True)
    return res


def planted_queries(P, nq, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    n, lp = P.shape[:2]
    t = (torch.arange(nq, device=dev) * 7919) % n
    rows = torch.stack([torch.randperm(lp, generator=g, device=dev)[:LQ] for _ in range(nq)])
    eps = torch.randn((nq, LQ, D), generator=g, device=dev) / D ** 0.5
    return F.normalize(P[t[:, None], rows].float() + 0.5 * eps, dim=-1).bfloat16(), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clustered_two_stage.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a rehearsal size: overheads only, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench needs the GPU: there is nothing to measure without one")
    import evdr_amd  # noqa: F401
    dev = torch.device("cuda:0")
    reps = max(a.reps, 5)
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "small": a.small, "iters": ITERS}
    res["build"] = build_legs(64 if a.small else 4096, LP, reps, 8 if a.small else 32, dev)
    torch.cuda.empty_cache()
    n, nq = (512, 64) if a.small else (20_000, 512)
    res["search"] = {}
    # structured pages: 64 prototypes per page, 256 tokens after pooling (factor 4 of 1030 patches would be 258)
    P = structured(n, LP, 64, 0.3, dev, SEED + 11)
    Q, t = planted_queries(P, nq, dev, SEED + 12)
    res["search"]["structured_K64_sigma0.3"] = search_legs("structured", P, None, Q, t, 258, 100, min(512, n), reps)
    del P
    torch.cuda.empty_cache()
    P = torch.cat([gen_chunk(lo, min(lo + 1000, n), LP, dev).bfloat16() for lo in range(0, n, 1000)])
    Q, t = planted_queries(P, nq, dev, SEED + 13)
    res["search"]["random_pages"] = search_legs("random", P, None, Q, t, 258, 100, min(512, n), reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
