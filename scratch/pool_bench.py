"""Pooled corpora, ONE process, alternating legs, median and spread of >= 5 runs; writes profiles/pooled_two_stage.json.

1. Building: `PageCorpus.from_pooled` of 4096 x 1030 x 128 bf16 pages (bf16 and fp8 kinds; windows of 4 patches, and 3 x 3 blocks of
   the 32 x 32 grid with the 6 remaining patches kept) against what the code could do for the same result before the fused kernel:
   pooling by `torch.index_add_` + l2_normalize + `from_tensor`.  HIP-event times around the whole preparation, allocation included
   on both sides.
2. Searching, at 1024 x 100 000 x 1030 x 128, k = 100, 512 candidates: `TwoStageRetriever(pooled bf16, exact bf16)` and `(pooled fp8,
   exact)`, each for f = 4 (windows) and f = 9 (3 x 3 blocks), against the exhaustive `exact.topk` and against the fp8 first stage of
   §4.6 -- time, parts (coarse pass, selection, rerank) and recall@10 / recall@100 against the exhaustive top-k, on planted queries
   (planted as bench.py plants them) and on random ones.  Random pages have no structure a mean could keep: the recall figures say
   what pooling costs on such pages, nothing about real documents.

    python scratch/pool_bench.py --out profiles/pooled_two_stage.json [--reps 5] [--small]
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

from fp8_bench import D, K, LQ, SEED, build, gen_chunk, planted, recall  # noqa: E402

LP, CANDIDATES = 1030, 512


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


def groupings(lp):
    from evdr_amd import ops
    side = int((lp - 6) ** 0.5) if lp > 6 else 0
    grid = ops.pool_groups_grid(side, side, 3, 3, first=0, lp=lp) if side and side * side + 6 == lp else ops.pool_groups_windows(lp, 9)
    return {"f4_windows": ops.pool_groups_windows(lp, 4), "f9_grid3x3": grid}


def torch_pooled(P, pm, mem, off, dt):
    """The same corpus without the fused kernel: index_add_ over the members, mean, l2_normalize, from_tensor."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    dev = P.device
    counts = (off[1:] - off[:-1]).long()
    gid = torch.repeat_interleave(torch.arange(counts.numel()), counts).to(dev)
    memd = mem.long().to(dev)
    x = P[:, memd].float()
    ok = torch.ones(P.shape[:2], dtype=torch.bool, device=dev) if pm is None else pm
    okm = ok[:, memd]
    sums = torch.zeros((P.shape[0], counts.numel(), D), dtype=torch.float32, device=dev).index_add_(1, gid, x * okm[:, :, None])
    cnt = torch.zeros((P.shape[0], counts.numel()), dtype=torch.float32, device=dev).index_add_(1, gid, okm.float())
    mean = sums / cnt.clamp_min(1.0)[:, :, None]
    pooled = mean / (mean.norm(dim=-1, keepdim=True) + 1e-12)
    return PageCorpus.from_tensor(pooled.bfloat16() if dt == torch.bfloat16 else pooled, cnt > 0, dtype=dt if dt == ops.FP8 else None)


def build_legs(n, lp, reps, dev):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    P = torch.cat([gen_chunk(lo, min(lo + 1000, n), lp, dev).bfloat16() for lo in range(0, n, 1000)])
    g = torch.Generator(device=dev).manual_seed(SEED + 3)
    pm = torch.arange(lp, device=dev)[None, :] < torch.randint(lp // 2, lp + 1, (n, 1), generator=g, device=dev)
    out = {}
    for gname, (mem, off) in groupings(lp).items():
        for kname, dt in (("bf16", torch.bfloat16), ("fp8", ops.FP8)):
            forms = {"from_pooled": lambda: PageCorpus.from_pooled(P, pm, mem, off, dtype=dt),
                     "torch_index_add_from_tensor": lambda: torch_pooled(P, pm, mem, off, dt)}
            for f in forms.values():
                timed(f)
            ms = {k: [] for k in forms}
            for _ in range(reps):
                for k, f in forms.items():
                    ms[k].append(timed(f)[1])
            a, b = forms["from_pooled"](), forms["torch_index_add_from_tensor"]()
            sa, sb = a.planes.view(torch.uint8), b.planes.view(torch.uint8)
            res = {k: summary(v) for k, v in ms.items()}
            res.update({"pages": n, "lp_src": lp, "ls": a.lp, "same_mask_words": bool(torch.equal(a.tilemask, b.tilemask)),
                        "plane_bytes_differing_from_torch_path": float((sa != sb).float().mean()),
                        "source_bytes": P.numel() * 2 + pm.numel(),
                        "from_pooled_source_GBps": (P.numel() * 2 + pm.numel()) / (res["from_pooled"]["median_ms"] * 1e-3) / 1e9,
                        "torch_over_from_pooled": res["torch_index_add_from_tensor"]["median_ms"] / res["from_pooled"]["median_ms"]})
            out[f"{gname}_{kname}"] = res
            print("build", gname, kname, json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}), flush=True)
            del a, b
    return out


def search_legs(n, nq, reps, dev):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    cb, c8 = build(n, LP, dev)
    g = torch.Generator(device=dev).manual_seed(SEED + 5)
    Qr = F.normalize(torch.randn((nq, LQ, D), generator=g, device=dev), dim=-1)
    Qp, target = planted(nq, cb, LP, dev)
    stages = {"fp8_same_tokens": c8}
    for gname, (mem, off) in groupings(LP).items():
        for kname, dt in (("bf16", torch.bfloat16), ("fp8", ops.FP8)):
            stages[f"pooled_{gname}_{kname}"] = PageCorpus.from_pooled(cb.planes[0], None, mem, off, dtype=dt)
    retr = {name: TwoStageRetriever(c, cb) for name, c in stages.items()}
    cands = min(CANDIDATES, n)
    qsets = {"planted": Qp, "random": Qr}

    def search(name, Q):
        coarse = stages[name]
        return retr[name].search(Q.bfloat16(), None, k=K, candidates=cands, Q_coarse=Q if coarse.fp8 else Q.bfloat16())

    res = {"shape": f"{nq}x{n}x{LP}x{D}", "k": K, "candidates": cands, "legs": {}}
    truth = {q: cb.topk(Q.bfloat16(), None, K) for q, Q in qsets.items()}              # warm-up of the exhaustive form, and the truth
    for name in stages:
        search(name, Qp)                                                               # warm-up (workspaces, first launches)
    t_ex = []
    ms = {name: [] for name in stages}
    parts = {name: [] for name in stages}
    for _ in range(reps):                                                              # alternating: exhaustive, then every first stage
        t_ex.append(timed(lambda: cb.topk(Qp.bfloat16(), None, K))[1])
        for name in stages:
            retr[name].part_events = []
            _, t = timed(lambda: search(name, Qp))
            ev = retr[name].part_events[0]
            retr[name].part_events = None
            ms[name].append(t)
            parts[name].append([ev[j].elapsed_time(ev[j + 1]) for j in range(3)])
    res["legs"]["exhaustive_bf16_topk"] = summary(t_ex)
    for name, coarse in stages.items():
        leg = summary(ms[name])
        leg.update({"first_stage_tokens": coarse.lp, "first_stage_kind": "fp8" if coarse.fp8 else "bf16",
                    "coarse_ms": statistics.median(p[0] for p in parts[name]), "select_ms": statistics.median(p[1] for p in parts[name]),
                    "rerank_ms": statistics.median(p[2] for p in parts[name]),
                    "speedup_over_exhaustive": statistics.median(t_ex) / leg["median_ms"]})
        for q, Q in qsets.items():
            s, i = search(name, Q)
            r = recall(truth[q][1], i)
            leg[f"{q}_recall@10"], leg[f"{q}_recall@100"] = r["recall@10"], r["recall@100"]
        leg["planted_top1"] = float((search(name, Qp)[1][:, 0].long() == target).float().mean())
        res["legs"][name] = leg
        print("search", name, json.dumps({k: v for k, v in leg.items() if k != "ms"}), flush=True)
    print("search exhaustive", json.dumps(res["legs"]["exhaustive_bf16_topk"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pooled_two_stage.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a rehearsal size (256 build pages, 4000 corpus pages): overheads only, not a measurement")
    ap.add_argument("--skip-search", action="store_true", help="the building legs only; the search legs are recorded as UNMEASURED")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench needs the GPU: there is nothing to measure without one")
    import evdr_amd  # noqa: F401
    dev = torch.device("cuda:0")
    reps = max(a.reps, 5)
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "small": a.small}
    res["build"] = build_legs(256 if a.small else 4096, LP, reps, dev)
    torch.cuda.empty_cache()
    res["search"] = "UNMEASURED" if a.skip_search else search_legs(4000 if a.small else 100_000, 1024, reps, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
