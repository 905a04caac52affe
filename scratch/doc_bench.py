"""Document-level search: what collapsing page scores to documents costs on one MI355X.

1. `evdr_doc_max` alone over a 1024 x 100 000 fp32 score block, at 1, 8 and 64 pages per document and for a skewed mix (documents of
   1..15 pages and one of 5 000), against
   - the torch route on the same box: `scatter_reduce(amax)` into (nq, n_docs), then a second pass for the best page (the lowest
     column whose score equals its document's maximum: `scatter_reduce(amin)` of masked column numbers), with the (nq, n) index
     tensor built once outside the timed call -- without the order key (NaN and -0.0 are not handled the same way; the block
     holds neither here);
   - a plain device copy of the score block (`Tensor.copy_`): the same bytes read once and written once, i.e. about twice the
     traffic of the segmented maximum, which writes (nq, n_docs) words only.  Both ratios are reported.
2. `PageCorpus.topk_docs` against `PageCorpus.topk` at the same shape (bf16 pages): the cost of collapsing on top of a page search.
3. `PageCorpus.rerank_docs` against `PageCorpus.rerank` at 512 candidates per query.

Times are HIP-event times around the call, mean / min / max of >= 5 launches after one warm-up of each form, one process.

    python scratch/doc_bench.py --out profiles/doc_search.json [--reps 5] [--small]
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

import evdr_amd  # noqa: E402,F401
from evdr_amd import ops  # noqa: E402
from evdr_amd.corpus import PageCorpus  # noqa: E402

D, SEED = 128, 13


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def summary(ms):
    return {"ms": ms, "mean_ms": statistics.fmean(ms), "min_ms": min(ms), "max_ms": max(ms)}


def measure(forms, reps):
    for f in forms.values():
        timed(f)
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, f in forms.items():
            ms[name].append(timed(f)[1])
    return {name: summary(v) for name, v in ms.items()}


def torch_route(scores, idx, n_docs, cols):
    """(doc_scores, doc_best): two scatter_reduce passes and the compare between them."""
    nq, n = scores.shape
    ds = torch.full((nq, n_docs), float("-inf"), dtype=torch.float32, device=scores.device)
    ds.scatter_reduce_(1, idx, scores, "amax", include_self=True)
    hit = scores == ds.gather(1, idx)
    best = torch.full((nq, n_docs), n, dtype=torch.int32, device=scores.device)
    best.scatter_reduce_(1, idx, torch.where(hit, cols[None, :], torch.full_like(cols, n)[None, :]), "amin", include_self=True)
    return ds, best


def doc_layout(case, n, gen, dev):
    """(n,) int32 document of each page for a named case; documents are runs of consecutive pages (a PDF's pages)."""
    if case.startswith("pages_"):
        per = int(case.split("_")[1])
        return (torch.arange(n, device=dev) // per).to(torch.int32)
    big = min(5000, n // 2)                                                # skewed: one document of 5 000 pages, the rest 1..15
    sizes = torch.randint(1, 16, (n,), generator=gen, device=dev)
    ends = torch.cumsum(sizes, 0)
    sizes = sizes[: int((ends < n - big).sum()) + 1]
    sizes[-1] = n - big - int(sizes[:-1].sum())
    sizes = torch.cat([sizes[: len(sizes) // 2], torch.tensor([big], device=dev), sizes[len(sizes) // 2:]])
    return torch.repeat_interleave(torch.arange(len(sizes), device=dev), sizes).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "doc_search.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a rehearsal size (64 x 4096 scores, 512 pages x 225): overheads only, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("doc_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    reps = max(args.reps, 5)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "small": args.small}

    # ---- 1. evdr_doc_max alone ----------------------------------------------------------------------------------------------------
    nq, n = (64, 4096) if args.small else (1024, 100_000)
    scores = torch.randn((nq, n), generator=gen, device=dev)
    copy_to = torch.empty_like(scores)
    cols = torch.arange(n, dtype=torch.int32, device=dev)
    res["doc_max"] = {"rows": nq, "columns": n, "score_bytes": nq * n * 4}
    for case in ("pages_1", "pages_8", "pages_64", "skewed"):
        doc = doc_layout(case, n, gen, dev)
        n_docs = int(doc.max().item()) + 1
        members, offsets = ops.doc_lists(doc, n_docs)
        out = (torch.empty((nq, n_docs), dtype=torch.float32, device=dev), torch.empty((nq, n_docs), dtype=torch.int32, device=dev))
        doc_long = doc.long()
        idx = doc_long[None, :].expand(nq, n).contiguous()
        r = measure({"doc_max": lambda: ops.doc_max(scores, members, offsets, out=out),
                     "torch": lambda: torch_route(scores, idx, n_docs, cols),
                     "copy": lambda: copy_to.copy_(scores)}, reps)
        ds, db = ops.doc_max(scores, members, offsets)
        tds, tdb = torch_route(scores, idx, n_docs, cols)
        r.update({"n_docs": n_docs, "largest_document": int(torch.bincount(doc_long).max().item()),
                  "torch_over_doc_max": r["torch"]["mean_ms"] / r["doc_max"]["mean_ms"],
                  "doc_max_over_copy": r["doc_max"]["mean_ms"] / r["copy"]["mean_ms"],
                  "score_bytes_per_s": nq * n * 4 / (r["doc_max"]["mean_ms"] * 1e-3),
                  "equals_torch_route": bool(torch.equal(ds, tds) and torch.equal(db, tdb))})
        res["doc_max"][case] = r
        print(case, json.dumps({a: b for a, b in r.items() if not isinstance(b, dict)}), flush=True)
    del scores, copy_to

    # ---- 2 / 3. on top of a page search and of a rerank -------------------------------------------------------------------------------
    nq, lq, npg, lp, k, r_cand = (64, 32, 512, 225, 10, 128) if args.small else (1024, 32, 100_000, 1030, 100, 512)
    res["search"] = {"queries": nq, "lq": lq, "pages": npg, "lp": lp, "k": k, "candidates": r_cand, "pages_per_document": 8}
    chunk = 4096
    P = torch.empty((npg, lp, D), dtype=torch.bfloat16, device=dev)
    for s in range(0, npg, chunk):
        P[s:s + chunk] = F.normalize(torch.randn((min(chunk, npg - s), lp, D), generator=gen, device=dev), dim=-1).bfloat16()
    Q = F.normalize(torch.randn((nq, lq, D), generator=gen, device=dev), dim=-1).bfloat16()
    qmask = torch.arange(lq, device=dev)[None, :] < torch.randint(lq // 2, lq + 1, (nq, 1), generator=gen, device=dev)
    corpus = PageCorpus.from_tensor(P, None)
    docs = corpus.documents((torch.arange(npg, device=dev) // 8).to(torch.int32))
    cand = torch.stack([torch.randperm(npg, generator=gen, device=dev)[:r_cand] for _ in range(nq)]).to(torch.int32).contiguous()
    sr = measure({"topk": lambda: corpus.topk(Q, qmask, k), "topk_docs": lambda: corpus.topk_docs(Q, qmask, k, docs),
                  "rerank": lambda: corpus.rerank(Q, qmask, cand, k), "rerank_docs": lambda: corpus.rerank_docs(Q, qmask, cand, k, docs)}, reps)
    res["search"].update(sr)
    res["search"].update({"topk_docs_over_topk": sr["topk_docs"]["mean_ms"] / sr["topk"]["mean_ms"],
                          "topk_docs_minus_topk_ms": sr["topk_docs"]["mean_ms"] - sr["topk"]["mean_ms"],
                          "rerank_docs_over_rerank": sr["rerank_docs"]["mean_ms"] / sr["rerank"]["mean_ms"],
                          "rerank_docs_minus_rerank_ms": sr["rerank_docs"]["mean_ms"] - sr["rerank"]["mean_ms"]})
    print("search", json.dumps({a: b for a, b in res["search"].items() if not isinstance(b, dict)}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
