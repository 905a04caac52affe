"""Token alignment: time of aligning the top-10 of 1024 queries over a bf16 corpus of 1030-patch pages with
`PageCorpus.align`, with and without the heat map, against the torch route on the same box: gather the listed pages from the source
tensor, `einsum`, masked `max` and `argmax` (queries taken `--chunk` at a time so that the gathered pages fit).

Times are HIP-event times around the call, mean / min / max of >= 5 launches after one warm-up of each form, one process.  Bytes are
counted from shapes: every listed page is read once per pair.  The two routes are compared on the way (indices equal wherever the
torch route's own top-two gap exceeds 2e-5).

    python scratch/align_bench.py --out profiles/align.json [--reps 5] [--pages 8192] [--small]
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
from evdr_amd.corpus import PageCorpus  # noqa: E402

D, SEED = 128, 12


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


def torch_route(Q, qmask, P, pmask, cand, chunk, heat):
    """(sim, patch[, heat]) of real entries by the rule of ops.align_reference, in the corpus dtype's fp32 products."""
    sims, patches, heats = [], [], []
    for s in range(0, Q.shape[0], chunk):
        idx = cand[s:s + chunk].long()
        pages, pm = P[idx], pmask[idx]                                          # (c, r, lp, d), (c, r, lp)
        dots = torch.einsum("qnd,qrmd->qrnm", Q[s:s + chunk].float(), pages.float())
        filled = torch.where(pm[:, :, None, :], dots, torch.full_like(dots, -1e4))
        v = filled.max(dim=-1)
        tv = qmask[s:s + chunk][:, None, :]
        sims.append(torch.where(tv, v.values, torch.zeros_like(v.values)))
        patches.append(torch.where(tv, v.indices, torch.full_like(v.indices, -1)).to(torch.int32))
        if heat:
            col = torch.where(tv[..., None], dots, torch.full_like(dots, float("-inf"))).max(dim=2).values
            heats.append(torch.where(pm, col, torch.full_like(col, float("-inf"))))
    out = (torch.cat(sims), torch.cat(patches))
    return out + (torch.cat(heats),) if heat else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pages", type=int, default=8192)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--small", action="store_true", help="a rehearsal size (64 queries, 256 pages x 225): overheads only, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    nq, lq, n, lp, k = (64, 32, 256, 225, 10) if args.small else (1024, 32, args.pages, 1030, 10)
    reps = max(args.reps, 5)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    P = F.normalize(torch.randn((n, lp, D), generator=gen, device=dev), dim=-1).bfloat16()
    pmask = torch.arange(lp, device=dev)[None, :] < torch.randint(lp // 2, lp + 1, (n, 1), generator=gen, device=dev)
    Q = F.normalize(torch.randn((nq, lq, D), generator=gen, device=dev), dim=-1).bfloat16()
    qmask = torch.arange(lq, device=dev)[None, :] < torch.randint(lq // 2, lq + 1, (nq, 1), generator=gen, device=dev)
    corpus = PageCorpus.from_tensor(P, pmask)
    cand = corpus.topk(Q, qmask, k)[1].contiguous()

    forms = {"align": lambda: corpus.align(Q, qmask, cand),
             "align_heat": lambda: corpus.align(Q, qmask, cand, heat=True),
             "hard_patches": lambda: corpus.hard_patches(Q, qmask, cand),
             "torch": lambda: torch_route(Q, qmask, P, pmask, cand, args.chunk, False),
             "torch_heat": lambda: torch_route(Q, qmask, P, pmask, cand, args.chunk, True)}
    for f in forms.values():
        timed(f)
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, f in forms.items():
            ms[name].append(timed(f)[1])
    res = {name: summary(v) for name, v in ms.items()}

    sim, patch, heat = corpus.align(Q, qmask, cand, heat=True)
    tsim, tpatch, theat = torch_route(Q, qmask, P, pmask, cand, args.chunk, True)
    valid = tpatch >= 0
    differ = (patch != tpatch) & valid
    fin = torch.isfinite(theat)
    page_bytes = nq * k * lp * D * 2
    res.update({"device": torch.cuda.get_device_name(0), "reps": reps, "small": args.small, "queries": nq, "lq": lq, "pages": n, "lp": lp,
                "k": k, "torch_chunk_queries": args.chunk, "listed_page_bytes": page_bytes,
                "align_bytes_per_s": page_bytes / (res["align"]["mean_ms"] * 1e-3),
                "torch_over_align": res["torch"]["mean_ms"] / res["align"]["mean_ms"],
                "torch_heat_over_align_heat": res["torch_heat"]["mean_ms"] / res["align_heat"]["mean_ms"],
                "max_abs_sim_difference": float((sim - tsim)[valid].abs().max()),
                "max_abs_heat_difference": float((heat - theat)[fin].abs().max()),
                "tokens": int(valid.sum()), "tokens_with_another_patch": int(differ.sum())})
    for name in forms:
        print(name, json.dumps(res[name]), flush=True)
    print(json.dumps({a: b for a, b in res.items() if not isinstance(b, dict)}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
