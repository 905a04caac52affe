"""Growable corpus: time of preparing 4096 pages x 1030 x 128 by chunked `append` (256 pages per launch) against
`PageCorpus.from_tensor` of the same pages, ONE process, alternating runs, per corpus kind; and the peak device memory of
`corpus_from_payload` at fp32, default path against chunk_pages=256.

`from_tensor`'s default path is the parent commit's code, untouched by the feature, so the comparison against the parent is made
inside one process on one box.  Times are HIP-event times around the whole preparation (allocation of the corpus included on both
sides; the fp32 append's status read-back included), median / min / max of >= 5 runs after one warm-up of each form.  Bytes are
counted from shapes: what the fused path must move (one read of source and mask, one write of planes and words) over its time.

    python scratch/ingest_bench.py --out profiles/ingest.json [--reps 5] [--small]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import evdr_amd  # noqa: E402,F401
from evdr_amd import ops  # noqa: E402
from evdr_amd.corpus import PageCorpus  # noqa: E402
from evdr_amd.utils.preprocess_data import corpus_from_payload  # noqa: E402

D, SEED = 128, 11


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


def kind_case(kind, n, lp, chunk, reps, dev):
    gen = torch.Generator(device=dev).manual_seed(SEED)
    P = F.normalize(torch.randn((n, lp, D), generator=gen, device=dev), dim=-1)
    pm = torch.arange(lp, device=dev)[None, :] < torch.randint(lp // 2, lp + 1, (n, 1), generator=gen, device=dev)
    if kind == "bf16":
        P = P.bfloat16()
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp8": ops.FP8}[kind]
    absmax = float(P.abs().max()) if kind == "fp32" else None          # the data's own binade: the planes must equal from_tensor's

    def chunked():
        c = PageCorpus.empty(n, lp, dt, dev, absmax=absmax)
        for s in range(0, n, chunk):
            c.append(P[s:s + chunk], pm[s:s + chunk])
        return c

    one_launch = lambda: PageCorpus.from_tensor(P, pm, dtype=dt if kind == "fp8" else None, capacity=n)      # noqa: E731
    whole = lambda: PageCorpus.from_tensor(P, pm, dtype=dt if kind == "fp8" else None)                      # noqa: E731
    forms = {"append_chunks": chunked, "from_tensor_capacity": one_launch, "from_tensor": whole}
    for f in forms.values():
        timed(f)
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            ms[k].append(timed(f)[1])
    a, b = chunked(), whole()
    same = bool(torch.equal(a.planes.view(torch.uint8), b.planes.view(torch.uint8)) and torch.equal(a.tilemask, b.tilemask)
                and torch.equal(a.pageflags, b.pageflags))
    src_b = P.numel() * P.element_size() + pm.numel()
    out_b = a.planes.numel() * a.planes.element_size() + a.tilemask.numel() * 4 + a.pageflags.numel() * 4
    res = {k: summary(v) for k, v in ms.items()}
    res.update({"pages": n, "lp": lp, "chunk_pages": chunk, "same_bits_as_from_tensor": same, "fused_bytes": src_b + out_b,
                "append_chunks_bytes_per_s": (src_b + out_b) / (res["append_chunks"]["median_ms"] * 1e-3),
                "append_over_from_tensor": res["append_chunks"]["median_ms"] / res["from_tensor"]["median_ms"]})
    return res


def payload_memory(n, lp, chunk, dev):
    rng = np.random.default_rng(SEED)
    docs = np.empty(n, dtype=object)
    for i in range(n):
        docs[i] = rng.standard_normal((lp - (i % 7), D)).astype(np.float32)
    out = {}
    for name, kw in (("default", {}), ("chunked", {"chunk_pages": chunk})):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        c, pm = corpus_from_payload(docs, None, None, dev, dtype=torch.float32, **kw)
        torch.cuda.synchronize()
        out[name + "_peak_bytes"] = torch.cuda.max_memory_allocated() - base
        out["resident_bytes"] = c.planes.numel() * 2 + c.tilemask.numel() * 4 + c.pageflags.numel() * 4
        del c, pm
    out.update({"pages": n, "lp": lp, "chunk_pages": chunk, "chunked_over_default": out["chunked_peak_bytes"] / out["default_peak_bytes"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a rehearsal size (64 pages x 225): overheads only, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    n, lp, chunk, n_mem = (64, 225, 16, 48) if args.small else (4096, 1030, 256, 1024)
    res = {"device": torch.cuda.get_device_name(0), "reps": max(args.reps, 5), "small": args.small, "kinds": {}}
    for kind in ("bf16", "fp32", "fp8"):
        res["kinds"][kind] = kind_case(kind, n, lp, chunk, max(args.reps, 5), dev)
        print(kind, json.dumps({k: v for k, v in res["kinds"][kind].items() if not isinstance(v, dict)}), flush=True)
        for k in ("append_chunks", "from_tensor_capacity", "from_tensor"):
            print("   ", k, json.dumps(res["kinds"][kind][k]), flush=True)
    res["payload_fp32_memory"] = payload_memory(n_mem, lp, chunk, dev)
    print("payload", json.dumps(res["payload_fp32_memory"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
