"""Cost of the mapped top-k (the ranking step of every rerank and shard merge): ops.topk(scores, 100, idx_map=m) with a shuffled map at
(1024, 512) and (1024, 800) with continuous random scores -- no tie at the cut, the common case -- and, for information, rows of 4096
equal scores, where the tie straddles the cut and topk_kernel runs its second select over the reported indices.  HIP events around each
call, warm-up, median of 50 launches, three repeats.  To compare two builds run it once per build, alternating, on one machine:
    python scratch/topk_mapped_bench.py --label change --out a.json
    python scratch/topk_mapped_bench.py --lib <path to another libevdr.so> --label parent --out b.json
profiles/topk_mapped_ties.json holds the figures of the change that added the second select."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import evdr_amd  # noqa: F401
from evdr_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of libevdr.so to time (default: the package's)")
ap.add_argument("--label", default="this build")
ap.add_argument("--out", default=None)
ap.add_argument("--launches", type=int, default=50)
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
dev = torch.device("cuda:0")
gen = torch.Generator().manual_seed(0)
rng = np.random.default_rng(0)


def case(nq, n, tied):
    sc = torch.full((nq, n), 0.5) if tied else torch.randn(nq, n, generator=gen)
    m = rng.permuted(np.tile(np.arange(n) + 1000, (nq, 1)), axis=1).astype(np.int32)
    return sc.to(dev), torch.from_numpy(m).to(dev)


def median_us(sc, m, launches, warm=10):
    for _ in range(warm):
        ops.topk(sc, 100, idx_map=m)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        ops.topk(sc, 100, idx_map=m)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)


out = {"label": args.label, "launches_per_median": args.launches, "unit": "us", "cases": {}}
cases = {"1024x512_random": case(1024, 512, False), "1024x800_random": case(1024, 800, False),
         "1x4096_all_equal": case(1, 4096, True), "1024x4096_all_equal": case(1024, 4096, True)}
for rep in range(3):                       # three repeats, the shapes interleaved
    for name, (sc, m) in cases.items():
        out["cases"].setdefault(name, []).append(round(median_us(sc, m, args.launches), 2))
_, ti = ops.topk(cases["1024x800_random"][0], 100, idx_map=cases["1024x800_random"][1])
out["checksum_1024x800"] = int(ti.long().sum().item())
print(json.dumps(out), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f)
