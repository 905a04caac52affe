"""Fuzz of the device ranking against a numpy reference: evdr_topk's order (NaN first, score desc with -0 == +0, index asc), the
two-level path for few long rows, a shuffled idx_map, and ops.topk_with_ties (device and host forms) -- random shapes, k, quantised
scores with long tie runs, NaN / +-inf / -0.0.  The case generator, the reference (rank_rule) and the checks are those of
tests/test_gpu_ranking_ties.py, which runs the first seeds in the suite.   usage: python scratch/fuzz_topk.py <first_seed> <count>"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import evdr_amd  # noqa: F401
from test_gpu_ranking_ties import fuzz_case, check_fuzz_case
dev = "cuda:0"
s0, cnt = int(sys.argv[1]), int(sys.argv[2])
bad = 0
for seed in range(s0, s0 + cnt):
    sc, k, what = fuzz_case(seed)
    try:
        check_fuzz_case(sc, k, seed, dev, what)
    except AssertionError as e:
        bad += 1
        print(f"FAIL {what}: {str(e)[:300]}", flush=True)
    if (seed - s0) % 50 == 49:
        print(f"... {seed - s0 + 1} seeds, {bad} failures", flush=True)
print(f"done: {cnt} seeds, {bad} failures")
