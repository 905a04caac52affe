"""Host simulation (torch on the CPU, no GPU) of the fp8 first stage of TwoStageRetriever: which share of the exhaustive bf16 top-k lies
inside the fp8 top-R, and for which share of the queries it lies inside completely.

The fp8 contract of DESIGN.md §4.5: one power of two per page / per query, (x * 2**k).to(float8_e4m3fn), products exact, fp32 sums.
Unit-norm Gaussian pages and 32-token random queries (no structure: the hardest case).  Pages are generated 200 at a time from a
seed, so the run needs memory for the two (nq, n) score blocks only.

    python scratch/sim_two_stage.py [--nq 32] [--pages 100000] [--lp 1030]        (the default size takes minutes of CPU)
"""
import argparse

import torch
import torch.nn.functional as F


def quant(x):
    """(groups, rows, d) -> dequantised e4m3 values with one power of two per group (amax * 2^k <= 448)."""
    k = torch.floor(torch.log2(448.0 / x.abs().amax(dim=(1, 2), keepdim=True)))
    return (x * 2.0 ** k).to(torch.float8_e4m3fn).float() * 2.0 ** -k


def maxsim(Q, P):
    return torch.einsum("qtd,pjd->qptj", Q, P).amax(-1).sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--pages", type=int, default=100_000)
    ap.add_argument("--lp", type=int, default=1030)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(1)
    Q = F.normalize(torch.randn((a.nq, 32, 128), generator=g), dim=-1)
    Qb, Q8 = Q.bfloat16().float(), quant(Q)
    sb, s8 = torch.empty((a.nq, a.pages)), torch.empty((a.nq, a.pages))
    for lo in range(0, a.pages, 200):
        P = F.normalize(torch.randn((min(200, a.pages - lo), a.lp, 128), generator=torch.Generator().manual_seed(1000 + lo)), dim=-1)
        sb[:, lo:lo + 200] = maxsim(Qb, P.bfloat16().float())
        s8[:, lo:lo + 200] = maxsim(Q8, quant(P))
    d = (s8 - sb).abs()
    print(f"|s_fp8 - s_bf16|: max {d.max():.3f} mean {d.mean():.3f}")
    for k in (1, 10, 100):
        top = sb.topk(min(k, a.pages), dim=1).indices
        for r in (k, 32, 64, 128, 256, 512, 1024, 2048, 4096):
            if r < k or r > a.pages:
                continue
            inside = (top[:, :, None] == s8.topk(r, dim=1).indices[:, None, :]).any(-1)
            print(f"k={k:3d} R={r:4d}: share inside {inside.float().mean():.4f}, queries complete {inside.all(1).float().mean():.2f}")


if __name__ == "__main__":
    main()
