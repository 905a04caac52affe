"""Seeded inputs of the pairwise ranking-loss tests (tests/test_pair_losses_host.py, tests/test_gpu_pair_losses.py) and the torch
pre-processing of lambda_loss (criterion.py:94-98) that sits in front of the LambdaLoss pair rule."""
import torch

FILL = -1e4          # what the reference's scorer writes for a masked page

KINDS = ("normal", "fill", "wide", "same", "constant")


def scores(kind: str, b: int, n: int, seed: int = 0):
    """(score_s, score_t), (b, n) fp32 on the CPU.
    normal:   s, t ~ N(10, 4^2), independent.
    fill:     `normal` with -1e4 in one column of s, another column of t and one column of both (two fill values meet in a pair);
              fewer columns where n < 3.
    wide:     s = 60 randn: margins beyond +-200.
    same:     s == t.
    constant: every row constant (s and t each)."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * b + n)
    s = torch.randn(b, n, generator=gen) * 4.0 + 10.0
    t = torch.randn(b, n, generator=gen) * 4.0 + 10.0
    if kind == "fill":
        cols = torch.randperm(n, generator=gen)[:3].tolist()
        s[:, cols[0]] = FILL
        t[:, cols[0]] = FILL
        if len(cols) > 1:
            s[:, cols[1]] = FILL
        if len(cols) > 2:
            t[:, cols[2]] = FILL
    elif kind == "wide":
        s = torch.randn(b, n, generator=gen) * 60.0
    elif kind == "same":
        s = t.clone()
    elif kind == "constant":
        s = s[:, :1].expand(b, n).contiguous()
        t = t[:, :1].expand(b, n).contiguous()
    elif kind != "normal":
        raise ValueError(kind)
    return s.contiguous(), t.contiguous()


def lambda_inputs(s: torch.Tensor, t: torch.Tensor):
    """(s_sorted, gain, disc, order) as lambda_loss forms them in fp32 on the tensors' device."""
    n = s.shape[1]
    t_sorted, order = t.sort(dim=1, descending=True)
    s_sorted = s.gather(1, order)
    disc = 1.0 / torch.log2(torch.arange(1, n + 1, device=s.device, dtype=torch.float) + 1.0)
    gain = torch.sigmoid(t_sorted)
    return s_sorted.contiguous(), gain.contiguous(), disc, order
