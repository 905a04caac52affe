"""Seeded inputs shared by tests/test_cluster_host.py and tests/test_gpu_cluster.py: structured pages whose patches
are noisy copies of K prototypes in shuffled order, and the masks the clustering cases use."""
import functools

import torch
import torch.nn.functional as F


def structured_pages(n: int, lp: int, d: int, K: int, sigma: float, seed: int):
    """(P (n, lp, d) fp32 unit rows, z (n, lp) the prototype of every patch): proto = l2norm(randn(n, K, d)), z = randint(K, (n, lp)),
    P = l2norm(proto[z] + sigma * randn(n, lp, d) / sqrt(d))."""
    gen = torch.Generator().manual_seed(seed)
    proto = F.normalize(torch.randn((n, K, d), generator=gen), dim=-1)
    z = torch.randint(K, (n, lp), generator=gen)
    noise = torch.randn((n, lp, d), generator=gen)
    P = F.normalize(proto.gather(1, z[:, :, None].expand(-1, -1, d)) + sigma * noise / d ** 0.5, dim=-1)
    return P, z


def case_mask(n: int, lp: int, seed: int) -> torch.Tensor:
    """A random 80 % mask; page 0 fully masked, page 1 with two valid patches."""
    gen = torch.Generator().manual_seed(seed + 7)
    pm = torch.rand((n, lp), generator=gen) < 0.8
    pm[0] = False
    pm[1] = False
    pm[1, lp // 3] = True
    pm[1, lp - 1] = True
    return pm


@functools.lru_cache(maxsize=None)
def case(lp: int, ls: int, d: int, dtype: torch.dtype, n: int):
    """(P of `dtype`, pmask) on the CPU, never modified: structured pages with K = ls, sigma = 0.5."""
    P, _ = structured_pages(n, lp, d, ls, 0.5, 100000 * lp + 100 * ls + d)
    return P.to(dtype), case_mask(n, lp, lp + ls)


@functools.lru_cache(maxsize=None)
def reference(lp: int, ls: int, d: int, dtype: torch.dtype, n: int, iters: int):
    """ops.cluster_reference on the CPU with the labels after every iteration: computed once per case, shared, never modified."""
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    P, pm = case(lp, ls, d, dtype, n)
    history = []
    out = ops.cluster_reference(P, pm, ls, iters, history)
    return out, history


def changes(history) -> list:
    """Labels that changed in every iteration of a reference run."""
    return [int((a != b).sum()) for a, b in zip(history[:-1], history[1:])]


@functools.lru_cache(maxsize=None)
def two_stage_case():
    """(P (64, 96, 128) fp32, pmask, Q (64, 8, 128) fp32) on the CPU, never modified: structured pages with K = 12, sigma = 0.3, the
    first 90 patches valid (page 3: the first 40); query q holds noisy copies (0.5 * randn / sqrt(d), renormalised) of eight of the
    patches 0..39 of page q."""
    n, lp, d = 64, 96, 128
    P, _ = structured_pages(n, lp, d, 12, 0.3, 2024)
    pm = torch.zeros((n, lp), dtype=torch.bool)
    pm[:, :90] = True
    pm[3, 40:] = False
    gen = torch.Generator().manual_seed(2025)
    pick = torch.stack([torch.randperm(40, generator=gen)[:8] for _ in range(n)])
    Q = P.gather(1, pick[:, :, None].expand(-1, -1, d)) + 0.5 * torch.randn((n, 8, d), generator=gen) / d ** 0.5
    return P, pm, F.normalize(Q, dim=-1)
