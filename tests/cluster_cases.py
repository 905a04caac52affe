"""Seeded inputs shared by tests/test_cluster_host.py and tests/test_gpu_cluster.py: structured pages whose patches
are noisy copies of K prototypes in shuffled order, the masks the clustering cases use, and the generated cases (near ties, the
rule's edges, geometry) with their CPU references, each built once and shared."""
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


# ---- cases built by a generator: (P, pmask or None, ls) ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built(builder, *args):
    """builder(*args) = (P, pmask or None, ls) on the CPU, built once per argument tuple, shared, never modified."""
    return builder(*args)


@functools.lru_cache(maxsize=None)
def built_reference(builder, args: tuple, iters: int):
    """(ops.cluster_reference's (members, offsets, labels), the labels after the start and after every iteration) of built(builder,
    *args): computed once on the CPU, shared, never modified."""
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    P, pm, ls = built(builder, *args)
    history = []
    out = ops.cluster_reference(P, pm, ls, iters, history)
    return out, history


def near_tie_pages(n: int, lp: int, d: int, eps: float, seed: int, dtype: torch.dtype) -> torch.Tensor:
    """(n, lp, d) pages of `dtype` whose patches are all within a few ulps of one unit row per page, so that the scores of a patch
    against the centroids differ in the last bits only and the summation order, a fused multiply-add or a centroid off by an ulp
    moves labels.  fp32: base + eps * randn with base = l2norm(randn(n, 1, d)).  bf16 / fp16: base.to(dtype) with every element moved,
    with probability eps, to the representable value next to it on a random side (moving all 128 columns of a bf16 row by an ulp
    spreads the scores over 1e-3 and leaves too few of them within an fp32 ulp of each other)."""
    gen = torch.Generator().manual_seed(seed)
    base = F.normalize(torch.randn((n, 1, d), generator=gen), dim=-1)
    if dtype is torch.float32:
        return base + eps * torch.randn((n, lp, d), generator=gen)
    move = (torch.rand((n, lp, d), generator=gen) < eps).to(torch.int16)
    side = torch.randint(0, 2, (n, lp, d), generator=gen, dtype=torch.int16) * 2 - 1
    bits = base.to(dtype).expand(n, lp, d).contiguous().view(torch.int16)
    return (bits + move * side).view(dtype)                           # sign-magnitude formats: +1 on the pattern is one ulp away from zero


def near_tie_case(lp: int, ls: int, d: int, dtype: torch.dtype, n: int, masked: bool):
    """Near-tie pages (eps = 1e-6 for fp32, 1 / 16 for bf16 / fp16; seed 5), unmasked or under a plain random 80 % mask."""
    P = near_tie_pages(n, lp, d, 1e-6 if dtype is torch.float32 else 1 / 16, 5, dtype)
    pm = (torch.rand((n, lp), generator=torch.Generator().manual_seed(lp + ls)) < 0.8) if masked else None
    return P, pm, ls


# (lp_src, ls, d, dtype, n, masked): the near-tie table; 700 / 313 keeps its centroids in the workspace
NEAR_TIE = ((64, 8, 128, torch.float32, 4, False), (300, 40, 100, torch.float32, 4, True), (700, 313, 32, torch.float32, 2, False),
            (64, 8, 128, torch.bfloat16, 4, False), (64, 8, 128, torch.float16, 4, False))
NEAR_TIE_ITERS = 4


# ---- the rule's edges ------------------------------------------------------------------------------------------------------------------
def tie_page():
    """Windows {p0, p1} and {p2, p3} of (1, 1, 1, -0.5) * e0 both have the centroid e0."""
    P = torch.zeros(1, 4, 8)
    P[0, :, 0] = torch.tensor([1.0, 1.0, 1.0, -0.5])
    return P, None, 2


def signed_zero_page():
    """Centroids ~ (e0 + e1) and (e2 - e0): p1 . c1 = -0.0 and p2 . c0 = +0.0 beside positive scores."""
    P = torch.zeros(1, 4, 8)
    P[0, 0, 0], P[0, 1, 1], P[0, 2, 2], P[0, 3, 0] = 1.0, 1.0, 1.0, -1.0
    return P, None, 2


def nan_patch_page():
    """Six structured patches in three groups; patch 4 holds one NaN and starts in group 2, whose centroid becomes NaN."""
    P, _ = structured_pages(1, 6, 16, 3, 0.3, 4)
    P[0, 4, 5] = float("nan")
    return P, None, 3


def all_nan_page():
    return torch.full((1, 5, 8), float("nan")), None, 2


def inf_page(dtype: torch.dtype):
    """Structured (2, 33, 64) pages, nine groups; page 0 holds +inf in patch 5 and -inf in patch 20 of column 3, page 1 both in patch 7
    (columns 3 and 40)."""
    P, _ = structured_pages(2, 33, 64, 9, 0.5, 77)
    P = P.to(dtype)
    P[0, 5, 3], P[0, 20, 3] = float("inf"), float("-inf")
    P[1, 7, 3], P[1, 7, 40] = float("inf"), float("-inf")
    return P, None, 9


def exact_row(d: int, seed: int) -> torch.Tensor:
    """A (d,) row of non-zero multiples of 1/8 in [-3/8, 3/8]: sums of up to 2**20 copies and their mean are exact in fp32."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.randint(1, 4, (d,), generator=gen) * (2 * torch.randint(0, 2, (d,), generator=gen) - 1)
    return k.float() / 8


def identical_page(lp: int, ls: int, d: int):
    """lp copies of one exact_row: every window's mean is that row exactly, every centroid the same bits, every patch tied."""
    return exact_row(d, lp + d).expand(1, lp, d).contiguous(), None, ls


def alternating_page(lp: int, ls: int, d: int):
    """Two distinct exact_rows repeated alternately."""
    rows = torch.stack([exact_row(d, 1), exact_row(d, 2)])
    return rows[torch.arange(lp) % 2][None].contiguous(), None, ls


def scaled_case(lp: int, ls: int, d: int, dtype: torch.dtype, scale: float):
    """Structured pages times `scale` (4 pages, the random mask of case_mask): 1e-25 in fp32 makes every square zero or denormal so that
    the + 1e-12 is the whole denominator; 1e25 in fp32 overflows the sum of squares; 3e4 in fp16 sits under the format's maximum."""
    P, _ = structured_pages(4, lp, d, ls, 0.5, 31 * lp + d)
    return (P * scale).to(dtype), case_mask(4, lp, lp), ls


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
BOUNDARY_NV = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 520)


def boundary_case(scattered: bool):
    """(11, 520, 64) structured pages, ls = 12, page i with BOUNDARY_NV[i] valid patches: the first nv, or nv scattered at random."""
    lp = 520
    P, _ = structured_pages(len(BOUNDARY_NV), lp, 64, 12, 0.5, 520)
    pm = torch.zeros((len(BOUNDARY_NV), lp), dtype=torch.bool)
    gen = torch.Generator().manual_seed(521)
    for i, nv in enumerate(BOUNDARY_NV):
        pm[i, torch.randperm(lp, generator=gen)[:nv] if scattered else torch.arange(nv)] = True
    return P, pm, 12


def plain_case(lp: int, ls: int, d: int, n: int, masked: bool, dtype: torch.dtype = torch.float32):
    """Structured pages of `dtype` with min(ls, lp, 16) prototypes; masked: the random mask of case_mask."""
    P, _ = structured_pages(n, lp, d, max(1, min(ls, lp, 16)), 0.5, 1000 * lp + 10 * ls + d)
    return P.to(dtype), case_mask(n, lp, lp + d) if masked else None, ls


def grid_walk_case():
    """1030 pages (33, 64), ls = 9: three rounds over the launch's 512 workgroups.  Page i has nv = (0, 1, 2, all, random)[i % 5] valid
    patches at random positions; every page with i % 7 == 0 is lp copies of one exact_row of its own, every page with i % 7 == 3 the
    same with its last valid patch negated (it scores -|v| against this page's centroids, about 0 against any other page's)."""
    n, lp, d = 1030, 33, 64
    P, _ = structured_pages(n, lp, d, 9, 0.5, 1030)
    gen = torch.Generator().manual_seed(1031)
    pm = torch.zeros((n, lp), dtype=torch.bool)
    for i in range(n):
        nv = (0, 1, 2, lp, int(torch.randint(3, lp, (1,), generator=gen)))[i % 5]
        pm[i, torch.randperm(lp, generator=gen)[:nv]] = True
        if i % 7 in (0, 3):
            P[i] = exact_row(d, 5000 + i)
            if i % 7 == 3 and nv:
                P[i, int(pm[i].nonzero().max())] *= -1.0
    return P, pm, 9
