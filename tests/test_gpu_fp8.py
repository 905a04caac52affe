"""fp8 (e4m3fn) corpora on the GPU: quantiser bytes against torch's own conversion, the MFMA lane maps on exact integers, parity with
an fp64 masked MaxSim of the dequantised operands, the non-finite rules, launch-to-launch stability, shard / merge layout, planted
retrieval at 64 x 20 000 x 1030 and the refusals (include/evdr.h "fp8 corpora").  The oracle lives here."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
DEV = "cuda"


def ref_shift(x: torch.Tensor) -> int:
    """k of the contract: the largest integer with amax * 2^k <= 448, amax over the finite elements (0 -> k = 0)."""
    a = x.float().abs()
    a = a[torch.isfinite(a)]
    amax = float(a.max()) if a.numel() else 0.0
    if amax == 0.0:
        return 0
    m, e = math.frexp(amax)                       # amax = m 2^e, m in [0.5, 1)
    return 9 - e if m <= 0.875 else 8 - e


def ref_bytes(x: torch.Tensor, k: int) -> torch.Tensor:
    y = (x.float() * 2.0 ** k).to(FP8).view(torch.uint8)
    return torch.nn.functional.pad(y, (0, 128 - x.shape[-1]))


def dequant(x8: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """(groups, rows, 128) bytes + (groups,) shifts -> fp64 values."""
    return x8.double() * torch.pow(2.0, -shift.double()).view(-1, *([1] * (x8.dim() - 1)))


def oracle(Q: torch.Tensor, P: torch.Tensor, qmask=None, pmask=None, chunk: int = 64) -> torch.Tensor:
    """The reference's masked MaxSim (evaluator/retrieval.py:166-213) in fp64: masked patches -1e4 before the max, masked tokens add
    0, an all-masked page scores 0."""
    nq, lq, _ = Q.shape
    npg, lp, _ = P.shape
    qm = torch.ones(nq, lq, dtype=torch.bool, device=Q.device) if qmask is None else qmask.bool()
    pm = torch.ones(npg, lp, dtype=torch.bool, device=Q.device) if pmask is None else pmask.bool()
    out = torch.empty(nq, npg, dtype=torch.float64, device=Q.device)
    for p0 in range(0, npg, chunk):
        Pc, pmc = P[p0:p0 + chunk], pm[p0:p0 + chunk]
        s = torch.einsum("qnd,pmd->qpnm", Q, Pc)
        s = s.masked_fill(~pmc[None, :, None, :], -1e4)
        mx = s.max(-1).values * qm[:, None, :]
        out[:, p0:p0 + chunk] = mx.sum(-1) * pmc.any(-1)[None, :]
    return out


def unit(*shape, gen):
    return torch.nn.functional.normalize(torch.randn(*shape, generator=gen, device=DEV), dim=-1)


# ---- 1. quantiser bytes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [64, 100, 128])
def test_quantiser_bytes_equal_torch(dtype, d):
    from evdr_amd import ops
    g = torch.Generator(device=DEV).manual_seed(11 + d)
    groups, rows = 24, 9
    x = torch.randn(groups, rows, d, generator=g, device=DEV)
    mags = torch.logspace(-15, 15, groups, device=DEV, dtype=torch.float64).float()
    x = x * mags[:, None, None]
    x[3] = 0.0                                                             # an all-zero group
    # RNE midpoints of e4m3 (between 1.0 and 1.125: 1.0625; 1.125 and 1.25: 1.1875) and e4m3 subnormals, scaled so amax = 448
    mid = torch.tensor([448.0, 1.0625, 1.1875, -1.0625, 2.0 ** -7 * 1.5, 2.0 ** -8, 3 * 2.0 ** -10, -2.0 ** -9 * 0.5], device=DEV)
    x[4].zero_()
    x[4, 0, :mid.numel()] = mid
    x[5].zero_()
    x[5, 1, :4] = torch.tensor([1e-3, 2.0 ** -10, 7.0, -6.5], device=DEV)   # amax 7 -> k = 6: subnormal range of the small ones
    x[6, 2, 5] = float("nan")                                               # non-finite elements never move amax
    x[6, 0, 1] = float("inf")
    x[7, 3, 0] = float("-inf")
    x[8] = float("nan")                                                     # a group with no finite element: k = 0
    x = x.to(dtype)
    x8, shift = ops.quantize_fp8(x, rows)
    assert x8.dtype == FP8 and tuple(x8.shape) == (groups, rows, 128) and tuple(shift.shape) == (groups,)
    for gi in range(groups):
        k = ref_shift(x[gi])
        assert int(shift[gi]) == k, (gi, int(shift[gi]), k)
        assert torch.equal(x8[gi].view(torch.uint8), ref_bytes(x[gi], k)), gi
    assert int(shift[3]) == 0 and int(shift[8]) == 0


def test_query_bytes_and_scores_do_not_depend_on_the_batch():
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    g = torch.Generator(device=DEV).manual_seed(5)
    P = unit(40, 77, 128, gen=g)
    Q = unit(9, 20, 128, gen=g)
    Q[4] *= 1e3                                                            # a query of another magnitude in the batch
    c = PageCorpus.from_tensor(P, dtype=FP8)
    x8, sh = ops.quantize_fp8(Q, 20)
    full = c.score(Q)
    for i in (0, 4, 8):
        a8, ash = ops.quantize_fp8(Q[i:i + 1], 20)
        assert torch.equal(a8.view(torch.uint8), x8[i:i + 1].view(torch.uint8)) and int(ash[0]) == int(sh[i])
        assert torch.equal(c.score(Q[i:i + 1]), full[i:i + 1])


# ---- 2. lane maps on exact integers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,lq,npg,lp", [(3, 32, 5, 64), (17, 19, 9, 1030), (300, 32, 11, 300), (2, 5, 7, 41)])
def test_lane_maps_exact_integers(nq, lq, npg, lp):
    from evdr_amd.corpus import PageCorpus
    g = torch.Generator(device=DEV).manual_seed(nq * 7 + lp)
    P = torch.randint(-8, 9, (npg, lp, 128), generator=g, device=DEV).float()
    P[:, :, 0] = 8.0                                                       # every page's amax is 8: k = 5, all values exact in e4m3
    Q = torch.randint(-8, 9, (nq, lq, 128), generator=g, device=DEV).float()
    Q[:, :, 1] = 8.0
    Q[:, 0, 2] = -8.0
    c = PageCorpus.from_tensor(P, dtype=FP8)
    assert torch.all(c.shift == 5)
    s = c.score(Q)
    ref = oracle(Q.double(), P.double())
    assert torch.equal(s.double(), ref), (s.double() - ref).abs().max()


# ---- 3. parity --------------------------------------------------------------------------------------------------------------
def _ragged(npg, lp, g, frac=0.3):
    pm = torch.rand(npg, lp, generator=g, device=DEV) > frac
    lens = torch.randint(1, lp + 1, (npg,), generator=g, device=DEV)
    pm[: npg // 2] = torch.arange(lp, device=DEV)[None, :] < lens[: npg // 2, None]     # ragged prefixes
    return pm


@pytest.mark.parametrize("nq,lq,npg,lp,masks", [
    (64, 32, 37, 1030, "none"), (5, 7, 101, 1030, "ragged"), (17, 33, 23, 41, "ragged"), (3, 64, 3, 4000, "ragged"),
    (1, 1, 257, 41, "none"), (0, 8, 5, 41, "none"), (3, 32, 0, 41, "none"), (64, 32, 1, 1030, "allmasked"),
    (5, 32, 2, 65500, "none"), (17, 7, 300, 100, "ragged"),
])
def test_parity_with_the_dequantised_oracle(nq, lq, npg, lp, masks):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    g = torch.Generator(device=DEV).manual_seed(nq + 3 * lq + npg + lp)
    P = unit(npg, lp, 128, gen=g)
    Q = unit(nq, lq, 128, gen=g)
    pmask = qmask = None
    if masks == "ragged":
        pmask = _ragged(npg, lp, g)
        if npg > 2:
            pmask[1] = False                                               # an all-masked page
        qmask = torch.rand(nq, lq, generator=g, device=DEV) > 0.3
        if nq > 1:
            qmask[0] = False                                               # an all-masked query
    elif masks == "allmasked":
        pmask = torch.zeros(npg, lp, dtype=torch.bool, device=DEV)
    if npg == 0:                                                           # an empty shard of a corpus
        c = PageCorpus.from_tensor(unit(3, lp, 128, gen=g), dtype=FP8).shard(3, 3)
    else:
        c = PageCorpus.from_tensor(P, pmask, dtype=FP8)
    assert c.planes.dtype == FP8 and c.planes.numel() == npg * lp * 128      # one byte per element
    s = c.score(Q, qmask)
    assert tuple(s.shape) == (nq, npg)
    if nq == 0 or npg == 0:
        return
    q8, qs = ops.quantize_fp8(Q, lq)
    ref = oracle(dequant(q8.float(), qs), dequant(c.planes[0].float(), c.shift), qmask, pmask)
    err = (s.double() - ref).abs().max().item()
    assert err <= 1e-4 * max(1.0, lq / 32), err
    if masks == "allmasked":
        assert torch.all(s == 0)
    if npg >= 10 and nq > 0:
        k = min(10, npg)
        ts, ti = c.topk(Q, qmask, k)
        rs, ri = torch.sort(ref, dim=1, descending=True, stable=True)
        ext = torch.cat([torch.full_like(rs[:, :1], float("inf")), rs, torch.full_like(rs[:, :1], float("-inf"))], 1)
        clear = ((ext[:, 0:k] - ext[:, 1:k + 1]) > 2e-4) & ((ext[:, 1:k + 1] - ext[:, 2:k + 2]) > 2e-4)   # rank i clear of both neighbours
        assert torch.equal(ti.long()[clear], ri[:, :k][clear])


# ---- 4. non-finite rules ----------------------------------------------------------------------------------------------------
def test_non_finite_rules():
    from evdr_amd.corpus import PageCorpus
    g = torch.Generator(device=DEV).manual_seed(9)
    npg, lp, nq, lq = 6, 77, 4, 12
    P = unit(npg, lp, 128, gen=g)
    Q = unit(nq, lq, 128, gen=g)
    pmask = torch.ones(npg, lp, dtype=torch.bool, device=DEV)
    pmask[2, 40:] = False
    pmask[5] = False                                                       # all-masked page
    qmask = torch.ones(nq, lq, dtype=torch.bool, device=DEV)
    qmask[1, 8:] = False
    clean = PageCorpus.from_tensor(P, pmask, dtype=FP8).score(Q, qmask)
    P2 = P.clone()
    P2[0, 3, 7] = float("nan")                                             # valid patch -> NaN column
    P2[1, 10, 0] = float("inf")
    P2[2, 50, 1] = float("nan")                                            # masked patch -> nothing changes
    P2[2, 60, 2] = float("-inf")
    s = PageCorpus.from_tensor(P2, pmask, dtype=FP8).score(Q, qmask)
    assert torch.isnan(s[:, 0]).all() and torch.isnan(s[:, 1]).all()
    assert torch.equal(s[:, 2:], clean[:, 2:])
    Q2 = Q.clone()
    Q2[1, 10, 3] = float("nan")                                            # masked token of query 1 -> NaN row where a patch is valid
    c = PageCorpus.from_tensor(P, pmask, dtype=FP8)
    s = c.score(Q2, qmask)
    assert torch.isnan(s[1, :5]).all() and s[1, 5].item() == 0.0
    assert torch.equal(s[[0, 2, 3]], c.score(Q, qmask)[[0, 2, 3]])


# ---- 5. stability and layout ------------------------------------------------------------------------------------------------
def test_stability_shards_merge_and_out_col():
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, merge_candidates, ShardedRetriever
    g = torch.Generator(device=DEV).manual_seed(21)
    npg, lp, nq, lq = 333, 1030, 40, 32
    P = unit(npg, lp, 128, gen=g).bfloat16()
    Q = unit(nq, lq, 128, gen=g)
    qmask = torch.rand(nq, lq, generator=g, device=DEV) > 0.2
    c = PageCorpus.from_tensor(P, dtype=FP8)
    assert c.planes.untyped_storage().nbytes() == npg * lp * 128
    a, b, d = c.score(Q, qmask), c.score(Q, qmask), c.score(Q, qmask)
    assert torch.equal(a, b) and torch.equal(a, d)
    lo, hi = c.shard(0, 150), c.shard(150, npg)
    assert torch.equal(lo.score(Q, qmask), a[:, :150]) and torch.equal(hi.score(Q, qmask), a[:, 150:])
    out = torch.full((nq, npg + 20), 12345.0, device=DEV)
    hi.score(Q, qmask, out=out, out_col=160)
    assert torch.equal(out[:, 160:160 + hi.n_pages], a[:, 150:])
    assert torch.all(out[:, :160] == 12345.0) and torch.all(out[:, 160 + hi.n_pages:] == 12345.0)
    k = 100
    ts, ti = c.topk(Q, qmask, k)
    s1, i1 = lo.topk(Q, qmask, k)
    s2, i2 = hi.topk(Q, qmask, k)
    ms, mi = merge_candidates(torch.cat([s1, s2], 1), torch.cat([i1, i2], 1), k)
    assert torch.equal(ms, ts) and torch.equal(mi, ti)
    r = ShardedRetriever(c).search(Q, qmask, k=k)
    assert torch.equal(r[0], ts) and torch.equal(r[1], ti)
    rt = ShardedRetriever(c).search(Q, qmask, k=k, with_ties=True)
    assert torch.equal(rt[0], ts) and torch.equal(rt[1], ti) and isinstance(rt[2], dict)
    # the constructor takes prepared fp8 planes with their shifts
    x8, sh = ops.quantize_fp8(P, lp)
    c2 = PageCorpus(x8[None], c.tilemask, c.pageflags, shift=sh)
    assert torch.equal(c2.score(Q, qmask), a)


# ---- 6. planted retrieval ---------------------------------------------------------------------------------------------------
def test_planted_queries_rank_first_at_20k_pages():
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    npg, lp, nq, lq = 20000, 1030, 64, 32
    planes, shifts = [], []
    g = torch.Generator(device=DEV)
    targets = (torch.arange(nq) * 7919) % npg
    gc = torch.Generator(device="cpu").manual_seed(4)
    rows = torch.stack([torch.randperm(lp, generator=gc)[:lq] for _ in range(nq)])
    eps = torch.nn.functional.normalize(torch.randn((nq, lq, 128), generator=gc), dim=-1).to(DEV)
    Q = torch.zeros(nq, lq, 128, device=DEV)
    for c0 in range(0, npg, 1000):
        g.manual_seed(1000 + c0)
        x = torch.nn.functional.normalize(torch.randn((1000, lp, 128), generator=g, device=DEV), dim=-1).bfloat16()
        x8, sh = ops.quantize_fp8(x, lp)
        planes.append(x8)
        shifts.append(sh)
        mine = ((targets >= c0) & (targets < c0 + 1000)).nonzero().flatten()
        for i in mine.tolist():
            Q[i] = torch.nn.functional.normalize(x[int(targets[i]) - c0, rows[i].to(DEV)].float() + 0.5 * eps[i], dim=-1)
        del x
    tilemask, pageflags = ops.pack_pmask(None, npg, lp, torch.device(DEV))
    c = PageCorpus(torch.cat(planes)[None], tilemask, pageflags, shift=torch.cat(shifts))
    del planes
    ts, ti = c.topk(Q, None, 100)
    assert torch.equal(ti[:, 0].cpu().long(), targets)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_on_an_fp8_corpus():
    from evdr_amd.corpus import PageCorpus, ShardedRetriever
    g = torch.Generator(device=DEV).manual_seed(2)
    c = PageCorpus.from_tensor(unit(20, 41, 128, gen=g), dtype=FP8)
    Q = unit(3, 8, 128, gen=g)
    with pytest.raises(ValueError, match="fp8"):
        c.topk(Q, None, 10, prefilter=True)
    with pytest.raises(ValueError, match="fp8"):
        ShardedRetriever(c).search(Q, None, k=10, prefilter=True)
    with pytest.raises(NotImplementedError, match="width"):
        c.score(unit(3, 8, 200, gen=g))
    with pytest.raises(NotImplementedError, match="width"):
        PageCorpus.from_tensor(unit(4, 41, 160, gen=g), dtype=FP8)
    # fp8 is never a default: a plain corpus of the same pages is not fp8
    assert PageCorpus.from_tensor(unit(4, 41, 128, gen=g)).planes.dtype != FP8
