"""The fp8 page-list forward (PageCorpus.score_pages on an fp8 corpus, evdr_maxsim_fwd_fp8_pages) and the filtered two-stage search
(TwoStageRetriever.search(..., subset=)) on the GPU: list scores against the product's own exhaustive fp8 scores (equal bits, NaN at
equal places) and against the dequantised torch oracle, holes, the non-finite rules, `out` views, stability, and the search against
exact.topk(subset=).  Helpers are restated here: the file stands alone."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaN == NaN (the positions of NaN scores are part of the answer)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def unit(gen, dev, *shape):
    return F.normalize(torch.randn(*shape, generator=gen, device=dev), dim=-1)


def ragged(gen, n, l, lo, dev):
    lens = torch.randint(lo, l + 1, (n,), generator=gen, device=dev)
    return torch.arange(l, device=dev)[None, :] < lens[:, None]


def ragged_pages(gen, npg, lp, dev, frac=0.3):
    """tests/test_gpu_fp8.py's page masks: random holes, ragged prefixes on the first half of the pages."""
    pm = torch.rand(npg, lp, generator=gen, device=dev) > frac
    lens = torch.randint(1, lp + 1, (npg,), generator=gen, device=dev)
    pm[: npg // 2] = torch.arange(lp, device=dev)[None, :] < lens[: npg // 2, None]
    return pm


def make(gen, nq, lq, npg, lp, dev, planted=True):
    """tests/test_gpu_candidates.py's generator: unit rows, planted queries lie near one page (score ~ 28 against ~ 9)."""
    P = unit(gen, dev, npg, lp, 128)
    Q = unit(gen, dev, nq, lq, 128)
    t = None
    if planted and npg > 0:
        t = torch.randint(0, npg, (nq,), generator=gen, device=dev)
        rows = torch.randint(0, lp, (nq, lq), generator=gen, device=dev)
        Q = F.normalize(P[t[:, None], rows] + 0.5 * Q, dim=-1)
    return Q, P, t


def dequant(x8: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """(groups, rows, 128) bytes + (groups,) shifts -> fp64 values."""
    return x8.double() * torch.pow(2.0, -shift.double()).view(-1, *([1] * (x8.dim() - 1)))


def oracle(Q, P, qmask=None, pmask=None, chunk=64):
    """The reference's masked MaxSim in fp64: masked patches -1e4 before the max, masked tokens add 0, an all-masked page scores 0."""
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


def shuffled_list(gen, npg, m, dev, must=()):
    """(m,) int32 local page indices in random order, with duplicates (m > npg, or by chance), holding every page of `must`."""
    lst = torch.randint(0, npg, (m,), generator=gen, device=dev, dtype=torch.int32)
    for i, p in enumerate(must):
        lst[(3 * i + 1) % m] = p
    lst[m - 1] = lst[0]                                    # at least one duplicate
    return lst


def last_kernel():
    from evdr_amd import _lib
    return _lib.load().evdr_last_fwd_kernel().decode()


# the instance the exhaustive dispatch picks from (nq, tiles); the page-list form takes the same one
def instance(nq, lp):
    tiles = (lp + 31) // 32
    if tiles >= 8:
        return (8 if nq > 256 else 4 if nq > 8 else 1, 11, 3)
    return (4 if nq > 8 else 1, 2, 4)


# ---- 1. bits ----------------------------------------------------------------------------------------------------------------
# page lengths 7, 33, 224 (7 tiles: the short-page instances), 225 (8 tiles: the first long-page one), 353 (12 tiles = ST + 1: the
# stage with the extra tile) and 1030; nq on each side of the instance boundaries 8 | 9 and 256 | 257; lq 1, 7, 32 (one slice),
# 33, 64 (two slices through the qlist workspace); every case ragged in pages and queries, with an all-masked page in the list
@pytest.mark.parametrize("lp,npg,nq,lq", [
    (7, 300, 9, 7), (7, 41, 257, 32), (33, 257, 1, 1), (33, 90, 8, 64), (224, 120, 8, 32), (224, 64, 9, 33),
    (225, 90, 257, 33), (225, 77, 8, 1), (353, 60, 9, 64), (353, 64, 1, 33), (1030, 40, 257, 32), (1030, 47, 8, 7),
    (1030, 43, 9, 1),
])
def test_list_scores_are_the_exhaustive_bits(dev, lp, npg, nq, lq):
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(lp * 7 + npg + nq + lq)
    P, Q = unit(gen, dev, npg, lp, 128), unit(gen, dev, nq, lq, 128)
    pm = ragged_pages(gen, npg, lp, dev)
    pm[1] = False                                          # an all-masked page
    pm[2] = True                                           # a dense one
    qm = torch.rand(nq, lq, generator=gen, device=dev) > 0.3
    if nq > 1:
        qm[0] = False                                      # an all-masked query
        qm[1] = True
    c = PageCorpus.from_tensor(P, pm, dtype=FP8)
    S = c.score(Q, qm).clone()
    for m in (1, 2 * npg // 3, npg + npg // 3):
        lst = shuffled_list(gen, npg, m, dev, must=(1, 2, 0, npg - 1) if m >= 12 else (1,))
        got = c.score_pages(Q, qm, lst)
        assert last_kernel() == "maxsim_fwd8_pages_kernel<%d,%d,%d>" % instance(nq, lp)
        assert got.shape == (nq, m)
        assert same(got, S[:, lst.long()]), (lp, npg, nq, lq, m)
        assert (got[:, lst == 1] == 0).all()               # the all-masked page: exact 0
    # the unmasked forms
    lst = shuffled_list(gen, npg, npg, dev)
    assert same(PageCorpus.from_tensor(P, dtype=FP8).score_pages(Q, None, lst), PageCorpus.from_tensor(P, dtype=FP8).score(Q)[:, lst.long()])


# ---- 2. oracle --------------------------------------------------------------------------------------------------------------
def test_against_the_dequantised_oracle(dev):
    """17 x 33 tokens over a 23-page x 41-patch ragged corpus, tests/test_gpu_fp8.py's tolerance 1e-4 * max(1, lq / 32)."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    nq, lq, npg, lp = 17, 33, 23, 41
    gen = torch.Generator(device=dev).manual_seed(nq + 3 * lq + npg + lp)
    P, Q = unit(gen, dev, npg, lp, 128), unit(gen, dev, nq, lq, 128)
    pm = ragged_pages(gen, npg, lp, dev)
    pm[1] = False
    qm = torch.rand(nq, lq, generator=gen, device=dev) > 0.3
    qm[0] = False
    c = PageCorpus.from_tensor(P, pm, dtype=FP8)
    lst = shuffled_list(gen, npg, 40, dev, must=(1, 0, npg - 1))
    got = c.score_pages(Q, qm, lst)
    q8, qs = ops.quantize_fp8(Q, lq)
    ref = oracle(dequant(q8.float(), qs), dequant(c.planes[0].float(), c.shift), qm, pm)[:, lst.long()]
    err = (got.double() - ref).abs().max().item()
    print("fp8 page list against the dequantised oracle: max |delta| =", err)
    assert err <= 1e-4 * max(1.0, lq / 32), err


# ---- 3. holes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lp,nq,lq", [(33, 9, 7), (1030, 9, 40), (225, 257, 32), (7, 3, 1)])
def test_holes_are_minus_inf(dev, lp, nq, lq):
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(lp + nq)
    npg = 70
    P, Q = unit(gen, dev, npg, lp, 128), unit(gen, dev, nq, lq, 128)
    pm, qm = ragged_pages(gen, npg, lp, dev), ragged(gen, nq, lq, 1, dev)
    if lq > 1:
        Q[2, 1, 5] = float("nan")                          # a NaN query: NaN on every listed page with a valid patch, -inf in holes
        qm[2, 1] = True
    c = PageCorpus.from_tensor(P, pm, dtype=FP8)
    S = c.score(Q, qm).clone()
    holes = (-1, npg, 2 ** 31 - 1, -(2 ** 31))
    valid = shuffled_list(gen, npg, 9, dev, must=(0, npg - 1))
    lists = [torch.tensor([h], dtype=torch.int32, device=dev) for h in holes]                       # a hole alone (m = 1)
    mixed = []
    for i, v in enumerate(valid.tolist()):                 # every hole value between valid entries
        mixed += [v, holes[i % 4]]
    lists.append(torch.tensor([-1] + mixed, dtype=torch.int32, device=dev))                         # a hole first and last
    lists.append(torch.tensor(mixed[:-1] + [npg], dtype=torch.int32, device=dev)[torch.randperm(len(mixed), generator=gen, device=dev)])
    lists.append(torch.tensor([holes[i % 4] for i in range(150)], dtype=torch.int32, device=dev))   # holes only, several workgroups
    for lst in lists:
        ok = (lst >= 0) & (lst < npg)
        got = c.score_pages(Q, qm, lst)
        want = torch.where(ok[None], S[:, lst.clamp(0, npg - 1).long()], torch.full_like(S[:, :1], NEG_INF))
        assert (got[:, ~ok] == NEG_INF).all(), (lp, nq, lq, lst.tolist()[:6])
        assert same(got, want), (lp, nq, lq, lst.tolist()[:6])


# ---- 4. non-finite rules ----------------------------------------------------------------------------------------------------
def test_non_finite_rules(dev):
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(9)
    npg, lp, nq, lq = 6, 77, 4, 12
    P, Q = unit(gen, dev, npg, lp, 128), unit(gen, dev, nq, lq, 128)
    pm = torch.ones(npg, lp, dtype=torch.bool, device=dev)
    pm[2, 40:] = False
    pm[5] = False                                          # all-masked page
    qm = torch.ones(nq, lq, dtype=torch.bool, device=dev)
    qm[1, 8:] = False
    lst = torch.tensor([5, 0, 2, -1, 1, 0, 3, 4, 6], dtype=torch.int32, device=dev)
    clean = PageCorpus.from_tensor(P, pm, dtype=FP8).score_pages(Q, qm, lst).clone()
    P2 = P.clone()
    P2[0, 3, 7] = float("nan")                             # valid patch -> flag bit 3 -> NaN column, wherever the page is listed
    P2[2, 50, 1] = float("nan")                            # masked patch -> nothing changes
    c2 = PageCorpus.from_tensor(P2, pm, dtype=FP8)
    assert (c2.pageflags[0].item() & 8) and not (c2.pageflags[2].item() & 8)
    s = c2.score_pages(Q, qm, lst)
    assert torch.isnan(s[:, [1, 5]]).all()
    keep = [0, 2, 3, 4, 6, 7, 8]
    assert torch.equal(s[:, keep], clean[:, keep])
    Q2 = Q.clone()
    Q2[1, 10, 3] = float("nan")                            # a MASKED token of query 1
    s = PageCorpus.from_tensor(P, pm, dtype=FP8).score_pages(Q2, qm, lst)
    assert torch.isnan(s[1, [1, 2, 4, 5, 6, 7]]).all()     # pages with a valid patch
    assert s[1, 0].item() == 0.0                           # the all-masked page: exact 0
    assert (s[1, [3, 8]] == NEG_INF).all()                 # holes
    assert torch.equal(s[[0, 2, 3]], clean[[0, 2, 3]])


# ---- 5. out views -----------------------------------------------------------------------------------------------------------
def test_out_views_leave_the_other_columns_untouched(dev):
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(5)
    npg, lp = 50, 225
    P = unit(gen, dev, npg, lp, 128)
    c = PageCorpus.from_tensor(P, ragged_pages(gen, npg, lp, dev), dtype=FP8)
    for nq, lq in ((12, 32), (1, 7), (5, 40)):
        Q = unit(gen, dev, nq, lq, 128)
        lst = shuffled_list(gen, npg, 33, dev)
        lst[4] = -1
        want = c.score_pages(Q, None, lst).clone()
        out = torch.full((nq, 33 + 20), 12345.0, device=dev)
        view = c.score_pages(Q, None, lst, out=out)
        assert view.data_ptr() == out.data_ptr() and same(out[:, :33], want) and torch.all(out[:, 33:] == 12345.0)
    assert c.score_pages(Q, None, lst[:0]).shape == (5, 0) and c.score_pages(Q[:0], None, lst).shape == (0, 33)


# ---- 6. stability -----------------------------------------------------------------------------------------------------------
def test_repeated_launches_alternated_with_exhaustive_ones_give_the_same_bits(dev):
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(21)
    setups = []
    for lp, npg, nq in ((1030, 200, 40), (100, 300, 300), (1030, 200, 8)):
        P, Q = unit(gen, dev, npg, lp, 128), unit(gen, dev, nq, 32, 128)
        c = PageCorpus.from_tensor(P, ragged_pages(gen, npg, lp, dev), dtype=FP8)
        setups.append((c, Q, ragged(gen, nq, 32, 1, dev), shuffled_list(gen, npg, npg // 2, dev)))
    first = None
    for rep in range(3):
        out = []
        for c, Q, qm, lst in setups:
            out.append(c.score_pages(Q, qm, lst).clone())
            out.append(c.score(Q, qm).clone())
        if first is None:
            first = out
        else:
            assert all(same(x, y) for x, y in zip(first, out))
    for (c, Q, qm, lst), i in zip(setups, range(0, 6, 2)):
        assert same(first[i], first[i + 1][:, lst.long()])


# ---- 7. filtered two-stage, exact part --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,lp", [("bf16", 1030), ("f32", 33)])
def test_every_page_surviving_gives_the_exact_subset_topk(dev, kind, lp):
    """candidates >= m: the search is exact.topk(subset=) bit for bit; m < k pads with (-inf, -1); m = 0 is all padding."""
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    gen = torch.Generator(device=dev).manual_seed(lp + 7)
    nq, lq, npg, base = 21, 32, 300, 300
    Q, P, _ = make(gen, nq, lq, npg, lp, dev, planted=False)
    pm, qm = ragged(gen, npg, lp, max(lp // 2, 1), dev), ragged(gen, nq, lq, 1, dev)
    if kind == "bf16":
        Q, P = Q.bfloat16(), P.bfloat16()
    exact = PageCorpus.from_tensor(P, pm, idx_base=base)
    ts = TwoStageRetriever(PageCorpus.from_tensor(P, pm, idx_base=base, dtype=FP8), exact)
    allow = torch.rand(npg, generator=gen, device=dev) < 0.2
    s = exact.subset(allow=allow)
    assert 30 <= s.m <= 100
    for k, cand in ((10, 128), (s.m, s.m), (100, 128), (100, 4096), (1, 100)):           # k = 100 > m: padding at the end
        gs, gi = ts.search(Q, qm, k=k, candidates=cand, subset=s)
        es, ei = exact.topk(Q, qm, k, subset=s)
        assert torch.equal(gi, ei) and same(gs, es), (kind, k, cand)
        assert ((gi < 0) | allow[(gi - base).clamp_min(0).long()]).all()
    assert (gi[:, 0] >= 0).all()
    gs, gi = ts.search(Q, qm, k=100, candidates=128, subset=s)
    assert (gi[:, s.m:] == -1).all() and (gs[:, s.m:] == NEG_INF).all() and (gi[:, :s.m] >= base).all()
    empty = exact.subset(allow=torch.zeros(npg, dtype=torch.bool, device=dev))
    gs, gi = ts.search(Q, qm, k=10, candidates=32, subset=empty)
    assert gs.shape == (nq, 10) and (gs == NEG_INF).all() and (gi == -1).all()
    ts.part_events = []
    ts.search(Q, qm, k=10, candidates=32, subset=s)
    assert len(ts.part_events) == 1 and len(ts.part_events[0]) == 4


# ---- 8. filtered two-stage, approximate part --------------------------------------------------------------------------------
def planted_setup(gen, dev, nq=64, lq=32, npg=3000, lp=225):
    """Planted queries (score ~ 28 against ~ 9, fp8 error <= 0.1); the subset holds the targets of the even queries and none of the odd
    ones, plus a random third of the other pages."""
    Q, P, t = make(gen, nq, lq, npg, lp, dev, planted=True)
    Q, P = Q.bfloat16(), P.bfloat16()
    allow = torch.rand(npg, generator=gen, device=dev) < 0.33
    inside = torch.arange(nq, device=dev) % 2 == 0
    allow[t[~inside]] = False
    allow[t[inside]] = True
    inside = allow[t]                                      # (an odd query's target may be an even query's too)
    return Q, P, t, allow, inside


def check_structure(gs, gi, exact, Q, allow, base=0):
    """Indices inside the subset (or padding), and every score `exact`'s bit pattern for that pair."""
    real = gi >= 0
    assert allow[(gi - base).clamp_min(0).long()][real].all()
    S = exact.score(Q, None)
    assert torch.equal(gs[real], S.gather(1, (gi - base).clamp_min(0).long())[real])
    assert (gs[~real] == NEG_INF).all()


def test_planted_queries_survive_a_filtered_fp8_first_stage(dev):
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    gen = torch.Generator(device=dev).manual_seed(8)
    Q, P, t, allow, inside = planted_setup(gen, dev)
    assert 16 <= int(inside.sum()) <= 48
    exact = PageCorpus.from_tensor(P)
    ts = TwoStageRetriever(PageCorpus.from_tensor(P, dtype=FP8), exact)
    gs, gi = ts.search(Q, None, k=10, candidates=32, subset=exact.subset(allow=allow))
    assert torch.equal(gi[inside, 0].long(), t[inside])
    assert not (gi[~inside] == t[~inside, None]).any()
    check_structure(gs, gi, exact, Q, allow)


# ---- 9. shards --------------------------------------------------------------------------------------------------------------
def test_shard_views_search_their_own_subset_and_merge_to_the_whole(dev):
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever, merge_candidates
    gen = torch.Generator(device=dev).manual_seed(12)
    nq, lq, npg, lp, base, k = 10, 32, 301, 1030, 70, 20
    Q, P, _ = make(gen, nq, lq, npg, lp, dev, planted=False)
    Q, P = Q.bfloat16(), P.bfloat16()
    pm = ragged(gen, npg, lp, lp // 2, dev)
    exact = PageCorpus.from_tensor(P, pm, idx_base=base)
    coarse = PageCorpus.from_tensor(P, pm, idx_base=base, dtype=FP8)
    glob = (torch.rand(npg, generator=gen, device=dev) < 0.5).nonzero().flatten() + base
    glob = torch.cat([glob, glob[:5], torch.tensor([-1, base + npg], device=dev)])
    glob = glob[torch.randperm(glob.numel(), generator=gen, device=dev)]
    # candidates >= the pages of each subset: both the whole search and the shards' are exact, so the merge must reproduce the whole
    ws, wi = TwoStageRetriever(coarse, exact).search(Q, None, k=k, candidates=512, subset=exact.subset(pages=glob))
    parts = []
    for lo, hi in ((0, 140), (140, npg)):
        ce, cc = exact.shard(lo, hi), coarse.shard(lo, hi)
        s, i = TwoStageRetriever(cc, ce).search(Q, None, k=k, candidates=512, subset=ce.subset(pages=glob))
        assert ((i < 0) | ((i >= base + lo) & (i < base + hi))).all()
        parts.append((s, i))
    ms, mi = merge_candidates(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)
    assert torch.equal(mi, wi) and same(ms, ws)
    es, ei = exact.topk(Q, None, k, subset=exact.subset(pages=glob))
    assert torch.equal(wi, ei) and same(ws, es)


# ---- 10. a non-fp8 first stage ----------------------------------------------------------------------------------------------
def test_a_pooled_bf16_first_stage_follows_the_subset(dev):
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    gen = torch.Generator(device=dev).manual_seed(10)
    Q, P, t, allow, inside = planted_setup(gen, dev, nq=32, npg=800, lp=1030)
    n, lp, d = P.shape
    g = lp // 41
    pooled = F.normalize(P[:, :g * 41].float().view(n, 41, g, d).mean(2), dim=-1).bfloat16()
    exact = PageCorpus.from_tensor(P)
    coarse = PageCorpus.from_tensor(pooled)
    assert coarse.lp == 41 and not coarse.fp8
    ts = TwoStageRetriever(coarse, exact)
    gs, gi = ts.search(Q, None, k=10, candidates=32, subset=exact.subset(allow=allow))
    check_structure(gs, gi, exact, Q, allow)
    assert (gi >= 0).all()
