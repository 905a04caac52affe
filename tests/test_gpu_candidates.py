"""Candidate scoring (PageCorpus.score_candidates / rerank), top-R selection (ops.select_topr) and the two-stage search
(TwoStageRetriever), against the product's own exhaustive path: equal bits, NaN at equal places."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaN == NaN (the positions of NaN scores are part of the answer); -0.0 != +0.0 is not at stake here."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def ragged(gen, n, l, lo, dev):
    lens = torch.randint(lo, l + 1, (n,), generator=gen, device=dev)
    return torch.arange(l, device=dev)[None, :] < lens[:, None]


def make(gen, nq, lq, npg, lp, dev, planted=True):
    """tests/test_gpu_prefilter.py's generator: unit rows, planted queries lie near one page (score ~ 28 against ~ 9)."""
    P = F.normalize(torch.randn((npg, lp, 128), generator=gen, device=dev), dim=-1)
    Q = F.normalize(torch.randn((nq, lq, 128), generator=gen, device=dev), dim=-1)
    if planted and npg > 0:
        t = torch.randint(0, npg, (nq,), generator=gen, device=dev)
        rows = torch.randint(0, lp, (nq, lq), generator=gen, device=dev)
        Q = F.normalize(P[t[:, None], rows] + 0.5 * Q, dim=-1)
    return Q, P


def lists(gen, nq, r, lo, hi, dev, holes=(-1,)):
    """(nq, r) int32 page indices in [lo, hi) -- with duplicates -- and about one entry in six replaced by a hole value."""
    cand = torch.randint(lo, hi, (nq, r), generator=gen, device=dev, dtype=torch.int32)
    pick = torch.randint(0, 6 * len(holes), (nq, r), generator=gen, device=dev)
    for i, h in enumerate(holes):
        cand = torch.where(pick == i, torch.full_like(cand, h), cand)
    return cand


def gathered(S, cand, idx_base=0):
    """What score_candidates must return, from the exhaustive block S of the corpus whose first page is idx_base."""
    n = S.shape[1]
    loc = cand.long() - idx_base
    ok = (loc >= 0) & (loc < n)
    return torch.where(ok, S.gather(1, loc.clamp(0, max(n - 1, 0))), torch.full_like(S[:, :1], NEG_INF).expand_as(loc)), ok


def lex_topk(scores, idx, k):
    """numpy: order key descending, index ascending; (-inf, -1) where fewer than k entries exist.  scores / idx: (nq, r) tensors."""
    from evdr_amd import ops
    key = ops._order_key(scores).cpu().numpy().astype(np.int64)
    sc, ix = scores.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    nq, r = sc.shape
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int32)
    for q in range(nq):
        order = np.lexsort((ix[q], -key[q]))[:k]
        out_s[q, :len(order)] = sc[q, order]
        out_i[q, :len(order)] = ix[q, order]
    hole = out_i < 0
    out_s[hole] = -np.inf
    return torch.from_numpy(out_s), torch.from_numpy(out_i)


def topr_rule(scores, r, idx_base=0):
    """numpy: the r columns with the largest order key, ties towards the lower index, ascending, -1 padding."""
    from evdr_amd import ops
    key = ops._order_key(scores).cpu().numpy().astype(np.int64)
    nq, n = key.shape
    out = np.full((nq, r), -1, dtype=np.int32)
    for q in range(nq):
        pick = np.sort(np.lexsort((np.arange(n), -key[q]))[:r])
        out[q, :len(pick)] = pick + idx_base
    return torch.from_numpy(out)


@pytest.mark.parametrize("kind,lp,npg", [
    ("f32", 7, 300), ("f32", 33, 300), ("f32", 224, 200), ("f32", 225, 200), ("f32", 1030, 120),
    ("bf16", 225, 200), ("bf16", 1030, 150),
    ("bf16", 7, 300), ("bf16", 33, 300), ("bf16", 224, 200),
])
def test_candidate_scores_are_the_exhaustive_scores(dev, kind, lp, npg):
    """1. score_candidates == score gathered at cand, holes -inf: equal bits for fp32 corpora at every page length and for bf16
    pages of >= 8 tiles.  For bf16 pages of 7 / 33 / 224 patches the exhaustive default is the flat ring kernel and the gate is 1e-4;
    the bits were compared on the GPU and are equal there too (both kernels chain the same products in the same order, DESIGN.md
    §4.6), so equality is asserted for those as well."""
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(lp * 7 + npg)
    for nq, lq, r in ((5, 1, 1), (9, 7, 37), (1, 7, 600), (6, 32, 4096), (33, 32, 130)):
        Q, P = make(gen, nq, lq, npg, lp, dev)
        pm = ragged(gen, npg, lp, max(1, lp // 2), dev)
        qm = ragged(gen, nq, lq, 1, dev)
        if kind == "bf16":
            Q, P = Q.bfloat16(), P.bfloat16()
        corpus = PageCorpus.from_tensor(P, pm)
        S = corpus.score(Q, qm)
        cand = lists(gen, nq, r, 0, npg, dev, holes=(-1, npg, 2 ** 30, -(2 ** 31)))
        if r > 2:
            cand[:, r // 2] = -1                                    # a hole in the middle of every row
            cand[:, r // 2 - 1] = npg - 1                           # the last page, next to it
        want, ok = gathered(S, cand)
        got = corpus.score_candidates(Q, qm, cand)
        assert got.shape == (nq, r) and got.dtype == torch.float32
        assert torch.equal(torch.isinf(got) & (got < 0), ~ok)       # holes, and only holes, are -inf
        diff = (got[ok] - want[ok]).abs().max().item() if ok.any() else 0.0
        print(f"{kind} lp={lp} nq={nq} lq={lq} r={r}: max |delta| = {diff:.3g}, bits equal = {same(got, want)}")
        assert diff <= 1e-4
        assert same(got, want), (kind, lp, nq, lq, r, diff)


def test_masked_pages_nan_pages_and_nan_query_tokens(dev):
    """2. an all-masked page scores exactly 0.0; a NaN page and a NaN query token put NaN where `score` puts it."""
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(11)
    for kind, lp in (("f32", 33), ("f32", 1030), ("bf16", 1030)):
        nq, lq, npg = 7, 7, 40
        Q, P = make(gen, nq, lq, npg, lp, dev)
        pm = ragged(gen, npg, lp, max(1, lp // 2), dev)
        qm = ragged(gen, nq, lq, 2, dev)
        pm[3] = False                                               # all-masked page
        P[5, 0, 0] = float("nan")                                   # valid patch of page 5
        P[6, lp - 1, 0] = float("nan")
        pm[6, lp - 1] = False                                       # masked patch: does not count
        Q[2, 1, 5] = float("nan")                                   # a token of query 2
        qm[2, 1] = True
        Q[4, lq - 1, 0] = float("nan")                              # masked token of query 4: counts as well
        qm[4, lq - 1] = False
        if kind == "bf16":
            Q, P = Q.bfloat16(), P.bfloat16()
        corpus = PageCorpus.from_tensor(P, pm)
        S = corpus.score(Q, qm)
        cand = torch.arange(npg, device=dev, dtype=torch.int32).flip(0)[None].repeat(nq, 1).contiguous()
        cand[:, 10] = -1
        got = corpus.score_candidates(Q, qm, cand)
        want, ok = gathered(S, cand)
        assert same(got, want)
        col = {p: npg - 1 - p for p in (3, 5, 6)}
        assert torch.equal(got[:, col[3]], torch.zeros(nq, device=dev))                 # exact 0, NaN queries included
        assert torch.isnan(got[:, col[5]]).all()
        assert not torch.isnan(got[[0, 1, 3, 5, 6], col[6]]).any()
        real = torch.ones(npg, dtype=torch.bool, device=dev)
        real[[col[3], 10]] = False
        assert torch.isnan(got[2][real]).all() and torch.isnan(got[4][real]).all()


def test_against_the_cpu_oracle(dev):
    """3. one case against the oracle instead of the product: |delta| <= 1e-4, the project's parity gate."""
    from oracle import maxsim_oracle as O
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(3)
    nq, lq, npg, lp, r = 8, 13, 60, 70, 50
    Q, P = make(gen, nq, lq, npg, lp, dev)
    pm, qm = ragged(gen, npg, lp, 20, dev), ragged(gen, nq, lq, 1, dev)
    cand = lists(gen, nq, r, 0, npg, dev)
    want, ok = gathered(O.maxsim_masked(Q.cpu(), P.cpu(), qm.cpu(), pm.cpu()), cand.cpu())
    got = PageCorpus.from_tensor(P, pm).score_candidates(Q, qm, cand).cpu()
    assert torch.equal(torch.isinf(got), ~ok)
    assert (got[ok] - want[ok]).abs().max().item() <= 1e-4


@pytest.mark.parametrize("kind,lp", [("f32", 33), ("bf16", 1030)])
def test_rerank_is_a_lexsort_of_the_candidate_scores(dev, kind, lp):
    """4. rerank == numpy lexsort (order key descending, index ascending) of score_candidates; (-inf, -1) padding."""
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(lp)
    nq, lq, npg = 12, 7, 90
    Q, P = make(gen, nq, lq, npg, lp, dev)
    pm, qm = ragged(gen, npg, lp, max(1, lp // 2), dev), ragged(gen, nq, lq, 1, dev)
    P[7, 0, 0] = float("nan")                                       # NaN scores rank first
    if kind == "bf16":
        Q, P = Q.bfloat16(), P.bfloat16()
    corpus = PageCorpus.from_tensor(P, pm, idx_base=1000)
    for r, k in ((300, 100), (64, 64), (40, 1), (128, 128)):
        cand = lists(gen, nq, r, 1000, 1000 + npg, dev, holes=(-1, 5, 1000 + npg))
        cand[0, 3:] = -1                                            # three real entries at most: padding from rank 4 on
        cand[1] = -1                                                # none at all
        sc = corpus.score_candidates(Q, qm, cand)
        clean = torch.where(torch.isinf(sc) & (sc < 0), torch.full_like(cand, -1), cand)
        ws, wi = lex_topk(sc, clean, k)
        ts, ti = corpus.rerank(Q, qm, cand, k)
        assert torch.equal(ti.cpu(), wi), (r, k)
        assert same(ts.cpu(), ws)
        assert (ti[1] == -1).all() and torch.isinf(ts[1]).all()
        if k > 3:
            assert (ti[0, 3:] == -1).all() and (ts[0, 3:] == NEG_INF).all()


def test_select_topr_follows_the_order_key_rule(dev):
    """5. select_topr == numpy (largest order keys, ties at the cut towards the lower index, ascending, -1 padding) on random rows,
    rows with exact ties across the cut, NaN rows, n < r, strided rows; for r <= 128 the sorted index set of ops.topk."""
    from evdr_amd import ops
    gen = torch.Generator(device=dev).manual_seed(5)
    cases = []
    for nq, n in ((7, 1000), (3, 100_003), (5, 257), (4, 50), (2, 4096), (3, 1)):
        x = torch.randn((nq, n), generator=gen, device=dev) * 9
        cases.append(x)
        t = torch.randint(0, 6, (nq, n), generator=gen, device=dev).float() - 2.0          # heavy ties, -0.0 / +0.0 among them
        t[0] = torch.where(t[0] == 0, torch.full_like(t[0], -0.0), t[0])
        cases.append(t)
        y = x.clone()
        y[torch.rand((nq, n), generator=gen, device=dev) < 0.3] = float("nan")
        y[-1] = float("nan")
        y[0, ::3] = float("inf")
        y[0, 1::3] = NEG_INF
        cases.append(y)
    big = torch.randn((6, 3000), generator=gen, device=dev)
    cases.append(big[:, 100:1900])                                  # row stride 3000, 1800 columns, 16-B misaligned or not
    cases.append(big[:, 1:1000])
    for x in cases:
        n = x.shape[1]
        for r in sorted({1, 2, 100, 128, 129, 512, 4096, min(4096, max(1, n - 1)), min(4096, n), min(4096, n + 1)}):
            got = ops.select_topr(x, r, idx_base=7)
            assert got.dtype == torch.int32 and got.shape == (x.shape[0], r)
            assert torch.equal(got.cpu(), topr_rule(x, r, 7)), (tuple(x.shape), r)
            if r <= 128:
                _, ti = ops.topk(x.contiguous(), r, idx_base=7)
                ti = torch.where(ti < 0, torch.full_like(ti, 2 ** 31 - 1), ti).sort(dim=1).values
                ti = torch.where(ti == 2 ** 31 - 1, torch.full_like(ti, -1), ti)
                assert torch.equal(got, ti), (tuple(x.shape), r)


@pytest.mark.parametrize("kind,lp", [("f32", 225), ("bf16", 1030)])
def test_shard_views_rerank_their_own_pages_and_merge_to_the_whole(dev, kind, lp):
    """6. two shard() views reranked on the same GLOBAL lists and merged == the whole corpus's rerank."""
    from evdr_amd.corpus import PageCorpus, merge_candidates
    gen = torch.Generator(device=dev).manual_seed(lp + 1)
    nq, lq, npg, base = 10, 32, 101, 50
    Q, P = make(gen, nq, lq, npg, lp, dev)
    pm, qm = ragged(gen, npg, lp, lp // 2, dev), ragged(gen, nq, lq, 1, dev)
    if kind == "bf16":
        Q, P = Q.bfloat16(), P.bfloat16()
    corpus = PageCorpus.from_tensor(P, pm, idx_base=base)
    a, b = corpus.shard(0, 37), corpus.shard(37, npg)
    for r, k in ((256, 100), (30, 10)):
        cand = lists(gen, nq, r, base, base + npg, dev, holes=(-1, 0, base + npg))
        cand[2] = -1
        cand[3, 5:] = base + 40                                     # duplicates of one page of the second shard
        ws, wi = corpus.rerank(Q, qm, cand, k)
        sa, ia = a.rerank(Q, qm, cand, k)
        sb, ib = b.rerank(Q, qm, cand, k)
        assert ((ia < 0) | ((ia >= base) & (ia < base + 37))).all() and ((ib < 0) | (ib >= base + 37)).all()
        ms, mi = merge_candidates(torch.cat([sa, sb], 1), torch.cat([ia, ib], 1), k)
        assert torch.equal(mi, wi) and same(ms, ws)
        want, _ = gathered(corpus.score(Q, qm), cand, base)
        assert same(a.score_candidates(Q, qm, cand), gathered(a.score(Q, qm), cand, base)[0])
        got_ab = torch.maximum(a.score_candidates(Q, qm, cand), b.score_candidates(Q, qm, cand))     # each entry has one owner
        assert same(got_ab, want)


def pooled(P, nout):
    """Pages mean-pooled to nout patches (a compressed copy of the same pages, another page length)."""
    n, lp, d = P.shape
    g = lp // nout
    return F.normalize(P[:, :g * nout].float().view(n, nout, g, d).mean(2), dim=-1)


def compose(coarse, exact, Qc, Q, qm, k, candidates):
    """The two-stage search done with torch / numpy on coarse.score and exact.score."""
    cand = topr_rule(coarse.score(Qc, qm), candidates, exact.idx_base).to(Q.device)
    sc, _ = gathered(exact.score(Q, qm), cand, exact.idx_base)
    return lex_topk(sc, cand, k)


@pytest.mark.parametrize("exact_kind", ["f32", "bf16"])
@pytest.mark.parametrize("coarse_kind", ["fp8", "pooled"])
def test_two_stage_retriever(dev, exact_kind, coarse_kind):
    """7. indices and score bits == the same composition done with torch; candidates >= n_pages gives exact.topk bit for bit."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    gen = torch.Generator(device=dev).manual_seed(len(exact_kind) * 10 + len(coarse_kind))
    nq, lq, npg, lp = 21, 32, 700, 1030
    Q, P = make(gen, nq, lq, npg, lp, dev, planted=False)
    pm, qm = ragged(gen, npg, lp, lp // 2, dev), ragged(gen, nq, lq, 1, dev)
    if exact_kind == "bf16":
        Q, P = Q.bfloat16(), P.bfloat16()
    exact = PageCorpus.from_tensor(P, pm)
    if coarse_kind == "fp8":
        coarse, Qc = PageCorpus.from_tensor(P, pm, dtype=ops.FP8), Q
    else:
        coarse, Qc = PageCorpus.from_tensor(pooled(P, 41).bfloat16()), Q.bfloat16()
        assert coarse.lp == 41
    ts = TwoStageRetriever(coarse, exact)
    for k, c in ((100, 128), (10, 64), (1, 1), (100, 512)):
        s, i = ts.search(Q, qm, k=k, candidates=c, Q_coarse=Qc)
        ws, wi = compose(coarse, exact, Qc, Q, qm, k, c)
        assert torch.equal(i.cpu(), wi), (k, c)
        assert same(s.cpu(), ws)
    for k, c in ((100, 700), (100, 1024), (7, 4096)):              # every page survives the first stage
        s, i = ts.search(Q, qm, k=k, candidates=c, Q_coarse=Qc)
        es, ei = exact.topk(Q, qm, k)
        assert torch.equal(i, ei) and same(s, es), (k, c)


def test_two_stage_small_corpus_and_default_queries(dev):
    """candidates > n_pages > k and n_pages < k: the padding of `topk`; Q_coarse defaults to Q."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    gen = torch.Generator(device=dev).manual_seed(77)
    for npg, k in ((60, 100), (150, 100)):
        Q, P = make(gen, 9, 7, npg, 225, dev)
        pm, qm = ragged(gen, npg, 225, 100, dev), ragged(gen, 9, 7, 1, dev)
        exact = PageCorpus.from_tensor(P, pm, idx_base=300)
        ts = TwoStageRetriever(PageCorpus.from_tensor(P, pm, idx_base=300, dtype=ops.FP8), exact)
        s, i = ts.search(Q, qm, k=k, candidates=256)
        es, ei = exact.topk(Q, qm, k)
        assert torch.equal(i, ei) and same(s, es)


def test_planted_queries_survive_an_fp8_first_stage(dev):
    """7 (end). planted score ~ 28 against ~ 9 for other pages, fp8 error <= 0.1: with 32 candidates the top-1 is the exhaustive
    top-1 for every query."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    gen = torch.Generator(device=dev).manual_seed(8)
    nq, lq, npg, lp = 64, 32, 3000, 225
    Q, P = make(gen, nq, lq, npg, lp, dev, planted=True)
    Q, P = Q.bfloat16(), P.bfloat16()
    exact = PageCorpus.from_tensor(P)
    ts = TwoStageRetriever(PageCorpus.from_tensor(P, dtype=ops.FP8), exact)
    s, i = ts.search(Q, None, k=10, candidates=32)
    es, ei = exact.topk(Q, None, 10)
    assert torch.equal(i[:, 0], ei[:, 0]) and torch.equal(s[:, 0], es[:, 0])


def test_repeated_and_alternating_launches_give_the_same_bits(dev):
    """8. two launches give the same bits; alternating two corpora does too."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    gen = torch.Generator(device=dev).manual_seed(9)
    setups = []
    for kind, lp, npg in (("bf16", 1030, 300), ("f32", 230, 500)):
        Q, P = make(gen, 17, 32, npg, lp, dev)
        pm, qm = ragged(gen, npg, lp, lp // 2, dev), ragged(gen, 17, 32, 1, dev)
        if kind == "bf16":
            Q, P = Q.bfloat16(), P.bfloat16()
        exact = PageCorpus.from_tensor(P, pm)
        ts = TwoStageRetriever(PageCorpus.from_tensor(P, pm, dtype=ops.FP8), exact)
        cand = lists(gen, 17, 200, 0, npg, dev, holes=(-1, npg))
        setups.append((exact, ts, Q, qm, cand))
    first = None
    for rep in range(4):
        out = []
        for exact, ts, Q, qm, cand in setups:
            out.append(exact.score_candidates(Q, qm, cand))
            out.extend(exact.rerank(Q, qm, cand, 50))
            out.extend(ts.search(Q, qm, k=20, candidates=100))
        if first is None:
            first = [o.clone() for o in out]
        else:
            for a, b in zip(first, out):
                assert same(a.float(), b.float()) and a.dtype == b.dtype
