"""The ranking contract under ties, on every path that ends in `evdr_topk`: score descending, REPORTED index ascending on ties -- also
when equal scores straddle the cut and the columns of an `idx_map` come in any order --, (-inf, -1) padding, NaN first, -0 == +0.

The reference is `rank_rule` below: numpy, order keys built from the raw float bits, one lexsort.  It is anchored on the CPU to
`oracle.maxsim_oracle.topk_rows` (test_rank_rule_is_the_oracle_ranking) before it judges a kernel.  Every comparison is bit equality of
indices and of score bits (NaN at equal places); nothing here has a tolerance.  Scores with many ties are drawn from VALUES, so that
a tie run is much longer than k.  The seeded sweep at the end is the one scratch/fuzz_topk.py runs (that script calls this module)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

gpu = pytest.mark.gpu

VALUES = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, np.inf, np.nan], dtype=np.float32)
KS = (1, 5, 12, 64)                                                 # the cuts of the corpus tests (see tie_corpus)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def order_key(scores: np.ndarray) -> np.ndarray:
    """fp32 -> uint32, a larger key ranks earlier: NaN of either sign is the greatest key, -0.0 counts as +0.0, otherwise the usual
    sign flip (negative floats: all bits inverted; others: sign bit set)."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    key = np.where((u & np.uint32(0x80000000)) != 0, ~u, u | np.uint32(0x80000000))
    return np.where(nan, np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def rank_rule(scores, reported, k):
    """(nq, n) scores and reported indices -> ((nq, k) fp32, (nq, k) int32): key descending, reported index (as uint32, so that -1
    holes come last among -inf scores) ascending, cut at k, (-inf, -1) padding.  Scores come back with -0.0 as +0.0."""
    sc = np.ascontiguousarray(scores, dtype=np.float32)
    rep = np.ascontiguousarray(np.broadcast_to(np.asarray(reported), sc.shape), dtype=np.int32)
    nq, n = sc.shape
    order = np.lexsort((rep.view(np.uint32), -order_key(sc).astype(np.int64)), axis=-1)[:, :k]
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int32)
    out_s[:, :order.shape[1]] = np.take_along_axis(sc, order, 1)
    out_i[:, :order.shape[1]] = np.take_along_axis(rep, order, 1)
    out_s[out_s == 0] = 0.0
    return out_s, out_i


def straddled(scores, k):
    """(nq,) bool: the k-th and the (k+1)-th key of the row are equal, i.e. a tie runs across the cut."""
    key = -np.sort(-order_key(scores).astype(np.int64), axis=1)
    return key[:, k - 1] == key[:, k] if key.shape[1] > k else np.zeros(key.shape[0], dtype=bool)


def host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def assert_ranking(got, want, what=""):
    """Indices equal, NaN at equal places, every other score equal bit for bit."""
    gs, gi, ws, wi = host(got[0]), host(got[1]), host(want[0]), host(want[1])
    assert gs.shape == ws.shape and gi.shape == wi.shape and gs.dtype == np.float32 and gi.dtype == np.int32, what
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, (what, "first differing (row, rank):", bad[0].tolist(), gi[bad[0][0]].tolist(), wi[bad[0][0]].tolist())
    gn, wn = np.isnan(gs), np.isnan(ws)
    assert np.array_equal(gn, wn), what
    assert np.array_equal(gs.view(np.uint32)[~gn], ws.view(np.uint32)[~wn]), what


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def topk_one_level(scores: torch.Tensor, k: int, idx_map=None, idx_base: int = 0):
    """evdr_topk with workspace_or_null = NULL: one workgroup per row, whatever the shape."""
    from evdr_amd import _lib as L
    nq, n = scores.shape
    assert scores.is_contiguous() and (idx_map is None or (idx_map.is_contiguous() and idx_map.dtype == torch.int32))
    ts = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    ti = torch.empty((nq, k), dtype=torch.int32, device=scores.device)
    with L.on(scores.device):
        L.check(L.load().evdr_topk(L.ptr(scores), L.ptr(idx_map), nq, n, n, idx_base, k, L.ptr(ts), L.ptr(ti), None, 0,
                                   L.current_stream_handle(scores.device)))
    return ts, ti


def shuffled_rows(rng, row, nq):
    """(nq, n): an independent random permutation of `row` in every row."""
    return rng.permuted(np.tile(row, (nq, 1)), axis=1)


# ---- host anchor: the reference against the oracle the project already trusts -----------------------------------------------------
@pytest.mark.parametrize("n,k", [(500, 100), (37, 100), (100, 100), (5000, 10), (1, 1), (20000, 128), (8193, 7)])
def test_rank_rule_is_the_oracle_ranking(n, k):
    """rank_rule with the identity map == oracle.topk_rows on the score rows of test_topk_vs_oracle (heavy ties, all equal, -inf
    stripes, +-0), plus the padding when n < k.  No GPU."""
    from oracle import maxsim_oracle as O
    gen = torch.Generator().manual_seed(n + k)
    s = torch.randn(9, n, generator=gen)
    s[0, : n // 2] = 1.5
    s[1] = 0.0
    s[2, ::3] = float("-inf")
    s[3, : min(n, 7)] = -0.0
    s[3, min(n, 7):] = -1.0
    if n > 3:
        s[3, 3] = 0.0
    ws, wi = O.topk_rows(s, k)
    gs, gi = rank_rule(s.numpy(), np.arange(n), k)
    keff = min(k, n)
    assert np.array_equal(gi[:, :keff], wi.numpy())
    assert np.array_equal(gs[:, :keff].view(np.uint32), (ws + 0.0).numpy().view(np.uint32))
    assert (gi[:, keff:] == -1).all() and (gs[:, keff:] == -np.inf).all()
    gs7, gi7 = rank_rule(s.numpy(), np.arange(n) + 7, k)
    assert np.array_equal(gi7[:, :keff], wi.numpy() + 7) and np.array_equal(gs7.view(np.uint32), gs.view(np.uint32))


def test_rank_rule_edges():
    """What the oracle's rows do not hold: NaN of either sign first, -1 holes last among -inf, a reversed map."""
    nan_neg = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
    s = np.array([[1.0, np.nan, -np.inf, -np.inf, nan_neg, 1.0, -0.0, 0.0]], dtype=np.float32)
    rep = np.array([[9, 8, -1, 6, 5, 4, 3, 2]], dtype=np.int32)
    gs, gi = rank_rule(s, rep, 10)
    assert gi[0].tolist() == [5, 8, 4, 9, 2, 3, 6, -1, -1, -1]
    assert np.isnan(gs[0, :2]).all() and gs[0, 2:].tolist() == [1.0, 1.0, 0.0, 0.0] + [-np.inf] * 4
    assert not np.signbit(gs[0, 4:6]).any()
    assert straddled(s, 1).tolist() == [True] and straddled(s, 2).tolist() == [False] and straddled(s, 8).tolist() == [False]


# ---- a. ops.topk / evdr_topk with a non-monotone idx_map, one workgroup per row ---------------------------------------------------
def tie_rows(rng, nq, n, k):
    """(nq, n) fp32 from VALUES; row 0 all equal, row 1 more than k NaNs (both signs), row 2 cut inside a +-0 run."""
    sc = VALUES[rng.integers(0, len(VALUES), (nq, n))]
    sc[0] = 0.5
    sc[1, :140] = np.nan                                            # > 128 NaNs (n = 129: the whole row)
    sc[1, :140:3] = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    above = min(k // 2, n // 4)
    row = np.where(np.arange(n) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    row[:above] = 0.5
    sc[2] = rng.permutation(row)                                    # `above` < k scores over a run of n - above > k zeros
    return np.ascontiguousarray(sc, dtype=np.float32)


def make_map(rng, kind, sc):
    """The idx_map of one case; "holes" also writes -inf under its -1 entries (a cleaned candidate list)."""
    nq, n = sc.shape
    if kind == "perm":
        return shuffled_rows(rng, np.arange(n) + 7000, nq).astype(np.int32)
    if kind == "reversed":
        return np.tile(np.arange(n)[::-1], (nq, 1)).astype(np.int32)
    if kind == "repeats":
        return (rng.integers(0, max(n // 3, 1), (nq, n)) + 100).astype(np.int32)
    assert kind == "holes"
    m = shuffled_rows(rng, np.arange(n) + 7000, nq).astype(np.int32)
    hole = rng.random((nq, n)) < 1 / 6
    m[hole] = -1
    sc[hole] = -np.inf
    return m


@gpu
@pytest.mark.parametrize("kind", ["perm", "reversed", "repeats", "holes"])
@pytest.mark.parametrize("nq,n", [(6, 300), (4, 129)])
def test_mapped_topk_keeps_the_lowest_reported_indices(dev, nq, n, kind):
    from evdr_amd import ops
    for k in (1, 7, 50, 128):
        rng = np.random.default_rng(1000 * n + k)
        sc = tie_rows(rng, nq, n, k)
        m = make_map(rng, kind, sc)
        if kind != "holes":                                         # (holes overwrite some of the built ties with -inf)
            assert straddled(sc, k)[:3].all()                       # the three built rows cut through a tie
        t, tm = torch.from_numpy(sc).to(dev), torch.from_numpy(m).to(dev)
        want = rank_rule(sc, m, k)
        got = ops.topk(t, k, idx_map=tm)
        assert_ranking(got, want, (nq, n, kind, k))
        assert_ranking(topk_one_level(t, k, tm), want, (nq, n, kind, k, "C ABI, no workspace"))
        again = ops.topk(t, k, idx_map=tm)                          # launch after launch: the same bits
        assert torch.equal(again[1], got[1]) and torch.equal(again[0].view(torch.int32), got[0].view(torch.int32))


@gpu
def test_mapped_topk_on_a_misaligned_column_slice(dev):
    """n = 4097 columns taken out of a wider matrix: the head and tail of the 16-byte row scan, with a shuffled map."""
    from evdr_amd import ops
    rng = np.random.default_rng(4097)
    wide = np.ascontiguousarray(VALUES[rng.integers(0, len(VALUES), (3, 4200))], dtype=np.float32)
    wide[0] = 0.5
    mwide = shuffled_rows(rng, np.arange(4200) + 7000, 3).astype(np.int32)
    t, tm = torch.from_numpy(wide).to(dev)[:, 3:4100], torch.from_numpy(mwide).to(dev)[:, 3:4100]
    assert t.shape[1] == 4097 and not t.is_contiguous()
    for k in (1, 50, 128):
        assert straddled(wide[:, 3:4100], k).all()
        assert_ranking(ops.topk(t, k, idx_map=tm), rank_rule(wide[:, 3:4100], mwide[:, 3:4100], k), k)
        assert_ranking(ops.topk(t, k, idx_base=11), rank_rule(wide[:, 3:4100], np.arange(4097) + 11, k), (k, "unmapped"))


# ---- b. the two-level form ---------------------------------------------------------------------------------------------------------
TWO_NQ, TWO_N, TWO_K, TWO_SEG = 3, 12289, 100, 3076                 # evdr_topk_segments(3, 12289) = 4 segments of 3076 columns (last: 3061)


def two_level_rows(rng, layout):
    if layout == "tie_in_every_segment":
        sc = VALUES[rng.integers(0, len(VALUES), (TWO_NQ, TWO_N))]                          # row 1: every value ~ 440 times per segment
        sc[0] = 0.5
        sc[0, rng.choice(TWO_N, 30, replace=False)] = np.inf
        sc[2] = np.array([-1.0, -0.0, 0.0, 0.5], dtype=np.float32)[rng.integers(0, 4, TWO_N)]
        return np.ascontiguousarray(sc, dtype=np.float32)
    # 40 distinct scores above 1.0 (10 per segment), then 1.0 on fewer than k columns of every segment -- each segment keeps all of
    # its own (10 + members <= k), so only the merge launch meets the straddle: 60 of the >= 100 tied columns make the cut
    assert layout == "tie_only_in_the_merge"
    sc = (rng.random((TWO_NQ, TWO_N)) * 0.9).astype(np.float32)
    for r, members in enumerate(((30, 30, 30, 30), (10, 60, 5, 45), (85, 5, 5, 5))):
        for s, cnt in enumerate(members):
            lo, hi = s * TWO_SEG, min((s + 1) * TWO_SEG, TWO_N)
            cols = rng.choice(np.arange(lo, hi), cnt + 10, replace=False)
            sc[r, cols[:cnt]] = 1.0
            sc[r, cols[cnt:]] = 2.0 + rng.permutation(40)[:10].astype(np.float32) + 40 * s
    return sc


@gpu
@pytest.mark.parametrize("kind", ["reversed", "perm"])
@pytest.mark.parametrize("layout", ["tie_in_every_segment", "tie_only_in_the_merge"])
def test_two_level_mapped_topk(dev, layout, kind):
    from evdr_amd import ops, _lib as L
    assert L.load().evdr_topk_workspace(TWO_NQ, TWO_N, TWO_K) > 0   # ops.topk takes the two-level form at this shape
    rng = np.random.default_rng(len(layout) * 10 + len(kind))
    sc = two_level_rows(rng, layout)
    m = make_map(rng, kind, sc)
    assert straddled(sc, TWO_K).all()
    t, tm = torch.from_numpy(sc).to(dev), torch.from_numpy(m).to(dev)
    want = rank_rule(sc, m, TWO_K)
    got = ops.topk(t, TWO_K, idx_map=tm)
    assert_ranking(got, want, (layout, kind, "two-level"))
    one = topk_one_level(t, TWO_K, tm)
    assert_ranking(one, want, (layout, kind, "one-level"))
    assert_ranking(got, one, (layout, kind, "two-level against one-level"))
    assert_ranking(ops.topk(t, TWO_K, idx_base=3), rank_rule(sc, np.arange(TWO_N) + 3, TWO_K), (layout, "unmapped"))


# ---- c. metamorphic: the answer does not depend on the order of the columns ---------------------------------------------------------
@gpu
@pytest.mark.parametrize("nq,n,ks", [(6, 300, (7, 50)), (TWO_NQ, TWO_N, (TWO_K,))])
def test_column_order_does_not_change_the_answer(dev, nq, n, ks):
    from evdr_amd import ops
    rng = np.random.default_rng(n)
    sc = np.ascontiguousarray(VALUES[rng.integers(0, len(VALUES), (nq, n))], dtype=np.float32)
    m = shuffled_rows(rng, np.arange(n) + 500, nq).astype(np.int32)                         # distinct reported indices
    for k in ks:
        first = ops.topk(torch.from_numpy(sc).to(dev), k, idx_map=torch.from_numpy(m).to(dev))
        first1 = topk_one_level(torch.from_numpy(sc).to(dev), k, torch.from_numpy(m).to(dev))
        for _ in range(3):
            p = np.stack([rng.permutation(n) for _ in range(nq)])
            ts, tm = (torch.from_numpy(np.take_along_axis(x, p, 1).copy()).to(dev) for x in (sc, m))
            assert_ranking(ops.topk(ts, k, idx_map=tm), first, (nq, n, k))
            assert_ranking(topk_one_level(ts, k, tm), first1, (nq, n, k, "one-level"))


# ---- d. merge_candidates on lists that are not rank-major --------------------------------------------------------------------------
@gpu
def test_merge_candidates_in_any_list_order(dev):
    """The corpus of test_sharded_merge_equals_single_shard (203 pages, P[50:60] = P[150:160], four shards): the per-shard top-k lists
    concatenated in reverse rank order, and shuffled, merge to the single-shard ranking.  Every k from 1 to 50, so that some cut
    falls between the two copies of a page (asserted)."""
    from evdr_amd.corpus import PageCorpus, shard_range, merge_candidates
    gen = torch.Generator().manual_seed(6)
    npg, world = 203, 4
    P = F.normalize(torch.randn(npg, 40, 128, generator=gen), dim=-1).bfloat16().to(dev)
    P[50:60] = P[150:160]
    Q = F.normalize(torch.randn(17, 32, 128, generator=gen), dim=-1).bfloat16().to(dev)
    full = PageCorpus.from_tensor(P)
    shards = []
    for r in range(world):
        lo, hi = shard_range(npg, r, world)
        shards.append(PageCorpus.from_tensor(P[lo:hi], None, idx_base=lo))
    S = host(full.score(Q, None))
    rng = np.random.default_rng(6)
    cut_rows = 0
    for k in range(1, 51):
        fs, fi = full.topk(Q, None, k)
        assert_ranking((fs, fi), rank_rule(S, np.arange(npg), k), k)
        cut_rows += int(straddled(S, k).sum())
        parts = [sh.topk(Q, None, k) for sh in shards]
        sc = torch.cat([p[0] for p in reversed(parts)], 1)
        ix = torch.cat([p[1] for p in reversed(parts)], 1)
        assert_ranking(merge_candidates(sc, ix, k), (fs, fi), (k, "reverse rank order"))
        perm = torch.from_numpy(np.stack([rng.permutation(world * k) for _ in range(Q.shape[0])])).to(dev)
        assert_ranking(merge_candidates(sc.gather(1, perm), ix.gather(1, perm), k), (fs, fi), (k, "shuffled"))
    assert cut_rows > 0


# ---- e / f. a corpus with duplicate pages --------------------------------------------------------------------------------------------
TIE_NPG, TIE_BASE = 90, 1000
TIE_NAN, TIE_BLANK, TIE_X = (5, 77), (30, 31, 32), (19, 69)


def tie_corpus(kind, lp, dev):
    """90 pages, P[10:20] = P[60:70], three identical "blank" pages (30, 31, 32), two NaN pages (5, 77); 12 queries of 7 tokens with
    ragged masks.  Built so that every k of KS cuts through a tie for some query, whatever the seed:
      * the NaN pages score NaN for every query: ranks 1 and 2 (k = 1);
      * even queries copy one token each from pages 10..16 (+ noise), so ranks 3..16 are seven tied pairs: ranks 5 | 6 are a pair (k = 5);
      * odd queries copy two tokens from the blank page and one each from pages 10..14: ranks 3..5 are the three blanks, then five
        tied pairs, ranks 12 | 13 among them (k = 12);
      * 25 pages are scaled by 1e-3 (scores ~ 0) and the pair (19, 69) by 0.3 (scores ~ 0.3 of an ordinary page's): 2 NaN + 61 ordinary
        pages rank above that pair, which sits at ranks 64 | 65 (k = 64).
    The tests assert from the reference that each k is straddled in at least one row; they do not rely on this account."""
    gen = torch.Generator().manual_seed(lp)
    P = F.normalize(torch.randn((TIE_NPG, lp, 128), generator=gen), dim=-1)
    noise = F.normalize(torch.randn((12, 7, 128), generator=gen), dim=-1)
    lens = torch.randint(lp // 2, lp + 1, (TIE_NPG,), generator=gen)
    pm = torch.arange(lp)[None, :] < lens[:, None]
    special = set(TIE_NAN) | set(TIE_BLANK) | set(range(10, 20)) | set(range(60, 70))
    plain = [p for p in range(TIE_NPG) if p not in special]
    P[plain[-25:]] *= 1e-3
    P[TIE_X[0]] *= 0.3
    P[60:70], pm[60:70] = P[10:20].clone(), pm[10:20].clone()
    for b in TIE_BLANK[1:]:
        P[b], pm[b] = P[TIE_BLANK[0]].clone(), pm[TIE_BLANK[0]].clone()
    page = torch.empty((12, 7), dtype=torch.long)
    for q in range(12):
        page[q] = torch.tensor([10 + t for t in range(7)] if q % 2 == 0 else [TIE_BLANK[0]] * 2 + [10 + t for t in range(5)])
    row = torch.arange(7)[None, :].expand(12, 7)
    Q = F.normalize(P[page, row] + 0.5 * noise, dim=-1)
    qm = torch.arange(7)[None, :] < torch.tensor([7, 7, 7, 7, 6, 5, 4, 3, 2, 1, 7, 7])[:, None]
    P[TIE_NAN[0], 0, 0] = float("nan")
    P[TIE_NAN[1], 1, 3] = float("nan")
    if kind == "bf16":
        Q, P = Q.bfloat16(), P.bfloat16()
    return Q.to(dev), qm.to(dev), P.to(dev), pm.to(dev)


def shuffled_lists(seed, nq, dev):
    """(nq, 90) int32: every page of the corpus once per query, in an order of its own."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(shuffled_rows(rng, np.arange(TIE_NPG) + TIE_BASE, nq).astype(np.int32)).to(dev)


@gpu
@pytest.mark.parametrize("kind,lp", [("f32", 33), ("bf16", 225)])
def test_rerank_of_shuffled_lists_is_the_exhaustive_topk(dev, kind, lp):
    from evdr_amd.corpus import PageCorpus, merge_candidates
    Q, qm, P, pm = tie_corpus(kind, lp, dev)
    corpus = PageCorpus.from_tensor(P, pm, idx_base=TIE_BASE)
    S = host(corpus.score(Q, qm))
    assert np.isnan(S[:, list(TIE_NAN)]).all() and np.isnan(S).sum() == 2 * 12
    a, b = corpus.shard(0, 37), corpus.shard(37, TIE_NPG)
    rng = np.random.default_rng(lp)
    for k in KS:
        cut = int(straddled(S, k).sum())
        print(f"{kind} lp={lp} k={k}: {cut} of 12 rows cut through a tie")
        assert cut >= 1, (kind, k)
        es, ei = corpus.topk(Q, qm, k)
        assert_ranking((es, ei), rank_rule(S, np.arange(TIE_NPG) + TIE_BASE, k), (kind, k, "exhaustive"))
        cand = shuffled_lists(lp + k, 12, dev)
        assert_ranking(corpus.rerank(Q, qm, cand, k), (es, ei), (kind, k, "rerank"))
        sa, ia = a.rerank(Q, qm, cand, k)
        sb, ib = b.rerank(Q, qm, cand, k)
        sc, ix = torch.cat([sa, sb], 1), torch.cat([ia, ib], 1)
        perm = torch.from_numpy(np.stack([rng.permutation(2 * k) for _ in range(12)])).to(dev)
        assert_ranking(merge_candidates(sc.gather(1, perm), ix.gather(1, perm), k), (es, ei), (kind, k, "two shard views, shuffled"))


@gpu
@pytest.mark.parametrize("kind,lp", [("f32", 33), ("bf16", 225)])
def test_internal_paths_on_the_duplicate_page_corpus(dev, kind, lp):
    """subset=, prefilter=True (fp32) and the two-stage search hand `evdr_topk` ascending lists; pinned on the same ties."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    Q, qm, P, pm = tie_corpus(kind, lp, dev)
    exact = PageCorpus.from_tensor(P, pm, idx_base=TIE_BASE)
    two = TwoStageRetriever(PageCorpus.from_tensor(P, pm, idx_base=TIE_BASE, dtype=ops.FP8), exact)
    # half of the duplicate run as whole pairs (10..14 with 60..64), the other half as single copies (15..19), two of the three blanks,
    # both NaN pages, every third other page
    pages = sorted(set(range(10, 20)) | set(range(60, 65)) | {30, 32} | set(TIE_NAN) | set(range(0, TIE_NPG, 3)))
    s = exact.subset(pages=torch.tensor(pages[::-1], device=dev) + TIE_BASE)
    assert s.m == len(pages)
    Ssub = host(exact.score(Q, qm, subset=s))
    glob = host(s.pages).astype(np.int64) + TIE_BASE
    assert glob.tolist() == [p + TIE_BASE for p in pages]
    S = host(exact.score(Q, qm))
    for k in KS:
        assert straddled(S, k).any() and (k > 5 or straddled(Ssub, k).any()), (kind, k)     # subset: NaN | NaN, and 5 | 6 of odd queries
        sub = exact.topk(Q, qm, k, subset=s)
        assert_ranking(sub, rank_rule(Ssub, glob, k), (kind, k, "subset"))
        full = exact.topk(Q, qm, k)
        if kind == "f32":
            assert_ranking(exact.topk(Q, qm, k, prefilter=True), full, (k, "prefilter"))
        assert_ranking(two.search(Q, qm, k=k, candidates=128), full, (kind, k, "two-stage"))
        assert_ranking(two.search(Q, qm, k=k, candidates=128, subset=s), sub, (kind, k, "two-stage, subset"))


# ---- g. the seeded sweep of scratch/fuzz_topk.py --------------------------------------------------------------------------------------
def fuzz_case(seed, nq=None, n=None, long_rows=True):
    """(scores (nq, n) fp32, k, description) of one seed: random shape and k, continuous or heavily quantised scores (long tie runs),
    then -0.0, NaN and +-inf sprinkled in by style.  nq / n override the drawn shape; long_rows=False keeps n <= 20 000."""
    rng = np.random.default_rng(seed)
    nq_ = int(rng.choice([1, 2, 3, 17, 64, 300]))
    n_ = int(rng.choice([1, 5, 99, 100, 101, 128, 129, 1000, 4095, 4096, 4097, 20000, 100000 if nq_ <= 3 and long_rows else 5000]))
    nq, n = nq_ if nq is None else nq, n_ if n is None else n
    k = int(rng.choice([1, 2, 10, 50, 100, 128]))
    sc = rng.standard_normal((nq, n)).astype(np.float32) * float(rng.choice([1e-3, 1.0, 1e3]))
    style = int(rng.integers(0, 5))
    if style >= 1:
        q = float(rng.choice([0.5, 2.0, 8.0]))
        sc = (np.round(sc * q / max(np.abs(sc).max(), 1e-9) * 4) / 4).astype(np.float32)      # heavy quantisation: long tie runs
    if style >= 2:
        z = sc == 0
        sc[z] = np.where(rng.random(z.sum()) < 0.5, -0.0, 0.0)
    if style >= 3:
        sc[rng.random(sc.shape) < 0.01] = np.nan
    if style >= 4:
        m = rng.random(sc.shape) < 0.01
        sc[m] = np.where(rng.random(m.sum()) < 0.5, np.inf, -np.inf)
    return sc, k, f"seed={seed} nq={nq} n={n} k={k} style={style}"


def check_fuzz_case(sc, k, seed, dev, what=""):
    """ops.topk with idx_base and with a shuffled idx_map against rank_rule; ops.topk_with_ties (device and host forms): rows whose k-th
    key is shared beyond the cut list every column at or above it, the other rows nothing."""
    from evdr_amd import ops
    nq, n = sc.shape
    t = torch.from_numpy(sc).to(dev)
    assert_ranking(ops.topk(t, k, idx_base=7), rank_rule(sc, np.arange(n) + 7, k), (what, "idx_base"))
    m = shuffled_rows(np.random.default_rng(seed + 10 ** 6), np.arange(n) + 31, nq).astype(np.int32)
    assert_ranking(ops.topk(t, k, idx_map=torch.from_numpy(m).to(dev)), rank_rule(sc, m, k), (what, "shuffled idx_map"))
    if n <= k:
        return
    key = order_key(sc).astype(np.int64)
    kth = -np.partition(-key, k - 1, axis=1)[:, k - 1]
    for form in (False, True):
        _, _, extra = ops.topk_with_ties(t, k, to_host=form)
        for r in range(nq):
            cand = np.nonzero(key[r] >= kth[r])[0]
            if len(cand) > k:
                assert r in extra, (what, form, r)
                assert np.array_equal(extra[r][0], cand) and np.array_equal(extra[r][1], sc[r, cand], equal_nan=True), (what, form, r)
            else:
                assert r not in extra, (what, form, r)


@gpu
@pytest.mark.parametrize("seed", list(range(40)))
def test_seeded_sweep(dev, seed):
    sc, k, what = fuzz_case(seed, long_rows=False)
    check_fuzz_case(sc, k, seed, dev, what)


@gpu
def test_seeded_sweep_long_rows(dev):
    sc, k, what = fuzz_case(40, nq=3, n=100001)
    check_fuzz_case(sc, k, 40, dev, what)
