"""Prefiltered fp32 top-k (PageCorpus.topk(..., prefilter=True), evdr_maxsim_topk_prefilter): the SAME bits as the exhaustive
fp32 top-k on every case -- ragged masks, short and long pages, k = 1..100, tiny corpora, forced fallback rows, NaN / Inf inputs,
shards -- a bound E_q that holds on adversarial inputs and is tight enough to prune (DESIGN.md "Prefiltered fp32 top-k")."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # golden_recipes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaN == NaN (the positions of NaN scores are part of the answer)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def check_equal(corpus, Q, qm, k, capacity=None):
    es, ei = corpus.topk(Q, qm, k)
    ps, pi = corpus.topk(Q, qm, k, prefilter=True, capacity=capacity)
    assert torch.equal(pi, ei), (pi != ei).nonzero()[:8]
    assert same(ps, es)
    return corpus.prefilter_stats()


def ragged(gen, n, l, lo, dev):
    lens = torch.randint(lo, l + 1, (n,), generator=gen, device=dev)
    return torch.arange(l, device=dev)[None, :] < lens[:, None]


def make(gen, nq, lq, npg, lp, dev, planted=True):
    P = F.normalize(torch.randn((npg, lp, 128), generator=gen, device=dev), dim=-1)
    Q = F.normalize(torch.randn((nq, lq, 128), generator=gen, device=dev), dim=-1)
    if planted and npg > 0:                          # a few queries lie near a page, like the bench's planted queries
        t = torch.randint(0, npg, (nq,), generator=gen, device=dev)
        rows = torch.randint(0, lp, (nq, lq), generator=gen, device=dev)
        Q = F.normalize(P[t[:, None], rows] + 0.5 * Q, dim=-1)
    return Q, P


@pytest.mark.parametrize("nq,lq,npg,lp,k,cap", [
    (40, 32, 300, 33, 10, None),
    (37, 7, 250, 7, 100, None),
    (70, 1, 500, 33, 10, None),                      # single-token queries: the coarse pass packs 32 to a tile
    (9, 32, 2500, 1030, 100, None),                  # a few thousand long pages
    (33, 7, 1200, 1030, 1, None),
    (12, 32, 60, 33, 100, None),                     # n_pages < k
    (20, 7, 150, 1030, 10, 150),                     # n_pages <= capacity
])
def test_bit_equal_to_the_exhaustive_top_k(dev, nq, lq, npg, lp, k, cap):
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(nq * 1000 + npg)
    Q, P = make(gen, nq, lq, npg, lp, dev)
    pm = ragged(gen, npg, lp, max(1, lp // 2), dev)
    qm = ragged(gen, nq, lq, 1, dev)
    st = check_equal(PageCorpus.from_tensor(P, pm), Q, qm, k, cap)
    assert st["queries"] == nq


def test_config1_against_the_reference_itself(dev, golden):
    """configs[1] (500 x 500 x 1030, ragged pages, masked query tails): the prefiltered top-100 is the exhaustive fp32 top-100 bit
    for bit, and its indices are the reference's own ranking wherever the reference's gap exceeds 2e-4."""
    import golden_recipes as R
    from oracle import maxsim_oracle as O
    from evdr_amd.corpus import PageCorpus
    want = torch.from_numpy(golden("config1_full")["scores"])
    Q, P, qm, pm, _ = R.config1_case()
    ws, wi = O.topk_rows(want, 100)
    gap_ok = (ws[:, :-1] - ws[:, 1:]) > 2e-4
    safe = torch.cat([gap_ok, gap_ok[:, -1:]], 1) & torch.cat([gap_ok[:, :1], gap_ok], 1)
    corpus = PageCorpus.from_tensor(P.to(dev), pm.to(dev))
    check_equal(corpus, Q.to(dev), qm.to(dev), 100)
    _, pi = corpus.topk(Q.to(dev), qm.to(dev), 100, prefilter=True)
    assert torch.equal(pi.cpu()[safe], wi[safe].to(torch.int32))


def _bound_case(dev, Q, P, qm, pm):
    """(exact, coarse, E) of one corpus / query set through the entries of the two passes and of the bound."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    c = PageCorpus.from_tensor(P, pm)
    qp, qa = ops.split_f32(Q)
    exact = c.score(Q, qm)
    coarse = ops.maxsim_forward_coarse(qp, qa, c.planes, c.amax, qm, c.tilemask, c.pageflags)
    E = ops.prefilter_query_bound(qp, qa, c.amax, qm, c.prefilter_bound())
    return exact, coarse, E


def test_the_bound_holds_on_adversarial_inputs(dev):
    """|exact - coarse| <= E_q for every pair: elements at fp16 rounding midpoints (|lo| as large as it gets), rows with norms from
    1e-3 to 1e3, one-hot rows, masked patches and all-masked pages."""
    gen = torch.Generator(device=dev).manual_seed(77)
    nq, lq, npg, lp = 24, 32, 160, 70

    def midpoints(x):
        # a midpoint of the fp16 grid after the planes' power-of-two scaling: the value itself sits halfway between two fp16 numbers
        h = x.half().float()
        _, e = torch.frexp(h)                          # |h| = m 2^e, m in [0.5, 1): the fp16 spacing there is 2^(e - 11)
        ulp = torch.ldexp(torch.ones_like(h), (e - 11).float())
        return h + 0.5 * ulp * torch.sign(torch.randn(x.shape, generator=gen, device=dev))
    P = torch.randn((npg, lp, 128), generator=gen, device=dev)
    Q = torch.randn((nq, lq, 128), generator=gen, device=dev)
    P = P * torch.logspace(-3, 3, npg * lp, device=dev).view(npg, lp, 1)[:, torch.randperm(lp, generator=gen, device=dev)] / 11.3
    Q = Q * torch.logspace(-3, 3, nq * lq, device=dev).view(nq, lq, 1) / 11.3
    P[:20] = F.normalize(P[:20], dim=-1)
    P[5, :, :] = 0.0
    P[5, torch.arange(lp, device=dev), torch.arange(lp, device=dev) % 128] = 1.0          # one-hot rows
    Q[3] = 0.0
    Q[3, torch.arange(lq, device=dev), (7 * torch.arange(lq, device=dev)) % 128] = 1.0
    P[20:40], Q[:6] = midpoints(P[20:40]), midpoints(Q[:6])
    # inputs the fp16 split scales as a whole: one tensor mixes magnitudes 1e-3..1e3 and rounds at midpoints (scaled by their own k)
    pm = ragged(gen, npg, lp, 1, dev)
    pm[7] = False                                     # all masked
    pm[9, ::3] = False                                # holes
    qm = ragged(gen, nq, lq, 1, dev)
    exact, coarse, E = _bound_case(dev, Q, P, qm, pm)
    ok = ~torch.isnan(exact)
    assert torch.equal(torch.isnan(exact), torch.isnan(coarse))
    diff = (exact.double() - coarse.double()).abs()
    assert bool((diff[ok] <= E.double()[:, None].expand_as(diff)[ok]).all()), (diff - E[:, None]).max()
    # midpoint rows alone (unit scale): the inputs where |lo| is largest relative to |hi|
    Pm = midpoints(F.normalize(torch.randn((60, 33, 128), generator=gen, device=dev), dim=-1))
    Qm = midpoints(F.normalize(torch.randn((16, 32, 128), generator=gen, device=dev), dim=-1))
    exact, coarse, E = _bound_case(dev, Qm, Pm, None, None)
    assert bool(((exact - coarse).abs() <= E[:, None]).all())
    assert float((exact - coarse).abs().max()) > 0.0                      # the two passes really differ


def test_the_bound_is_tight_enough_to_prune(dev):
    """Unit-norm rows: E_q <= Lq * 2^-9.  Seeded random unit-norm data at 256 x 6 847 x 1030, k = 100: mean candidate count
    below MAX_FRACTION of the corpus, and the answer is bit-equal.  Measured on MI355X: max E_q = 0.0176 (32 * 2^-10.8), candidates
    135 / 160.6 / 188 (min / mean / max) = 2.35 % of the corpus; MAX_FRACTION = that with a 2x margin."""
    from evdr_amd.corpus import PageCorpus
    MAX_FRACTION = 0.047
    gen = torch.Generator(device=dev).manual_seed(6847)
    Q, P = make(gen, 256, 32, 6847, 1030, dev, planted=False)
    corpus = PageCorpus.from_tensor(P)
    del P
    from evdr_amd import ops
    qp, qa = ops.split_f32(Q)
    E = ops.prefilter_query_bound(qp, qa, corpus.amax, None, corpus.prefilter_bound())
    assert float(E.max()) <= 32 * 2.0 ** -9, float(E.max())
    st = check_equal(corpus, Q, None, 100)
    print("tightness", float(E.max()), st)
    assert st["fallback_rows"] == 0
    assert st["candidates_mean"] < MAX_FRACTION * 6847, st


def test_fallback_rows_stay_exact(dev):
    """capacity = k on a corpus of near-duplicate pages: rows fall back to the exhaustive pass, prefilter_stats() reports them,
    and the answer is still the exhaustive one."""
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(5)
    base = F.normalize(torch.randn((1, 33, 128), generator=gen, device=dev), dim=-1)
    P = F.normalize(base + 1e-4 * torch.randn((400, 33, 128), generator=gen, device=dev), dim=-1)
    Q = F.normalize(base[:, :16].expand(20, -1, -1) + 0.3 * torch.randn((20, 16, 128), generator=gen, device=dev), dim=-1)
    Q[:10] = F.normalize(torch.randn((10, 16, 128), generator=gen, device=dev), dim=-1)
    st = check_equal(PageCorpus.from_tensor(P), Q, None, 10, capacity=10)
    assert st["fallback_rows"] > 0 and st["capacity"] == 10, st


def test_non_finite_inputs_land_where_the_exhaustive_path_puts_them(dev):
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(11)
    Q, P = make(gen, 30, 16, 300, 40, dev)
    pm = ragged(gen, 300, 40, 20, dev)
    P[4, 2, 7] = float("nan")                        # valid patch: page 4 scores NaN
    P[8, 0, 1] = float("inf")
    P[12, 39, 3] = float("nan")
    pm[12, 39] = False                               # ... in a masked patch: ignored
    pm[15] = False                                   # all masked
    qm = ragged(gen, 30, 16, 4, dev)
    Q[2, 0, 5] = float("nan")                        # valid token
    Q[6, 15, 0] = float("nan")
    qm[6, 15] = False                                # masked token: still NaN, like the reference
    corpus = PageCorpus.from_tensor(P, pm)
    for k in (1, 10, 100):
        check_equal(corpus, Q, qm, k)


def test_shards_merge_to_the_single_corpus_answer(dev):
    from evdr_amd.corpus import PageCorpus, ShardedRetriever, merge_candidates
    gen = torch.Generator(device=dev).manual_seed(3)
    Q, P = make(gen, 50, 32, 900, 70, dev)
    pm = ragged(gen, 900, 70, 30, dev)
    full = PageCorpus.from_tensor(P, pm)
    es, ei = full.topk(Q, None, 100)
    parts = [ShardedRetriever(full.shard(lo, hi)).search(Q, None, 100, prefilter=True) for lo, hi in ((0, 300), (300, 610), (610, 900))]
    ms, mi = merge_candidates(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), 100)
    assert torch.equal(mi, ei) and same(ms, es)
    assert full.shard(0, 300).prefilter_bound() is full._pf_bound


def test_c_abi_direct(dev):
    """evdr_maxsim_topk_prefilter through ctypes with torch-allocated buffers == evdr_maxsim_topk on the same planes."""
    from evdr_amd import _lib as L, ops
    from evdr_amd.corpus import PageCorpus
    gen = torch.Generator(device=dev).manual_seed(19)
    Q, P = make(gen, 21, 32, 700, 100, dev)
    c = PageCorpus.from_tensor(P)
    qp, qa = ops.split_f32(Q)
    bound = torch.empty(2, dtype=torch.float32, device=dev)
    lib = L.load()
    s = L.current_stream_handle(dev)
    nq, np_, lp, k, cap = 21, 700, 100, 50, 300
    L.check(lib.evdr_prefilter_corpus_bound(L.ptr(c.planes), L.ptr(c.tilemask), L.ptr(c.pageflags), np_, lp, c.p_stride, c.p_plane_stride,
                                            L.ptr(bound), s))
    ws = torch.empty(lib.evdr_maxsim_topk_prefilter_workspace(nq, np_, cap), dtype=torch.uint8, device=dev)
    ts, ti = torch.empty((nq, k), device=dev), torch.empty((nq, k), dtype=torch.int32, device=dev)
    L.check(lib.evdr_maxsim_topk_prefilter(L.ptr(qp), L.ptr(c.planes), None, L.ptr(c.tilemask), L.ptr(c.pageflags), nq, 32, np_, lp, 2,
                                           c.p_stride, c.p_plane_stride, L.ptr(qa), L.ptr(c.amax), L.ptr(bound), 1000, k, cap, L.ptr(ts),
                                           L.ptr(ti), None, L.ptr(ws), ws.numel(), s))
    ws2 = torch.empty(lib.evdr_maxsim_topk_workspace(nq, np_), dtype=torch.uint8, device=dev)
    es, ei = torch.empty_like(ts), torch.empty_like(ti)
    L.check(lib.evdr_maxsim_topk(L.ptr(qp), L.ptr(c.planes), None, L.ptr(c.tilemask), L.ptr(c.pageflags), nq, 32, np_, lp, 2, c.p_stride,
                                 c.p_plane_stride, L.ptr(qa), L.ptr(c.amax), 1000, k, L.ptr(es), L.ptr(ei), L.ptr(ws2), ws2.numel(), s))
    assert torch.equal(ti, ei) and same(ts, es)
