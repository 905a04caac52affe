"""Growable corpora (PageCorpus.empty / append / replace / from_tensor(capacity=), ops.corpus_ingest, evdr_corpus_ingest; DESIGN.md
§4.9) against the product's own whole-tensor preparation: equal bits in planes, words and scores.  The fp32 kind laid out for a larger
absmax than the data's, and the chunked payload loader at fp32, are held to the README's parity gates against the CPU oracle."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

NPG = 11
KINDS = ("bf16", "fp32", "fp8")
LPS = (7, 33, 225)
# every kind at the three page lengths; 1030 patches once; width 64 once per kind
CASES = [(k, lp, 128) for k in KINDS for lp in LPS] + [("fp32", 1030, 128)] + [(k, 33, 64) for k in KINDS]
SCORE_GATE, GAP_GATE = 1e-4, 2e-4                                   # README "parity"


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def pages_of(lp: int, d: int = 128):
    """(P fp32 (11, lp, d), pmask): page 0 fully valid (and holding the largest finite element, 0.96875), 1 all-masked, 2 a ragged
    prefix, 3 with a hole, 4 a valid range between masked ends, 5 with a NaN in a valid patch, 6 with an Inf in a masked patch, the
    rest random masks.  Pages 5..10 are valid only in their first lp - 5 patches and zero behind: what a chunk of lp_src = lp - 5
    becomes in the corpus.  Never modified by a test."""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1000 * lp + d)
    P = F.normalize(torch.randn((NPG, lp, d), generator=gen, device=dev), dim=-1)
    pm = torch.rand((NPG, lp), generator=gen, device=dev) < 0.7
    pm[0] = True
    P[0, 0, 0] = 0.96875
    pm[1] = False
    pm[2] = torch.arange(lp, device=dev) < (lp + 1) // 2
    pm[3] = True
    pm[3, 1] = False
    pm[4] = False
    pm[4, 2:lp - 1] = True
    pm[5, 0] = True
    P[5, 0, 3] = float("nan")
    pm[6, 0], pm[6, 1] = True, False
    P[6, 1, 7] = float("inf")
    P[5:, lp - 5:] = 0.0
    pm[5:, lp - 5:] = False
    return P, pm


def cast(kind: str, P: torch.Tensor) -> torch.Tensor:
    return P.bfloat16() if kind == "bf16" else P


def reference(kind: str, P: torch.Tensor, pm: torch.Tensor, idx_base: int = 0):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    return PageCorpus.from_tensor(cast(kind, P), pm, idx_base=idx_base, dtype=ops.FP8 if kind == "fp8" else None)


def finite_absmax(P: torch.Tensor) -> float:
    a = P.float().abs()
    return float(torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max())


def empty_like_ref(kind: str, capacity: int, lp: int, dev, P: torch.Tensor, idx_base: int = 0, scale: float = 1.0):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp8": ops.FP8}[kind]
    return PageCorpus.empty(capacity, lp, dt, dev, idx_base=idx_base, absmax=scale * finite_absmax(P) if kind == "fp32" else None)


def appended(kind: str, P: torch.Tensor, pm: torch.Tensor, dev, capacity: int = NPG + 2, idx_base: int = 0, scale: float = 1.0):
    """empty + appends of 1, 4 and 6 pages; the last chunk is handed over lp - 5 patches long."""
    lp = P.shape[1]
    c = empty_like_ref(kind, capacity, lp, dev, P, idx_base, scale)
    Pk = cast(kind, P)
    assert c.append(Pk[0:1], pm[0:1]) == idx_base
    assert c.append(Pk[1:5], pm[1:5]) == idx_base + 1
    assert c.append(Pk[5:, :lp - 5], pm[5:, :lp - 5]) == idx_base + 5
    assert c.n_pages == NPG and c.capacity == capacity
    return c


def queries(kind: str, dev, d: int = 128):
    """(Q, qmask) sets: 4 x 32 with ragged masks, lq = 1, lq = 40."""
    gen = torch.Generator(device=dev).manual_seed(77)
    out = []
    for nq, lq in ((4, 32), (3, 1), (2, 40)):
        Q = F.normalize(torch.randn((nq, lq, d), generator=gen, device=dev), dim=-1)
        qm = torch.arange(lq, device=dev)[None, :] < torch.randint(1, lq + 1, (nq, 1), generator=gen, device=dev)
        out.append((cast(kind, Q), qm))
    return out


def assert_same_corpus(a, b, with_amax: bool = False):
    assert a.n_pages == b.n_pages and a.lp == b.lp and a.nplanes == b.nplanes and a.fp8 == b.fp8
    assert a.planes.dtype == b.planes.dtype
    assert torch.equal(a.planes.view(torch.uint8) if a.fp8 else a.planes.view(torch.int16), b.planes.view(torch.uint8) if b.fp8 else b.planes.view(torch.int16))
    assert torch.equal(a.tilemask, b.tilemask)
    assert torch.equal(a.pageflags, b.pageflags)
    assert (a.shift is None) == (b.shift is None)
    if a.shift is not None:
        assert torch.equal(a.shift, b.shift)
    if with_amax and a.amax is not None:
        assert torch.equal(a.amax, b.amax)


def assert_same_scores(kind: str, a, b, dev, d: int = 128):
    lst = torch.tensor([3, 0, a.n_pages, -1, a.n_pages - 1, 3], dtype=torch.int32, device=dev)
    for Q, qm in queries(kind, dev, d):
        assert torch.equal(bits(a.score(Q, qm)), bits(b.score(Q, qm)))
        (sa, ia), (sb, ib) = a.topk(Q, qm, 5), b.topk(Q, qm, 5)
        assert torch.equal(bits(sa), bits(sb)) and torch.equal(ia, ib)
        assert torch.equal(bits(a.score_pages(Q, qm, lst)), bits(b.score_pages(Q, qm, lst)))


@pytest.mark.parametrize("kind,lp,d", CASES)
def test_append_equals_prepare(dev, kind, lp, d):
    P, pm = pages_of(lp, d)
    a, b = appended(kind, P, pm, dev), reference(kind, P, pm)
    assert_same_corpus(a, b)
    assert a.planes.stride(0) != b.planes.stride(0) or a.nplanes == 1          # the plane stride of the reserved storage is in play
    assert_same_scores(kind, a, b, dev, d)


@pytest.mark.parametrize("kind,lp", [(k, lp) for k in KINDS for lp in LPS])
def test_from_tensor_with_capacity_then_append(dev, kind, lp):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    P, pm = pages_of(lp)
    dt = ops.FP8 if kind == "fp8" else None
    b = reference(kind, P, pm)
    whole = PageCorpus.from_tensor(cast(kind, P), pm, dtype=dt, capacity=NPG + 2)
    assert whole.capacity == NPG + 2 and whole.n_pages == NPG and b.capacity == b.n_pages == NPG
    assert_same_corpus(whole, b, with_amax=True)
    a = PageCorpus.from_tensor(cast(kind, P[:5]), pm[:5], dtype=dt, capacity=NPG)   # page 0 holds the absmax: the word is the whole tensor's
    assert a.append(cast(kind, P[5:]), pm[5:]) == 5
    assert_same_corpus(a, b, with_amax=True)
    assert_same_scores(kind, a, b, dev)


def oracle_scores(Q, P, qm, pm):
    from oracle import maxsim_oracle as O
    return O.maxsim_masked(Q.float().cpu(), P.float().cpu(), qm.cpu(), pm.cpu())


def assert_within_gates(corpus, Q, qm, want: torch.Tensor, k: int = 5) -> float:
    """Scores within 1e-4 of the oracle's; top-k indices equal wherever the oracle's neighbouring gaps exceed 2e-4.  Returns the deviation."""
    got = corpus.score(Q, qm).cpu()
    dev_max = float((got - want).abs().max())
    print(f"max |score - oracle| = {dev_max:.3e}")
    assert dev_max <= SCORE_GATE
    ws, wi = torch.sort(want, dim=1, descending=True, stable=True)
    gs, gi = corpus.topk(Q, qm, k)
    gi = gi.cpu() - corpus.idx_base
    gap = ws[:, :-1] - ws[:, 1:]                                                 # gap[j] between ranks j and j + 1
    big = torch.full((want.shape[0], 1), float("inf"))
    safe = (torch.cat([big, gap], 1)[:, :k] > GAP_GATE) & (torch.cat([gap, big], 1)[:, :k] > GAP_GATE)
    assert torch.equal(gi[safe].long(), wi[:, :k][safe])
    return dev_max


@pytest.mark.parametrize("lp", LPS)
def test_fp32_laid_out_two_binades_above_the_data(dev, lp):
    P, pm = pages_of(lp)
    P = torch.where(torch.isfinite(P), P, torch.zeros_like(P))                   # the oracle's NaN / Inf rules differ (include/evdr.h)
    c = appended("fp32", P, pm, dev, scale=4.0)
    ref = reference("fp32", P, pm)
    assert int(ref.amax.item()) >> 23 == (int(c.amax.item()) >> 23) - 2
    Q, qm = queries("fp32", dev)[0]
    assert_within_gates(c, Q, qm, oracle_scores(Q, P, qm, pm))


@pytest.mark.parametrize("factor", (1.0, 2.0))
def test_fp32_out_of_range_is_refused_and_the_slot_reused(dev, factor):
    lp = 33
    P, pm = pages_of(lp)
    c = empty_like_ref("fp32", NPG, lp, dev, P)
    c.append(P[0:1], pm[0:1])
    top = 2.0 ** (((int(c.amax.item()) >> 23) & 0xFF) - 126)                    # first value above the corpus's binade
    bad = P[1:5].clone()
    bad[2, 4, 9] = -factor * top                                                # 2 x the binade top (the issue's case), and the top itself
    with pytest.raises(ValueError, match="binade"):
        c.append(bad, pm[1:5])
    assert c.n_pages == 1 and c.planes.shape[1] == 1
    c.append(P[1:5], pm[1:5])
    c.append(P[5:, :lp - 5], pm[5:, :lp - 5])
    b = reference("fp32", P, pm)
    assert_same_corpus(c, b)
    assert_same_scores("fp32", c, b, dev)


@pytest.mark.parametrize("kind", KINDS)
def test_replace(dev, kind):
    lp, base = 33, 100
    P, pm = pages_of(lp)
    gen = torch.Generator(device=dev).manual_seed(5)
    new = F.normalize(torch.randn((2, lp, 128), generator=gen, device=dev), dim=-1)
    new_pm = torch.rand((2, lp), generator=gen, device=dev) < 0.6
    new_pm[:, 0] = True
    a = reference(kind, P, pm, idx_base=base)                                    # a corpus without reserved storage can be edited too
    view = a.shard(2, 9)
    sub = None if kind == "fp8" else a.subset(pages=torch.tensor([base + 3, base + 8, base + 9]))
    before = [t.clone() for t in (a.planes, a.tilemask, a.pageflags)]
    # refused before any write: duplicates, indices of another corpus, and (fp32) pages above the corpus's binade
    for pages in (torch.tensor([base + 3, base + 3]), torch.tensor([base - 1, base + 3]), torch.tensor([base + 3, base + NPG]),
                  torch.tensor([base + 8, base + 8], device=dev)):
        with pytest.raises(ValueError, match="duplicate|outside"):
            a.replace(pages, cast(kind, new), new_pm)
    if kind == "fp32":
        far = new.clone()
        far[1, 0, 0] = 4.0
        with pytest.raises(ValueError, match="binade"):
            a.replace(torch.tensor([base + 3, base + 8]), far, new_pm)
    for t, t0 in zip((a.planes, a.tilemask, a.pageflags), before):
        assert torch.equal(t.view(torch.uint8), t0.view(torch.uint8))
    a.replace(torch.tensor([base + 3]), cast(kind, new[0:1]), new_pm[0:1])
    a.replace(torch.tensor([base + 8], device=dev), cast(kind, new[1:2, :lp - 5]), new_pm[1:2, :lp - 5])
    P2, pm2 = P.clone(), pm.clone()
    P2[3], pm2[3] = new[0], new_pm[0]
    P2[8], pm2[8] = new[1], new_pm[1]
    P2[8, lp - 5:], pm2[8, lp - 5:] = 0.0, False
    b = reference(kind, P2, pm2, idx_base=base)
    assert a.n_pages == NPG
    assert_same_corpus(a, b, with_amax=True)
    assert_same_scores(kind, a, b, dev)
    Q, qm = queries(kind, dev)[0]
    assert torch.equal(bits(view.score(Q, qm)), bits(b.shard(2, 9).score(Q, qm)))
    assert view.idx_base == base + 2 and view.n_pages == 7
    if sub is not None:
        assert sub.belongs_to(a)
        assert torch.equal(bits(a.score(Q, qm, subset=sub)), bits(b.score(Q, qm, subset=b.subset(pages=torch.tensor([base + 3, base + 8, base + 9])))))


def test_prefilter_bound_follows_appends(dev):
    from evdr_amd import ops
    lp = 33
    P, pm = pages_of(lp)
    P = P.clone()
    P[:5] *= 0.1                                                                # the pages appended later have the larger norms
    c = empty_like_ref("fp32", NPG, lp, dev, P)
    c.append(P[:5], pm[:5])
    view = c.shard(0, 5)
    small = c.prefilter_bound().clone()
    c.append(P[5:], pm[5:])
    b = reference("fp32", P, pm)
    want = ops.prefilter_corpus_bound(b.planes, b.tilemask, b.pageflags)
    assert torch.equal(c.prefilter_bound(), want) and not torch.equal(small, want)
    assert torch.equal(view.prefilter_bound(), want)                            # a bound over more pages holds for every view
    Q, qm = queries("fp32", dev)[0]
    (s0, i0), (s1, i1) = c.topk(Q, qm, 3, prefilter=False), c.topk(Q, qm, 3, prefilter=True)
    assert torch.equal(bits(s0), bits(s1)) and torch.equal(i0, i1)
    c.replace(torch.tensor([0]), P[0:1] * 0.5, pm[0:1])
    assert c._pf_bound is None


@pytest.mark.parametrize("kind", KINDS)
def test_capacity(dev, kind):
    from evdr_amd.corpus import PageCorpus
    lp = 7
    P, pm = pages_of(lp)
    c = appended(kind, P, pm, dev, capacity=NPG, idx_base=40)                   # filled to exactly its capacity
    assert c.n_pages == c.capacity == NPG
    assert_same_corpus(c, reference(kind, P, pm))
    with pytest.raises(ValueError, match="capacity"):
        c.append(cast(kind, P[:1]), pm[:1])
    assert c.append(cast(kind, P[:0]), pm[:0]) == 40 + NPG and c.n_pages == NPG  # b = 0: a no-op
    with pytest.raises(ValueError, match="capacity"):
        reference(kind, P, pm).append(cast(kind, P[:1]), pm[:1])                # from_tensor without capacity= has no room
    wide = PageCorpus.from_tensor(torch.randn((3, lp, 256), device=dev))
    with pytest.raises(NotImplementedError, match="256"):
        wide.append(torch.randn((1, lp, 128), device=dev))
    with pytest.raises(NotImplementedError, match="256"):
        wide.replace(torch.tensor([0]), torch.randn((1, lp, 128), device=dev))
    with pytest.raises(NotImplementedError, match="256"):
        PageCorpus.from_tensor(torch.randn((3, lp, 256), device=dev), capacity=4)


def test_two_stage_over_grown_corpora(dev):
    from evdr_amd.corpus import TwoStageRetriever
    lp = 33
    P, pm = pages_of(lp)
    coarse, exact = appended("fp8", P, pm, dev, capacity=NPG + 1, idx_base=7), appended("bf16", P, pm, dev, capacity=NPG + 1, idx_base=7)
    ts = TwoStageRetriever(coarse, exact)
    ref = TwoStageRetriever(reference("fp8", P, pm, idx_base=7), reference("bf16", P, pm, idx_base=7))
    Q, qm = queries("bf16", dev)[0]
    (s0, i0), (s1, i1) = ts.search(Q, qm, k=3, candidates=8), ref.search(Q, qm, k=3, candidates=8)
    assert torch.equal(bits(s0), bits(s1)) and torch.equal(i0, i1)
    exact.append(P[:1].bfloat16(), pm[:1])
    with pytest.raises(ValueError, match="n_pages"):
        ts.search(Q, qm, k=3, candidates=8)
    coarse.append(P[:1], pm[:1])
    assert ts.search(Q, qm, k=3, candidates=8)[0].shape == (4, 3)


@pytest.mark.parametrize("kind", KINDS)
def test_cabi_destination_list(dev, kind):
    """evdr_corpus_ingest through its destination list into storage pre-filled with a byte pattern: a hole (-1) and an index >= capacity
    are skipped, their pages and every page not listed keep the pattern, the listed pages are from_tensor's."""
    from evdr_amd import ops
    lp, cap = 33, 9
    P, pm = pages_of(lp)
    src, spm = cast(kind, P[[0, 2, 3, 5, 6]]), pm[[0, 2, 3, 5, 6]]
    b = reference(kind, P[[0, 2, 3, 5, 6]], spm)
    dst = torch.tensor([3, -1, 0, cap + 2, 7], dtype=torch.int32, device=dev)
    pat = lambda shape, dt: torch.full(shape, 0xA5, dtype=torch.uint8, device=dev).view(dt).reshape(shape[:-1] + (-1,))  # noqa: E731
    pdt = {"bf16": torch.bfloat16, "fp32": torch.float16, "fp8": ops.FP8}[kind]
    esz = 1 if kind == "fp8" else 2
    planes = pat((b.nplanes, cap, lp, 128 * esz), pdt)
    tilemask, pageflags = pat((cap, 2 * 4), torch.int32), pat((cap * 4,), torch.int32).reshape(cap)
    shift = pat((cap * 4,), torch.int32).reshape(cap) if kind == "fp8" else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.corpus_ingest(src, spm, planes, tilemask, pageflags, shift, b.amax, first_page=0, dst_pages=dst, status=status)
    assert int(status.item()) == 0
    raw = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
    for page in range(cap):
        words = [raw(planes[:, page]), raw(tilemask[page]), raw(pageflags[page:page + 1])] + ([raw(shift[page:page + 1])] if shift is not None else [])
        if page in (3, 0, 7):
            s = {3: 0, 0: 2, 7: 4}[page]
            want = [raw(b.planes[:, s]), raw(b.tilemask[s]), raw(b.pageflags[s:s + 1])] + ([raw(b.shift[s:s + 1])] if shift is not None else [])
            assert all(torch.equal(x, y) for x, y in zip(words, want)), page
        else:
            assert all(bool((x == 0xA5).all()) for x in words), page


def test_corpus_from_payload_in_chunks(dev):
    from evdr_amd.utils.preprocess_data import corpus_from_payload
    from oracle import maxsim_oracle as O
    rng = np.random.default_rng(3)
    lens = [5, 33, 1, 20, 33, 12, 7]
    docs = np.empty(len(lens), dtype=object)
    attn = np.empty(len(lens), dtype=object)
    for i, n in enumerate(lens):
        docs[i] = rng.standard_normal((n, 128)).astype(np.float32)
        attn[i] = rng.random(n) < 0.8
    attn[1][:] = True
    a, pma = corpus_from_payload(docs, attn, None, dev, chunk_pages=3)
    b, pmb = corpus_from_payload(docs, attn, None, dev)
    assert torch.equal(pma, pmb) and a.capacity == a.n_pages == len(lens)
    assert_same_corpus(a, b)
    with pytest.raises(ValueError, match="normalize"):
        corpus_from_payload(docs, attn, None, dev, dtype=torch.float32, normalize=False, chunk_pages=3)
    f, pmf = corpus_from_payload(docs, attn, None, dev, dtype=torch.float32, chunk_pages=3)
    assert f.nplanes == 2 and int(f.amax.item()) == 0x3F800000
    P = torch.zeros((len(lens), 33, 128))
    for i, n in enumerate(lens):
        P[i, :n] = O.l2_normalize(torch.from_numpy(docs[i]) * pmf[i, :n].cpu().unsqueeze(-1))
    Q, qm = queries("fp32", dev)[0]
    assert_within_gates(f, Q, qm, oracle_scores(Q, P, qm, pmf))
