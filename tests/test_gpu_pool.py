"""Pooled corpora on the GPU (csrc/pool.hip; ops.pool_pages, PageCorpus.from_pooled / append_pooled / replace_pooled; DESIGN.md
§4.10): the fused kernel against ops.pool_reference run on the CPU (equal bits), a pooled corpus against the existing ingest path fed
with the pooled pages (equal bits in planes, words and scores), growth and replacement, the fp32 refusals, and the pooled corpus as
the first stage of a two-stage search."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

N = 5
KINDS = ("bf16", "fp32", "fp8")
GROUPINGS = ("win7", "win33", "win225", "grid227", "perpage33")
# width 128, width 64 (whole octets of zero columns), width 20 (rows not 16-byte aligned: element-wise access), every source dtype
SOURCES = ((128, torch.float32), (64, torch.bfloat16), (20, torch.float16), (128, torch.bfloat16))


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def grouping(name: str):
    """(lp_src, members, offsets) on the CPU.  win*: windows of 3 / 4 / 4 patches (ls = 3 / 9 / 57, ragged last window); grid227: a
    15 x 15 grid from patch 1 in 3 x 3 blocks plus one extra patch in front and one behind (ls = 27); perpage33: per-page random lists
    of 40 members in [-3, 36) -- holes on both sides, repeated patches -- under random offsets with empty groups that stop short of
    the list's end (ls = 9)."""
    from evdr_amd import ops
    if name.startswith("win"):
        lp = int(name[3:])
        return (lp,) + ops.pool_groups_windows(lp, 3 if lp == 7 else 4)
    if name == "grid227":
        return (227,) + ops.pool_groups_grid(15, 15, 3, 3, first=1, lp=227)
    gen = torch.Generator().manual_seed(33)
    members = torch.randint(-3, 36, (N, 40), generator=gen, dtype=torch.int32)
    cuts = torch.sort(torch.randint(0, 38, (N, 9), generator=gen), dim=1).values
    cuts[:, 3] = cuts[:, 2]                                           # an empty group in every page
    offsets = torch.cat([torch.zeros(N, 1, dtype=torch.int64), cuts], dim=1).to(torch.int32)
    return 33, members, offsets


@functools.lru_cache(maxsize=None)
def source(name: str, d: int, dtype: torch.dtype):
    """(P (5, lp_src, d) of `dtype`, pmask) on the CPU, never modified: page 0 fully valid, page 1 all masked, page 2 with its first
    group masked out, the rest masked at random."""
    lp, _, off = grouping(name)
    gen = torch.Generator().manual_seed(1000 * lp + d)
    P = torch.randn((N, lp, d), generator=gen).to(dtype)
    pm = torch.rand((N, lp), generator=gen) < 0.7
    pm[0] = True
    pm[1] = False
    pm[2, : max(int(off.reshape(-1, off.shape[-1])[0, 1]), 1)] = False
    return P, pm


@functools.lru_cache(maxsize=None)
def expected(name: str, d: int, dtype: torch.dtype, normalize: bool):
    """ops.pool_reference on the CPU: computed once per case, shared, never modified."""
    from evdr_amd import ops
    _, mem, off = grouping(name)
    P, pm = source(name, d, dtype)
    return ops.pool_reference(P, pm, mem, off, normalize=normalize)


# ---- 1. the kernel against the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", SOURCES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("name", GROUPINGS)
def test_pool_pages_equals_reference(dev, name, d, dtype):
    from evdr_amd import ops
    lp, mem, off = grouping(name)
    P, pm = source(name, d, dtype)
    for normalize in (False, True):
        want, wmask = expected(name, d, dtype, normalize)
        got, gmask = ops.pool_pages(P.to(dev), pm.to(dev), mem, off, normalize=normalize)
        assert got.dtype == torch.float32 and gmask.dtype == torch.bool and tuple(got.shape) == (N, off.shape[-1] - 1, d)
        assert torch.equal(gmask.cpu(), wmask), (name, normalize)
        diff = (bits(got.cpu()) - bits(want)).abs()
        print(f"{name} d={d} {dtype} normalize={normalize}: {int((diff != 0).sum())} of {diff.numel()} words differ, max {int(diff.max())} ulp")
        assert torch.equal(bits(got.cpu()), bits(want)), (name, normalize)
    if name == "win33":                                               # no mask = every patch valid; groupings given on the device
        want, wmask = ops.pool_reference(P, None, mem, off)
        got, gmask = ops.pool_pages(P.to(dev), None, mem.to(dev), off.to(dev).long())
        assert torch.equal(bits(got.cpu()), bits(want)) and torch.equal(gmask.cpu(), wmask) and bool(wmask.all())


# ---- 2. a pooled corpus against the ingest path fed with the pooled pages ---------------------------------------------------------------
def corpus_dtype(kind: str):
    from evdr_amd import ops
    return {"bf16": torch.bfloat16, "fp32": torch.float32, "fp8": ops.FP8}[kind]


def via_append(kind: str, Pbar: torch.Tensor, mask: torch.Tensor, dev, lp=None, capacity=None, absmax=1.0, idx_base=0):
    """The existing path: PageCorpus.empty + append of the plain pooled pages (rounded by .bfloat16() for a bf16 corpus)."""
    from evdr_amd.corpus import PageCorpus
    c = PageCorpus.empty(Pbar.shape[0] if capacity is None else capacity, Pbar.shape[1] if lp is None else lp, corpus_dtype(kind), dev,
                         idx_base=idx_base, absmax=absmax if kind == "fp32" else None)
    c.append(Pbar.bfloat16() if kind == "bf16" else Pbar, mask)
    return c


def assert_same_corpus(a, b):
    assert a.n_pages == b.n_pages and a.lp == b.lp and a.nplanes == b.nplanes and a.fp8 == b.fp8 and a.planes.dtype == b.planes.dtype
    view = torch.uint8 if a.fp8 else torch.int16
    assert torch.equal(a.planes.view(view), b.planes.view(view))
    assert torch.equal(a.tilemask, b.tilemask)
    assert torch.equal(a.pageflags, b.pageflags)
    assert (a.shift is None) == (b.shift is None) and (a.shift is None or torch.equal(a.shift, b.shift))
    assert (a.amax is None) == (b.amax is None) and (a.amax is None or torch.equal(a.amax, b.amax))


def queries(kind: str, dev, d: int):
    gen = torch.Generator(device=dev).manual_seed(77)
    Q = F.normalize(torch.randn((3, 8, d), generator=gen, device=dev), dim=-1)
    qm = torch.arange(8, device=dev)[None, :] < torch.tensor([[8], [3], [5]], device=dev)
    return (Q.bfloat16() if kind == "bf16" else Q), qm


def assert_same_scores(kind: str, a, b, dev, d: int):
    Q, qm = queries(kind, dev, d)
    lst = torch.tensor([3, 0, a.n_pages, -1, a.n_pages - 1, 3], dtype=torch.int32, device=dev)
    assert torch.equal(bits(a.score(Q, qm)), bits(b.score(Q, qm)))
    (sa, ia), (sb, ib) = a.topk(Q, qm, 3), b.topk(Q, qm, 3)
    assert torch.equal(bits(sa), bits(sb)) and torch.equal(ia, ib)
    assert torch.equal(bits(a.score_pages(Q, qm, lst)), bits(b.score_pages(Q, qm, lst)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,d,dtype", [("win7", 128, torch.float32), ("win33", 128, torch.bfloat16), ("win225", 64, torch.bfloat16),
                                          ("grid227", 128, torch.float16), ("perpage33", 20, torch.float16), ("perpage33", 128, torch.float32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_from_pooled_equals_append_of_pooled_pages(dev, kind, name, d, dtype):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    _, mem, off = grouping(name)
    P, pm = (t.to(dev) for t in source(name, d, dtype))
    a = PageCorpus.from_pooled(P, pm, mem, off, dtype=corpus_dtype(kind), idx_base=40)
    b = via_append(kind, *ops.pool_pages(P, pm, mem, off), dev, idx_base=40)
    assert a.lp == off.shape[-1] - 1 and a.capacity == a.n_pages == N and a.idx_base == 40
    assert_same_corpus(a, b)
    assert_same_scores(kind, a, b, dev, d)
    if kind != "fp32":                                                # unnormalised means: the same bits again (fp32 needs a bound: test 4)
        a = PageCorpus.from_pooled(P, pm, mem, off, dtype=corpus_dtype(kind), normalize=False)
        assert_same_corpus(a, via_append(kind, *ops.pool_pages(P, pm, mem, off, normalize=False), dev))


def test_from_pooled_default_kind(dev):
    from evdr_amd.corpus import PageCorpus
    _, mem, off = grouping("win33")
    P, pm = (t.to(dev) for t in source("win33", 128, torch.bfloat16))
    c = PageCorpus.from_pooled(P, pm, mem, off)
    assert c.nplanes == 1 and c.planes.dtype == torch.bfloat16 and c.amax is None
    c = PageCorpus.from_pooled(P.float(), pm, mem, off)
    assert c.nplanes == 2 and int(c.amax.item()) == 0x3F800000        # unit vectors: laid out for absmax = 1.0


# ---- 3. growth and replacement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ("win33", "perpage33"))
def test_append_and_replace_pooled(dev, kind, name):
    from evdr_amd.corpus import PageCorpus
    _, mem, off = grouping(name)
    P, pm = (t.to(dev) for t in source(name, 128, torch.float32))
    rows = (lambda t, sel: t[sel]) if mem.dim() == 2 else (lambda t, sel: t)      # a per-page grouping goes with its pages
    dt = corpus_dtype(kind)
    c = PageCorpus.from_pooled(P[:2], pm[:2], rows(mem, slice(0, 2)), rows(off, slice(0, 2)), dtype=dt, capacity=N + 1, idx_base=10)
    view = c.shard(0, 2)                                              # made before the pages change
    assert c.append_pooled(P[2:], pm[2:], rows(mem, slice(2, N)), rows(off, slice(2, N))) == 12
    assert c.n_pages == N and c.capacity == N + 1
    full = PageCorpus.from_pooled(P, pm, mem, off, dtype=dt, idx_base=10)
    assert_same_corpus(c, full)
    assert_same_scores(kind, c, full, dev, 128)
    # pages 1 and 3 take the pooled pages of source pages 4 and 0 (a device list of global indices, out of order)
    sel = [4, 0]
    c.replace_pooled(torch.tensor([13, 11], device=dev), P[sel], pm[sel], rows(mem, sel), rows(off, sel))
    order = [0, 0, 2, 4, 4]
    final = PageCorpus.from_pooled(P[order], pm[order], rows(mem, order), rows(off, order), dtype=dt, idx_base=10)
    assert_same_corpus(c, final)
    assert_same_corpus(view, final.shard(0, 2))                       # the earlier view sees the new content
    assert_same_scores(kind, c, final, dev, 128)
    # a pooled page shorter than the corpus's pages is padded with masked zero tokens
    _, mem7, off7 = grouping("win7")
    P7, pm7 = (t.to(dev) for t in source("win7", 128, torch.float32))
    e = PageCorpus.empty(N, 9, dt, dev, absmax=1.0 if kind == "fp32" else None)
    e.append_pooled(P7, pm7, mem7, off7)
    from evdr_amd import ops
    assert_same_corpus(e, via_append(kind, *ops.pool_pages(P7, pm7, mem7, off7), dev, lp=9))


@pytest.mark.parametrize("kind", KINDS)
def test_destination_list_with_holes(dev, kind):
    """ops.corpus_pool_ingest (evdr_corpus_pool_ingest) through its destination list into storage pre-filled with a byte pattern: a
    hole (-1) and an index >= capacity are skipped, their pages and every page not listed keep the pattern, the listed pages are
    from_pooled's."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    lp_src, mem, off = grouping("win33")
    P, pm = (t.to(dev) for t in source("win33", 128, torch.float32))
    ls, cap = off.shape[0] - 1, 9
    b = PageCorpus.from_pooled(P, pm, mem, off, dtype=corpus_dtype(kind))
    dst = torch.tensor([3, -1, 0, cap + 2, 7], dtype=torch.int32, device=dev)
    pat = lambda shape, dt: torch.full(shape, 0xA5, dtype=torch.uint8, device=dev).view(dt).reshape(shape[:-1] + (-1,))  # noqa: E731
    pdt = {"bf16": torch.bfloat16, "fp32": torch.float16, "fp8": ops.FP8}[kind]
    esz = 1 if kind == "fp8" else 2
    planes = pat((b.nplanes, cap, ls, 128 * esz), pdt)
    tilemask, pageflags = pat((cap, 1 * 4), torch.int32), pat((cap * 4,), torch.int32).reshape(cap)
    shift = pat((cap * 4,), torch.int32).reshape(cap) if kind == "fp8" else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.corpus_pool_ingest(P, pm, mem, off, planes, tilemask, pageflags, shift, b.amax, first_page=0, dst_pages=dst, status=status)
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


# ---- 4. the fp32 kind ---------------------------------------------------------------------------------------------------------------------
def test_fp32_refuses_a_pooled_element_above_the_binade(dev):
    from evdr_amd.corpus import PageCorpus
    _, mem, off = grouping("win33")
    P, pm = (t.to(dev) for t in source("win33", 128, torch.float32))
    small = F.normalize(P, dim=-1) * 0.5                              # every mean below 0.5: fits a corpus laid out for absmax = 0.5
    big = small.clone()
    big[3, 4:8] = 0.75                                                # one group's mean is 0.75 wherever it has a valid member
    pmb = pm.clone()
    pmb[3, 4] = True
    with pytest.raises(ValueError, match="binade"):
        PageCorpus.from_pooled(big, pmb, mem, off, normalize=False, absmax=0.4)
    with pytest.raises(ValueError, match="absmax"):
        PageCorpus.from_pooled(big, pmb, mem, off, normalize=False)  # unnormalised means have no default bound
    c = PageCorpus.from_pooled(small, pm, mem, off, normalize=False, absmax=0.4, capacity=2 * N)
    assert c.n_pages == N and int(c.amax.item()) == int(bits(torch.tensor([0.4]))[0])
    before = [t.clone() for t in (c.planes, c.tilemask, c.pageflags)]
    with pytest.raises(ValueError, match="binade"):
        c.append_pooled(big, pmb, mem, off, normalize=False)
    assert c.n_pages == N and all(torch.equal(x, y) for x, y in zip(before, (c.planes, c.tilemask, c.pageflags)))
    store = [t.clone() for t in c._store[:3]]
    with pytest.raises(ValueError, match="binade"):
        c.replace_pooled(torch.tensor([0, 1, 2, 3, 4]), big, pmb, mem, off, normalize=False)
    assert all(torch.equal(x, y) for x, y in zip(store, c._store[:3]))                # bit-unchanged, the slots behind n_pages too
    c.replace_pooled(torch.tensor([4, 3]), small[[0, 1]], pm[[0, 1]], mem, off, normalize=False)
    want = PageCorpus.from_pooled(small[[0, 1, 2, 1, 0]], pm[[0, 1, 2, 1, 0]], mem, off, normalize=False, absmax=0.4)
    assert_same_corpus(c, want)
    # renormalised, the same pages fit the default layout (absmax = 1.0) whatever their scale
    assert PageCorpus.from_pooled(big * 100.0, pmb, mem, off).n_pages == N


@pytest.mark.parametrize("kind", KINDS)
def test_nonfinite_member_sets_the_flag_bit(dev, kind):
    from evdr_amd.corpus import PageCorpus
    _, mem, off = grouping("win33")
    P, pm = (t.clone().to(dev) for t in source("win33", 128, torch.float32))
    P[0, 5, 3] = float("inf")                                         # page 0, a valid patch of group 1
    P[2, 0, 0] = float("nan")                                         # page 2, a MASKED patch: skipped, the page stays clean
    P[3, 32, 9] = float("-inf")                                       # page 3, the ragged last group
    pm[3, 32] = True
    for normalize in (True, False):
        c = PageCorpus.from_pooled(P, pm, mem, off, dtype=corpus_dtype(kind), normalize=normalize, absmax=8.0 if kind == "fp32" else None)
        assert ((c.pageflags & 8) != 0).tolist() == [True, False, False, True, False]
        Q, qm = queries(kind, dev, 128)
        s = c.score(Q, qm)
        assert bool(torch.isnan(s[:, [0, 3]]).all()) and bool(torch.isfinite(s[:, [2, 4]]).all())


# ---- 5. the pooled corpus as a first stage ---------------------------------------------------------------------------------------------------
def test_two_stage_with_every_page_a_candidate(dev):
    """Groups of 4 identical patches, unnormalised means: the pooled corpus holds the pages' own patches once each, so it scores what
    the exact corpus scores, and with every page a candidate the two-stage search IS the exhaustive top-k."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    n, ls = 12, 8
    gen = torch.Generator(device=dev).manual_seed(9)
    base = F.normalize(torch.randn((n, ls, 128), generator=gen, device=dev), dim=-1)
    P = base.repeat_interleave(4, dim=1)                              # (n, 32, 128)
    pm = torch.ones((n, 32), dtype=torch.bool, device=dev)
    pm[1, 4:8] = False                                                # a whole group masked: a masked pooled token
    pm[2, 9] = False                                                  # one member masked: the mean of the other three is the same patch
    mem, off = ops.pool_groups_windows(32, 4)
    exact = PageCorpus.from_tensor(P, pm, idx_base=20, capacity=n)
    # laid out for the exact corpus's own absmax: the same power of two, so a pooled token's planes are its patch's planes
    pooled = PageCorpus.from_pooled(P, pm, mem, off, normalize=False, absmax=float(P.abs().max()), idx_base=20)
    assert pooled.lp == ls and torch.equal(bits(ops.pool_pages(P, pm, mem, off, normalize=False)[0][0]), bits(base[0]))
    Q = F.normalize(torch.randn((3, 8, 128), generator=gen, device=dev), dim=-1)
    qm = torch.arange(8, device=dev)[None, :] < torch.tensor([[8], [2], [6]], device=dev)
    gap = (pooled.score(Q, qm) - exact.score(Q, qm)).abs().max().item()
    print(f"max |pooled - exact| = {gap:.3g}")
    assert gap <= 1e-5
    ts = TwoStageRetriever(pooled, exact)
    want = exact.topk(Q, qm, 3)
    got = ts.search(Q, qm, k=3, candidates=n)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])
    allow = torch.ones(n, dtype=torch.bool, device=dev)
    allow[[0, 5, 6]] = False
    sub = exact.subset(allow=allow)
    want = exact.topk(Q, qm, 3, subset=sub)
    got = ts.search(Q, qm, k=3, candidates=n, subset=sub)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("kind", KINDS)
def test_two_stage_finds_planted_pages(dev, kind):
    """64 pages of random unit patches pooled in windows of 4; query q holds eight pooled tokens of page q.  The pooled pass ranks
    page q first by a wide margin (8 exact matches against random cosines), the exact rerank of 8 candidates keeps it first (each
    token has cosine ~0.5 with the four members of its group, ~0.25 at most with anything else)."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    n = 64
    gen = torch.Generator(device=dev).manual_seed(11)
    P = F.normalize(torch.randn((n, 32, 128), generator=gen, device=dev), dim=-1)
    mem, off = ops.pool_groups_windows(32, 4)
    Q = ops.pool_pages(P, None, mem, off)[0]                          # (64, 8, 128): unit vectors
    if kind == "bf16":
        P, Q = P.bfloat16(), Q.bfloat16()
    exact = PageCorpus.from_tensor(P)
    pooled = PageCorpus.from_pooled(P, None, mem, off, dtype=corpus_dtype(kind))
    top, idx = TwoStageRetriever(pooled, exact).search(Q, None, k=3, candidates=8)
    assert idx[:, 0].tolist() == list(range(n))
    assert torch.allclose(top[:, 0], exact.topk(Q, None, 1)[0][:, 0], rtol=0, atol=1e-4)       # the exact corpus's own score of that page
