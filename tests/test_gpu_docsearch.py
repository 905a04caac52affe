"""Document-level search on the GPU: evdr_doc_max and evdr_collapse_topk against ops.doc_max_reference /
ops.doc_reference / ops.collapse_reference on both sides of every geometry constant, and the Python paths end to end.  Every
comparison is bit equality (docsearch_cases.assert_bits): no tolerance anywhere."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import docsearch_cases as C

gpu = pytest.mark.gpu
pytestmark = gpu


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def dt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def strided(sc, dev, pad=7):
    """(nq, n) host scores -> a device view with row_stride = n + pad (the padding holds NaN: never to be read as a member)."""
    nq, n = sc.shape
    buf = torch.full((nq, n + pad), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :n] = dt(sc, dev)
    return buf[:, :n]


def list_reference(sc, lists, idx_map, idx_base):
    """ops.doc_max_reference for CSR lists of any kind (duplicates, holes, a column in several documents): every valid member becomes
    a column of its own, carrying its score column, its document and the index it reports."""
    from evdr_amd import ops
    n = sc.shape[1]
    mem, off = C.csr(lists)
    docof = np.repeat(np.arange(len(lists)), np.diff(off))
    ok = (mem >= 0) & (mem < n)
    cols = mem[ok].astype(np.int64)
    rep = (idx_map[cols].astype(np.int64) if idx_map is not None else cols) + idx_base
    return ops.doc_max_reference(torch.from_numpy(np.ascontiguousarray(sc[:, cols])), torch.from_numpy(docof[ok]), len(lists),
                                 torch.from_numpy(rep))


def run_doc_max(dev, sc, lists, idx_map=None, idx_base=0):
    from evdr_amd import ops
    mem, off = C.csr(lists)
    return ops.doc_max(strided(sc, dev), dt(mem, dev), dt(off, dev), None if idx_map is None else dt(idx_map, dev), idx_base)


def maps_for(rng, n):
    """idx_map variants: none; descending, so that the lowest reported index is the LAST column; a random injective map."""
    return [("none", None), ("descending", ((n - 1 - np.arange(n)) * 2 + 5).astype(np.int32)),
            ("shuffled", (rng.permutation(n) * 3).astype(np.int32))]


# ---- evdr_doc_max -----------------------------------------------------------------------------------------------------------------
def special_sizes():
    from evdr_amd import ops
    return [0, 1, 2, 3, 63, 64, 65, ops.DOC_LONG - 1, ops.DOC_LONG, ops.DOC_LONG + 1]


def doc_block_sizes():
    from evdr_amd import ops
    return [1, ops.DOC_BLOCK - 1, ops.DOC_BLOCK, ops.DOC_BLOCK + 1]


@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("nd_i", [0, 1, 2, 3])
def test_doc_max_is_the_reference(dev, n, nd_i):
    """nq on both sides of DOC_ROWS, n_docs on both sides of DOC_BLOCK, document sizes on both sides of DOC_LONG (and 0, 1, 63..65), a
    long document on either side of the workgroup's document range, one document holding every page; members ascending,
    descending and shuffled, with duplicates and out-of-range holes added; with and without idx_map; row_stride > n."""
    from evdr_amd import ops
    n_docs = doc_block_sizes()[nd_i]
    rng = np.random.default_rng(1000 * n + n_docs)
    sizes = rng.choice(special_sizes(), n_docs).tolist()
    for edge in (ops.DOC_BLOCK - 1, ops.DOC_BLOCK):                   # the last document of one workgroup, the first of the next
        if edge < n_docs:
            sizes[edge] = ops.DOC_LONG + 33
    for order_i, order in enumerate(("ascending", "descending", "shuffled")):
        lists = C.sized_lists(rng, n, sizes, order)
        lists[rng.integers(0, n_docs)] = list(range(n)) if order != "descending" else list(range(n))[::-1]   # every page
        if order == "shuffled":                                       # duplicates and holes, anywhere in a document
            for d in rng.integers(0, n_docs, 6):
                extra = [-1, n, 2 ** 31 - 1, -2 ** 31] + list(lists[d][:3])
                merged = list(lists[d]) + extra
                lists[d] = [merged[i] for i in rng.permutation(len(merged))]
        for nq in (1, 3, ops.DOC_ROWS, ops.DOC_ROWS + 1):
            sc = C.tie_scores(rng, nq, n)
            name, idx_map = maps_for(rng, n)[(order_i + nq) % 3]
            idx_base = (0, 1000)[nq % 2]
            got = run_doc_max(dev, sc, lists, idx_map, idx_base)
            C.assert_bits(got, list_reference(sc, lists, idx_map, idx_base), (n, n_docs, order, nq, name))


def test_doc_max_absent_documents_and_empty_shapes(dev):
    """Documents whose pages are all -inf, documents without pages, a block without columns: (-inf, -1) everywhere."""
    from evdr_amd import ops
    rng = np.random.default_rng(7)
    n = 200
    sc = C.tie_scores(rng, 5, n)
    lists = C.sized_lists(rng, n, [3, 0, 40, 70, 1, 0], "shuffled")
    for d in (0, 2, 3):
        sc[:, lists[d]] = -np.inf
    sc[2, lists[3][5]] = -0.0                                           # one row of the long all -inf document has a page after all
    ds, db = run_doc_max(dev, sc, lists)
    C.assert_bits((ds, db), list_reference(sc, lists, None, 0), "absent")
    ds, db = C.host(ds), C.host(db)
    assert (db[:, [0, 1, 2, 5]] == -1).all() and np.isneginf(ds[:, [0, 1, 2, 5]]).all()
    assert db[2, 3] == lists[3][5] and ds[2, 3] == 0 and not np.signbit(ds[2, 3]) and (np.delete(db[:, 3], 2) == -1).all()
    # n = 0: every member is a hole; n_docs = 0 and nq = 0: nothing to write
    mem, off = C.csr([[0, 1], [5]])
    ds, db = ops.doc_max(torch.empty((3, 0), dtype=torch.float32, device=dev), dt(mem, dev), dt(off, dev))
    assert np.isneginf(C.host(ds)).all() and (C.host(db) == -1).all() and ds.shape == (3, 2)
    ds, db = ops.doc_max(strided(sc, dev), torch.empty(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
    assert ds.shape == (5, 0) and db.shape == (5, 0)
    ds, db = ops.doc_max(torch.empty((0, n), dtype=torch.float32, device=dev), dt(mem, dev), dt(off, dev))
    assert ds.shape == (0, 2)


def test_doc_max_clamps_bad_offsets(dev):
    """Offsets outside [0, nm] or descending never become an address: a document's start is clamped to [0, nm] and its end to
    [start, nm] (include/evdr.h), and the launch is clean."""
    from evdr_amd import ops
    rng = np.random.default_rng(11)
    sc = C.tie_scores(rng, 3, 50)
    mem = rng.permutation(50).astype(np.int32)
    off = np.array([-5, 10, 4, 2 ** 31 - 1, 60], dtype=np.int32)         # ranges: [0,10) [10,10) [4,50) [50,50)
    ds, db = ops.doc_max(dt(sc, dev), dt(mem, dev), dt(off, dev))
    torch.cuda.synchronize()
    lists = [mem[:10].tolist(), [], mem[4:].tolist(), []]
    C.assert_bits((ds, db), list_reference(sc, lists, None, 0), "clamped offsets")


def test_doc_max_repeats_its_bits_and_replays_in_a_graph(dev):
    """Two launches give equal bits; one captured launch into preallocated outputs, replayed on a single stream after the inputs
    changed in place, gives the new inputs' answer."""
    from evdr_amd import ops
    rng = np.random.default_rng(21)
    nq, n = 11, 700
    sizes = [ops.DOC_LONG + 5, 1, 0, 3, 200, 2] * 30
    lists = C.sized_lists(rng, n, sizes, "shuffled")
    mem, off = C.csr(lists)
    mem_d, off_d = dt(mem, dev), dt(off, dev)
    sc = C.tie_scores(rng, nq, n)
    block = strided(sc, dev)
    a = ops.doc_max(block, mem_d, off_d, idx_base=3)
    b = ops.doc_max(block, mem_d, off_d, idx_base=3)
    assert np.array_equal(C.host(a[0]).view(np.uint32), C.host(b[0]).view(np.uint32)) and torch.equal(a[1], b[1])
    out = (torch.empty_like(a[0]), torch.empty_like(a[1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.doc_max(block, mem_d, off_d, idx_base=3, out=out)           # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.doc_max(block, mem_d, off_d, idx_base=3, out=out)
    sc2 = C.tie_scores(rng, nq, n)
    block.copy_(dt(sc2, dev))
    g.replay()
    torch.cuda.synchronize()
    C.assert_bits(out, list_reference(sc2, lists, None, 3), "replay")
    C.assert_bits(a, list_reference(sc, lists, None, 3), "first launch")


def torch_composition(dev, block, mem_d, off_d, k, idx_map, idx_base):
    """evdr_doc_topk's three steps, each through its own Python binding."""
    from evdr_amd import ops
    ds, db = ops.doc_max(block, mem_d, off_d, idx_map, idx_base)
    nq, n_docs = ds.shape
    ts, td = ops.topk(ds, k) if n_docs else (torch.full((nq, k), float("-inf"), device=dev), torch.full((nq, k), -1, dtype=torch.int32, device=dev))
    real = (td >= 0) & ~torch.isneginf(ts)
    tp = torch.where(real, db.gather(1, td.clamp_min(0).long()), torch.full_like(td, -1)) if n_docs else torch.full_like(td, -1)
    return ts, torch.where(real, td, torch.full_like(td, -1)), tp


@pytest.mark.parametrize("n,n_docs,k", [(65, 1, 5), (1000, 257, 128), (1000, 40, 100), (300, 255, 1), (9000, 3000, 10)])
def test_doc_topk_is_the_reference_and_the_composition(dev, n, n_docs, k):
    """evdr_doc_topk through ctypes == ops.doc_reference == doc_max + topk + gather composed in Python; partitioned columns with -1
    pages, padding when fewer than k documents are present, with and without idx_map.  (9000, 3000) at 3 rows takes evdr_topk's
    two-level form."""
    from evdr_amd import ops
    rng = np.random.default_rng(n + n_docs + k)
    doc = rng.integers(-1, n_docs, n).astype(np.int32)
    doc[rng.random(n) < 0.3] = rng.integers(0, max(n_docs // 8, 1))      # one large document
    mem_t, off_t = ops.doc_lists(torch.from_numpy(doc), n_docs)
    mem_d, off_d = mem_t.to(dev), off_t.to(dev)
    for nq in (3, 9):
        sc = C.tie_scores(rng, nq, n)
        sc[:, doc % 3 == 0] = -np.inf                                     # a third of the documents absent: padding appears
        for name, idx_map in maps_for(rng, n)[:2]:
            block = strided(sc, dev)
            got = ops.doc_topk(block, mem_d, off_d, k, None if idx_map is None else dt(idx_map, dev), idx_base=17)
            rep = (np.arange(n) if idx_map is None else idx_map.astype(np.int64)) + 17
            want = ops.doc_reference(torch.from_numpy(sc), torch.from_numpy(doc), n_docs, k, torch.from_numpy(rep))
            C.assert_bits(got, want, (n, n_docs, k, nq, name, "reference"))
            comp = torch_composition(dev, block, mem_d, off_d, k, None if idx_map is None else dt(idx_map, dev), 17)
            C.assert_bits(got, comp, (n, n_docs, k, nq, name, "composition"))


# ---- evdr_collapse_topk -----------------------------------------------------------------------------------------------------------
SPARSE_IDS = np.array([0, 1, 2, 3, 5, 8, 1000, 65536, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1], dtype=np.int64)


def collapse_rows(rng, r, k):
    """7 rows of r entries (scores, document ids, pages): 0 one document; 1 all distinct; 2 fewer distinct documents than k; 3 random
    with holes, sparse ids and duplicated (document, page) entries; 4 one score everywhere (the lower id wins at the cut, the lower
    page inside a document); 5 NaN of both signs on top of a tie-heavy row; 6 nothing but holes."""
    sc = C.tie_scores(rng, 7, r)
    doc = SPARSE_IDS[rng.integers(0, len(SPARSE_IDS), (7, r))]
    page = rng.integers(0, max(r // 2, 2), (7, r))
    doc[0] = 2 ** 31 - 1
    doc[1] = rng.permutation(r) * 7 + 3
    doc[2] = rng.integers(0, max(min(k - 1, 3), 1), r)
    holes = rng.random(r) < 0.3
    doc[3, holes] = rng.choice([-1, -7, -2 ** 31], int(holes.sum()))
    sc[4] = 0.5
    doc[4] = rng.integers(0, k + 40, r)
    sc[5, rng.random(r) < 0.2] = np.nan
    sc[5, rng.random(r) < 0.2] = C.NAN_NEG
    doc[6] = -1 - rng.integers(0, 5, r)
    return sc, doc.astype(np.int32), page.astype(np.int32)


@pytest.mark.parametrize("r", [1, 2, 63, 64, 65, 257, 1000, 4096])
@pytest.mark.parametrize("k", [1, 5, 128])
def test_collapse_topk_is_the_reference(dev, r, k):
    """Both document forms against ops.collapse_reference, row_stride > r, and every row permuted: the result does not move."""
    from evdr_amd import ops
    rng = np.random.default_rng(r * 131 + k)
    sc, doc, page = collapse_rows(rng, r, k)
    want = ops.collapse_reference(torch.from_numpy(sc), torch.from_numpy(doc), torch.from_numpy(page), k)
    got = ops.collapse_topk(strided(sc, dev, 3), dt(page, dev), k, doc=dt(doc, dev))
    C.assert_bits(got, want, (r, k, "explicit ids"))
    perm = np.stack([rng.permutation(r) for _ in range(sc.shape[0])])
    take = lambda a: np.take_along_axis(a, perm, 1)
    C.assert_bits(ops.collapse_topk(dt(take(sc), dev), dt(take(page), dev), k, doc=dt(take(doc), dev)), want, (r, k, "permuted"))
    # the doc_of_page form: a table of np pages from idx_base on; entries outside it, and pages without a document, are holes
    npg, base = max(r // 2, 2) - 1, 1000                                  # the largest page value falls outside the table
    table = SPARSE_IDS[rng.integers(0, len(SPARSE_IDS), npg)]
    table[rng.random(npg) < 0.2] = -1
    gpage = page.astype(np.int64) + base
    gpage[3, rng.random(r) < 0.2] = rng.choice([-1, 0, base - 1, base + npg, 2 ** 31 - 1, -2 ** 31], 1)
    local = gpage - base
    inside = (local >= 0) & (local < npg)
    doc2 = np.where(inside, table[np.clip(local, 0, npg - 1)], -1).astype(np.int32)
    gpage = gpage.astype(np.int32)
    want2 = ops.collapse_reference(torch.from_numpy(sc), torch.from_numpy(doc2), torch.from_numpy(gpage), k)
    got2 = ops.collapse_topk(strided(sc, dev, 3), dt(gpage, dev), k, doc_of_page=dt(table.astype(np.int32), dev), idx_base=base)
    C.assert_bits(got2, want2, (r, k, "doc_of_page"))


def test_collapse_topk_hand_made_rows(dev):
    """The rule's corners on rows small enough to read: lower id at the cut, lower page inside a document, the same page twice, NaN
    first, -0 = +0 reported as +0, -inf entries absent, padding."""
    from evdr_amd import ops
    big = 2 ** 31 - 1
    sc = np.array([[0.5, 0.5, 0.5, 0.5, 0.5, 0.5],
                   [1.0, np.nan, -0.0, 0.0, -np.inf, 1.0],
                   [2.0, 2.0, 2.0, 1.0, 3.0, -np.inf]], dtype=np.float32)
    doc = np.array([[9, 4, big, 4, 7, 9], [3, 8, 5, 5, 6, 2], [1, 1, 1, 1, -1, 0]], dtype=np.int32)
    page = np.array([[50, 41, 7, 40, 70, 20], [11, 12, 14, 13, 15, 16], [33, 33, 30, 1, 2, 3]], dtype=np.int32)
    ts, td, tp = (C.host(x) for x in ops.collapse_topk(dt(sc, dev), dt(page, dev), 3, doc=dt(doc, dev)))
    assert td.tolist() == [[4, 7, 9], [8, 2, 3], [1, -1, -1]] and tp.tolist() == [[40, 70, 20], [12, 16, 11], [30, -1, -1]]
    assert np.isnan(ts[1, 0]) and ts[1, 1:].tolist() == [1.0, 1.0] and ts[2].tolist() == [2.0, -np.inf, -np.inf]
    ts, td, tp = (C.host(x) for x in ops.collapse_topk(dt(sc, dev), dt(page, dev), 5, doc=dt(doc, dev)))
    assert td[1].tolist() == [8, 2, 3, 5, -1] and tp[1].tolist() == [12, 16, 11, 13, -1] and ts[1, 3] == 0 and not np.signbit(ts[1, 3])
    assert td[0].tolist() == [4, 7, 9, big, -1] and tp[0, 3] == 7


# ---- end to end -------------------------------------------------------------------------------------------------------------------
NPG, BASE, NDOC = 70, 1000, 13


def doc_corpus(kind, dev, npg=NPG, lp=33):
    """npg pages x lp patches x 128, 9 queries of 5 tokens with ragged masks.  Pages 20..24 are byte-identical copies of pages 5..9
    and sit in OTHER documents; page 41 is a copy of page 40 in the SAME document; queries copy tokens of the copied pages, so the
    copies score at the top and tie exactly.  Documents are interleaved over the whole corpus (they span any cut), two pages have
    no document, document 12 has no page."""
    gen = torch.Generator().manual_seed(npg * 100 + lp)
    P = F.normalize(torch.randn((npg, lp, 128), generator=gen), dim=-1)
    lens = torch.randint(lp // 2 + 1, lp + 1, (npg,), generator=gen)
    pm = torch.arange(lp)[None, :] < lens[:, None]
    doc = (torch.arange(npg) * 5) % (NDOC - 1)
    if npg >= 42:
        P[20:25], pm[20:25] = P[5:10].clone(), pm[5:10].clone()
        P[41], pm[41] = P[40].clone(), pm[40].clone()
        doc[20:25] = (doc[5:10] + 1) % (NDOC - 1)
        doc[41] = doc[40]
        src = [5, 6, 7, 8, 9, 40, 40, 5, 6]
    else:
        P[7], pm[7] = P[2].clone(), pm[2].clone()
        doc[7] = (doc[2] + 1) % (NDOC - 1)
        src = [2] * 9
    doc[3], doc[npg - 1] = -1, -1
    noise = F.normalize(torch.randn((9, 5, 128), generator=gen), dim=-1)
    Q = F.normalize(P[torch.tensor(src)][:, :5] + 0.4 * noise, dim=-1)
    qm = torch.arange(5)[None, :] < torch.tensor([5, 5, 4, 3, 5, 2, 5, 1, 5])[:, None]
    if kind == "bf16":
        Q, P = Q.bfloat16(), P.bfloat16()
    return Q.to(dev), qm.to(dev), P.to(dev), pm.to(dev), doc.to(torch.int32).to(dev)


def make_corpus(kind, P, pm, **kw):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    return PageCorpus.from_tensor(P, pm, idx_base=BASE, dtype=ops.FP8 if kind == "fp8" else None, **kw)


def cpu_rule(S, doc, k, reported):
    """The rule applied on the CPU to a score block the GPU produced."""
    from evdr_amd import ops
    return ops.doc_reference(S.cpu(), doc.cpu(), NDOC, k, reported.cpu())


@pytest.mark.parametrize("kind,npg,lp", [("bf16", NPG, 33), ("f32", NPG, 33), ("fp8", NPG, 33), ("f32", 12, 7)])
def test_topk_docs_is_the_rule_on_the_score_block(dev, kind, npg, lp):
    """topk_docs == ops.doc_reference on the CPU over the GPU's own score() block, for k below and above the number of documents
    present; with subset= too (not on fp8, where subsets are refused).  The copied pages tie exactly: the lower page is reported."""
    Q, qm, P, pm, doc = doc_corpus(kind, dev, npg, lp)
    corpus = make_corpus(kind, P, pm)
    docs = corpus.documents(doc, n_docs=NDOC)
    S = corpus.score(Q, qm)
    pages = torch.arange(npg, device=dev) + BASE
    for k in (1, 5, 12, 64):
        got = corpus.topk_docs(Q, qm, k, docs)
        C.assert_bits(got, cpu_rule(S, doc, k, pages), (kind, npg, k))
    s, d, p = (C.host(x) for x in corpus.topk_docs(Q, qm, 13, docs))
    if npg == NPG:
        assert (d[:, 12] == -1).all() and (d[:, :12] >= 0).all()        # 12 documents have a page; document 12 has none: padding
        assert not np.isin(p, [BASE + 3, BASE + npg - 1]).any()         # the pages without a document never show
        assert p[5, 0] == BASE + 40 and p[6, 0] == BASE + 40            # 40 and 41 tie inside one document: the lower page
        assert p[0, 0] == BASE + 5 and p[0, 1] == BASE + 20 and np.array_equal(s[0, :1].view(np.uint32), s[0, 1:2].view(np.uint32))
        assert d[0, 0] != d[0, 1]                                       # the copies sit in two documents with one score: id order
    if kind == "fp8":
        return
    keep = torch.tensor([p_ for p_ in range(npg) if p_ % 4 != 1 and p_ != 5], device=dev) + BASE
    sub = corpus.subset(pages=keep.flip(0))
    dsub = corpus.documents(doc, n_docs=NDOC, subset=sub)
    Ssub = corpus.score(Q, qm, subset=sub)
    for k in (1, 7, 64):
        got = corpus.topk_docs(Q, qm, k, dsub, subset=sub)
        C.assert_bits(got, cpu_rule(Ssub, doc[sub.pages.long()], k, sub.pages.long() + BASE), (kind, npg, k, "subset"))


@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_rerank_docs_of_every_page_is_topk_docs(dev, kind):
    """A list naming every page (shuffled per query, with foreign entries and repeats mixed in) gives topk_docs's answer."""
    Q, qm, P, pm, doc = doc_corpus(kind, dev)
    corpus = make_corpus(kind, P, pm)
    docs = corpus.documents(doc, n_docs=NDOC)
    rng = np.random.default_rng(3)
    rows = [np.concatenate([rng.permutation(NPG) + BASE, [-1, 5, BASE + NPG, BASE + 7, BASE + 7]]) for _ in range(9)]
    cand = dt(np.stack([row[rng.permutation(len(row))] for row in rows]).astype(np.int32), dev)
    for k in (1, 5, 12, 64):
        C.assert_bits(corpus.rerank_docs(Q, qm, cand, k, docs), corpus.topk_docs(Q, qm, k, docs), (kind, k))


@pytest.mark.parametrize("kind", ["bf16", "f32", "fp8"])
def test_two_shard_views_merge_to_the_whole_corpus(dev, kind):
    """shard(0, 40) and shard(40, 70), each with the documents of its own slice (documents span the cut): their topk_docs,
    concatenated in either order and merged, equal the whole corpus's answer; ShardedRetriever.search_docs on one rank is topk_docs."""
    from evdr_amd.corpus import ShardedRetriever, merge_doc_candidates, pack_doc_candidates, unpack_doc_candidates
    Q, qm, P, pm, doc = doc_corpus(kind, dev)
    corpus = make_corpus(kind, P, pm)
    docs = corpus.documents(doc, n_docs=NDOC)
    a, b = corpus.shard(0, 40), corpus.shard(40, NPG)
    da, db_ = a.documents(doc[:40], n_docs=NDOC), b.documents(doc[40:], n_docs=NDOC)
    assert len(set(doc[:40].tolist()) & set(doc[40:].tolist())) >= 5
    for k in (1, 5, 12, 64):
        want = corpus.topk_docs(Q, qm, k, docs)
        pa, pb = a.topk_docs(Q, qm, k, da), b.topk_docs(Q, qm, k, db_)
        for first, second in ((pa, pb), (pb, pa)):
            lists = unpack_doc_candidates(torch.stack([pack_doc_candidates(*first), pack_doc_candidates(*second)]))
            C.assert_bits(merge_doc_candidates(*lists, k), want, (kind, k))
        C.assert_bits(ShardedRetriever(corpus).search_docs(Q, qm, k, docs), want, (kind, k, "one rank"))


def test_two_stage_search_docs_with_every_page_is_exact(dev):
    """TwoStageRetriever.search_docs with candidates = n_pages: every page reaches the rerank, so the answer is exact.topk_docs's,
    with an fp8 first stage and with a subset."""
    from evdr_amd.corpus import TwoStageRetriever
    Q, qm, P, pm, doc = doc_corpus("bf16", dev)
    exact, coarse = make_corpus("bf16", P, pm), make_corpus("fp8", P, pm)
    docs = exact.documents(doc, n_docs=NDOC)
    ts = TwoStageRetriever(coarse, exact)
    for k in (1, 12, 64):
        C.assert_bits(ts.search_docs(Q, qm, k, NPG, docs), exact.topk_docs(Q, qm, k, docs), k)
    sub = exact.subset(allow=torch.arange(NPG, device=dev) % 3 != 0)
    dsub = exact.documents(doc, n_docs=NDOC, subset=sub)
    C.assert_bits(ts.search_docs(Q, qm, 12, NPG, docs, subset=sub), exact.topk_docs(Q, qm, 12, dsub, subset=sub), "subset")


def test_documents_made_before_an_append_are_refused(dev):
    Q, qm, P, pm, doc = doc_corpus("bf16", dev)
    corpus = make_corpus("bf16", P[:60], pm[:60], capacity=NPG)
    docs = corpus.documents(doc[:60], n_docs=NDOC)
    before = corpus.topk_docs(Q, qm, 5, docs)
    corpus.append(P[60:], pm[60:])
    cand = torch.arange(8, dtype=torch.int32, device=dev).repeat(9, 1) + BASE
    with pytest.raises(ValueError, match="documents"):
        corpus.topk_docs(Q, qm, 5, docs)
    with pytest.raises(ValueError, match="documents"):
        corpus.rerank_docs(Q, qm, cand, 5, docs)
    fresh = corpus.documents(doc, n_docs=NDOC)                             # rebuilt: the appended pages join their documents
    whole = make_corpus("bf16", P, pm)
    C.assert_bits(corpus.topk_docs(Q, qm, 5, fresh), whole.topk_docs(Q, qm, 5, whole.documents(doc, n_docs=NDOC)), "after append")
    assert before[0].shape == (9, 5)


def test_ops_refuse_wrong_dtypes_devices_and_outputs(dev):
    """What the bindings check on device tensors before any launch."""
    from evdr_amd import ops
    sc = torch.zeros((2, 6), dtype=torch.float32, device=dev)
    mem = torch.arange(6, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 3, 6], dtype=torch.int32, device=dev)
    ids = torch.zeros((2, 6), dtype=torch.int32, device=dev)
    for bad in (dict(members=mem.long()), dict(members=mem.cpu()), dict(offsets=off.long()), dict(offsets=off[:0]),
                dict(idx_map=mem.long()), dict(idx_map=mem[:5]), dict(out=(torch.empty((2, 3), device=dev), torch.empty((2, 2), dtype=torch.int32, device=dev)))):
        args = dict(dict(members=mem, offsets=off), **bad)
        with pytest.raises(ValueError):
            ops.doc_max(sc, **args)
    with pytest.raises(RuntimeError):
        ops.doc_max(sc.double(), mem, off)
    for k in (0, 129):
        with pytest.raises(ValueError, match="k="):
            ops.doc_topk(sc, mem, off, k)
        with pytest.raises(ValueError, match="k="):
            ops.collapse_topk(sc, ids, k, doc=ids)
    for bad in (dict(page=ids.long(), doc=ids), dict(page=ids, doc=ids[:, :5]), dict(page=ids.cpu(), doc=ids), dict(page=ids, doc_of_page=mem.long()),
                dict(page=ids, doc_of_page=ids)):
        with pytest.raises(ValueError):
            ops.collapse_topk(sc, bad.pop("page"), 2, **bad)
    with pytest.raises(ValueError, match="r="):
        ops.collapse_topk(torch.zeros((1, 4097), device=dev), torch.zeros((1, 4097), dtype=torch.int32, device=dev), 2,
                          doc=torch.zeros((1, 4097), dtype=torch.int32, device=dev))
    got = ops.collapse_topk(sc, ids, 2, doc_of_page=torch.zeros(0, dtype=torch.int32, device=dev))    # an empty table: all holes
    assert (C.host(got[1]) == -1).all() and np.isneginf(C.host(got[0])).all()
