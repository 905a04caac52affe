"""Document-level search without a GPU: the torch statements of the rule against a loop, `ops.doc_lists`, the
three-array candidate message, the C-ABI and Python refusals, and the kernels' compile-time resources."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import docsearch_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def doc_of_col_from(lists, n):
    out = np.full(n, -1, dtype=np.int32)
    for d, cols in enumerate(lists):
        out[np.asarray(cols, dtype=np.int64)] = d
    return out


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,nq,n,n_docs,k", [(0, 3, 1, 1, 1), (1, 4, 12, 5, 3), (2, 5, 40, 9, 12), (3, 2, 30, 30, 5), (4, 3, 25, 2, 4)])
def test_doc_reference_is_the_loop(seed, nq, n, n_docs, k):
    """ops.doc_max_reference / ops.doc_reference against the entry-by-entry loop: partitioned columns, -1 columns, empty documents,
    with and without a (descending, shifted) reported map."""
    from evdr_amd import ops
    rng = np.random.default_rng(seed)
    sc = C.tie_scores(rng, nq, n)
    doc = rng.integers(-1, n_docs, n).astype(np.int32)
    lists = [np.flatnonzero(doc == d).tolist() for d in range(n_docs)]
    for reported in (None, (np.arange(n)[::-1] * 3 + 7).astype(np.int32)):
        rep_t = None if reported is None else torch.from_numpy(reported.copy())
        got = ops.doc_max_reference(torch.from_numpy(sc), torch.from_numpy(doc), n_docs, rep_t)
        C.assert_bits(got, C.loop_doc_max(sc, lists, reported), ("doc_max", seed, reported is None))
        got = ops.doc_reference(torch.from_numpy(sc), torch.from_numpy(doc), n_docs, k, rep_t)
        C.assert_bits(got, C.loop_docs(sc, lists, k, reported), ("doc", seed, reported is None))


def test_doc_reference_edges():
    """Hand-made rows: NaN of either sign first, -0 ties with +0 and comes back +0, -inf is absent, the lower page wins inside a
    document, the lower document id wins across documents, absent documents only pad."""
    from evdr_amd import ops
    s = np.array([[1.0, C.NAN_NEG, -np.inf, -0.0, 0.0, 1.0, -np.inf, 0.5]], dtype=np.float32)
    doc = np.array([3, 0, 1, 2, 2, 4, 1, -1], dtype=np.int32)            # doc 1: all -inf; doc 5: no page; column 7: no document
    ts, td, tp = ops.doc_reference(torch.from_numpy(s), torch.from_numpy(doc), 6, 8)
    assert td[0].tolist() == [0, 3, 4, 2, -1, -1, -1, -1] and tp[0].tolist() == [1, 0, 5, 3, -1, -1, -1, -1]
    assert np.isnan(ts[0, 0].item()) and ts[0, 1:4].tolist() == [1.0, 1.0, 0.0] and not np.signbit(ts[0, 3].item())
    assert (ts[0, 4:] == float("-inf")).all()
    rep = torch.tensor([9, 8, 7, 6, 5, 4, 3, 2], dtype=torch.int32)        # descending map: the LOWER reported index is the later column
    _, td, tp = ops.doc_reference(torch.from_numpy(s), torch.from_numpy(doc), 6, 3, rep)
    assert td[0].tolist() == [0, 3, 4] and tp[0].tolist() == [8, 9, 4]
    ds, db = ops.doc_max_reference(torch.from_numpy(s), torch.from_numpy(doc), 6, rep)
    assert db[0].tolist() == [8, -1, 5, 9, 4, -1] and ds[0, 1].item() == float("-inf") and ds[0, 2].item() == 0.0


@pytest.mark.parametrize("seed,nq,r,k", [(0, 3, 1, 1), (1, 4, 17, 5), (2, 3, 60, 128), (3, 2, 33, 7)])
def test_collapse_reference_is_the_loop(seed, nq, r, k):
    """ops.collapse_reference against the loop: sparse ids up to 2^31 - 1, holes, -inf entries, duplicate pages; a permutation of
    every row does not move the result."""
    from evdr_amd import ops
    rng = np.random.default_rng(seed)
    sc = C.tie_scores(rng, nq, r)
    ids = np.array([0, 1, 5, 1000, 2 ** 31 - 1, 2 ** 31 - 2, 77, -1, -5], dtype=np.int64)
    doc = ids[rng.integers(0, len(ids), (nq, r))].astype(np.int32)
    page = rng.integers(0, 9, (nq, r)).astype(np.int32)
    want = C.loop_collapse(sc, doc, page, k)
    C.assert_bits(ops.collapse_reference(torch.from_numpy(sc), torch.from_numpy(doc), torch.from_numpy(page), k), want, seed)
    perm = np.stack([rng.permutation(r) for _ in range(nq)])
    take = lambda a: torch.from_numpy(np.take_along_axis(a, perm, 1).copy())
    C.assert_bits(ops.collapse_reference(take(sc), take(doc), take(page), k), want, (seed, "permuted"))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_list_naming_every_page_gives_the_block_answer(seed):
    from evdr_amd import ops
    rng = np.random.default_rng(seed)
    nq, n, n_docs, k = 4, 37, 8, 6
    sc = C.tie_scores(rng, nq, n)
    doc = rng.integers(-1, n_docs, n).astype(np.int32)
    base = 1000
    block = ops.doc_reference(torch.from_numpy(sc), torch.from_numpy(doc), n_docs, k, torch.arange(n, dtype=torch.int32) + base)
    perm = np.stack([rng.permutation(n) for _ in range(nq)])
    lst = ops.collapse_reference(torch.from_numpy(np.take_along_axis(sc, perm, 1).copy()), torch.from_numpy(doc[perm].copy()),
                                 torch.from_numpy((perm + base).astype(np.int32)), k)
    C.assert_bits(lst, block, seed)


# ---- ops.doc_lists ----------------------------------------------------------------------------------------------------------------
def test_doc_lists_on_cpu_tensors():
    from evdr_amd import ops
    doc = torch.tensor([2, 0, -1, 2, 0, 5, 2, -1, 0], dtype=torch.int32)             # interleaved, -1 pages, documents 1, 3, 4 empty
    members, offsets = ops.doc_lists(doc, 8)                                         # n_docs beyond the largest id: 6 and 7 empty too
    assert members.dtype == torch.int32 and offsets.dtype == torch.int32
    assert offsets.tolist() == [0, 3, 3, 6, 6, 6, 7, 7, 7]
    assert members.tolist() == [1, 4, 8, 0, 3, 6, 5]                                 # stable: columns ascend inside a document
    members, offsets = ops.doc_lists(doc, 3)                                         # ids outside [0, n_docs) are dropped like -1
    assert offsets.tolist() == [0, 3, 3, 6] and members.tolist() == [1, 4, 8, 0, 3, 6]
    members, offsets = ops.doc_lists(torch.zeros(0, dtype=torch.int32), 2)
    assert members.tolist() == [] and offsets.tolist() == [0, 0, 0]
    members, offsets = ops.doc_lists(doc, 0)
    assert members.tolist() == [] and offsets.tolist() == [0]
    rng = np.random.default_rng(5)
    big = rng.integers(-1, 40, 500).astype(np.int32)
    members, offsets = ops.doc_lists(torch.from_numpy(big), 40)
    for d in range(40):
        assert members[offsets[d]:offsets[d + 1]].tolist() == np.flatnonzero(big == d).tolist()
    with pytest.raises(ValueError):
        ops.doc_lists(torch.zeros((2, 2), dtype=torch.int32), 2)
    with pytest.raises(ValueError):
        ops.doc_lists(torch.zeros(3), 2)
    with pytest.raises(ValueError):
        ops.doc_lists(doc, -1)


def test_geometry_constants_are_the_header():
    from evdr_amd import ops, _lib as L
    text = open(os.path.join(ROOT, "include", "evdr.h")).read()
    for name, value in (("EVDR_DOC_BLOCK", ops.DOC_BLOCK), ("EVDR_DOC_ROWS", ops.DOC_ROWS), ("EVDR_DOC_LONG", ops.DOC_LONG)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", text)
        assert m and int(m.group(1)) == value == getattr(L, name), name
    assert 1 < ops.DOC_LONG and ops.DOC_ROWS >= 1 and ops.DOC_BLOCK % 64 == 0


# ---- the three-array message ------------------------------------------------------------------------------------------------------
def test_doc_candidate_message_round_trip():
    from evdr_amd.corpus import pack_doc_candidates, unpack_doc_candidates
    rng = np.random.default_rng(3)
    world, nq, k = 3, 5, 4
    parts = []
    for _ in range(world):
        parts.append((torch.from_numpy(C.tie_scores(rng, nq, k)), torch.from_numpy(rng.integers(-1, 2 ** 31 - 1, (nq, k)).astype(np.int32)),
                      torch.from_numpy(rng.integers(-1, 1000, (nq, k)).astype(np.int32))))
    msgs = [pack_doc_candidates(*p) for p in parts]
    assert all(m.shape == (nq, 3 * k) and m.dtype == torch.int32 and m.is_contiguous() for m in msgs)
    got = unpack_doc_candidates(torch.stack(msgs))
    want = tuple(torch.cat([p[i] for p in parts], dim=1) for i in range(3))
    C.assert_bits(got, want)                                                         # rank-major, NaN payloads and -0.0 bits intact
    assert np.array_equal(C.host(got[0]).view(np.uint32), C.host(want[0]).view(np.uint32))


# ---- C-ABI argument errors: all before any HIP call -------------------------------------------------------------------------------
def test_doc_max_argument_errors(lib):
    from evdr_amd import _lib as L
    P = 64                                                                           # a fake non-null pointer: nothing is dereferenced
    ok = dict(scores=P, members=P, offsets=P, idx_map=None, nq=2, n=5, row_stride=5, nm=5, n_docs=3, idx_base=0, ds=P, doc_stride=3, db=P)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.evdr_doc_max(a["scores"], a["members"], a["offsets"], a["idx_map"], a["nq"], a["n"], a["row_stride"], a["nm"], a["n_docs"],
                                a["idx_base"], a["ds"], a["doc_stride"], a["db"], None)
    for bad in (dict(nq=-1), dict(n=-1), dict(nm=-1), dict(n_docs=-1), dict(scores=None), dict(members=None), dict(offsets=None),
                dict(ds=None), dict(db=None), dict(row_stride=4), dict(doc_stride=2)):
        assert call(**bad) == L.EVDR_ERR_ARG, bad
        assert lib.evdr_last_error()
    assert call(n_docs=2 ** 31) == L.EVDR_ERR_SHAPE and call(nq=2 ** 31) == L.EVDR_ERR_SHAPE
    assert call(nq=0, scores=None, members=None, offsets=None, ds=None, db=None) == L.EVDR_OK       # nothing to do, nothing written
    assert call(n_docs=0, offsets=None, ds=None, db=None, doc_stride=0) == L.EVDR_OK


def test_collapse_topk_argument_errors(lib):
    from evdr_amd import _lib as L
    P = 64
    ok = dict(scores=P, page=P, doc=P, dop=None, np_=0, base=0, nq=2, r=8, row_stride=8, k=4, ts=P, td=P, tp=P)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.evdr_collapse_topk(a["scores"], a["page"], a["doc"], a["dop"], a["np_"], a["base"], a["nq"], a["r"], a["row_stride"], a["k"],
                                      a["ts"], a["td"], a["tp"], None)
    for bad in (dict(nq=-1), dict(np_=-1), dict(r=0), dict(r=L.EVDR_SELECT_MAX + 1), dict(k=0), dict(k=L.EVDR_TOPK_MAX + 1),
                dict(doc=P, dop=P), dict(doc=None, dop=None), dict(scores=None), dict(page=None), dict(ts=None), dict(td=None),
                dict(tp=None), dict(row_stride=7)):
        assert call(**bad) == L.EVDR_ERR_ARG, bad
    assert call(doc=P, dop=P) == L.EVDR_ERR_ARG and b"both" in lib.evdr_last_error()
    assert call(doc=None, dop=None) == L.EVDR_ERR_ARG and b"neither" in lib.evdr_last_error()
    assert call(np_=2 ** 31, doc=None, dop=P) == L.EVDR_ERR_SHAPE
    assert call(nq=0, scores=None, page=None, ts=None, td=None, tp=None) == L.EVDR_OK
    assert call(nq=0, k=0) == L.EVDR_ERR_ARG                                         # an invalid k never passes silently


def test_doc_topk_argument_errors(lib):
    from evdr_amd import _lib as L
    P = 64
    need = lib.evdr_doc_topk_workspace(2, 3)
    assert need >= 2 * 2 * 3 * 4 and lib.evdr_doc_topk_workspace(0, 3) == 0 and lib.evdr_doc_topk_workspace(2, 0) == 0
    assert lib.evdr_doc_topk_workspace(-1, 3) == 0
    assert lib.evdr_doc_topk_workspace(4, 100000) >= 2 * 4 * 100000 * 4 + lib.evdr_topk_workspace(4, 100000, L.EVDR_TOPK_MAX)
    ok = dict(scores=P, members=P, offsets=P, idx_map=None, nq=2, n=5, row_stride=5, nm=5, n_docs=3, idx_base=0, k=2, ts=P, td=P, tp=P,
              ws=P, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.evdr_doc_topk(a["scores"], a["members"], a["offsets"], a["idx_map"], a["nq"], a["n"], a["row_stride"], a["nm"], a["n_docs"],
                                 a["idx_base"], a["k"], a["ts"], a["td"], a["tp"], a["ws"], a["wsb"], None)
    for bad in (dict(nq=-1), dict(n=-1), dict(nm=-1), dict(n_docs=-1), dict(k=0), dict(k=L.EVDR_TOPK_MAX + 1), dict(scores=None),
                dict(members=None), dict(offsets=None), dict(ts=None), dict(td=None), dict(tp=None), dict(row_stride=4)):
        assert call(**bad) == L.EVDR_ERR_ARG, bad
    assert call(ws=None) == L.EVDR_ERR_WORKSPACE and call(wsb=need - 1) == L.EVDR_ERR_WORKSPACE
    assert b"workspace" in lib.evdr_last_error()
    assert call(n_docs=2 ** 31) == L.EVDR_ERR_SHAPE
    assert call(nq=0, scores=None, ts=None, td=None, tp=None, ws=None, wsb=0) == L.EVDR_OK


# ---- Python refusals: all before any device work ----------------------------------------------------------------------------------
def fake_corpus(n_pages=6, idx_base=100):
    """A PageCorpus that owns no device memory: enough for the argument checks, which run before anything touches the GPU."""
    from evdr_amd.corpus import PageCorpus
    c = PageCorpus(torch.zeros((1, n_pages, 4, 128), dtype=torch.bfloat16), torch.zeros((n_pages, 1), dtype=torch.int32),
                   torch.zeros((n_pages,), dtype=torch.int32), idx_base=idx_base)
    return c


def test_documents_and_their_refusals():
    from evdr_amd.corpus import PageCorpus, PageDocuments
    c = fake_corpus()
    doc = torch.tensor([4, 4, -1, 0, 9, 0], dtype=torch.int32)
    d = c.documents(doc)
    assert isinstance(d, PageDocuments) and d.n_docs == 10 and d.subset is None and d.idx_map is None and d.belongs_to(c)
    assert d.offsets.tolist() == [0, 2, 2, 2, 2, 4, 4, 4, 4, 4, 5] and d.members.tolist() == [3, 5, 0, 1, 4]
    assert c.documents(doc, n_docs=12).n_docs == 12
    with pytest.raises(ValueError, match="n_docs"):
        c.documents(doc, n_docs=9)                                                    # an id outside [0, n_docs)
    for bad in (doc.long(), doc[:5], doc.float(), doc.tolist()):
        with pytest.raises(ValueError, match="doc_of_page"):
            c.documents(bad)
    if torch.cuda.is_available():                                                     # a tensor on another device than the corpus's
        with pytest.raises(ValueError, match="doc_of_page"):
            c.documents(doc.cuda())
    sub = c.subset(pages=torch.tensor([105, 101, 103]))
    ds = c.documents(doc, subset=sub)
    assert ds.subset is sub and ds.idx_map is sub.pages and ds.n_docs == 10
    assert ds.members.tolist() == [1, 2, 0] and ds.offsets.tolist() == [0, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3]   # columns of [1, 3, 5]
    other = fake_corpus()
    Q = torch.zeros((2, 3, 128), dtype=torch.bfloat16)
    cand = torch.zeros((2, 4), dtype=torch.int32)
    for call in (lambda: other.topk_docs(Q, None, 2, d), lambda: other.rerank_docs(Q, None, cand, 2, d),
                 lambda: c.shard(0, 3).topk_docs(Q, None, 2, d), lambda: c.topk_docs(Q, None, 2, "docs")):
        with pytest.raises(ValueError, match="documents"):
            call()
    with pytest.raises(ValueError, match="subset"):
        other.documents(doc, subset=sub)
    with pytest.raises(ValueError, match="subset"):
        c.topk_docs(Q, None, 2, d, subset=sub)                                        # documents built without the subset
    with pytest.raises(ValueError, match="subset"):
        c.topk_docs(Q, None, 2, ds)                                                   # ... and with it, searched without
    for k in (0, 129):
        with pytest.raises(ValueError, match="k="):
            c.topk_docs(Q, None, k, d)
    with pytest.raises(ValueError, match="k="):
        c.rerank_docs(Q, None, cand, 5, d)                                            # k > r
    with pytest.raises(ValueError, match="cand"):
        c.rerank_docs(Q, None, cand.long(), 2, d)
    # a stale n_pages: the corpus the documents were made for has grown (what append does to n_pages)
    grown = types.SimpleNamespace(_identity=c._identity, n_pages=c.n_pages + 1, idx_base=c.idx_base)
    assert d.belongs_to(c) and not d.belongs_to(grown)
    sh = c.shard(2, 6)
    dsh = sh.documents(doc[2:6], n_docs=10)                                           # a view builds its own from its slice
    assert dsh.belongs_to(sh) and not dsh.belongs_to(c) and dsh.members.tolist() == [1, 3, 2]


def test_ops_refusals():
    from evdr_amd import ops
    s = torch.zeros((2, 4))
    i = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="exactly one"):
        ops.collapse_topk(s, i, 2)                                                    # neither document form
    with pytest.raises(ValueError, match="exactly one"):
        ops.collapse_topk(s, i, 2, doc=i, doc_of_page=torch.zeros(9, dtype=torch.int32))   # both
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.collapse_topk(s, i, 2, doc=i)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.doc_max(s, torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.doc_topk(s, torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 1)


def test_world_times_k_is_bounded():
    from evdr_amd.corpus import _check_doc_world
    _check_doc_world(32, 128)
    _check_doc_world(4096, 1)
    with pytest.raises(ValueError, match="world"):
        _check_doc_world(33, 128)
    with pytest.raises(ValueError, match="world"):
        _check_doc_world(4097, 1)


# ---- compile-time resources -------------------------------------------------------------------------------------------------------
def test_doc_kernels_use_no_scratch():
    """scratch/kres.py over csrc/docs.hip: the three kernels compile for gfx950 without scratch memory and without VGPR spills (the
    per-row words of evdr_doc_max stay in registers)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scratch", "kres.py"), "docs.hip"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    rows = [ln for ln in r.stdout.splitlines() if re.match(r"(doc_max|collapse_topk|doc_finish)_kernel\(", ln)]
    assert r.returncode == 0 and len(rows) == 3, (r.stdout[-1500:], r.stderr[-500:])
    for ln in rows:
        m = re.search(r"VGPR\s+(\d+) AGPR\s+(\d+) spill\s+(\d+) sspill\s+\d+ scratch\s+(\d+)", ln)
        assert m and int(m.group(3)) == 0 and int(m.group(4)) == 0, ln
