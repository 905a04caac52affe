"""Document-level search: a numpy statement of the rule, written entry by entry, and the case builders the host and
the GPU tests share.  Every comparison made with these is bit equality: indices equal, NaN at equal places, every other score equal
bit for bit (the convention of assert_ranking in tests/test_gpu_ranking_ties.py)."""
import numpy as np
import torch

# the tie-heavy value set of tests/test_gpu_ranking_ties.py
VALUES = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, np.inf, np.nan], dtype=np.float32)
NAN_NEG = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
KEY_NINF = 0x007FFFFF


def order_key(x) -> int:
    """One fp32 -> evdr_topk's order key (csrc/topk.hip) as a Python int."""
    u = int(np.array([x], dtype=np.float32).view(np.uint32)[0])
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return 0xFFFFFFFF
    if u == 0x80000000:
        u = 0
    return (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)


def key_to_float(k: int) -> np.float32:
    u = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def loop_doc_max(scores, lists, reported=None, idx_base=0):
    """The per-document rule as a plain loop.  scores (nq, n); lists: one sequence of columns per document (any order, duplicates, and
    columns outside [0, n) are holes); reported (n,) or None.  -> (doc_scores (nq, n_docs) fp32, doc_best (nq, n_docs) int32)."""
    sc = np.asarray(scores, dtype=np.float32)
    nq, n = sc.shape
    ds = np.full((nq, len(lists)), -np.inf, dtype=np.float32)
    db = np.full((nq, len(lists)), -1, dtype=np.int32)
    for q in range(nq):
        for d, cols in enumerate(lists):
            best = None
            for c in cols:
                c = int(c)
                if c < 0 or c >= n:
                    continue
                key = order_key(sc[q, c])
                if key == KEY_NINF:
                    continue
                rep = ((int(reported[c]) if reported is not None else c) + idx_base) & 0xFFFFFFFF
                if best is None or key > best[0] or (key == best[0] and rep < best[1]):
                    best = (key, rep)
            if best is not None:
                ds[q, d] = key_to_float(best[0])
                db[q, d] = np.array([best[1]], dtype=np.uint32).view(np.int32)[0]
    return ds, db


def loop_rank(doc_scores, doc_ids, doc_best, k):
    """Rows of per-document (score, id, best page; best page -1 = absent) -> (nq, k) x 3: key desc, id asc, (-inf, -1, -1) padding."""
    nq = doc_scores.shape[0]
    ts = np.full((nq, k), -np.inf, dtype=np.float32)
    td = np.full((nq, k), -1, dtype=np.int32)
    tp = np.full((nq, k), -1, dtype=np.int32)
    for q in range(nq):
        ids = doc_ids[q] if np.ndim(doc_ids) == 2 else doc_ids
        rows = [(-order_key(doc_scores[q, j]), int(ids[j]), j) for j in range(doc_scores.shape[1]) if doc_best[q, j] != -1]
        for slot, (nkey, d, j) in enumerate(sorted(rows)[:k]):
            ts[q, slot], td[q, slot], tp[q, slot] = key_to_float(-nkey), d, doc_best[q, j]
    return ts, td, tp


def loop_docs(scores, lists, k, reported=None, idx_base=0):
    """Block form, loop by loop: documents are numbered by their place in `lists`."""
    ds, db = loop_doc_max(scores, lists, reported, idx_base)
    return loop_rank(ds, np.arange(len(lists)), db, k)


def loop_collapse(scores, doc, page, k):
    """List form, loop by loop: entries (score, document id, page); negative id or -inf score = hole; sparse ids."""
    sc, dc, pg = np.asarray(scores, dtype=np.float32), np.asarray(doc), np.asarray(page)
    nq, r = sc.shape
    ts = np.full((nq, k), -np.inf, dtype=np.float32)
    td = np.full((nq, k), -1, dtype=np.int32)
    tp = np.full((nq, k), -1, dtype=np.int32)
    for q in range(nq):
        best = {}
        for i in range(r):
            d, key = int(dc[q, i]), order_key(sc[q, i])
            if d < 0 or key == KEY_NINF:
                continue
            rep = int(pg[q, i]) & 0xFFFFFFFF
            if d not in best or key > best[d][0] or (key == best[d][0] and rep < best[d][1]):
                best[d] = (key, rep)
        for slot, (nkey, d, rep) in enumerate(sorted((-kr[0], d, kr[1]) for d, kr in best.items())[:k]):
            ts[q, slot], td[q, slot] = key_to_float(-nkey), d
            tp[q, slot] = np.array([rep], dtype=np.uint32).view(np.int32)[0]
    return ts, td, tp


def host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def assert_bits(got, want, what=""):
    """A tuple of arrays against another: shapes and dtypes equal, integers equal, floats NaN at equal places and otherwise equal
    bit for bit."""
    assert len(got) == len(want), what
    for pos, (g, w) in enumerate(zip(got, want)):
        g, w = host(g), host(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, pos, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float32:
            gn, wn = np.isnan(g), np.isnan(w)
            assert np.array_equal(gn, wn), (what, pos, "NaN places")
            bad = np.argwhere((g.view(np.uint32) != w.view(np.uint32)) & ~gn)
        else:
            bad = np.argwhere(g != w)
        assert bad.size == 0, (what, pos, "first difference at", bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- case builders ----------------------------------------------------------------------------------------------------------------
def tie_scores(rng, nq, n):
    """(nq, n) fp32: half of the entries from VALUES (exact ties, NaN of both signs, both zeros, both infinities), half random floats."""
    sc = VALUES[rng.integers(0, len(VALUES), (nq, n))].copy()
    mix = rng.random((nq, n)) < 0.5
    sc[mix] = rng.standard_normal((nq, n)).astype(np.float32)[mix]
    sc[rng.random((nq, n)) < 0.02] = NAN_NEG
    return np.ascontiguousarray(sc, dtype=np.float32)


def csr(lists):
    """One sequence of columns per document -> (members int32, offsets int32)."""
    offsets = np.zeros(len(lists) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    members = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if lists else np.zeros(0, dtype=np.int32)
    return members.astype(np.int32), offsets


def sized_lists(rng, n, sizes, order="shuffled"):
    """Documents of the given sizes over the columns 0..n-1: columns are dealt out in a random order, wrapping round when the sizes
    ask for more than n (a column may then sit in several documents, which the CSR form allows).  order: how a document lists its
    columns -- "ascending", "descending" or "shuffled"."""
    need = int(sum(sizes))
    deck = np.concatenate([rng.permutation(n) for _ in range(need // max(n, 1) + 1)])[:need] if need else np.zeros(0, dtype=np.int64)
    lists, at = [], 0
    for s in sizes:
        cols = np.array(deck[at:at + s], dtype=np.int64)
        at += s
        if order != "shuffled":
            cols = np.sort(cols)
            if order == "descending":
                cols = cols[::-1]
        lists.append(cols.tolist())
    return lists
