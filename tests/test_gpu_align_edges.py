"""Token alignment on the GPU at its edges (csrc/align.hip; cases in tests/align_cases.py, their power shown without a
GPU in tests/test_align_cases_host.py): exact selection on pages of exact ties, rows far from unit norm, non-finite inputs, the -1e4
corner on every encoding of the page-flag word, launch geometry, the C entry on strided planes, graph capture, two streams and
growable corpora.

Exact selection needs no float64 reference and no tolerance: with nq = lq copies of a query and qmask = eye(lq), row n of the heat
output IS the kernel's product row V[n, :] (the products do not depend on the query mask: §4.12 "Order"), and every other output of
every other launch is a pure function of V and the masks, checked with torch.equal.

Magnitudes.  A finite value lies within 1e-5 * |q_n| * |p_m| of the float64 product of the rounded inputs: the project's bound
128 * 2^-24 * sum|a b| <= 7.7e-6 |q||p| (Cauchy-Schwarz), + 2.4e-7 for the dropped lo x lo plane, + the representation, < 1e-6
(test_align_cases_host.py).  sim is checked at the patch the kernel names; sim against the reference's maximum and heat against the
reference's column maximum with the largest norm that can stand behind them (the valid patches' / the valid tokens').  An index
follows rule 2 of tests/test_gpu_align.py with the gap scaled the same way: 2e-5 * |q_n| * max_m |p_m|."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu

NINF = float("-inf")
VALUE_REL, GAP_REL, NEAR_TIE_CAP, SUM_REL = 1e-5, 2e-5, 0.01, 1e-4
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaN == NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def same3(got, want) -> bool:
    return same(got[0], want[0]) and torch.equal(got[1], want[1]) and (len(want) < 3 or same(got[2], want[2]))


def corpus_of(c, dev, **kw):
    from evdr_amd.corpus import PageCorpus
    return PageCorpus.from_tensor(c["P"].to(dev), c["pmask"].to(dev), idx_base=c["base"], **kw)


def align_case(corpus, c, dev, heat=True):
    return corpus.align(c["Q"].to(dev), c["qmask"].to(dev), c["cand"].to(dev), heat=heat)


def check_case(c, got, what, sums=None):
    """Fills bit for bit, finite values within VALUE_REL of float64 scaled by the norms, indices by rule 2 with the scaled gap; `sums`
    (score_candidates' output) within SUM_REL * sum_n |q_n| * max_m |p_m|.  Returns the largest value error over its bound."""
    sim, patch, heat = (t.cpu() for t in got)
    rs, rp, rh = c["ref"]
    loc, qn, pn, pmax, qmask, pmask = c["loc"], c["qn"], c["pn"], c["pmax"], c["qmask"], c["pmask"]
    fill = rp < 0                                                    # masked tokens, holes, empty pages, NaN pairs
    assert torch.equal(patch < 0, fill) and torch.equal(patch[fill], rp[fill]), what
    assert same(sim[fill], rs[fill]), what                           # the exact 0 / -inf / NaN
    fin_h = torch.isfinite(rh)
    assert torch.equal(torch.isfinite(heat), fin_h) and same(heat[~fin_h], rh[~fin_h]), what
    valid = ~fill
    worst = 0.0
    if valid.any():
        q, i, n = valid.nonzero(as_tuple=True)
        m = patch[valid].long()
        page = loc[q, i]
        assert bool(((m >= 0) & (m < pmask.shape[1])).all()), what
        # sim at the patch the kernel names: a valid patch's product within its own bound, a masked one the exact -1e4
        named_valid = pmask[page, m]
        d = c["filled"][q, i, n, m]
        err = (sim[valid].double() - d).abs()
        tol = VALUE_REL * qn[q, n] * pn[page, m]
        assert bool((err[~named_valid] == 0).all()), what
        ratio = (err[named_valid] / tol[named_valid]).max().item() if named_valid.any() else 0.0
        print(f"{what}: sim at the named patch {ratio:.3f} of its bound")
        assert ratio <= 1.0, (what, "sim at the named patch", ratio)
        # sim against the float64 maximum
        best = c["filled"][q, i, n].max(dim=-1).values
        ratio2 = ((sim[valid].double() - best).abs() / (VALUE_REL * qn[q, n] * pmax[page])).max().item()
        assert ratio2 <= 1.0, (what, "sim", ratio2)
        # indices: exact where the top-two gap exceeds the scaled GAP, within it elsewhere, those tokens under the cap
        scale = qn[q, n] * pmax[page]
        near = c["gap"][valid] <= GAP_REL * scale
        assert torch.equal(m[~near], rp[valid].long()[~near]), (what, int((m[~near] != rp[valid].long()[~near]).sum()))
        assert bool((best[near] - d[near] <= GAP_REL * scale[near]).all()), what
        share = near.sum().item() / valid.sum().item()
        assert share <= NEAR_TIE_CAP, (what, share)
        worst = max(ratio, ratio2)
    if fin_h.any():
        dots = c["dots"].masked_fill(~qmask[:, None, :, None], NINF)
        h64 = dots.max(dim=2).values                                 # (nq, r, lp)
        qtop = torch.where(qmask, qn, torch.zeros_like(qn)).max(dim=1).values
        tol = VALUE_REL * qtop[:, None, None] * pn[loc]
        ratio3 = ((heat.double() - h64).abs()[fin_h] / tol[fin_h]).max().item()
        print(f"{what}: heat {ratio3:.3f} of its bound")
        assert ratio3 <= 1.0, (what, "heat", ratio3)
        worst = max(worst, ratio3)
    if sums is not None:
        sums = sums.cpu()
        total = torch.where(patch >= 0, sim, torch.zeros_like(sim)).double().sum(-1)
        real = (c["cand"].long() >= c["base"]) & (c["cand"].long() < c["base"] + pmask.shape[0])
        assert torch.equal(torch.isfinite(sums), real), what
        bound = SUM_REL * torch.where(qmask, qn, torch.zeros_like(qn)).sum(-1)[:, None] * pmax[loc]
        assert bool(((total - sums.double()).abs()[real] <= bound[real]).all()), (what, "token sums")
    return worst


# ---- a. exact selection ------------------------------------------------------------------------------------------------------------------
TIE_CASES = [(kind, lp, v) for kind in ac.KINDS for lp in ac.TIE_LPS for v in ac.tie_variants(lp)]


@pytest.mark.parametrize("kind,lp,variant", TIE_CASES)
def test_selection_is_exact_on_tie_pages(dev, kind, lp, variant):
    """Launch A (lq copies of the query, qmask = eye, heat) reads the kernel's own products V; launch B (the query once, all tokens
    valid / a random part of them) must then be, bit for bit, max / first arg-max of where(pmask, V, -1e4) and the column maxima of
    V.  Teeth: a token aimed at a row with two valid copies or more sees its maximum on ALL of them (identical rows, identical
    bits), so the index is decided by the tie rule at the levels tests/test_align_cases_host.py counts."""
    from evdr_amd.corpus import PageCorpus
    c = ac.tie_page(kind, lp, 0, variant)
    pm = c["pmask"][0]
    corpus = PageCorpus.from_tensor(c["P"].to(dev), c["pmask"].to(dev))
    P64 = c["P"][0].double()
    for lq in (1, 16, 17, 32):
        what = f"{kind} lp={lp} {variant} lq={lq}"
        Q1 = c["Q"][:lq]
        zero = torch.zeros((lq, 1), dtype=torch.int32, device=dev)
        simA, patchA, heatA = (t.cpu() for t in corpus.align(Q1[None].expand(lq, -1, -1).contiguous().to(dev),
                                                             torch.eye(lq, dtype=torch.bool, device=dev), zero, heat=True))
        V = heatA[:, 0, :]
        assert bool((V[:, ~pm] == NINF).all()) and bool(torch.isfinite(V[:, pm]).all()), what
        err = (V.double() - Q1.double() @ P64.T)[:, pm].abs().max().item()
        assert err <= 1e-5, (what, err)                              # unit rows: the project's own bound
        filled = torch.where(pm[None], V, torch.full_like(V, -1e4))
        top = filled.max(dim=1).values
        first = torch.where(filled == top[:, None], torch.arange(lp)[None], torch.full((1, lp), ac.BIG)).min(dim=1).values.to(torch.int32)
        for n in range(lq):                                          # teeth: exact ties on every valid copy of the aimed row
            copies = [m for m in c["rows"][c["row_of_token"][n]] if bool(pm[m])]
            at = (filled[n] == top[n]).nonzero().flatten().tolist()
            assert len(copies) >= 2 and set(copies) <= set(at), (what, n, copies, at)
        # launch A itself: token n of query n, everything else masked
        diag = torch.eye(lq, dtype=torch.bool)
        assert torch.equal(simA[:, 0][diag], top) and torch.equal(patchA[:, 0][diag], first), what
        assert bool((simA[:, 0][~diag] == 0).all()) and bool((patchA[:, 0][~diag] == -1).all()), what
        gen = torch.Generator().manual_seed(lp + lq)
        part = torch.rand(lq, generator=gen) < 0.6
        part[int(torch.randint(lq, (1,), generator=gen))] = True
        for tv in (torch.ones(lq, dtype=torch.bool), part):
            simB, patchB, heatB = (t.cpu() for t in corpus.align(Q1[None].to(dev), tv[None].to(dev), zero[:1], heat=True))
            assert torch.equal(simB[0, 0], torch.where(tv, top, torch.zeros_like(top))), what
            assert torch.equal(patchB[0, 0], torch.where(tv, first, torch.full_like(first, -1))), (what, patchB[0, 0].tolist(), first.tolist())
            col = torch.where(pm, V[tv].max(dim=0).values, torch.full((lp,), NINF))
            assert torch.equal(heatB[0, 0], col), what
            sim2, patch2 = corpus.align(Q1[None].to(dev), tv[None].to(dev), zero[:1])
            assert torch.equal(sim2.cpu(), simB) and torch.equal(patch2.cpu(), patchB), what


# ---- b. magnitudes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,lp,lq", ac.SPREAD)
def test_rows_of_mixed_norms(dev, kind, lp, lq):
    c = ac.spread_case(kind, lp, lq)
    corpus = corpus_of(c, dev)
    got = align_case(corpus, c, dev)
    sums = corpus.score_candidates(c["Q"].to(dev), c["qmask"].to(dev), c["cand"].to(dev))
    check_case(c, got, f"spread {kind} lp={lp} lq={lq}", sums)


@pytest.mark.parametrize("scale", ac.SCALES, ids=lambda s: s if isinstance(s, str) else f"{s[0]:.3g}x{s[1]:.3g}")
def test_whole_tensor_scales(dev, scale):
    """fp32 corpora are fp16 planes of x * 2^k with one k per tensor, undone by an exact power of two per product sum.  "e144": that
    power is a subnormal number when taken in one step; "e150": it is below the smallest fp32 number, while the products themselves
    (about 2^-120) are ordinary fp32 values.  The forward kernels scale by one pre-computed factor and return 0 there (include/evdr.h:
    "magnitude limit"), so the candidate sums are compared everywhere except on "e150"."""
    c = ac.scaled_case(65, 17, scale)
    corpus = corpus_of(c, dev)
    got = align_case(corpus, c, dev)
    sums = None if scale == "e150" else corpus.score_candidates(c["Q"].to(dev), c["qmask"].to(dev), c["cand"].to(dev))
    check_case(c, got, f"scaled {scale}", sums)


def test_growable_corpus_laid_out_three_binades_above_its_data(dev):
    from evdr_amd.corpus import PageCorpus
    c = ac.spread_case("f32", 65, 17)
    corpus = PageCorpus.empty(ac.MAG_NP + 2, 65, torch.float32, dev, idx_base=c["base"], absmax=8.0 * float(c["P"].abs().max()))
    corpus.append(c["P"][:3].to(dev), c["pmask"][:3].to(dev))
    corpus.append(c["P"][3:].to(dev), c["pmask"][3:].to(dev))
    sums = corpus.score_candidates(c["Q"].to(dev), c["qmask"].to(dev), c["cand"].to(dev))
    check_case(c, align_case(corpus, c, dev), "grown, absmax x 8", sums)


# ---- c. non-finite inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ac.KINDS)
def test_infinities_follow_the_rule(dev, kind):
    """+Inf / -Inf in a valid patch: a NaN pair.  Inf in a masked patch (lp = 40 crosses a tile boundary, the patch sits in the second
    tile): an ordinary pair, finite wherever the reference is.  Inf in a masked token and in a valid token: NaN pairs on every page
    with a valid patch.  The NaN pairs are the NaN entries of score_candidates."""
    from evdr_amd import ops
    lp, lq = 40, 17
    gen = torch.Generator().manual_seed(23)
    P = ac.rounded(F.normalize(torch.randn(5, lp, 128, generator=gen), dim=-1), kind)
    Q = ac.rounded(F.normalize(torch.randn(4, lq, 128, generator=gen), dim=-1), kind)
    pmask = torch.rand(5, lp, generator=gen) > 0.2
    qmask = torch.rand(4, lq, generator=gen) > 0.2
    P[0, 7, 3], pmask[0, 7] = float("inf"), True                     # valid patch, +Inf
    P[1, 30, 90], pmask[1, 30] = float("-inf"), True                 # valid patch, -Inf, second tile
    P[2, 20, 5], pmask[2, 20] = float("inf"), False                  # masked patch
    P[2, 39, 127], pmask[2, 39] = float("-inf"), False               # masked patch, the last of the page
    pmask[4] = False                                                 # a page without a valid patch never scores NaN
    Q[1, 4, 100], qmask[1, 4] = float("inf"), False                  # masked token: still a NaN pair
    Q[2, 16, 0], qmask[2, 16] = float("-inf"), True                  # valid token (the second token block)
    Q[3, 0, 0], qmask[3] = float("inf"), False                       # a query without a valid token: nothing to align, heat NaN
    cand = torch.arange(5, dtype=torch.int32)[None].expand(4, -1).contiguous()
    c = ac.with_reference(Q, qmask, P, pmask, cand, 0)
    corpus = corpus_of(c, dev)
    sim, patch, heat = align_case(corpus, c, dev)
    check_case(c, (sim, patch, heat), f"infinities {kind}")
    nan_pair = torch.isnan(heat).all(-1).cpu()
    assert torch.equal(nan_pair, torch.isnan(heat).any(-1).cpu())
    assert nan_pair.tolist() == [[True, True, False, False, False]] + [[True, True, True, True, False]] * 3
    sc = corpus.score_candidates(c["Q"].to(dev), c["qmask"].to(dev), c["cand"].to(dev)).cpu()
    has_token = qmask.any(-1)
    assert torch.equal(torch.isnan(sim).any(-1).cpu(), nan_pair & has_token[:, None])
    assert torch.equal(torch.isnan(sc)[has_token], nan_pair[has_token])
    assert bool(torch.isfinite(sim.cpu()[0, 2]).all()) and bool(torch.isfinite(heat.cpu()[0, 2][pmask[2]]).all())
    assert bool((ops.hard_patch(sim, patch).cpu()[nan_pair] == -1).all())


# ---- d. the -1e4 corner on every encoding of the flag word --------------------------------------------------------------------------------
def _corner(kind, lp, npg, masked):
    """Rows -120 e_1 against tokens 120 e_1 (every valid product -14400 < -1e4); `masked[p]` = the masked patches of page p."""
    P = torch.zeros(npg, lp, 128)
    P[:, :, 0] = -120.0
    pmask = torch.ones(npg, lp, dtype=torch.bool)
    for p, idx in masked.items():
        pmask[p, idx] = False
    return ac.rounded(P, kind), pmask


def _corner_expect(pmask, lq, qmask=None):
    """(sim, patch, heat) of one page for every token valid (or qmask): the fill at the first masked patch, else -14400 at patch 0."""
    lp = pmask.shape[0]
    masked = (~pmask).nonzero().flatten()
    v, at = (-1e4, int(masked[0])) if masked.numel() else (-14400.0, 0)
    tv = torch.ones(lq, dtype=torch.bool) if qmask is None else qmask
    sim = torch.where(tv, torch.full((lq,), v), torch.zeros(lq))
    patch = torch.where(tv, torch.full((lq,), at, dtype=torch.int32), torch.full((lq,), -1, dtype=torch.int32))
    heat = torch.where(pmask, torch.full((lp,), -14400.0), torch.full((lp,), NINF))
    return sim, patch, heat


@pytest.mark.parametrize("kind", ac.KINDS)
def test_masked_fill_corner_on_every_flag_encoding(dev, kind):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    lq = 5
    Q = torch.zeros(2, lq, 128)
    Q[:, :, 0] = 120.0
    Q = ac.rounded(Q, kind)
    qmask = torch.ones(2, lq, dtype=torch.bool)
    qmask[1, 2] = False
    # lp = 40: a masked prefix with a valid tail (one range, va = 10 > 0), the same with a hole behind it (mask words), one valid patch
    # at the very end, a fully valid page
    P, pmask = _corner(kind, 40, 4, {0: torch.arange(10), 1: torch.tensor(list(range(10)) + [25]), 2: torch.arange(39)})
    cand = torch.tensor([[0, 1, 2, 3], [3, 2, 1, 0]], dtype=torch.int32)
    corpus = PageCorpus.from_tensor(P.to(dev), pmask.to(dev))
    flags = corpus.pageflags.cpu().tolist()
    assert flags[0] & 4 and (flags[0] >> 4) & 0xFFF == 10 and not flags[1] & 4 and flags[2] & 4 and (flags[2] >> 4) & 0xFFF == 39
    got = tuple(t.cpu() for t in corpus.align(Q.to(dev), qmask.to(dev), cand.to(dev), heat=True))
    ref = ops.align_reference(Q, qmask, P, pmask, cand, heat=True)
    assert same3(got, ref)
    assert ref[1][0].tolist() == [[0] * lq, [0] * lq, [0] * lq, [0] * lq] and ref[0][0, :3].eq(-1e4).all() and ref[0][0, 3].eq(-14400.0).all()
    for q in range(2):
        for i in range(4):
            want = _corner_expect(pmask[int(cand[q, i])], lq, qmask[q])
            assert all(torch.equal(g[q, i], w) for g, w in zip(got, want)), (q, i)
    # lp = 4100: patches 0..4096 masked (va = 4097: the range encoding is abandoned, first masked index 0); only patch 4099 masked (one
    # range [0, 4099): the first masked patch is its end)
    P, pmask = _corner(kind, 4100, 2, {0: torch.arange(4097), 1: torch.tensor([4099])})
    corpus = PageCorpus.from_tensor(P.to(dev), pmask.to(dev))
    flags = corpus.pageflags.cpu().tolist()
    assert not flags[0] & 4 and (flags[0] >> 16) & 0xFFFF == 0 and flags[1] & 4 and (flags[1] >> 16) & 0xFFFF == 4099
    cand = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32)
    got = tuple(t.cpu() for t in corpus.align(Q.to(dev), qmask.to(dev), cand.to(dev), heat=True))
    for q in range(2):
        for i in range(2):
            want = _corner_expect(pmask[int(cand[q, i])], lq, qmask[q])
            assert all(torch.equal(g[q, i], w) for g, w in zip(got, want)), (q, i)
    assert got[1][0].tolist() == [[0] * lq, [4099] * lq]


@pytest.mark.parametrize("kind", ac.KINDS)
def test_the_longest_page(dev, kind):
    """lp = 65535: the flag word keeps the first masked index in 16 bits and 0xFFFF says "none".  Page 0 masks patch 65534 alone (the
    -1e4 corner: sim = -1e4 at 65534), page 1 is fully valid (-14400 at patch 0); then a fully valid page of ordinary rows, whose last
    tile holds 15 patches, with the tokens aimed at patches 0, 65520 (the last tile's first) and 65534 (the page's last)."""
    from evdr_amd.corpus import PageCorpus
    lp, lq = 65535, 2
    P, pmask = _corner(kind, lp, 2, {0: torch.tensor([65534])})
    Q = torch.zeros(1, lq, 128)
    Q[:, :, 0] = 120.0
    corpus = PageCorpus.from_tensor(P.to(dev), pmask.to(dev))
    flags = corpus.pageflags.cpu().tolist()
    assert flags[0] & 2 and (flags[0] >> 16) & 0xFFFF == 65534 and not flags[1] & 2
    cand = torch.tensor([[0, 1]], dtype=torch.int32)
    got = tuple(t.cpu() for t in corpus.align(ac.rounded(Q, kind).to(dev), None, cand.to(dev), heat=True))
    for i in range(2):
        want = _corner_expect(pmask[i], lq)
        assert all(torch.equal(g[0, i], w) for g, w in zip(got, want)), i
    assert got[1][0].tolist() == [[65534, 65534], [0, 0]]
    del corpus, P
    gen = torch.Generator().manual_seed(65535)
    P = ac.rounded(F.normalize(torch.randn(1, lp, 128, generator=gen), dim=-1), kind)
    aim = [0, 65520, 65534]
    Q = ac.rounded(F.normalize(P[0, aim].float() + 0.2 * F.normalize(torch.randn(3, 128, generator=gen), dim=-1), dim=-1), kind)[None]
    corpus = PageCorpus.from_tensor(P.to(dev), None)
    sim, patch, heat = (t.cpu() for t in corpus.align(Q.to(dev), None, torch.zeros((1, 1), dtype=torch.int32, device=dev), heat=True))
    dots = Q[0].double() @ P[0].double().T                           # (3, lp); unit rows: the project's 1e-5
    top2 = dots.topk(2, dim=-1).values
    assert bool((top2[:, 0] - top2[:, 1] > 0.1).all())               # no near tie: the index is the reference's
    assert patch[0, 0].tolist() == aim == dots.argmax(-1).tolist()
    assert (sim[0, 0].double() - dots.max(-1).values).abs().max().item() <= 1e-5
    assert (heat[0, 0].double() - dots.max(0).values).abs().max().item() <= 1e-5 and int(heat[0, 0].argmax()) in aim


# ---- e. geometry --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ac.KINDS)
def test_seventy_thousand_queries(dev, kind):
    """nq = 70 000 > 65 535 (the grid is one-dimensional): seven distinct single-token queries (one of them masked) tiled, query q
    listing page (q // 7) % 4.  The first 28 queries hold every distinct (query, page) pair and are checked against the reference;
    every later block of 28 must repeat their bits."""
    c = ac.small_case(kind, 17, 1, 4, 7, 17)
    qmask = c["qmask"].clone()
    qmask[5] = False
    pair_q, pair_p = torch.arange(28) % 7, (torch.arange(28) // 7) % 4
    c28 = ac.with_reference(c["Q"][pair_q], qmask[pair_q], c["P"], c["pmask"], pair_p.to(torch.int32)[:, None].contiguous(), 0)
    nq = 70000
    corpus = corpus_of(c28, dev)
    Q = c28["Q"].to(dev).repeat(nq // 28, 1, 1)
    qm = c28["qmask"].to(dev).repeat(nq // 28, 1)
    cand = c28["cand"].to(dev).repeat(nq // 28, 1)
    got = corpus.align(Q, qm, cand, heat=True)
    assert tuple(got[0].shape) == (nq, 1, 1) and tuple(got[2].shape) == (nq, 1, 17)
    check_case(c28, tuple(t[:28] for t in got), f"{kind} nq=70000, the 28 distinct pairs")
    for t in got:
        blocks = t.view(nq // 28, 28, -1)
        assert (same if t.is_floating_point() else torch.equal)(blocks, blocks[:1].expand_as(blocks).contiguous()), kind
    assert torch.equal(got[1][-28:], got[1][:28]) and int((got[1] >= 0).sum()) == (nq // 28) * int((c28["ref"][1] >= 0).sum())


@pytest.mark.parametrize("kind", ac.KINDS)
def test_the_longest_list(dev, kind):
    """nq = 1, r = 4096 over np = 8: every page, duplicates and the three kinds of hole.  The reference is computed once per distinct
    entry; every list position must hold the bits of its entry's first occurrence."""
    base = 1000
    c = ac.small_case(kind, 33, 17, 8, 1, 4096)
    distinct = torch.tensor([[base + p for p in range(8)] + [-1, base - 1, base + 8]], dtype=torch.int32)
    c11 = ac.with_reference(c["Q"], c["qmask"], c["P"], c["pmask"], distinct, base)
    gen = torch.Generator().manual_seed(4096)
    which = torch.cat([torch.arange(11), torch.randint(11, (4096 - 11,), generator=gen)])[torch.randperm(4096, generator=gen)]
    cand = distinct[0][which][None].contiguous()
    got = corpus_of(c11, dev).align(c11["Q"].to(dev), c11["qmask"].to(dev), cand.to(dev), heat=True)
    firsts = torch.tensor([int((which == e).nonzero()[0]) for e in range(11)])
    check_case(c11, tuple(t[:, firsts.to(dev)] for t in got), f"{kind} r=4096, the 11 distinct entries")
    for t in got:
        assert (same if t.is_floating_point() else torch.equal)(t[0], t[0, firsts.to(dev)][which.to(dev)]), kind


@pytest.mark.parametrize("scattered", [False, True], ids=["prefix", "scattered"])
@pytest.mark.parametrize("lq", [1, 16, 17, 32])
@pytest.mark.parametrize("kind", ac.KINDS)
def test_valid_counts_around_the_tile_and_round_sizes(dev, kind, lq, scattered):
    c = ac.counts_case(kind, lq, scattered)
    corpus = corpus_of(c, dev)
    got = align_case(corpus, c, dev)
    sums = corpus.score_candidates(c["Q"].to(dev), c["qmask"].to(dev), c["cand"].to(dev))
    check_case(c, got, f"{kind} lq={lq} {'scattered' if scattered else 'prefix'}", sums)
    assert int(c["qmask"][:4].sum()) == 4


@pytest.mark.parametrize("base", [-5, 0, I32_MAX - 6], ids=["negative", "zero", "top"])
def test_idx_base_at_the_ends_of_int32(dev, base):
    """Pages [base, base + 6); INT32_MIN and INT32_MAX are holes at every base (with the top base INT32_MAX is base + np exactly)."""
    c = ac.small_case("bf16", 33, 17, 6, 2, 31)
    cand = torch.tensor([[base + 5, I32_MIN, base, I32_MAX, base + 2, base - 1 if base > I32_MIN else I32_MIN],
                         [I32_MAX, base + 1, base + 1, I32_MIN, base + 4, base + 3]], dtype=torch.int64).clamp(I32_MIN, I32_MAX).to(torch.int32)
    cb = ac.with_reference(c["Q"], c["qmask"], c["P"], c["pmask"], cand, base)
    holes = (cand.long() < base) | (cand.long() >= base + 6)
    assert int(holes.sum()) == 5 and torch.equal(cb["ref"][0][holes], torch.full((5, 17), NINF))
    check_case(cb, align_case(corpus_of(cb, dev), cb, dev), f"idx_base={base}")


# ---- f. the C entry, directly ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [1, 5])
@pytest.mark.parametrize("kind", ac.KINDS)
def test_c_abi_direct_with_page_and_plane_strides(dev, kind, gap):
    """evdr_maxsim_align through ctypes on planes that are rows of a wider buffer: p_stride = lp * 128 + 8 * gap elements, a plane
    stride that is not np * p_stride, base pointers 16 bytes into their allocations, every element between and behind the pages NaN;
    with and without the heat output.  The outputs must have the bits of the dense layout."""
    from evdr_amd import _lib as L
    c = ac.small_case(kind, 33, 17, 5, 3, 7 + gap)
    corpus = corpus_of(c, dev)
    Q, qm, cand = c["Q"].to(dev), c["qmask"].to(dev), c["cand"].to(dev)
    dense = corpus.align(Q, qm, cand, heat=True)
    qp, qa = corpus._query_planes(Q)
    npl, npg, lp, _ = corpus.planes.shape
    nq, lq = 3, 17
    p_stride = lp * 128 + 8 * gap
    plane_stride = npg * p_stride + 64
    nan_bits = 0x7FC0 if kind == "bf16" else 0x7E00
    pbuf = torch.full((8 + npl * plane_stride + 256,), nan_bits, dtype=torch.int16, device=dev)
    pages = pbuf[8:8 + npl * plane_stride].view(npl, plane_stride)[:, :npg * p_stride].view(npl, npg, p_stride)
    pages[:, :, :lp * 128] = corpus.planes.view(torch.int16).reshape(npl, npg, lp * 128)
    qbuf = torch.full((8 + qp.numel() + 256,), nan_bits, dtype=torch.int16, device=dev)
    qbuf[8:8 + qp.numel()] = qp.view(torch.int16).flatten()
    assert pbuf.data_ptr() % 256 == 0 and (p_stride * 2) % 16 == 0 and plane_stride != npg * p_stride
    lib = L.load()
    esz = 2
    for want_heat in (True, False):
        sim = torch.full((nq, 5, lq), 7.0, device=dev)
        patch = torch.full((nq, 5, lq), 7, dtype=torch.int32, device=dev)
        heat = torch.full((nq, 5, lp), 7.0, device=dev) if want_heat else None
        L.check(lib.evdr_maxsim_align(qbuf.data_ptr() + 8 * esz, pbuf.data_ptr() + 8 * esz, L.ptr(qm), L.ptr(corpus.tilemask),
                                      L.ptr(corpus.pageflags), L.ptr(cand), 5, 0, L.ptr(sim), L.ptr(patch), L.ptr(heat), nq, lq, npg, lp,
                                      npl, p_stride, plane_stride, L.ptr(qa), L.ptr(corpus.amax), L.current_stream_handle(dev)))
        assert same(sim, dense[0]) and torch.equal(patch, dense[1]), (kind, gap, want_heat)
        if want_heat:
            assert same(heat, dense[2]), (kind, gap)
    assert bool((pages[:, :, lp * 128:] == nan_bits).all()) and bool((pbuf[-256:] == nan_bits).all()) and bool((pbuf[:8] == nan_bits).all())
    check_case(c, dense, f"c abi {kind} gap={gap}")


# ---- g. launch forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_heat", [False, True], ids=["noheat", "heat"])
@pytest.mark.parametrize("kind", ac.KINDS)
def test_graph_capture_replays_the_eager_bits(dev, kind, want_heat):
    """One captured launch of ops.maxsim_align on static query planes, mask and list; two replays with the query and the list changed
    in place in between, each equal to the eager call on the same contents."""
    from evdr_amd import ops
    a, b = ac.small_case(kind, 65, 17, 6, 3, 101), ac.small_case(kind, 65, 17, 6, 3, 102)
    corpus = corpus_of(a, dev)
    planes = [corpus._query_planes(x["Q"].to(dev)) for x in (a, b)]
    lists = [a["cand"].to(dev), a["cand"].flip(1).contiguous().to(dev)]
    lists[1][0, 0] = -1
    masks = [a["qmask"].to(dev), b["qmask"].to(dev)]

    def run(qp, qa, qm, cand):
        return ops.maxsim_align(qp, qa, corpus.planes, corpus.amax, qm, corpus.tilemask, corpus.pageflags, cand, idx_base=0, heat=want_heat)
    eager = [tuple(t.clone() for t in run(planes[k][0], planes[k][1], masks[k], lists[k])) for k in (0, 1)]
    assert not same3(eager[0], eager[1])
    qp, qa = planes[0][0].clone(), None if planes[0][1] is None else planes[0][1].clone()
    qm, cand = masks[0].clone(), lists[0].clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(qp, qa, qm, cand)                                        # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(qp, qa, qm, cand)
    for k in (1, 0):
        qp.copy_(planes[k][0])
        if qa is not None:
            qa.copy_(planes[k][1])
        qm.copy_(masks[k])
        cand.copy_(lists[k])
        graph.replay()
        torch.cuda.synchronize()
        assert same3(out, eager[k]), (kind, want_heat, k)


def test_two_streams_alternate_shapes_without_a_sync(dev):
    cases = (ac.small_case("bf16", 65, 17, 6, 3, 201), ac.small_case("f32", 1030, 32, 4, 3, 202))
    corpora = [corpus_of(c, dev) for c in cases]
    args = [tuple(c[k].to(dev) for k in ("Q", "qmask", "cand")) for c in cases]
    serial = [corpus.align(*a, heat=True) for corpus, a in zip(corpora, args)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    outs = []
    for r in range(6):
        k = (r + r // 2) % 2                                         # stream 0: small, large, small; stream 1: large, small, large
        with torch.cuda.stream(streams[r % 2]):
            outs.append((k, corpora[k].align(*args[k], heat=True)))
    torch.cuda.synchronize()
    for r, (k, got) in enumerate(outs):
        assert same3(got, serial[k]), f"launch {r} on stream {r % 2}, shape {k}"
    for c, got in zip(cases, serial):
        check_case(c, got, "two streams, serial run")


@pytest.mark.parametrize("kind", ac.KINDS)
def test_growable_corpus_slots_views_and_replace(dev, kind):
    """A list entry naming a reserved but unfilled slot is a hole, for the corpus and for a view taken before an append; after the
    append the same list aligns the new page on the corpus while the old view still reports a hole; after replace() the alignment is
    that of from_tensor of the new contents."""
    from evdr_amd.corpus import PageCorpus
    c = ac.small_case(kind, 65, 17, 6, 3, 301)
    P, pm, Q, qm = (c[k].to(dev) for k in ("P", "pmask", "Q", "qmask"))
    base = 50
    cand = (c["cand"] + base).to(dev)                                # every query lists the slots 0..5
    kw = dict(absmax=float(c["P"].abs().max())) if kind == "f32" else {}       # from_tensor's own absmax word
    grown = PageCorpus.empty(8, 65, ac.DTYPE[kind], dev, idx_base=base, **kw)
    grown.append(P[:4], pm[:4])
    view = grown.shard(0, 4)
    whole = PageCorpus.empty(8, 65, ac.DTYPE[kind], dev, idx_base=base, **kw)
    whole.append(P, pm)
    want = whole.align(Q, qm, cand, heat=True)
    before, seen = grown.align(Q, qm, cand, heat=True), view.align(Q, qm, cand, heat=True)
    for got in (before, seen):
        assert same3(tuple(t[:, :4] for t in got), tuple(t[:, :4] for t in want))
        assert bool((got[0][:, 4:] == NINF).all()) and bool((got[1][:, 4:] == -1).all()) and bool((got[2][:, 4:] == NINF).all())
    assert grown.append(P[4:], pm[4:]) == base + 4
    assert same3(grown.align(Q, qm, cand, heat=True), want)
    assert same3(view.align(Q, qm, cand, heat=True), seen)           # the old view keeps its range: slots 4, 5 stay holes
    # replace page 2 by page 5's content (and its mask)
    grown.replace(torch.tensor([base + 2]), P[5:6], pm[5:6])
    P2, pm2 = P.clone(), pm.clone()
    P2[2], pm2[2] = P[5], pm[5]
    fresh = PageCorpus.from_tensor(P2, pm2, idx_base=base)
    assert ac.shift_of(P2) == ac.shift_of(P)                         # fp32: the same power of two, hence the same planes
    got = grown.align(Q, qm, cand, heat=True)
    assert same3(got, fresh.align(Q, qm, cand, heat=True))
    assert same3(tuple(t[:, 2] for t in got), tuple(t[:, 5] for t in want))
    c2 = ac.with_reference(c["Q"], c["qmask"], P2.cpu(), pm2.cpu(), c["cand"] + base, base)
    check_case(c2, got, f"{kind} after replace")


@pytest.mark.parametrize("width", [64, 100])
@pytest.mark.parametrize("kind", ac.KINDS)
def test_narrow_corpora_ride_on_zero_columns(dev, kind, width):
    gen = torch.Generator().manual_seed(400 + width)
    P = ac.rounded(F.normalize(torch.randn(4, 33, width, generator=gen), dim=-1), kind)
    Q = ac.rounded(F.normalize(torch.randn(3, 17, width, generator=gen), dim=-1), kind)
    pmask = torch.rand(4, 33, generator=gen) < 0.8
    pmask[:, 0] = True
    qmask = torch.rand(3, 17, generator=gen) < 0.8
    qmask[:, 0] = True
    cand = torch.arange(4, dtype=torch.int32)[None].expand(3, -1).contiguous()
    c = ac.with_reference(Q, qmask, P, pmask, cand, 0)               # the reference on the unpadded rows
    corpus = corpus_of(c, dev)
    assert corpus.planes.shape[-1] == 128
    check_case(c, align_case(corpus, c, dev), f"{kind} width {width}",
               corpus.score_candidates(Q.to(dev), qmask.to(dev), cand.to(dev)))
