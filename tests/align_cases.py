"""Seeded inputs shared by tests/test_align_cases_host.py and tests/test_gpu_align_edges.py, each built once on the
CPU and never modified: tie pages (exact ties placed so that every level of the kernel's selection has one to decide), rows of mixed
and of extreme magnitude, and the geometry cases.

The selection has three levels (csrc/align.hip).  A lane (c = m & 15) of wave w = (m >> 4) & 3 walks the tiles w, w + 4, ... of its
wave (round = m >> 6) and keeps the first maximum with a strict >; the 16 lanes of a wave are reduced, ties to the lower index; the
four waves are merged through LDS, ties to the lower index; the masked patches' -1e4 joins last.  Which copy of a tied row each level
sees decides what a wrong rule at that level changes:
  walk    two equal products in the SAME lane of the SAME wave, in different rounds (m and m + 64);
  lanes   two equal products in one wave, in different lanes;
  merge   two equal products in different waves.
Copies that all lie in different lanes, tiles, waves and rounds would reach the merge only -- `>=` in the walk or a lane reduction
that prefers the higher index would pass them --, so the placement below gives every row of a page of two rounds or more one pair of
each kind."""
import functools

import torch
import torch.nn.functional as F

from cluster_cases import near_tie_pages

KINDS = ("bf16", "f32")
DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}
TIE_LPS = (16, 17, 63, 64, 65, 127, 128, 129, 257, 1030)
TIE_LQ = 32
BIG = 0x7FFFFFFF


def rounded(x: torch.Tensor, kind: str) -> torch.Tensor:
    return x.to(DTYPE[kind])


def tie_variants(lp: int) -> tuple:
    """Mask variants of a tie page: "none" (every patch valid), "random" (80 % + a whole tile + a whole mask word), and, on pages of
    four tiles or more, "tile0" (80 % + tile 0) and "wave" (80 % + every tile of wave 1).  Shorter pages would be left with no valid
    patch, or with one."""
    return ("none", "random", "tile0", "wave") if lp >= 63 else ("none", "random")


# ---- tie pages -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_rows(lp: int) -> tuple:
    """The fixed permutation: ceil(lp / 4) rows, each a sorted tuple of the positions that hold its copies; every position of the page
    belongs to exactly one row.
    A block of 128 positions (two rounds of the four waves) holds 32 rows (w, k), w = 0..3, k = 0..7, each kept if the page has all four
    of its positions:
        c0 = (round 0, wave w, lane 2k)            the lowest copy
        c2 = (round 0, wave w, lane 2k + 1)        the same tile, the next lane                 -> the lane reduction
        c1 = (round 1, wave w, lane 2k)            the same wave and lane, the next round       -> the walk's >
        c3 = (round 1, wave (w + 1) & 3, 2k + 1)   another wave (a LOWER one for w = 3)          -> the merge
    Four copies in three tiles, two rounds, two waves and two lanes.  The positions no such row took (all of a page of 65 patches
    or fewer, the tail of a longer one) are paired with their neighbour, and pair i shares a row with pair i + ceil(pairs / 2): two
    adjacent lanes of one tile and two of a tile half the remainder further on -- on a page of 64 patches the tiles T and T + 2, i.e.
    a lane pair and a wave pair; the last rows of an odd remainder have three, two or one copy."""
    rows, used = [], set()
    for b in range((lp + 127) // 128):
        for w in range(4):
            for k in range(8):
                at = lambda rnd, wave, lane: 128 * b + 64 * rnd + 16 * wave + lane   # noqa: E731
                c = (at(0, w, 2 * k), at(0, w, 2 * k + 1), at(1, w, 2 * k), at(1, (w + 1) & 3, 2 * k + 1))
                if max(c) < lp:
                    rows.append(tuple(sorted(c)))
                    used.update(c)
    left = [m for m in range(lp) if m not in used]
    duos = [left[i:i + 2] for i in range(0, len(left), 2)]
    half = (len(duos) + 1) // 2
    for r in range(half):
        rows.append(tuple(sorted(duos[r] + (duos[r + half] if r + half < len(duos) else []))))
    assert len(rows) == (lp + 3) // 4 and sorted(m for row in rows for m in row) == list(range(lp))
    return tuple(rows)


def _structural(lp: int, variant: str) -> torch.Tensor:
    """The patches a variant masks by rule (True = masked), before the random 80 %."""
    s = torch.zeros(lp, dtype=torch.bool)
    ntiles = (lp + 15) // 16
    if variant == "random":
        if ntiles >= 4:
            s[32:48] = True                                              # tile 2: a whole tile, the low half of word 1
        if ntiles >= 8:
            s[96:128] = True                                             # word 3: tiles 6 and 7
    elif variant == "tile0":
        s[:16] = True
    elif variant == "wave":
        for t in range(1, ntiles, 4):                                    # every tile wave 1 owns
            s[16 * t:16 * t + 16] = True
    return s


@functools.lru_cache(maxsize=None)
def tie_page(kind: str, lp: int, seed: int = 0, variant: str = "none") -> dict:
    """One page of ceil(lp / 4) near-tie rows (cluster_cases.near_tie_pages: eps 1e-6 for fp32, 1 / 16 for bf16), row i copied to
    the positions tie_rows(lp)[i], its mask, and a query of 32 tokens that each pick one chosen row.
    Mask ("random", "tile0", "wave"; "none" masks nothing): the variant's structural part (a whole tile and a whole 32-patch word;
    tile 0; every tile of wave 1) over a random 80 %.  The rows with four copies that the structural part leaves alone are split in
    turn into class V -- all four copies forced valid -- and class M -- the lowest copy forced masked, the other three valid --;
    further rows lose their lowest copy until a quarter of all rows have.
    Query: token n is l2norm(row - mean row) of a class V row (n even) or a class M row (n odd), rounded to the dtype: its product
    with its own row exceeds every other row's by about |row - mean|, far above the accumulation error, so the token's maximum lies
    on the copies of that row (asserted on the host), and every level has an exact tie to decide for half of the tokens or more.
    Returns P (1, lp, 128), pmask (1, lp), Q (32, 128), rows, row_of_token (32,), klass (32,) of "V" / "M"."""
    rows = tie_rows(lp)
    src = near_tie_pages(1, len(rows), 128, 1e-6 if kind == "f32" else 1 / 16, 1000 * lp + seed, DTYPE[kind])[0]
    P = torch.empty((lp, 128), dtype=DTYPE[kind])
    for i, row in enumerate(rows):
        P[list(row)] = src[i]
    # rows a token may be aimed at: four copies, and the row's own token prefers it to every other row by a clear margin (float64; two
    # bf16 rows that moved the same few elements can come too close)
    mean = P.double().mean(0)
    aim = F.normalize(src.double() - mean, dim=-1) @ src.double().T
    own = aim.diagonal().clone()
    aim.fill_diagonal_(float("-inf"))
    full = [i for i, row in enumerate(rows) if len(row) == 4 and float(own[i] - aim[i].max()) > 2e-6]
    pm = torch.ones(lp, dtype=torch.bool)
    if variant == "none":
        vrows, mrows = full, []
    else:
        gen = torch.Generator().manual_seed(77 * lp + seed + len(variant))
        s = _structural(lp, variant)
        pm = (torch.rand(lp, generator=gen) < 0.8) & ~s
        free = [i for i in full if not bool(s[list(rows[i])].any())]
        vrows, mrows = free[0::2], free[1::2]
        for i in vrows:
            pm[list(rows[i])] = True
        for i in mrows:
            pm[list(rows[i])] = True
            pm[rows[i][0]] = False
        lowest_masked = lambda: sum(1 for row in rows if not bool(pm[row[0]]))   # noqa: E731
        for i, row in enumerate(rows):
            if lowest_masked() * 4 >= len(rows):
                break
            if i not in vrows and i not in mrows:
                pm[row[0]] = False
    assert vrows, (lp, variant)
    tok, row_of_token, klass = [], [], []
    for n in range(TIE_LQ):
        cls = mrows if (n % 2 == 1 and mrows) else vrows
        i = cls[((n // 2) * 11) % len(cls)]                               # a stride that visits every wave's rows
        tok.append(F.normalize(src[i].double() - mean, dim=-1))
        row_of_token.append(i)
        klass.append("M" if cls is mrows else "V")
    Q = rounded(torch.stack(tok).float(), kind)
    return dict(P=P[None], pmask=pm[None], Q=Q, rows=rows, row_of_token=tuple(row_of_token), klass=tuple(klass), lp=lp, kind=kind)


def products_fp32(Q: torch.Tensor, P: torch.Tensor) -> torch.Tensor:
    """(lq, lp) fp32 products on the CPU, every pair summed by the same reduction: identical patch rows give identical bits."""
    return (Q.float()[:, None, :] * P.float()[None, :, :]).sum(-1)


def select(V: torch.Tensor, pmask: torch.Tensor, walk_ge: bool = False, lanes_high: bool = False, merge: str = "low"):
    """The kernel's three-level selection on a product matrix V (lq, lp) and a mask (lp,), in plain torch: (value (lq,), index (lq,)).
    walk_ge: `>=` in the tile walk (the LAST round of a lane's maximum); lanes_high: the lane reduction prefers the higher index;
    merge: "low" (the rule), "high" (the higher index), "first" / "last" (the wave order decides, not the index)."""
    lq, lp = V.shape
    rounds = (lp + 63) // 64
    ninf = float("-inf")
    v = torch.full((lq, rounds * 64), ninf)
    v[:, :lp] = torch.where(pmask[None, :], V, torch.full_like(V, ninf))
    idx = torch.arange(rounds * 64).view(rounds, 4, 16)
    v = v.view(lq, rounds, 4, 16)

    def pick(val, ix, dim, high):
        """(max, the lowest / highest index among the entries that attain it) along dim; -inf keeps BIG."""
        top = val.max(dim=dim, keepdim=True).values
        hit = (val == top) & (val > ninf)
        if high:
            out = torch.where(hit, ix, torch.full_like(ix, -1)).max(dim=dim).values
            out = torch.where(out < 0, torch.full_like(out, BIG), out)
        else:
            out = torch.where(hit, ix, torch.full_like(ix, BIG)).min(dim=dim).values
        return top.squeeze(dim), out

    ix = idx[None].expand(lq, -1, -1, -1)
    val, ix = pick(v, ix, 1, walk_ge)                                    # rounds -> (lq, 4, 16)
    val, ix = pick(val, ix, 2, lanes_high)                               # lanes  -> (lq, 4)
    if merge in ("low", "high"):
        val, ix = pick(val, ix, 1, merge == "high")
    else:
        top = val.max(dim=1, keepdim=True).values
        hit = (val == top) & (val > ninf)
        order = torch.arange(4)[None].expand(lq, -1)
        w = torch.where(hit, order, torch.full_like(order, 9 if merge == "first" else -1))
        w = (w.min(1).values if merge == "first" else w.max(1).values).clamp(0, 3)
        val, ix = top[:, 0], ix.gather(1, w[:, None])[:, 0]
    if not bool(pmask.all()):                                            # the masked patches' -1e4 at the first masked index
        fm = int((~pmask).nonzero()[0])
        take = (val < -1e4) | ((val == -1e4) & (fm < ix))
        val = torch.where(take, torch.full_like(val, -1e4), val)
        ix = torch.where(take, torch.full_like(ix, fm), ix)
    return val, ix


# ---- magnitudes --------------------------------------------------------------------------------------------------------------------------
MAG_NP, MAG_NQ, MAG_BASE = 4, 3, 40


def _mag_masks_and_list(lp: int, lq: int, gen):
    lens = torch.randint(max(1, lp // 2), lp + 1, (MAG_NP,), generator=gen)
    lens[0] = lp
    pmask = (torch.arange(lp)[None, :] < lens[:, None]) & (torch.rand(MAG_NP, lp, generator=gen) > 0.1)
    pmask[:, 0] = True
    qmask = torch.rand(MAG_NQ, lq, generator=gen) > 0.2
    qmask[:, 0] = True
    b = MAG_BASE
    cand = torch.tensor([[b + 0, b + 1, b + 2, b + 3, -1], [b + 3, b + 3, b + 0, b + MAG_NP, b + 2], [b + 1, b + 2, b - 1, b + 0, b + 3]],
                        dtype=torch.int32)
    return pmask, qmask, cand


def with_reference(Q, qmask, P, pmask, cand, base) -> dict:
    """The case and what the magnitude checks need, in float64 of the rounded inputs: `dots` (nq, r, lq, lp) of the listed pages
    (holes read page 0 and are never looked at), `filled` with -1e4 on the masked patches, the top-two `gap` of every token, the row
    norms `qn` (nq, lq) and `pn` (np, lp), `pmax` (np,) = the largest norm of a VALID patch, and ops.align_reference's outputs."""
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    npg, lp, _ = P.shape
    loc = (cand.long() - base).clamp(0, npg - 1)
    dots = torch.einsum("qnd,qrmd->qrnm", Q.double(), P.double()[loc])
    filled = torch.where(pmask[loc][:, :, None, :], dots, torch.full_like(dots, -1e4))
    top = filled.topk(min(2, lp), dim=-1).values
    gap = top[..., 0] - top[..., 1] if lp > 1 else torch.full_like(top[..., 0], float("inf"))
    qn, pn = Q.double().norm(dim=-1), P.double().norm(dim=-1)
    pmax = torch.where(pmask, pn, torch.zeros_like(pn)).max(dim=-1).values
    ref = ops.align_reference(Q, qmask, P, pmask, cand, idx_base=base, heat=True)
    return dict(Q=Q, qmask=qmask, P=P, pmask=pmask, cand=cand, base=base, loc=loc, dots=dots, filled=filled, gap=gap, qn=qn, pn=pn,
                pmax=pmax, ref=ref)


@functools.lru_cache(maxsize=None)
def spread_case(kind: str, lp: int, lq: int, seed: int = 0) -> dict:
    """Rows of mixed norms in one tensor: unit Gaussian rows times 2^j * (1 + u), j uniform in -6..6 and u in [0, 1) per row, rounded
    to the corpus dtype; ragged and randomly masked pages, masked tokens, a list with duplicates and the three kinds of hole."""
    gen = torch.Generator().manual_seed(50000 + 100 * lp + lq + 7919 * seed)

    def rows(n, length):
        x = F.normalize(torch.randn(n, length, 128, generator=gen), dim=-1)
        j = torch.randint(-6, 7, (n, length, 1), generator=gen).float()
        return rounded(x * torch.exp2(j) * (1 + torch.rand(n, length, 1, generator=gen)), kind)
    P, Q = rows(MAG_NP, lp), rows(MAG_NQ, lq)
    pmask, qmask, cand = _mag_masks_and_list(lp, lq, gen)
    return with_reference(Q, qmask, P, pmask, cand, MAG_BASE)


SPREAD = (("bf16", 65, 17), ("bf16", 129, 32), ("f32", 65, 17), ("f32", 129, 32), ("f32", 33, 16))

# whole-tensor scales of fp32 unit rows (sq, sp); "e144" / "e150": both tensors scaled so that their absmax is 1.5 * 2^-58 / 1.5 * 2^-61,
# i.e. the shifts of the fp16 planes sum to kq + kp = 144 / 150
SCALES = ((2.0 ** -40, 2.0 ** 30), (3e-4, 1.0), (1.0, 37.5), (1e3, 1e-3), (2.0 ** 60, 2.0 ** -60), "e144", "e150")
EDGE_ABSMAX = {"e144": 1.5 * 2.0 ** -58, "e150": 1.5 * 2.0 ** -61}


@functools.lru_cache(maxsize=None)
def scaled_case(lp: int, lq: int, scale) -> dict:
    """fp32 unit rows times one scale per tensor: scale = (sq, sp), or "e144" / "e150" (see SCALES).  Seeded by the shape alone, so
    that every scale sees the same directions."""
    gen = torch.Generator().manual_seed(60000 + 100 * lp + lq)
    P = F.normalize(torch.randn(MAG_NP, lp, 128, generator=gen), dim=-1)
    Q = F.normalize(torch.randn(MAG_NQ, lq, 128, generator=gen), dim=-1)
    if isinstance(scale, str):
        P = P * (EDGE_ABSMAX[scale] / P.abs().max().double()).float()
        Q = Q * (EDGE_ABSMAX[scale] / Q.abs().max().double()).float()
    else:
        Q, P = Q * scale[0], P * scale[1]
    pmask, qmask, cand = _mag_masks_and_list(lp, lq, gen)
    return with_reference(Q.float(), qmask, P.float(), pmask, cand, MAG_BASE)


def shift_of(x: torch.Tensor) -> int:
    """k of the fp16 hi/lo planes of an fp32 tensor: 141 - the biased exponent of its absmax (evdr_h2_shift)."""
    e = (int(x.float().abs().max().view(torch.int32)) >> 23) & 0xFF
    return 0 if e in (0, 255) else 141 - e


def split_emulation(Q: torch.Tensor, P: torch.Tensor) -> torch.Tensor:
    """(nq, np, lq, lp) float64: the products as the fp16 hi/lo planes represent them -- hi = fp16(x * 2^k), lo = fp16(x * 2^k - hi),
    lo x hi + hi x lo + hi x hi summed in float64 and scaled back, lo x lo dropped."""
    def split(x):
        k = shift_of(x)
        f = torch.ldexp(x.double(), torch.tensor(k)).float()
        hi = f.half()
        lo = (f - hi.float()).half()
        return hi.double(), lo.double(), k
    qh, ql, kq = split(Q)
    ph, pl, kp = split(P)
    e = lambda a, b: torch.einsum("qnd,pmd->qpnm", a, b)                 # noqa: E731
    return torch.ldexp(e(ql, ph) + e(qh, pl) + e(qh, ph), torch.tensor(-(kq + kp)))


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
VALID_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def counts_case(kind: str, lq: int, scattered: bool) -> dict:
    """lp = 80, page i with VALID_COUNTS[i] valid patches (the first nv, or nv scattered); query j < 4 has ONE valid token, at position
    (0, 15, 16, 31)[j] clamped to lq - 1, query 4 a random 80 % mask; every query lists every page."""
    lp, npg = 80, len(VALID_COUNTS)
    gen = torch.Generator().manual_seed(70000 + lq + 1000 * scattered + (kind == "f32"))
    P = rounded(F.normalize(torch.randn(npg, lp, 128, generator=gen), dim=-1), kind)
    Q = rounded(F.normalize(torch.randn(5, lq, 128, generator=gen), dim=-1), kind)
    pmask = torch.zeros(npg, lp, dtype=torch.bool)
    for i, nv in enumerate(VALID_COUNTS):
        pmask[i, torch.randperm(lp, generator=gen)[:nv] if scattered else torch.arange(nv)] = True
    qmask = torch.zeros(5, lq, dtype=torch.bool)
    for j, at in enumerate((0, 15, 16, 31)):
        qmask[j, min(at, lq - 1)] = True
    qmask[4] = torch.rand(lq, generator=gen) < 0.8
    qmask[4, 0] = True
    cand = torch.arange(npg, dtype=torch.int32)[None].expand(5, -1).contiguous()
    return with_reference(Q, qmask, P, pmask, cand, 0)


@functools.lru_cache(maxsize=None)
def small_case(kind: str, lp: int, lq: int, npg: int, nq: int, seed: int, masked: bool = True) -> dict:
    """Unit rows of `kind`, random 80 % page and token masks (first patch / token valid), every query listing every page."""
    gen = torch.Generator().manual_seed(80000 + seed)
    P = rounded(F.normalize(torch.randn(npg, lp, 128, generator=gen), dim=-1), kind)
    Q = rounded(F.normalize(torch.randn(nq, lq, 128, generator=gen), dim=-1), kind)
    pmask = torch.rand(npg, lp, generator=gen) < (0.8 if masked else 2.0)
    pmask[:, 0] = True
    qmask = torch.rand(nq, lq, generator=gen) < (0.8 if masked else 2.0)
    qmask[:, 0] = True
    cand = torch.arange(npg, dtype=torch.int32)[None].expand(nq, -1).contiguous()
    return with_reference(Q, qmask, P, pmask, cand, 0)


def geometry_cases():
    """Every (name, case) of the geometry, C-entry and launch-form tests that is held to the index rule: the host test asserts their
    near-tie share, a condition on the inputs alone."""
    for kind in KINDS:
        for lq in (1, 16, 17, 32):
            for scattered in (False, True):
                yield f"counts {kind} lq={lq} scattered={scattered}", counts_case(kind, lq, scattered)
        yield f"nq 70000 {kind}", small_case(kind, 17, 1, 4, 7, 17)
        yield f"r 4096 {kind}", small_case(kind, 33, 17, 8, 1, 4096)
        for gap in (1, 5):
            yield f"c abi {kind} gap={gap}", small_case(kind, 33, 17, 5, 3, 7 + gap)
        yield f"growable {kind}", small_case(kind, 65, 17, 6, 3, 301)
    yield "idx_base", small_case("bf16", 33, 17, 6, 2, 31)
    yield "streams bf16", small_case("bf16", 65, 17, 6, 3, 201)
    yield "streams f32", small_case("f32", 1030, 32, 4, 3, 202)
