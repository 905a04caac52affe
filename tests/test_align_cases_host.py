"""The power of the cases of tests/test_gpu_align_edges.py (tests/align_cases.py), shown on the CPU before a GPU
sees them: the tie pages give every level of the kernel's selection an exact tie to decide, the magnitude cases keep the near-tie
share of the index rule under its cap, and the fp16 hi/lo planes represent their products well inside the value bound.

Tie pages.  align_cases.select restates the selection (walk with a strict >, 16-lane reduction, four-wave merge, the -1e4 join) on a
CPU fp32 product matrix; with the rule in place it must return the first index of the maximum.  Each mutation below is then applied
alone and the valid tokens (all 32) whose pick changes are counted, per (kind, lp, mask variant); the counts are the same for bf16
and fp32, they depend on the placement and the mask only:

    mutation                                  lp = 16, 17        63, 64, 65         127, 128, 129, 257, 1030
    first -> last index of the maximum        32                 32                 32
    >= in the tile walk                       0 (one round)      0 (one round)      32 unmasked, 16 masked (class V)
    lane reduction to the higher index        32                 32 unm., 16 m.     32
    merge to the higher index                 0 (one tile *)     32                 32
    merge by wave order: first + last wave    0                  0 + 32             32 in all, 0..17 of them by "first"
    lowest copy even if masked                16 masked (class M), 0 unmasked (nothing is masked)
    (*) lp = 17: patch 16 alone is in a second tile, in a row of three copies that no token is aimed at.

"At least half of the valid tokens" is asserted for every mutation at every level a page has: the walk needs two rounds (lp >= 127
here), the merge two tiles that hold copies of one row (lp >= 63), the masked-lowest rule a mask.  A merge that lets the wave order
decide is two mutants -- the first or the last wave that holds the maximum wins --; a row's cross-wave copy lies either in a later or
in an earlier wave, so each row is caught by exactly one of them and the two counts are asserted together; "first" needs a copy in
a LOWER wave at a HIGHER index, i.e. a second round and a row of wave 3 (none is left whole by the "random" variant's masked tiles).

Magnitudes.  Share of valid tokens whose float64 top-two gap is <= 2e-5 * |q_n| * max_m |p_m| (valid patches), per case, cap 1 %:
0 of 152..324 valid tokens in every spread case, 0 of 164 in every scaled case; the geometry cases at most 0.71 %.
Representation error of the fp16 hi/lo planes over |q_n| |p_m|, worst fp32 spread case: 3.4e-8 (bound 1e-6)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_cases as ac  # noqa: E402

NEAR_TIE_CAP, GAP_REL, REPR_TOL = 0.01, 2e-5, 1e-6
TIE_CASES = [(kind, lp, v) for kind in ac.KINDS for lp in ac.TIE_LPS for v in ac.tie_variants(lp)]


def _pairs(row, pm):
    """The kinds of exact tie the lowest VALID copy of a row has with its other valid copies."""
    valid = [m for m in row if bool(pm[m])]
    out = set()
    if len(valid) >= 2:
        m0 = valid[0]
        for m in valid[1:]:
            same_wave = ((m >> 4) & 3) == ((m0 >> 4) & 3)
            if same_wave and (m & 15) == (m0 & 15):
                out.add("walk")
            elif same_wave:
                out.add("lanes")
            else:
                out.add("merge")
    return out


@pytest.mark.parametrize("lp", ac.TIE_LPS)
def test_tie_rows_place_a_pair_for_every_level(lp):
    rows = ac.tie_rows(lp)
    assert len(rows) == (lp + 3) // 4
    assert sorted(m for row in rows for m in row) == list(range(lp))       # a permutation: every position in exactly one row
    everything = torch.ones(lp, dtype=torch.bool)
    block = [row for row in rows if len(row) == 4 and row[0] + 64 in row]  # rows of a two-round block
    assert len(block) == (32 * (lp // 128) if lp != 127 else 31)
    for row in block:
        assert len({m >> 4 for m in row}) == 3 and len({m >> 6 for m in row}) == 2
        assert len({(m >> 4) & 3 for m in row}) == 2 and len({m & 15 for m in row}) == 2
        assert row[0] + 64 in row and row[0] + 1 in row                    # the walk's pair, the lane pair (same tile)
        assert _pairs(row, everything) == {"walk", "lanes", "merge"}
    rest = [row for row in rows if row not in block]
    tiles_left = len({m >> 4 for row in rest for m in row})
    for row in rest:
        if len(row) >= 2:
            assert row[1] == row[0] + 1 and "lanes" in _pairs(row, everything) or (row[0] & 15) == 15
        if len(row) == 4 and tiles_left >= 4:
            assert len({(m >> 4) & 3 for m in row}) == 2 and "merge" in _pairs(row, everything)
        assert len({(m >> 4, m & 15) for m in row}) == len(row)
    assert sum(len(row) < 4 for row in rows) <= 2


@pytest.mark.parametrize("kind,lp,variant", TIE_CASES)
def test_tie_pages_have_teeth(kind, lp, variant):
    c = ac.tie_page(kind, lp, 0, variant)
    rows, pm = c["rows"], c["pmask"][0]
    ntiles = (lp + 15) // 16
    # ---- the mask
    if variant == "none":
        assert bool(pm.all())
    else:
        share = pm.float().mean().item()
        assert 0.35 <= share <= 0.9, share
        assert sum(1 for row in rows if not bool(pm[row[0]])) * 4 >= len(rows)        # the lowest copy masked in a quarter of the rows
        tiles_masked = [t for t in range(ntiles) if not bool(pm[16 * t:16 * t + 16].any())]
        if variant == "random" and ntiles >= 4:
            assert 2 in tiles_masked
        if variant == "random" and ntiles >= 8:
            assert 6 in tiles_masked and 7 in tiles_masked                             # mask word 3
        if variant == "tile0":
            assert 0 in tiles_masked
        if variant == "wave":
            assert all(t in tiles_masked for t in range(1, ntiles, 4))
    # ---- every row ties or is absent from the "must tie" set
    must_tie = {i for i, row in enumerate(rows) if sum(bool(pm[m]) for m in row) >= 2}
    assert set(c["row_of_token"]) <= must_tie
    # ---- the products: token n's maximum lies on the copies of its row, on all of the valid ones
    V = ac.products_fp32(c["Q"], c["P"][0])
    ninf = torch.full_like(V, float("-inf"))
    top = torch.where(pm[None], V, ninf).max(dim=1).values
    for n, i in enumerate(c["row_of_token"]):
        at = set(((V[n] == top[n]) & pm).nonzero().flatten().tolist())
        assert at == {m for m in rows[i] if bool(pm[m])} and len(at) >= 2, (n, i, at)
    # ---- the rule, then each mutation alone
    val, first = ac.select(V, pm)
    want = torch.where((V == top[:, None]) & pm[None], torch.arange(lp)[None], torch.full((1, lp), ac.BIG)).min(dim=1).values
    assert torch.equal(first, want) and torch.equal(val, top)
    last = torch.where((V == top[:, None]) & pm[None], torch.arange(lp)[None], torch.full((1, lp), -1)).max(dim=1).values
    even_masked = torch.where(V == top[:, None], torch.arange(lp)[None], torch.full((1, lp), ac.BIG)).min(dim=1).values
    changed = {
        "last index": int((last != first).sum()),
        "walk >=": int((ac.select(V, pm, walk_ge=True)[1] != first).sum()),
        "lanes high": int((ac.select(V, pm, lanes_high=True)[1] != first).sum()),
        "merge high": int((ac.select(V, pm, merge="high")[1] != first).sum()),
        "merge first wave": int((ac.select(V, pm, merge="first")[1] != first).sum()),
        "merge last wave": int((ac.select(V, pm, merge="last")[1] != first).sum()),
        "masked lowest": int((even_masked != first).sum()),
    }
    print(f"tie page {kind} lp={lp} {variant}: {changed}")
    half = ac.TIE_LQ // 2
    assert changed["last index"] >= half
    assert changed["lanes high"] >= half
    if lp >= 127:
        assert changed["walk >="] >= half
    else:
        assert changed["walk >="] == 0                                                 # no wave owns two tiles that hold copies
    if lp >= 63:
        assert changed["merge high"] >= half
        assert changed["merge first wave"] + changed["merge last wave"] >= half
        assert changed["merge last wave"] > 0
        if lp >= 127 and variant != "random":                                          # "random" leaves only rows of wave 0 whole
            assert changed["merge first wave"] > 0                                     # rows of wave 3: the other wave's copy is in wave 0
    if variant != "none":
        assert changed["masked lowest"] >= half
    # what the count predicts, row by row
    levels = [_pairs(rows[i], pm) for i in c["row_of_token"]]
    assert changed["walk >="] == sum("walk" in s for s in levels)
    assert changed["lanes high"] >= sum("lanes" in s and "walk" not in s for s in levels)
    assert changed["merge high"] == sum("merge" in s for s in levels)


def _share(c):
    valid = c["ref"][1] >= 0
    loc = c["loc"]
    scale = c["qn"][:, None, :] * c["pmax"][loc][:, :, None]
    near = valid & (c["gap"] <= GAP_REL * scale)
    return int(near.sum()), int(valid.sum())


def test_magnitude_cases_stay_under_the_near_tie_cap():
    """A condition on the inputs alone (float64 on the CPU): the tokens the index rule may exempt are at most 1 % of a case."""
    for args in ac.SPREAD:
        near, valid = _share(ac.spread_case(*args))
        print(f"spread {args}: {near} of {valid} valid tokens near a tie ({near / valid:.2%})")
        assert valid >= 50 and near <= NEAR_TIE_CAP * valid, args
    for scale in ac.SCALES:
        near, valid = _share(ac.scaled_case(65, 17, scale))
        print(f"scaled {scale}: {near} of {valid} valid tokens near a tie ({near / valid:.2%})")
        assert valid >= 50 and near <= NEAR_TIE_CAP * valid, scale


def test_geometry_cases_stay_under_the_near_tie_cap():
    worst = 0.0
    for name, c in ac.geometry_cases():
        near, valid = _share(c)
        worst = max(worst, near / max(valid, 1))
        assert near <= NEAR_TIE_CAP * valid, (name, near, valid)
    print(f"geometry cases: worst near-tie share {worst:.2%}")


def test_scaled_edge_cases_sit_on_their_shifts():
    for name, total in (("e144", 144), ("e150", 150)):
        c = ac.scaled_case(65, 17, name)
        lo = {"e144": 2.0 ** -58, "e150": 2.0 ** -61}[name]
        for x in (c["Q"], c["P"]):
            assert lo <= float(x.abs().max()) < 2 * lo
        assert ac.shift_of(c["Q"]) + ac.shift_of(c["P"]) == total
        # the true products are normal fp32 numbers, and so are the reference's sims
        s = c["ref"][0][c["ref"][1] >= 0]
        assert bool((s.abs() >= 2.0 ** -126).all()) and s.numel() > 50


def test_the_plane_split_keeps_its_products_inside_the_value_bound():
    """fp16 hi/lo planes of x * 2^k, one k per tensor, lo x lo dropped: the products they represent lie within 1e-6 |q_n| |p_m| of
    the float64 products on every fp32 spread case (rows 12 binades apart share one shift), so the 1e-5 the GPU tests allow is not
    used up by the representation."""
    worst = 0.0
    for args in ac.SPREAD:
        if args[0] != "f32":
            continue
        c = ac.spread_case(*args)
        emu = ac.split_emulation(c["Q"], c["P"])
        ref = torch.einsum("qnd,pmd->qpnm", c["Q"].double(), c["P"].double())
        rel = ((emu - ref).abs() / (c["qn"][:, None, :, None] * c["pn"][None, :, None, :])).max().item()
        print(f"plane split {args}: {rel:.2e} of |q||p|")
        worst = max(worst, rel)
        assert rel <= REPR_TOL, (args, rel)
    assert worst > 0.0
