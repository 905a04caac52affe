"""Pooled corpora (evdr_corpus_pool_ingest, evdr_pool_pages, ops.pool_*, PageCorpus.from_pooled / append_pooled / replace_pooled;
DESIGN.md §4.10): the grouping helpers, the pooling rule as ops.pool_reference states it, C-ABI argument errors and the Python-side
refusals -- all before any device work and without a GPU -- and the no-scratch listing of the kernel's instances."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def groups_of(members, offsets):
    return [members[offsets[g]:offsets[g + 1]].tolist() for g in range(len(offsets) - 1)]


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- grouping helpers ----------------------------------------------------------------------------------------------------------
def test_windows_cover_every_patch_once():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    for lp, f in ((8, 4), (7, 3), (33, 4), (225, 4), (5, 9), (1, 1)):
        mem, off = ops.pool_groups_windows(lp, f)
        assert mem.dtype == off.dtype == torch.int32 and not mem.is_cuda
        g = groups_of(mem, off)
        assert len(g) == (lp + f - 1) // f and int(off[0]) == 0 and int(off[-1]) == lp
        assert bool((off[1:] >= off[:-1]).all())
        assert sorted(sum(g, [])) == list(range(lp))                  # every patch in exactly one group
        assert all(len(x) == f for x in g[:-1]) and len(g[-1]) == lp - f * (len(g) - 1)      # the last window may be ragged
        assert all(x == list(range(x[0], x[0] + len(x))) for x in g)
    assert groups_of(*ops.pool_groups_windows(7, 3)) == [[0, 1, 2], [3, 4, 5], [6]]
    for bad in ((0, 2), (4, 0)):
        with pytest.raises(ValueError, match="pool_groups_windows"):
            ops.pool_groups_windows(*bad)


def test_grid_blocks_and_extra_patches():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    # a 3 x 4 grid from patch 1 of a 15-patch page, 2 x 2 blocks: ragged bottom row of blocks; patches 0, 13, 14 are outside
    mem, off = ops.pool_groups_grid(3, 4, 2, 2, first=1, lp=15)
    assert groups_of(mem, off) == [[0], [1, 2, 5, 6], [3, 4, 7, 8], [9, 10], [11, 12], [13], [14]]
    mem, off = ops.pool_groups_grid(3, 4, 2, 2, first=1, lp=15, extra="drop")
    assert groups_of(mem, off) == [[1, 2, 5, 6], [3, 4, 7, 8], [9, 10], [11, 12]]
    for rows, cols, fr, fc, first, lp in ((15, 15, 3, 3, 1, 227), (32, 32, 2, 2, 0, 1030), (5, 7, 2, 3, 0, None), (4, 4, 4, 4, 3, 19)):
        for extra in ("own", "drop"):
            mem, off = ops.pool_groups_grid(rows, cols, fr, fc, first=first, extra=extra, lp=lp)
            total = first + rows * cols if lp is None else lp
            g = groups_of(mem, off)
            assert int(off[0]) == 0 and int(off[-1]) == mem.numel() and bool((off[1:] >= off[:-1]).all())
            grid = set(range(first, first + rows * cols))
            flat = sum(g, [])
            assert len(flat) == len(set(flat))                        # nobody twice
            assert grid <= set(flat)                                  # every patch of the grid in exactly one group
            outside = set(range(total)) - grid
            nblocks = -(-rows // fr) * -(-cols // fc)
            if extra == "own":
                assert set(flat) == set(range(total)) and len(g) == nblocks + len(outside)
                assert all(len(x) == 1 for x in g if x[0] in outside)
            else:
                assert set(flat) == grid and len(g) == nblocks
            for x in g:                                               # a block spans at most fr rows and fc columns of the grid
                if x[0] in grid:
                    r, c = [(i - first) // cols for i in x], [(i - first) % cols for i in x]
                    assert max(r) // fr == min(r) // fr and max(c) // fc == min(c) // fc and len(x) <= fr * fc
    with pytest.raises(ValueError, match="extra"):
        ops.pool_groups_grid(2, 2, 1, 1, extra="keep")
    with pytest.raises(ValueError, match="pool_groups_grid"):
        ops.pool_groups_grid(2, 2, 1, 1, first=1, lp=4)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_reference_states_the_rule():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    gen = torch.Generator().manual_seed(5)
    row = torch.randn(24, generator=gen)
    P = torch.randn(2, 9, 24, generator=gen)
    P[:, 0:4] = row                                                   # four identical members
    mem = torch.tensor([0, 1, 2, 3, 4, 5, -1, 9, 6, 7, 8], dtype=torch.int32)
    off = torch.tensor([0, 4, 6, 6, 8, 11], dtype=torch.int32)        # group 2 is empty, group 3 holds holes only
    pm = torch.ones(2, 9, dtype=torch.bool)
    pm[1, 5] = False
    pm[1, 6:9] = False
    out, mask = ops.pool_reference(P, pm, mem, off, normalize=False)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 5, 24) and mask.dtype == torch.bool
    assert torch.equal(bits(out[:, 0]), bits(row.expand(2, 24)))      # x + x + x + x and / 4 are exact: the member's own bits
    assert torch.equal(bits(out[0, 1]), bits((P[0, 4] + P[0, 5]) / 2))
    assert torch.equal(bits(out[1, 1]), bits(P[1, 4]))                # the masked member is skipped, the count is 1
    assert mask.tolist() == [[True, True, False, False, True], [True, True, False, False, False]]
    assert not out[:, 2:4].any() and not out[1, 4].any()              # empty / holes only / all masked: zero, masked tokens
    assert torch.equal(bits(out[0, 4]), bits(((P[0, 6] + P[0, 7]) + P[0, 8]) / 3))
    # no mask = every patch valid
    out2, mask2 = ops.pool_reference(P, None, mem, off, normalize=False)
    assert torch.equal(bits(out2[0]), bits(out[0])) and bool(mask2[1, 4])
    # the groups permute with the lists
    perm = [3, 0, 4, 2, 1]
    g = groups_of(mem, off)
    pmem = torch.tensor(sum((g[i] for i in perm), []), dtype=torch.int32)
    poff = torch.tensor([0] + torch.tensor([len(g[i]) for i in perm]).cumsum(0).tolist(), dtype=torch.int32)
    for normalize in (False, True):
        a, am = ops.pool_reference(P, pm, mem, off, normalize=normalize)
        b, bm = ops.pool_reference(P, pm, pmem, poff, normalize=normalize)
        assert torch.equal(bits(a[:, perm]), bits(b)) and torch.equal(am[:, perm], bm)
    # the per-page form with the same lists in every row is the shared form
    a, am = ops.pool_reference(P, pm, mem, off)
    b, bm = ops.pool_reference(P, pm, mem[None].repeat(2, 1), off[None].repeat(2, 1))
    assert torch.equal(bits(a), bits(b)) and torch.equal(am, bm)
    # normalize=True is l2_normalize of the means, to rounding; masked tokens stay zero
    want = out / (out.norm(dim=-1, keepdim=True) + 1e-12)
    assert torch.allclose(a, want, rtol=0, atol=1e-6) and not a[:, 2].any()
    # bf16 / fp16 pages convert exactly
    h, _ = ops.pool_reference(P.half(), pm, mem, off, normalize=False)
    assert torch.equal(bits(h), bits(ops.pool_reference(P.half().float(), pm, mem, off, normalize=False)[0]))


def test_reference_adds_in_list_order():
    """1 + 2^-24 rounds back to 1 (twice), 2^-24 + 2^-24 + 1 does not: reversing ONE group's list moves its mean by one ulp."""
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    P = torch.zeros(1, 4, 8)
    P[0, 0], P[0, 1], P[0, 2] = 1.0, 2.0 ** -24, 2.0 ** -24
    off = torch.tensor([0, 4, 8], dtype=torch.int32)
    fwd = ops.pool_reference(P, None, torch.tensor([0, 1, 2, 3, 0, 1, 2, 3], dtype=torch.int32), off, normalize=False)[0]
    rev = ops.pool_reference(P, None, torch.tensor([0, 1, 2, 3, 3, 2, 1, 0], dtype=torch.int32), off, normalize=False)[0]
    assert torch.equal(bits(fwd[0, 0]), bits(torch.full((8,), 0.25)))
    assert torch.equal(bits(fwd[0, 0]), bits(rev[0, 0])) and torch.equal(bits(fwd[0, 1]), bits(fwd[0, 0]))
    assert bool((bits(rev[0, 1]) - bits(fwd[0, 1]) == 1).all())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound(lib):
    from evdr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evdr.h")).read(), flags=re.S)
    for name in ("evdr_corpus_pool_ingest", "evdr_pool_pages"):
        assert re.search(r"EVDR_API\s+[\w \*]+?\b" + name + r"\s*\(", header)
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_pool_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def src_args(src=1, src_dtype=L.EVDR_F32, b=2, lp_src=40, d_src=128, src_stride=None, members=1, offsets=1, m=40, ls=10, per_page=0,
                 normalize=1, **_):
        # pointers are fake: nothing is dereferenced on the host
        return (src, src_dtype, None, b, lp_src, d_src, lp_src * d_src if src_stride is None else src_stride, members, offsets, m, ls,
                per_page, normalize)

    def ingest(planes=16, kind=L.EVDR_CORPUS_BF16, capacity=8, lp=10, p_stride=None, plane_stride=8 * 10 * 128, words=1, shift=None,
               amax=None, first=0, dst=None, **kw):
        return lib.evdr_corpus_pool_ingest(*src_args(**kw), planes, kind, capacity, lp, lp * 128 if p_stride is None else p_stride,
                                           plane_stride, words, words, shift, amax, first, dst, None, None)

    def plain(out=16, d_out=128, out_mask=1, **kw):
        return lib.evdr_pool_pages(*src_args(**kw), out, d_out, out_mask, None)

    def refused(call, code, text, **kw):
        rc = call(**kw)
        return rc == code and text in lib.evdr_last_error()

    for call in (ingest, plain):                                      # the source and the grouping: both calls
        assert refused(call, L.EVDR_ERR_ARG, b"src_dtype", src_dtype=5)
        assert refused(call, L.EVDR_ERR_ARG, b"negative", b=-1) and refused(call, L.EVDR_ERR_ARG, b"negative", m=-1)
        assert refused(call, L.EVDR_ERR_ARG, b"negative", lp_src=-1)
        assert refused(call, L.EVDR_ERR_ARG, b"flags", per_page=2) and refused(call, L.EVDR_ERR_ARG, b"flags", normalize=-1)
        assert refused(call, L.EVDR_ERR_SHAPE, b"ls", ls=0) and refused(call, L.EVDR_ERR_SHAPE, b"ls", ls=65536, lp=65535)
        assert refused(call, L.EVDR_ERR_SHAPE, b"d_src", d_src=129, d_out=129) and refused(call, L.EVDR_ERR_SHAPE, b"d_src", d_src=0, d_out=0)
        assert refused(call, L.EVDR_ERR_ARG, b"null", src=None) and refused(call, L.EVDR_ERR_ARG, b"null", members=None)
        assert refused(call, L.EVDR_ERR_ARG, b"null", offsets=None)
        assert refused(call, L.EVDR_ERR_ARG, b"src_stride", src_stride=40 * 128 - 1)
    assert refused(plain, L.EVDR_ERR_SHAPE, b"d_out", d_src=64, d_out=96)
    assert refused(plain, L.EVDR_ERR_ARG, b"null", out=None) and refused(plain, L.EVDR_ERR_ARG, b"null", out_mask=None)
    assert plain(b=0, src=None, members=None, offsets=None, out=None, out_mask=None) == L.EVDR_OK
    # the corpus side follows evdr_corpus_ingest
    assert refused(ingest, L.EVDR_ERR_SHAPE, b"ls", ls=11)            # ls > lp
    assert refused(ingest, L.EVDR_ERR_ARG, b"absmax", kind=L.EVDR_CORPUS_F16_HILO)
    assert refused(ingest, L.EVDR_ERR_ARG, b"shifts", kind=L.EVDR_CORPUS_FP8)
    assert refused(ingest, L.EVDR_ERR_ARG, b"capacity", first=7) and refused(ingest, L.EVDR_ERR_ARG, b"capacity", first=-1)
    assert refused(ingest, L.EVDR_ERR_SHAPE, b"256", kind=L.EVDR_CORPUS_F16_WIDE, amax=1)
    assert refused(ingest, L.EVDR_ERR_ARG, b"kind", kind=3)
    assert refused(ingest, L.EVDR_ERR_SHAPE, b"lp", lp=0, ls=1) and refused(ingest, L.EVDR_ERR_SHAPE, b"lp", lp=65536)
    assert refused(ingest, L.EVDR_ERR_ARG, b"null", planes=None) and refused(ingest, L.EVDR_ERR_ARG, b"null", words=None)
    assert refused(ingest, L.EVDR_ERR_ARG, b"p_stride", p_stride=9 * 128) and refused(ingest, L.EVDR_ERR_ARG, b"aligned", p_stride=10 * 128 + 4)
    assert refused(ingest, L.EVDR_ERR_ARG, b"aligned", planes=8)
    assert ingest(b=0, src=None, planes=None, words=None, members=None, offsets=None) == L.EVDR_OK
    assert ingest(b=0, first=8) == L.EVDR_OK and refused(ingest, L.EVDR_ERR_ARG, b"capacity", b=0, first=9)
    assert refused(ingest, L.EVDR_ERR_ARG, b"null", first=100, dst=1, planes=None)


def test_python_entry_points_refuse_before_any_device_work():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    P = torch.zeros(2, 40, 128)
    mem, off = ops.pool_groups_windows(40, 4)
    calls = (lambda *a: ops.pool_pages(*a), lambda *a: PageCorpus.from_pooled(*a, dtype=torch.bfloat16),
             lambda *a: PageCorpus.empty(4, 10, torch.bfloat16, "cpu").append_pooled(*a))
    for call in calls:
        with pytest.raises(ValueError, match="pages must be"):
            call(P[0], None, mem, off)
        with pytest.raises(NotImplementedError, match="width-256"):
            call(torch.zeros(2, 40, 256), None, mem, off)
        with pytest.raises(ValueError, match="fp32, bf16 or fp16"):
            call(P.double(), None, mem, off)
        with pytest.raises(ValueError, match="pmask"):
            call(P, torch.ones(2, 39, dtype=torch.bool), mem, off)
        with pytest.raises(ValueError, match="int32 or int64"):
            call(P, None, mem.float(), off)
        with pytest.raises(ValueError, match="int32 or int64"):
            call(P, None, mem, off.to(torch.int16))
        with pytest.raises(ValueError, match="shared by all pages"):
            call(P, None, mem, off[None])
        with pytest.raises(ValueError, match="one row per page"):
            call(P, None, mem[None].repeat(3, 1), off[None].repeat(3, 1))
        with pytest.raises(ValueError, match="ls"):
            call(P, None, mem, off[:1])
        for bad in (off + 1, off.flip(0), torch.cat([off[:-1], off[-1:] + 1])):       # not from 0, decreasing, past the members
            with pytest.raises(ValueError, match="non-decreasing"):
                call(P, None, mem, bad)
        with pytest.raises(RuntimeError, match="GPU only"):          # everything in order: it gets as far as the device check
            call(P, torch.ones(2, 40, dtype=torch.bool), mem.long(), off.long())
    # from_pooled: kind, absmax, capacity
    with pytest.raises(ValueError, match="dtype"):
        PageCorpus.from_pooled(P, None, mem, off, dtype=torch.float16)
    with pytest.raises(ValueError, match="absmax"):
        PageCorpus.from_pooled(P, None, mem, off, normalize=False)   # fp32 kind, unnormalised: the bound is the caller's to give
    with pytest.raises(ValueError, match="absmax"):
        PageCorpus.from_pooled(P, None, mem, off, dtype=ops.FP8, absmax=1.0)
    with pytest.raises(ValueError, match="capacity"):
        PageCorpus.from_pooled(P, None, mem, off, capacity=1)
    # append_pooled / replace_pooled: page length, capacity, index list, width-256 corpora; a refused call changes nothing
    tm, pf = torch.zeros(8, 1, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    c = PageCorpus(torch.zeros(1, 8, 10, 128, dtype=torch.bfloat16), tm, pf, 100)
    short = PageCorpus.empty(4, 9, torch.bfloat16, "cpu")
    with pytest.raises(ValueError, match="do not fit"):
        short.append_pooled(P, None, mem, off)
    with pytest.raises(ValueError, match="capacity"):
        c.append_pooled(P, None, mem, off)                           # no reserved storage
    with pytest.raises(ValueError, match="capacity"):
        PageCorpus.empty(1, 10, torch.bfloat16, "cpu").append_pooled(P, None, mem, off)
    e = PageCorpus.empty(4, 10, torch.bfloat16, "cpu", idx_base=7)
    assert e.append_pooled(P[:0], None, mem, off) == 7 and e.n_pages == 0
    for bad, what in ((torch.tensor([100, 100]), "duplicate"), (torch.tensor([99, 100]), "outside"), (torch.tensor([100]), "pages must be")):
        with pytest.raises(ValueError, match=what):
            c.replace_pooled(bad, P, None, mem, off)
    with pytest.raises(ValueError, match="do not fit"):
        short.replace_pooled(torch.tensor([0, 1]), P, None, mem, off)
    with pytest.raises(RuntimeError, match="GPU only"):
        c.replace_pooled(torch.tensor([107, 100]), P, None, mem, off)
    c.replace_pooled(torch.zeros(0, dtype=torch.int64), P[:0], None, mem, off)        # b = 0: a no-op
    wide = PageCorpus(torch.zeros(4, 8, 10, 128, dtype=torch.float16), tm, pf, 0, torch.full((1,), 0x3F800000, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="width-256"):
        wide.append_pooled(P, None, mem, off)
    with pytest.raises(NotImplementedError, match="width-256"):
        wide.replace_pooled(torch.tensor([0, 1]), P, None, mem, off)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.corpus_pool_ingest(P, None, mem, off, c.planes, c.tilemask, c.pageflags)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_pool_instances_use_no_scratch():
    """scratch/kres.py over csrc/pool.hip: the 24 instances (3 source dtypes x 4 destinations x aligned / element-wise access) compile
    for gfx950 without scratch memory and without VGPR spills."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scratch", "kres.py"), "pool.hip", "corpus_pool_ingest_kernel"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    rows = [ln for ln in r.stdout.splitlines() if "corpus_pool_ingest_kernel<" in ln]
    assert r.returncode == 0 and len(rows) == 24, (r.stdout[-1500:], r.stderr[-500:])
    for ln in rows:
        m = re.search(r"VGPR\s+(\d+) AGPR\s+(\d+) spill\s+(\d+) sspill\s+\d+ scratch\s+(\d+)", ln)
        assert m and int(m.group(3)) == 0 and int(m.group(4)) == 0, ln
