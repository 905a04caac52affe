"""Token clustering (evdr_cluster_pages, ops.cluster_pages / cluster_reference, PageCorpus.from_clustered / append_clustered; DESIGN.md
§4.11): the rule as ops.cluster_reference states it, the tie and NaN rules, planted groups, C-ABI argument errors and the Python-side
refusals -- all before any device work and without a GPU -- the no-scratch listing of the kernel's instances, and the power of the
near-tie cases of tests/test_gpu_cluster.py: assigns formed in another arithmetic must move labels on them."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def groups_of(members, offsets):
    return [members[offsets[g]:offsets[g + 1]].tolist() for g in range(len(offsets) - 1)]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_reference_states_the_rule():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    import cluster_cases as cc
    for lp, ls, d in ((7, 3, 128), (33, 9, 64), (12, 20, 24)):
        P, _ = cc.structured_pages(5, lp, d, min(ls, lp), 0.5, lp)
        pm = cc.case_mask(5, lp, lp)
        pm[3] = True
        for iters in (0, 3):
            mem, off, lab = ops.cluster_reference(P, pm, ls, iters)
            assert mem.dtype == off.dtype == lab.dtype == torch.int32
            assert tuple(mem.shape) == (5, lp) and tuple(off.shape) == (5, ls + 1) and tuple(lab.shape) == (5, lp)
            for page in range(5):
                valid = pm[page].nonzero().flatten().tolist()
                nv, g = len(valid), min(ls, len(valid))
                grp = groups_of(mem[page], off[page])
                assert int(off[page, 0]) == 0 and int(off[page, ls]) == nv and bool((off[page, 1:] >= off[page, :-1]).all())
                assert sorted(sum(grp, [])) == valid                     # every valid patch in exactly one group, masked ones in none
                assert all(x == sorted(x) for x in grp)                   # ascending inside a group
                assert bool((mem[page, nv:] == -1).all())                 # holes behind offsets[ls]
                assert all(not x for x in grp[g:])                        # nv < ls: groups >= nv stay empty
                assert bool((lab[page][~pm[page]] == -1).all())
                assert all(int(lab[page, p]) == j for j, x in enumerate(grp) for p in x)
                if iters == 0:                                            # equal contiguous windows over the valid patches
                    assert [int(lab[page, p]) for p in valid] == [i * g // nv for i in range(nv)]
            assert not off[0].any() and bool((mem[0] == -1).all())       # a fully masked page
            assert groups_of(mem[1], off[1])[:2] == [[lp // 3], [lp - 1]] or ls == 1
    # no mask = every patch valid; iters = 0 is pool_groups_windows when f divides lp
    mem, off, _ = ops.cluster_reference(torch.randn(2, 12, 8), None, 4, 0)
    wmem, woff = ops.pool_groups_windows(12, 3)
    assert torch.equal(mem, wmem[None].expand(2, -1)) and torch.equal(off, woff[None].expand(2, -1))
    # bf16 / fp16 pages convert exactly
    P, _ = cc.structured_pages(3, 33, 64, 9, 0.5, 1)
    for dt in (torch.bfloat16, torch.float16):
        a = ops.cluster_reference(P.to(dt), None, 9, 3)
        b = ops.cluster_reference(P.to(dt).float(), None, 9, 3)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_ties_go_to_the_lower_group_and_an_emptied_group_keeps_its_centroid():
    """Windows {p0, p1} and {p2, p3} of (1, 1, 1, -0.5) * e0 both have the centroid e0: every patch is tied and goes to group 0.
    Group 1 is reported empty and keeps e0: in the next iteration p3 scores -0.5 against both and stays in group 0 -- against a zero
    centroid it would score 0 and move."""
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    import cluster_cases as cc
    P, _, ls = cc.tie_page()
    for iters in (1, 2, 5):
        history = []
        mem, off, lab = ops.cluster_reference(P, None, ls, iters, history)
        assert history[0].tolist() == [[0, 0, 1, 1]]
        assert lab.tolist() == [[0, 0, 0, 0]] and off.tolist() == [[0, 4, 4]] and mem.tolist() == [[0, 1, 2, 3]]
    # -0.0 and +0.0 are one score: patches orthogonal to both centroids stay tied
    P, _, ls = cc.signed_zero_page()                                   # centroids ~ (e0 + e1), (e2 - e0); p1 . c1 = -0.0
    _, _, lab = ops.cluster_reference(P, None, ls, 1)
    assert lab.tolist() == [[0, 0, 1, 1]]


def test_a_nan_patch_gets_label_zero():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    import cluster_cases as cc
    P, _, _ = cc.nan_patch_page()                                      # patch 4 starts in group 2, whose centroid becomes NaN
    mem, off, lab = ops.cluster_reference(P, None, 3, 1)
    assert int(lab[0, 4]) == 0                                         # every score of the patch is NaN: nothing exceeds -inf
    assert all(int(lab[0, p]) in (0, 1) for p in (0, 1, 2, 3, 5))     # the others choose among their non-NaN scores
    ref = ops.cluster_reference(torch.nan_to_num(P), None, 3, 0)
    assert torch.equal(ops.cluster_reference(P, None, 3, 0)[2], ref[2])
    # a page of NaN only: every label 0 from the first assign on
    _, off, lab = ops.cluster_reference(cc.all_nan_page()[0], None, 2, 2)
    assert lab.tolist() == [[0] * 5] and off.tolist() == [[0, 5, 5]]


# ---- power of the near-tie cases: assigns in another arithmetic ------------------------------------------------------------------------
def _scores_rule(x, cent):
    """The rule's assign: octet sums ascending, product rounded before the add, then the tree of adjacent pairs."""
    s = torch.zeros(x.shape[:2] + (cent.shape[1], 16), dtype=torch.float32)
    for j in range(8):
        s = s + x[..., j] * cent[..., j]
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def _scores_fp64(x, cent):
    """An exact dot product (fp64 holds every product exactly), rounded to fp32 once."""
    return (x.double() * cent.double()).sum((-1, -2)).float()


def _scores_sequential(x, cent):
    """One fp32 accumulator over the 128 columns from left to right, every product and every sum rounded."""
    xs, cs = x.flatten(-2), cent.flatten(-2)
    s = torch.zeros(x.shape[:2] + (cent.shape[1],), dtype=torch.float32)
    for c in range(xs.shape[-1]):
        s = s + xs[..., c] * cs[..., c]
    return s


def _scores_fused(x, cent):
    """The rule's octet / tree order with every multiply-add fused: the product is exact in fp64, and the sum is rounded to fp32
    (through fp64's 53 bits first, which differs from one rounding in rare half-way cases only: a mutant either way)."""
    s = torch.zeros(x.shape[:2] + (cent.shape[1], 16), dtype=torch.float32)
    for j in range(8):
        s = (s.double() + x[..., j].double() * cent[..., j].double()).float()
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def _centroids_fp64(P, ok, labels, ls):
    """Group means and their normalisation in fp64, rounded to fp32 once."""
    x = P.double()
    onehot = (labels[:, :, None] == torch.arange(ls)[None, None, :]) & ok[:, :, None]
    cnt = onehot.sum(1)
    mean = torch.einsum("bpl,bpd->bld", onehot.double(), x) / cnt.clamp_min(1)[:, :, None]
    c = mean / (mean.norm(dim=-1, keepdim=True) + 1e-12)
    return c.float(), cnt > 0


MUTANTS = {"fp64": _scores_fp64, "sequential": _scores_sequential, "fused": _scores_fused}


def mutant_changes(builder, args, iters, mutant):
    """Labels per iteration that a mutant assign gives differently from ops.cluster_reference.  The mutant follows the reference's label
    history: iteration t starts from the reference's labels and centroids (kept ones included) and only the scores -- for
    "centroid64" only the fresh centroids -- are formed in the other arithmetic."""
    from evdr_amd import ops
    import cluster_cases as cc
    P, pm, ls = cc.built(builder, *args)
    _, history = cc.built_reference(builder, args, iters)
    b, lp, d = P.shape
    ok = torch.ones((b, lp), dtype=torch.bool) if pm is None else pm.bool()
    live = torch.arange(ls)[None] < ok.sum(1, keepdim=True).clamp_max(ls)
    x = torch.nn.functional.pad(P.float(), (0, 128 - d)).view(b, lp, 1, 16, 8)
    cent = torch.zeros((b, ls, d))
    out = []
    for before, after in zip(history[:-1], history[1:]):
        c, has = ops.pool_reference(P, ok, *ops._cluster_lists(before.long(), ls), normalize=True)
        kept = torch.where(has[:, :, None], c, cent)
        if mutant == "centroid64":
            c64, _ = _centroids_fp64(P, ok, before.long(), ls)
            used, score = torch.where(has[:, :, None], c64, cent), _scores_rule
        else:
            used, score = kept, MUTANTS[mutant]
        cent = kept
        s = score(x, torch.nn.functional.pad(used, (0, 128 - d)).view(b, 1, ls, 16, 8))
        s = torch.where(torch.isnan(s) | ~live[:, None, :], torch.full_like(s, float("-inf")), s)
        labels = torch.where(ok, s.argmax(-1), torch.full((b, lp), -1))
        out.append(int((labels != after.long()).sum()))
    return out


def test_near_tie_cases_tell_other_arithmetics_apart():
    """What makes the near-tie GPU cases worth running: on every case of cc.NEAR_TIE the rule keeps moving labels, and an assign formed
    in another arithmetic gives other labels -- so a kernel that summed in another order, fused a multiply-add or formed a centroid
    an ulp off could not pass them.  Asked for: every fp32 case, every score mutant, every iteration >= 20 labels; every half-precision
    case, every mutant, >= 1 label over the run; labels moved by the rule in two consecutive iterations on every case.  Seen (labels
    per iteration, 4 iterations; rule = moved by the reference itself):
      (64, 8, 128) fp32         rule 221 189 168 164      fp64 123 139 86 110      sequential 200 197 195 208     fused 73 94 63 66
                                centroid64 164 134 136 127
      (300, 40, 100) fp32, mask rule 944 791 840 671      fp64 624 669 519 366     sequential 885 904 890 886     fused 411 420 349 334
                                centroid64 801 722 697 542
      (700, 313, 32) fp32       rule 1396 1348 1330 1319  fp64 1303 891 1193 1158  sequential 1361 1335 1340 1339 fused 959 751 883 854
                                centroid64 1252 1084 1173 1177
      (64, 8, 128) bf16         rule 75 35 24 13          fp64 45 19 9 6           sequential 112 76 71 45        fused 37 11 6 3
                                centroid64 46 15 13 4
      (64, 8, 128) fp16         rule 223 154 142 144      fp64 114 88 105 89       sequential 172 148 192 196     fused 69 41 88 50
                                centroid64 123 86 114 111
    The fourth mutant (centroids formed in fp64 and rounded once, the rule's assign) changed 104..181 labels in every iteration on
    each of the seeds 0..9 of the (64, 8, 128) fp32 case, so it stays and is held to the same conditions."""
    import evdr_amd  # noqa: F401
    import cluster_cases as cc
    for args in cc.NEAR_TIE:
        _, history = cc.built_reference(cc.near_tie_case, args, cc.NEAR_TIE_ITERS)
        moved = cc.changes(history)
        seen = {m: mutant_changes(cc.near_tie_case, args, cc.NEAR_TIE_ITERS, m) for m in tuple(MUTANTS) + ("centroid64",)}
        print(args, "rule", moved, seen)
        assert any(a > 0 and b > 0 for a, b in zip(moved[:-1], moved[1:])), (args, moved)
        for m, counts in seen.items():
            if args[3] is torch.float32:
                assert min(counts) >= 20, (args, m, counts)
            else:
                assert sum(counts) >= 1, (args, m, counts)


def test_identical_and_alternating_patches():
    """lp copies of one row whose sums and means are exact: every window has the same centroid bits, every patch is tied and goes to
    group 0, and groups 1.. stay emptied with their centroids for the iterations that follow.  Two rows alternately: equal rows have
    equal scores, so they share a label."""
    import evdr_amd  # noqa: F401
    import cluster_cases as cc
    for args in ((300, 40, 64), (700, 313, 32)):
        (mem, off, lab), history = cc.built_reference(cc.identical_page, args, 3)
        lp, ls = args[:2]
        assert history[0][0].tolist() == [i * ls // lp for i in range(lp)]
        assert all(not h.any() for h in history[1:])
        assert mem[0].tolist() == list(range(lp)) and off[0].tolist() == [0] + [lp] * ls
    (_, off, lab), _ = cc.built_reference(cc.alternating_page, (33, 9, 64), 3)
    assert len(set(lab[0, 0::2].tolist())) == 1 and len(set(lab[0, 1::2].tolist())) == 1 and int(lab[0, 0]) != int(lab[0, 1])


def test_the_largest_page_the_header_allows_is_quick_on_the_cpu():
    """lp_src = 65535: the start labels at the largest i * g (65534 * 4096, ls = 4096, no iteration, no score tensor), and one
    iteration at ls = 16 (a 67 MB score temporary; pool_reference walks the 4096 members of a window) -- 0.4 s on the CPU, so the
    GPU case keeps lp_src = 65535."""
    import evdr_amd  # noqa: F401
    import cluster_cases as cc
    (_, off, lab), _ = cc.built_reference(cc.plain_case, (65535, 4096, 8, 1, False), 0)
    assert lab[0].tolist() == [i * 4096 // 65535 for i in range(65535)] and int(lab[0, -1]) == 4095 and int(off[0, -1]) == 65535
    (_, off, lab), history = cc.built_reference(cc.plain_case, (65535, 16, 8, 1, False), 1)
    assert cc.changes(history)[0] > 0 and int(off[0, -1]) == 65535


def objective(P, pm, labels, ls):
    """Mean cosine of a valid patch to the pooled token of its group."""
    from evdr_amd import ops
    tok, _ = ops.pool_reference(P, pm, *ops._cluster_lists(labels.long(), ls), normalize=True)
    own = tok.gather(1, labels.clamp_min(0).long()[:, :, None].expand(-1, -1, P.shape[-1]))
    cos = (torch.nn.functional.normalize(P.float(), dim=-1) * own).sum(-1)
    ok = labels >= 0
    return float(cos[ok].mean())


def test_planted_groups_are_a_fixed_point_and_the_objective_never_falls():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    import cluster_cases as cc
    n, K, f, d = 3, 12, 8, 64
    # in window order: equal groups of f patches, one prototype each
    proto = torch.nn.functional.normalize(torch.randn((n, K, d), generator=torch.Generator().manual_seed(12)), dim=-1)
    planted = torch.arange(K).repeat_interleave(f)[None].expand(n, -1)
    noise = torch.randn((n, K * f, d), generator=torch.Generator().manual_seed(13))
    Pw = torch.nn.functional.normalize(proto[:, planted[0]] + 0.05 * noise / d ** 0.5, dim=-1)
    history = []
    ops.cluster_reference(Pw, None, K, 4, history)
    assert all(torch.equal(h, planted.to(torch.int32)) for h in history)
    # shuffled: the objective does not decrease from one iteration to the next (1e-6: the rounding of an fp32 mean of cosines)
    P, _ = cc.structured_pages(n, K * f, d, K, 0.05, 11)
    history = []
    ops.cluster_reference(P, None, K, 8, history)
    obj = [objective(P, None, h, K) for h in history]
    assert all(b >= a - 1e-6 for a, b in zip(obj[:-1], obj[1:])), obj
    assert obj[-1] > obj[0] + 0.1, obj                                 # and clustering found structure the windows miss


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound(lib):
    from evdr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evdr.h")).read(), flags=re.S)
    for name in ("evdr_cluster_pages", "evdr_cluster_pages_workspace"):
        assert re.search(r"EVDR_API\s+[\w \*]+?\b" + name + r"\s*\(", header)
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_cluster_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def call(src=1, src_dtype=L.EVDR_F32, b=2, lp_src=40, d_src=128, src_stride=None, ls=10, iters=8, members=1, offsets=1, labels=None,
             ws=256, ws_bytes=None):
        # pointers are fake: nothing is dereferenced on the host
        need = lib.evdr_cluster_pages_workspace(lp_src, ls)
        return lib.evdr_cluster_pages(src, src_dtype, None, b, lp_src, d_src, lp_src * d_src if src_stride is None else src_stride, ls, iters,
                                      members, offsets, labels, ws, need if ws_bytes is None else ws_bytes, None)

    def refused(code, text, **kw):
        rc = call(**kw)
        return rc == code and text in lib.evdr_last_error()

    assert refused(L.EVDR_ERR_ARG, b"src_dtype", src_dtype=5)
    for name in ("b", "lp_src", "d_src", "ls", "iters"):
        assert refused(L.EVDR_ERR_ARG, b"negative", **{name: -1})
    assert refused(L.EVDR_ERR_SHAPE, b"d_src", d_src=129) and refused(L.EVDR_ERR_SHAPE, b"d_src", d_src=0)
    assert refused(L.EVDR_ERR_SHAPE, b"lp_src", lp_src=0) and refused(L.EVDR_ERR_SHAPE, b"lp_src", lp_src=65536)
    assert refused(L.EVDR_ERR_SHAPE, b"ls", ls=0) and refused(L.EVDR_ERR_SHAPE, b"ls", ls=4097)
    assert refused(L.EVDR_ERR_SHAPE, b"iters", iters=65)
    for name in ("src", "members", "offsets", "ws"):
        assert refused(L.EVDR_ERR_ARG, b"null", **{name: None})
    assert refused(L.EVDR_ERR_ARG, b"src_stride", src_stride=40 * 128 - 1)
    assert refused(L.EVDR_ERR_ARG, b"workspace", ws_bytes=lib.evdr_cluster_pages_workspace(40, 10) - 1)
    assert refused(L.EVDR_ERR_ARG, b"workspace", ws=264)               # not 16-byte aligned
    assert call(b=0, src=None, members=None, offsets=None, ws=None, ws_bytes=0) == L.EVDR_OK
    # the workspace belongs to the grid: no page count goes in; labels always, centroids when they do not fit the LDS
    small, large = lib.evdr_cluster_pages_workspace(1030, 312), lib.evdr_cluster_pages_workspace(1030, 313)
    assert small >= 1030 * 4 and large >= small + 313 * 512 and small % 256 == 0
    assert lib.evdr_cluster_pages_workspace(65535, 4096) < 2 ** 31
    for bad in ((0, 4), (65536, 4), (40, 0), (40, 4097), (-1, -1)):
        assert lib.evdr_cluster_pages_workspace(*bad) == 0


def test_python_entry_points_refuse_before_any_device_work():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    P = torch.zeros(2, 40, 128)
    calls = (lambda P, pm, **kw: ops.cluster_pages(P, pm, **kw), lambda P, pm, **kw: PageCorpus.from_clustered(P, pm, **kw),
             lambda P, pm, ls=10, **kw: ops.cluster_reference(P, pm, ls, kw.pop("iters", 8), **kw))
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="pages must be"):
            call(P[0], None, ls=10)
        with pytest.raises(ValueError, match="pages must be"):
            call(P[:, :0], None, ls=10)
        with pytest.raises(NotImplementedError, match="width-256"):
            call(torch.zeros(2, 40, 256), None, ls=10)
        with pytest.raises(ValueError, match="fp32, bf16 or fp16"):
            call(P.double(), None, ls=10)
        with pytest.raises(ValueError, match="pmask"):
            call(P, torch.ones(2, 39, dtype=torch.bool), ls=10)
        for bad in (0, 4097, 2.5):
            with pytest.raises(ValueError, match="ls must be"):
                call(P, None, ls=bad)
        for bad in (-1, 65, 1.5):
            with pytest.raises(ValueError, match="iters must be"):
                call(P, None, ls=10, iters=bad)
        if i < 2:
            with pytest.raises(ValueError, match="exactly one"):
                call(P, None)
            with pytest.raises(ValueError, match="exactly one"):
                call(P, None, ls=10, factor=4)
            for bad in (0, 1.5):
                with pytest.raises(ValueError, match="factor must be"):
                    call(P, None, factor=bad)
            with pytest.raises(RuntimeError, match="GPU only"):      # everything in order: it gets as far as the device check
                call(P, torch.ones(2, 40, dtype=torch.bool), factor=4)
    # from_clustered: kind, absmax, capacity, chunk size
    with pytest.raises(ValueError, match="dtype"):
        PageCorpus.from_clustered(P, None, ls=10, dtype=torch.float16)
    with pytest.raises(ValueError, match="absmax"):
        PageCorpus.from_clustered(P, None, ls=10, normalize=False)
    with pytest.raises(ValueError, match="absmax"):
        PageCorpus.from_clustered(P, None, ls=10, dtype=ops.FP8, absmax=1.0)
    with pytest.raises(ValueError, match="capacity"):
        PageCorpus.from_clustered(P, None, ls=10, capacity=1)
    with pytest.raises(ValueError, match="chunk_pages"):
        PageCorpus.from_clustered(P, None, ls=10, chunk_pages=0)
    # append_clustered: arguments, capacity, width-256 corpora; a refused call changes nothing
    e = PageCorpus.empty(4, 10, torch.bfloat16, "cpu", idx_base=7)
    with pytest.raises(ValueError, match="pages must be"):
        e.append_clustered(P[0], None)
    with pytest.raises(ValueError, match="iters must be"):
        e.append_clustered(P, None, iters=65)
    with pytest.raises(ValueError, match="chunk_pages"):
        e.append_clustered(P, None, chunk_pages=0)
    with pytest.raises(ValueError, match="capacity"):
        PageCorpus.empty(1, 10, torch.bfloat16, "cpu").append_clustered(P, None)
    with pytest.raises(RuntimeError, match="GPU only"):
        e.append_clustered(P, None)
    assert e.append_clustered(P[:0], None) == 7 and e.n_pages == 0
    tm, pf = torch.zeros(8, 1, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    wide = PageCorpus(torch.zeros(4, 8, 10, 128, dtype=torch.float16), tm, pf, 0, torch.full((1,), 0x3F800000, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="width-256"):
        wide.append_clustered(P, None)
    with pytest.raises(ValueError, match="exceeds"):
        PageCorpus.empty(1, 5000, torch.bfloat16, "cpu").append_clustered(P, None)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_cluster_instances_use_no_scratch():
    """scratch/kres.py over csrc/cluster.hip: the 12 instances (3 source dtypes x aligned / element-wise access x centroids in LDS /
    in the workspace) compile for gfx950 without scratch memory and without VGPR spills."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scratch", "kres.py"), "cluster.hip", "cluster_pages_kernel"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    rows = [ln for ln in r.stdout.splitlines() if "cluster_pages_kernel<" in ln]
    assert r.returncode == 0 and len(rows) == 12, (r.stdout[-1500:], r.stderr[-500:])
    for ln in rows:
        m = re.search(r"VGPR\s+(\d+) AGPR\s+(\d+) spill\s+(\d+) sspill\s+\d+ scratch\s+(\d+)", ln)
        assert m and int(m.group(3)) == 0 and int(m.group(4)) == 0, ln
