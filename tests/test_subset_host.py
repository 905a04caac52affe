"""Page-subset search (PageCorpus.subset / score / topk with subset=, ops.maxsim_forward_pages, evdr_maxsim_fwd_pages):
exports, C-ABI argument errors, Python-side refusals, subset() normalisation and the compile-time checks of the new kernel instances,
all without a GPU."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["evdr_maxsim_fwd_pages"]


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_entry_is_declared_exported_and_bound(lib):
    from evdr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evdr.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"EVDR_API\s+[\w \*]+?\b" + n + r"\s*\(", header), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.evdr_version() == 303


def test_pages_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def score(nq=4, lq=8, np_=64, lp=40, nplanes=1, m=16, ptr=1, pages=1, out=1, out_stride=None, p_stride=None, qlist=None):
        # pointers are fake: nothing is dereferenced on the host
        return lib.evdr_maxsim_fwd_pages(ptr, ptr, None, ptr, ptr, pages, m, out, m if out_stride is None else out_stride,
                                         nq, lq, np_, lp, nplanes, lp * 128 if p_stride is None else p_stride, np_ * lp * 128,
                                         None, None, qlist, None)
    assert score(nplanes=3) == L.EVDR_ERR_ARG
    assert score(nplanes=4) == L.EVDR_ERR_SHAPE and b"256" in lib.evdr_last_error()
    assert score(ptr=None) == L.EVDR_ERR_ARG
    assert score(pages=None) == L.EVDR_ERR_ARG and score(out=None) == L.EVDR_ERR_ARG
    assert score(nq=-1) == L.EVDR_ERR_ARG and score(np_=-1) == L.EVDR_ERR_ARG and score(m=-1) == L.EVDR_ERR_ARG
    assert score(lq=-1) == L.EVDR_ERR_ARG and score(lp=-1) == L.EVDR_ERR_ARG
    assert score(out_stride=15) == L.EVDR_ERR_ARG and b"stride" in lib.evdr_last_error()
    assert score(p_stride=39 * 128) == L.EVDR_ERR_ARG
    assert score(lp=0) == L.EVDR_ERR_SHAPE
    assert score(lq=0) == L.EVDR_ERR_SHAPE
    assert score(np_=0) == L.EVDR_ERR_SHAPE                             # a list over an empty corpus: every entry would be a hole
    assert score(lq=33) == L.EVDR_ERR_WORKSPACE and b"qlist" in lib.evdr_last_error()
    assert score(lq=70) == L.EVDR_ERR_WORKSPACE
    assert score(nq=0) == L.EVDR_OK
    assert score(m=0) == L.EVDR_OK
    assert score(nq=0, ptr=None, pages=None, out=None) == L.EVDR_OK     # empty calls take no pointers


def _corpus(kind, np_=8, lp=40, idx_base=0):
    """A PageCorpus over host tensors: the argument checks of a subset call come before any device work."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    tm, pf = torch.zeros(np_, 2, dtype=torch.int32), torch.zeros(np_, dtype=torch.int32)
    if kind == "bf16":
        return PageCorpus(torch.zeros(1, np_, lp, 128, dtype=torch.bfloat16), tm, pf, idx_base)
    if kind == "fp8":
        return PageCorpus(torch.zeros(1, np_, lp, 128, dtype=ops.FP8), tm, pf, idx_base, shift=torch.zeros(np_, dtype=torch.int32))
    return PageCorpus(torch.zeros(4 if kind == "wide" else 2, np_, lp, 128, dtype=torch.float16), tm, pf, idx_base,
                      torch.zeros(1, dtype=torch.int32))


def test_python_refusals_come_before_any_device_work():
    import evdr_amd  # noqa: F401
    from evdr_amd.corpus import PageSubset, ShardedRetriever
    Q = torch.zeros(3, 8, 128, dtype=torch.bfloat16)
    allow = torch.ones(8, dtype=torch.bool)
    bf = _corpus("bf16")
    s = bf.subset(allow=allow)
    assert isinstance(s, PageSubset) and s.m == 8 and len(s) == 8
    # corpus kinds the feature does not cover: building a subset, and searching with one
    for kind, q in (("fp8", Q), ("wide", torch.zeros(3, 8, 256))):
        with pytest.raises(NotImplementedError, match="fp8|width-256"):
            _corpus(kind).subset(allow=allow)
        with pytest.raises(NotImplementedError, match="fp8|width-256"):
            _corpus(kind).score(q, None, subset=s)
        with pytest.raises(NotImplementedError, match="fp8|width-256"):
            _corpus(kind).topk(q, None, 5, subset=s)
    # exactly one of allow / pages; their types and shapes
    with pytest.raises(ValueError, match="exactly one"):
        bf.subset()
    with pytest.raises(ValueError, match="exactly one"):
        bf.subset(allow=allow, pages=torch.arange(3))
    for bad in (torch.ones(7, dtype=torch.bool), torch.ones(8, dtype=torch.int32), torch.ones(8, 1, dtype=torch.bool)):
        with pytest.raises(ValueError, match="allow"):
            bf.subset(allow=bad)
    for bad in (torch.zeros(3), torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="pages"):
            bf.subset(pages=bad)
    # prefilter with a subset
    f32 = _corpus("f32")
    with pytest.raises(ValueError, match="prefilter"):
        f32.topk(Q.float(), None, 5, prefilter=True, subset=f32.subset(allow=allow))
    # a subset of another corpus: another tensor, another size, a view with a different idx_base
    for other in (_corpus("bf16"), _corpus("bf16", np_=9), bf.shard(1, 8), _corpus("f32")):
        with pytest.raises(ValueError, match="another corpus"):
            other.score(Q if other.nplanes == 1 else Q.float(), None, subset=s)
        with pytest.raises(ValueError, match="another corpus"):
            other.topk(Q if other.nplanes == 1 else Q.float(), None, 5, subset=s)
    with pytest.raises(ValueError, match="another corpus"):
        bf.score(Q, None, subset=torch.arange(8, dtype=torch.int32))
    # the view of ALL pages at the same idx_base is the same corpus; it gets as far as the device check
    with pytest.raises(RuntimeError, match="GPU only"):
        bf.shard(0, 8).score(Q, None, subset=s)
    with pytest.raises(RuntimeError, match="GPU only"):
        bf.topk(Q, None, 5, subset=s)
    # the retriever: ties need the full block
    with pytest.raises(ValueError, match="ties"):
        ShardedRetriever(bf).search(Q, None, k=5, with_ties=True, subset=s)
    with pytest.raises(ValueError, match="another corpus"):
        ShardedRetriever(_corpus("bf16")).search(Q, None, k=5, subset=s)


def test_ops_wrapper_refuses_before_device_work():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.maxsim_forward_pages(torch.zeros(1, 3, 8, 128, dtype=torch.bfloat16), None, torch.zeros(1, 8, 40, 128, dtype=torch.bfloat16),
                                 None, None, torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32),
                                 torch.zeros(4, dtype=torch.int32))


def test_subset_normalisation_is_a_sorted_set():
    """subset() against a plain Python set: ascending, duplicates merged, entries the corpus does not own dropped (int32 and int64 lists,
    idx_base != 0), the mask form, and the empty results."""
    import evdr_amd  # noqa: F401
    gen = torch.Generator().manual_seed(5)
    for idx_base, n in ((0, 50), (1000, 37)):
        c = _corpus("bf16", np_=n, idx_base=idx_base)
        for dtype in (torch.int64, torch.int32):
            raw = torch.randint(idx_base - 20, idx_base + n + 20, (200,), generator=gen).to(dtype)
            raw = torch.cat([raw, torch.tensor([-1, idx_base + n, 2 ** 30, -(2 ** 31), idx_base, idx_base + n - 1]).to(dtype)])
            want = sorted({int(v) - idx_base for v in raw.tolist() if idx_base <= int(v) < idx_base + n})
            s = c.subset(pages=raw)
            assert s.pages.dtype == torch.int32 and s.pages.dim() == 1 and s.pages.is_contiguous()
            assert s.pages.tolist() == want and s.m == len(want)
            assert c.subset(pages=raw.flip(0)).pages.tolist() == want
        allow = torch.rand(n, generator=gen) < 0.3
        s = c.subset(allow=allow)
        assert s.pages.tolist() == [i for i in range(n) if allow[i]] and s.m == int(allow.sum())
        deleted = torch.zeros(n, dtype=torch.bool)
        deleted[[0, n - 1, 7]] = True
        assert c.subset(allow=~deleted).pages.tolist() == [i for i in range(n) if i not in (0, n - 1, 7)]
        for empty in (c.subset(allow=torch.zeros(n, dtype=torch.bool)), c.subset(pages=torch.tensor([-1, idx_base + n])),
                      c.subset(pages=torch.zeros(0, dtype=torch.int64))):
            assert empty.m == 0 and tuple(empty.pages.shape) == (0,) and empty.pages.dtype == torch.int32


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not available")
def test_pages_instances_pass_the_ring_audit_and_use_no_scratch():
    """The four shared-list instances (maxsim_fwd16s_pages_kernel<QW, NPL, ST>: bf16 with one and four queries per wave on 8-tile stages,
    fp16 hi/lo with one and two on 4-tile stages) are in the audited listing, each passes scratch/audit_ring_isa.py (rule C: no scratch
    access), and the listing holds at least the 30 earlier instances plus these four."""
    audit = os.path.join(ROOT, "scratch", "audit_ring_isa.py")
    r = subprocess.run([sys.executable, audit], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and re.match(r"^\d+ instances audited, 0 failing$", lines[-1]), (r.stdout[-1500:], r.stderr[-500:])
    assert int(lines[-1].split()[0]) >= 34
    pages = [ln for ln in lines if "maxsim_fwd16s_pages_kernel<" in ln]
    assert len(pages) == 4 and all(ln.startswith("ok") for ln in pages), pages
    for inst in ("<1, 1, 8>", "<4, 1, 8>", "<1, 2, 4>", "<2, 2, 4>"):
        assert any("maxsim_fwd16s_pages_kernel" + inst in ln for ln in pages), (inst, pages)
