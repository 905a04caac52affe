"""Growable corpora (evdr_corpus_ingest, ops.corpus_ingest, PageCorpus.empty / append / replace): exports, C-ABI
argument errors and the Python-side refusals, all before any device work and without a GPU."""
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


def test_entry_is_declared_exported_and_bound(lib):
    from evdr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evdr.h")).read(), flags=re.S)
    assert re.search(r"EVDR_API\s+[\w \*]+?\bevdr_corpus_ingest\s*\(", header)
    assert hasattr(lib, "evdr_corpus_ingest") and "evdr_corpus_ingest" in _lib.SIGNATURES
    for name in ("EVDR_CORPUS_BF16", "EVDR_CORPUS_F16_HILO", "EVDR_CORPUS_F16_WIDE", "EVDR_CORPUS_FP8"):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == getattr(_lib, name)


def test_ingest_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def ingest(src=1, src_dtype=L.EVDR_BF16, b=2, lp_src=40, d_src=128, src_stride=None, planes=16, kind=L.EVDR_CORPUS_BF16, capacity=8,
               lp=40, p_stride=None, plane_stride=8 * 40 * 128, words=1, shift=None, amax=None, first=0, dst=None):
        # pointers are fake: nothing is dereferenced on the host
        return lib.evdr_corpus_ingest(src, src_dtype, None, b, lp_src, d_src, lp_src * d_src if src_stride is None else src_stride,
                                      planes, kind, capacity, lp, lp * 128 if p_stride is None else p_stride, plane_stride, words, words,
                                      shift, amax, first, dst, None, None)

    def refused(code, text, **kw):
        rc = ingest(**kw)
        return rc == code and text in lib.evdr_last_error()

    assert refused(L.EVDR_ERR_SHAPE, b"lp_src", lp_src=41)
    assert refused(L.EVDR_ERR_SHAPE, b"d_src", d_src=129) and refused(L.EVDR_ERR_SHAPE, b"d_src", d_src=0)
    assert refused(L.EVDR_ERR_ARG, b"bf16 corpus", src_dtype=L.EVDR_F32) and refused(L.EVDR_ERR_ARG, b"bf16 corpus", src_dtype=L.EVDR_F16)
    assert refused(L.EVDR_ERR_ARG, b"absmax", kind=L.EVDR_CORPUS_F16_HILO, src_dtype=L.EVDR_F32)
    assert refused(L.EVDR_ERR_ARG, b"shifts", kind=L.EVDR_CORPUS_FP8)
    assert refused(L.EVDR_ERR_ARG, b"capacity", first=7) and refused(L.EVDR_ERR_ARG, b"capacity", first=-1)
    assert refused(L.EVDR_ERR_SHAPE, b"256", kind=L.EVDR_CORPUS_F16_WIDE, src_dtype=L.EVDR_F32, amax=1)
    assert refused(L.EVDR_ERR_ARG, b"kind", kind=3) and refused(L.EVDR_ERR_ARG, b"src_dtype", src_dtype=5)
    assert refused(L.EVDR_ERR_ARG, b"negative", b=-1) and refused(L.EVDR_ERR_ARG, b"negative", lp_src=-1)
    assert refused(L.EVDR_ERR_SHAPE, b"lp", lp=0, lp_src=0) and refused(L.EVDR_ERR_SHAPE, b"lp", lp=65536)
    assert refused(L.EVDR_ERR_ARG, b"null", src=None) and refused(L.EVDR_ERR_ARG, b"null", planes=None) and refused(L.EVDR_ERR_ARG, b"null", words=None)
    assert refused(L.EVDR_ERR_ARG, b"src_stride", src_stride=40 * 128 - 1)
    assert refused(L.EVDR_ERR_ARG, b"p_stride", p_stride=39 * 128) and refused(L.EVDR_ERR_ARG, b"aligned", p_stride=40 * 128 + 4)
    assert refused(L.EVDR_ERR_ARG, b"aligned", planes=8)
    assert refused(L.EVDR_ERR_ARG, b"aligned", kind=L.EVDR_CORPUS_FP8, shift=1, p_stride=40 * 128 + 8)
    # b = 0 writes nothing and takes no pointers; a destination list lifts the first_page rule (its entries are checked on the device)
    assert ingest(b=0, src=None, planes=None, words=None) == L.EVDR_OK
    assert ingest(b=0, first=8) == L.EVDR_OK and refused(L.EVDR_ERR_ARG, b"capacity", b=0, first=9)
    assert refused(L.EVDR_ERR_ARG, b"null", first=100, dst=1, planes=None)


def _corpus(kind, np_=8, lp=40, idx_base=0):
    """A PageCorpus over host tensors: the argument checks of append / replace come before any device work."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    tm, pf = torch.zeros(np_, 2, dtype=torch.int32), torch.zeros(np_, dtype=torch.int32)
    if kind == "bf16":
        return PageCorpus(torch.zeros(1, np_, lp, 128, dtype=torch.bfloat16), tm, pf, idx_base)
    if kind == "fp8":
        return PageCorpus(torch.zeros(1, np_, lp, 128, dtype=ops.FP8), tm, pf, idx_base, shift=torch.zeros(np_, dtype=torch.int32))
    return PageCorpus(torch.zeros(4 if kind == "wide" else 2, np_, lp, 128, dtype=torch.float16), tm, pf, idx_base,
                      torch.full((1,), 0x3F800000, dtype=torch.int32))


def test_empty_checks_its_arguments():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    for dt, kw, nplanes, pdt in ((torch.bfloat16, {}, 1, torch.bfloat16), (torch.float32, {"absmax": 1.0}, 2, torch.float16), (ops.FP8, {}, 1, ops.FP8)):
        c = PageCorpus.empty(6, 40, dt, "cpu", idx_base=12, **kw)
        assert (c.n_pages, c.capacity, c.lp, c.idx_base, c.nplanes) == (0, 6, 40, 12, nplanes)
        assert tuple(c.planes.shape) == (nplanes, 0, 40, 128) and c.planes.dtype == pdt and c.p_stride == 40 * 128
        assert tuple(c.tilemask.shape) == (0, 2) and tuple(c.pageflags.shape) == (0,)
        assert (c.shift is not None) == (dt == ops.FP8) and (c.amax is not None) == (dt == torch.float32)
    assert int(PageCorpus.empty(1, 8, torch.float32, "cpu", absmax=1.0).amax) == 0x3F800000
    assert int(PageCorpus.empty(1, 8, torch.float32, "cpu", absmax=0.75).amax) == 0x3F400000
    assert _corpus("bf16").capacity == 8                              # a corpus without reserved storage: capacity == n_pages
    for bad in (None, 0.0, -1.0, float("inf"), float("nan"), 1e-60, 1e60):
        with pytest.raises(ValueError, match="absmax"):
            PageCorpus.empty(4, 40, torch.float32, "cpu", absmax=bad)
    for dt in (torch.bfloat16, ops.FP8):
        with pytest.raises(ValueError, match="absmax"):
            PageCorpus.empty(4, 40, dt, "cpu", absmax=1.0)
    with pytest.raises(ValueError, match="dtype"):
        PageCorpus.empty(4, 40, torch.float16, "cpu")
    with pytest.raises(ValueError, match="capacity"):
        PageCorpus.empty(-1, 40, torch.bfloat16, "cpu")
    with pytest.raises(ValueError, match="lp"):
        PageCorpus.empty(4, 0, torch.bfloat16, "cpu")


def test_append_and_replace_refuse_before_any_device_work():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    bf = PageCorpus.empty(4, 40, torch.bfloat16, "cpu", idx_base=10)
    page = torch.zeros(2, 40, 128, dtype=torch.bfloat16)
    # dtype rules follow from_tensor: a bf16 corpus takes bf16 only, the others fp32 / bf16 / fp16
    with pytest.raises(RuntimeError, match="bf16 corpus needs bf16 pages"):
        bf.append(page.float())
    for kind in ("f32", "fp8"):
        with pytest.raises(ValueError, match="fp32, bf16 or fp16"):
            _corpus(kind).replace(torch.tensor([0, 1]), page.double())
    # shapes
    for bad in (torch.zeros(2, 41, 128, dtype=torch.bfloat16), torch.zeros(2, 40, 129, dtype=torch.bfloat16), torch.zeros(40, 128, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="pages"):
            bf.append(bad)
    with pytest.raises(ValueError, match="pmask"):
        bf.append(page, torch.ones(2, 39, dtype=torch.bool))
    # capacity, before the device check; b = 0 is a no-op that needs no device either
    with pytest.raises(ValueError, match="capacity"):
        bf.append(torch.zeros(5, 40, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="capacity"):
        _corpus("bf16").append(page)                                 # no reserved storage
    with pytest.raises(ValueError, match="capacity"):
        PageCorpus.empty(4, 40, torch.bfloat16, "cpu").shard(0, 0).append(page)
    assert bf.append(page[:0]) == 10 and bf.n_pages == 0
    with pytest.raises(RuntimeError, match="GPU only"):              # everything in order: it gets as far as the device check
        bf.append(page, torch.ones(2, 40, dtype=torch.bool))
    assert bf.n_pages == 0
    # width-256 corpora
    wide = _corpus("wide")
    with pytest.raises(NotImplementedError, match="width-256"):
        wide.append(torch.zeros(1, 40, 256))
    with pytest.raises(NotImplementedError, match="width-256"):
        wide.replace(torch.tensor([0]), torch.zeros(1, 40, 256))
    with pytest.raises(NotImplementedError, match="width-256"):
        PageCorpus.from_tensor(torch.zeros(2, 40, 200), capacity=4)
    with pytest.raises(ValueError, match="capacity"):
        PageCorpus.from_tensor(torch.zeros(5, 40, 128), capacity=4)
    # replace: indices owned by this corpus, below n_pages, no duplicates, one per page
    c = _corpus("bf16", idx_base=100)
    for bad, what in ((torch.tensor([100, 100]), "duplicate"), (torch.tensor([99, 100]), "outside"), (torch.tensor([100, 108]), "outside"),
                      (torch.tensor([100]), "pages must be"), (torch.tensor([100.0, 101.0]), "pages must be"), (torch.tensor([[100, 101]]), "pages must be")):
        with pytest.raises(ValueError, match=what):
            c.replace(bad, page)
    with pytest.raises(RuntimeError, match="GPU only"):
        c.replace(torch.tensor([107, 100]), page)
    c.replace(torch.zeros(0, dtype=torch.int64), page[:0])           # b = 0: a no-op
    # ops.corpus_ingest: the thin wrapper's own refusals
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.corpus_ingest(page, None, c.planes, c.tilemask, c.pageflags)
    # a pair whose corpora no longer hold the same pages
    ts = TwoStageRetriever(_corpus("fp8"), _corpus("bf16"))
    ts.coarse.n_pages = 7                                            # what an append to one corpus of the pair leaves behind
    with pytest.raises(ValueError, match="n_pages 7 vs 8"):
        ts.search(torch.zeros(3, 8, 128, dtype=torch.bfloat16), None, k=5, candidates=8)


def test_chunked_payload_loader_checks_its_arguments():
    import numpy as np
    import evdr_amd  # noqa: F401
    from evdr_amd.utils.preprocess_data import corpus_from_payload
    docs = np.empty(2, dtype=object)
    docs[0], docs[1] = np.zeros((3, 128), dtype=np.float32), np.zeros((5, 128), dtype=np.float32)
    with pytest.raises(ValueError, match="normalize"):
        corpus_from_payload(docs, None, None, "cpu", dtype=torch.float32, normalize=False, chunk_pages=1)
    with pytest.raises(ValueError, match="chunk_pages"):
        corpus_from_payload(docs, None, None, "cpu", chunk_pages=0)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_ingest_instances_use_no_scratch():
    """scratch/kres.py over csrc/ingest.hip: the 14 instances (7 source / kind pairs x aligned / element-wise reads) compile for gfx950
    without scratch memory and without VGPR spills."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scratch", "kres.py"), "ingest.hip", "corpus_ingest_kernel"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    rows = [ln for ln in r.stdout.splitlines() if "corpus_ingest_kernel<" in ln]
    assert r.returncode == 0 and len(rows) == 14, (r.stdout[-1500:], r.stderr[-500:])
    for ln in rows:
        m = re.search(r"VGPR\s+(\d+) AGPR\s+(\d+) spill\s+(\d+) sspill\s+\d+ scratch\s+(\d+)", ln)
        assert m and int(m.group(3)) == 0 and int(m.group(4)) == 0, ln
