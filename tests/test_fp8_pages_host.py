"""fp8 page-list forward and the filtered two-stage search: the export, the C-ABI status codes and the Python-side
refusals that need no device."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "evdr_maxsim_fwd_fp8_pages"


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_entry_is_declared_and_exported(lib):
    from evdr_amd import _lib
    header = open(os.path.join(ROOT, "include", "evdr.h")).read()
    assert re.search(r"EVDR_API int " + ENTRY + r"\(", header)
    assert hasattr(lib, ENTRY) and ENTRY in _lib.SIGNATURES
    section = header[header.index("fp8 corpora: OCP e4m3fn"):header.index("EVDR_API int evdr_quantize_fp8(")]      # the fp8 section's comment
    assert ENTRY in section and "BIT-EQUAL" in section[section.index(ENTRY):]
    assert _lib.ABI_VERSION == 303 and lib.evdr_version() == 303


def test_status_codes_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def f(nq=4, lq=8, np_=16, lp=40, m=5, ptr=1, pages=1, out=1, qs=1, ps=1, ws=None, out_stride=None, p_stride=None):
        return lib.evdr_maxsim_fwd_fp8_pages(ptr, ptr, None, ptr, ptr, pages, m, out, m if out_stride is None else out_stride, nq, lq,
                                             np_, lp, lp * 128 if p_stride is None else p_stride, qs, ps, ws, None)
    # nothing to do: OK, nothing launched, null pointers accepted
    assert f(nq=0) == L.EVDR_OK and f(m=0) == L.EVDR_OK
    assert f(nq=0, ptr=None, pages=None, out=None, qs=None, ps=None) == L.EVDR_OK
    assert f(m=0, ptr=None, pages=None, out=None, qs=None, ps=None) == L.EVDR_OK
    assert f(m=0, np_=0, ptr=None, pages=None, out=None) == L.EVDR_OK
    # a list over an empty corpus
    assert f(np_=0) == L.EVDR_ERR_SHAPE and b"empty corpus" in lib.evdr_last_error()
    # long queries need the qlist workspace
    assert f(lq=33) == L.EVDR_ERR_WORKSPACE and b"qlist" in lib.evdr_last_error()
    assert f(lq=64) == L.EVDR_ERR_WORKSPACE
    # argument errors
    assert f(ptr=None) == L.EVDR_ERR_ARG and b"null" in lib.evdr_last_error()
    assert f(pages=None) == L.EVDR_ERR_ARG and f(out=None) == L.EVDR_ERR_ARG
    assert f(qs=None) == L.EVDR_ERR_ARG and f(ps=None) == L.EVDR_ERR_ARG
    assert f(m=-1) == L.EVDR_ERR_ARG and f(nq=-1) == L.EVDR_ERR_ARG
    assert f(out_stride=4) == L.EVDR_ERR_ARG
    assert f(p_stride=40 * 128 - 16) == L.EVDR_ERR_ARG and f(p_stride=40 * 128 + 8) == L.EVDR_ERR_ARG
    # shapes out of range, zero-length token axes
    assert f(lp=70000) == L.EVDR_ERR_SHAPE and f(m=2 ** 31) == L.EVDR_ERR_SHAPE
    assert f(lq=0) == L.EVDR_ERR_SHAPE and f(lp=0) == L.EVDR_ERR_SHAPE


def _corpus(kind, np_=8, lp=40, idx_base=0):
    """A PageCorpus over host tensors: the argument checks come before any device work."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    tm, pf = torch.zeros(np_, 2, dtype=torch.int32), torch.zeros(np_, dtype=torch.int32)
    if kind == "bf16":
        return PageCorpus(torch.zeros(1, np_, lp, 128, dtype=torch.bfloat16), tm, pf, idx_base)
    if kind == "fp8":
        return PageCorpus(torch.zeros(1, np_, lp, 128, dtype=ops.FP8), tm, pf, idx_base, shift=torch.zeros(np_, dtype=torch.int32))
    return PageCorpus(torch.zeros(4 if kind == "wide" else 2, np_, lp, 128, dtype=torch.float16), tm, pf, idx_base,
                      torch.zeros(1, dtype=torch.int32))


def test_two_stage_subset_refusals_come_before_any_device_work():
    import evdr_amd  # noqa: F401
    from evdr_amd.corpus import TwoStageRetriever
    Q = torch.zeros(3, 8, 128, dtype=torch.bfloat16)
    allow = torch.ones(8, dtype=torch.bool)
    exact = _corpus("bf16")
    ts = TwoStageRetriever(_corpus("fp8", lp=7), exact)
    s = exact.subset(allow=allow)
    # a subset of another corpus: another tensor, the coarse corpus's kind of list, a raw tensor
    for other in (_corpus("bf16").subset(allow=allow), _corpus("f32").subset(allow=allow), torch.arange(8, dtype=torch.int32)):
        with pytest.raises(ValueError, match="another corpus"):
            ts.search(Q, None, k=2, candidates=4, subset=other)
    # a view of the same pages with another idx_base
    whole = _corpus("bf16", np_=16)
    view = whole.shard(8, 16)
    ts_view = TwoStageRetriever(_corpus("fp8", idx_base=8), view)
    with pytest.raises(ValueError, match="another corpus"):
        ts_view.search(Q, None, k=2, candidates=4, subset=whole.shard(0, 8).subset(allow=allow))
    with pytest.raises(ValueError, match="another corpus"):
        ts_view.search(Q, None, k=2, candidates=4, subset=whole.subset(allow=torch.ones(16, dtype=torch.bool)))
    # a width-256 first stage
    wide = TwoStageRetriever(_corpus("wide"), exact)
    with pytest.raises(NotImplementedError, match="width-256"):
        wide.search(Q, None, k=2, candidates=4, subset=s, Q_coarse=torch.zeros(3, 8, 256))
    # the argument checks of the unfiltered search still come first
    with pytest.raises(ValueError, match="candidates"):
        ts.search(Q, None, k=5, candidates=4, subset=s)
    # a valid subset gets as far as the device check: the existing error, not a TypeError
    with pytest.raises(RuntimeError, match="GPU only"):
        ts.search(Q, None, k=2, candidates=4, subset=s)
    with pytest.raises(RuntimeError, match="GPU only"):
        ts_view.search(Q, None, k=2, candidates=4, subset=view.subset(pages=torch.tensor([9, 3, 12])))


def test_score_pages_refusals_come_before_any_device_work():
    import evdr_amd  # noqa: F401
    Q = torch.zeros(3, 8, 128, dtype=torch.bfloat16)
    good = torch.tensor([1, 0, 1], dtype=torch.int32)
    for kind in ("fp8", "bf16", "f32"):
        c = _corpus(kind)
        q = Q if kind != "f32" else Q.float()
        for bad in (good.long(), good.float(), good[None], good.to("meta"), [1, 0, 1]):
            with pytest.raises(ValueError, match="pages"):
                c.score_pages(q, None, bad)
        with pytest.raises(RuntimeError, match="GPU only"):
            c.score_pages(q, None, good)
    with pytest.raises(NotImplementedError, match="width-256"):
        _corpus("wide").score_pages(torch.zeros(3, 8, 256), None, good)


def test_ops_wrapper_refuses_before_device_work():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    q8 = torch.zeros(3, 8, 128, dtype=ops.FP8)
    p8 = torch.zeros(8, 40, 128, dtype=ops.FP8)
    z = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.maxsim_forward_fp8_pages(q8, z[:3], p8, z, None, torch.zeros(8, 2, dtype=torch.int32), z, torch.zeros(2, dtype=torch.int32))


def test_pinned_fp8_refusals_point_to_the_new_paths():
    import evdr_amd  # noqa: F401
    c = _corpus("fp8")
    with pytest.raises(NotImplementedError, match="fp8") as e:
        c.subset(allow=torch.ones(8, dtype=torch.bool))
    assert "score_pages" in str(e.value) and "TwoStageRetriever" in str(e.value)
