"""Prefiltered fp32 top-k (PageCorpus.topk(..., prefilter=True)): exports, C-ABI argument errors and the Python-side rejections,
all without a GPU."""
import ctypes

import pytest
import torch

NEW = ["evdr_prefilter_corpus_bound", "evdr_prefilter_query_bound", "evdr_maxsim_fwd_coarse",
       "evdr_maxsim_topk_prefilter_workspace", "evdr_maxsim_topk_prefilter"]


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_prefilter_entries_are_exported(lib):
    from evdr_amd import _lib
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n


def test_prefilter_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def topk(nq=4, lq=8, np_=64, lp=40, nplanes=2, k=10, cap=64, ptr=1, ws=None, wsb=0, bound=1):
        return lib.evdr_maxsim_topk_prefilter(ptr, ptr, None, ptr, ptr, nq, lq, np_, lp, nplanes, lp * 128, np_ * lp * 128, ptr, ptr,
                                              bound, 0, k, cap, ptr, ptr, None, ws, wsb, None)
    assert topk(nplanes=1) == L.EVDR_ERR_ARG and b"nplanes" in lib.evdr_last_error()
    assert topk(nplanes=4) == L.EVDR_ERR_ARG
    assert topk(lq=33) == L.EVDR_ERR_SHAPE and b"lq" in lib.evdr_last_error()
    assert topk(k=0) == L.EVDR_ERR_ARG and topk(k=129) == L.EVDR_ERR_ARG
    assert topk(k=10, cap=9) == L.EVDR_ERR_ARG and b"capacity" in lib.evdr_last_error()
    assert topk(nq=-1) == L.EVDR_ERR_ARG
    assert topk(ptr=None) == L.EVDR_ERR_ARG
    assert topk(bound=None) == L.EVDR_ERR_ARG
    assert topk() == L.EVDR_ERR_WORKSPACE                            # pointers are fake: nothing is dereferenced on the host
    assert topk(ws=1, wsb=16) == L.EVDR_ERR_WORKSPACE
    assert topk(nq=0) == L.EVDR_OK
    need = lib.evdr_maxsim_topk_prefilter_workspace(4, 64, 64)
    assert need >= 4 * 64 * 4 + 2 * 4 * 64 * 4
    assert lib.evdr_maxsim_topk_prefilter_workspace(-1, 64, 64) == 0 and lib.evdr_maxsim_topk_prefilter_workspace(4, 64, 0) == 0
    rc = lib.evdr_maxsim_fwd_coarse(1, 1, None, 1, 1, 1, 64, 4, 33, 64, 40, 40 * 128, 64 * 40 * 128, 1, 1, None)
    assert rc == L.EVDR_ERR_SHAPE
    rc = lib.evdr_maxsim_fwd_coarse(None, None, None, None, None, None, 64, 4, 8, 64, 40, 40 * 128, 64 * 40 * 128, None, None, None)
    assert rc == L.EVDR_ERR_ARG
    rc = lib.evdr_maxsim_fwd_coarse(1, 1, None, 1, 1, 1, 10, 4, 8, 64, 40, 40 * 128, 64 * 40 * 128, 1, 1, None)
    assert rc == L.EVDR_ERR_ARG and b"out_stride" in lib.evdr_last_error()
    assert lib.evdr_prefilter_query_bound(1, None, 4, 33, 1, 1, 1, 1, None) == L.EVDR_ERR_SHAPE
    assert lib.evdr_prefilter_query_bound(None, None, 4, 8, None, None, None, None, None) == L.EVDR_ERR_ARG
    assert lib.evdr_prefilter_query_bound(None, None, 0, 8, None, None, None, None, None) == L.EVDR_OK
    assert lib.evdr_prefilter_corpus_bound(1, 1, 1, 64, 40, 40 * 128, 64 * 40 * 128, None, None) == L.EVDR_ERR_ARG
    assert lib.evdr_prefilter_corpus_bound(None, None, None, 64, 40, 40 * 128, 64 * 40 * 128, 1, None) == L.EVDR_ERR_ARG
    assert lib.evdr_prefilter_corpus_bound(1, 1, 1, 64, 40, 39 * 128, 64 * 40 * 128, 1, None) == L.EVDR_ERR_ARG
    assert lib.evdr_version() == 303


def _corpus(nplanes, np_=8, lp=40):
    """A PageCorpus over host tensors: the argument checks of a prefiltered call come before any device work."""
    from evdr_amd.corpus import PageCorpus
    if nplanes == 1:
        planes, amax = torch.zeros(1, np_, lp, 128, dtype=torch.bfloat16), None
    else:
        planes, amax = torch.zeros(nplanes, np_, lp, 128, dtype=torch.float16), torch.zeros(1, dtype=torch.int32)
    return PageCorpus(planes, torch.zeros(np_, 2, dtype=torch.int32), torch.zeros(np_, dtype=torch.int32), 0, amax)


def test_python_rejects_what_the_prefilter_does_not_cover():
    import evdr_amd  # noqa: F401
    from evdr_amd.corpus import ShardedRetriever
    Q = torch.zeros(3, 8, 128)
    with pytest.raises(ValueError, match="bf16"):
        _corpus(1).topk(Q.bfloat16(), None, 5, prefilter=True)
    with pytest.raises(NotImplementedError, match="width-256"):
        _corpus(4).topk(torch.zeros(3, 8, 256), None, 5, prefilter=True)
    fp32 = _corpus(2)
    with pytest.raises(NotImplementedError, match="32 tokens"):
        fp32.topk(torch.zeros(3, 33, 128), None, 5, prefilter=True)
    for k in (0, 129):
        with pytest.raises(ValueError, match="outside"):
            fp32.topk(Q, None, k, prefilter=True)
    with pytest.raises(ValueError, match="capacity"):
        fp32.topk(Q, None, 10, prefilter=True, capacity=9)
    with pytest.raises(ValueError, match="with_ties"):
        ShardedRetriever(fp32).search(Q, None, 5, with_ties=True, prefilter=True)
    with pytest.raises(RuntimeError, match="no prefiltered"):
        fp32.prefilter_stats()


def test_shard_views_share_the_corpus_bound():
    import evdr_amd  # noqa: F401
    c = _corpus(2, np_=9)
    a, b = c.shard(0, 4), c.shard(4, 9)
    assert a._bound_owner is c and b._bound_owner is c and b.shard(1, 3)._bound_owner is c
    c._pf_bound = torch.ones(2)                       # what the first prefiltered call of any of them computes, once
    assert a.prefilter_bound() is c._pf_bound and b.prefilter_bound() is c._pf_bound
