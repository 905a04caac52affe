"""Candidate scoring, top-R selection and the two-stage search: exports, C-ABI argument errors, the Python-side
refusals and the compile-time checks of the new kernel instance, all without a GPU."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["evdr_maxsim_fwd_candidates_workspace", "evdr_maxsim_fwd_candidates", "evdr_select_topr"]


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_entries_are_declared_exported_and_bound(lib):
    from evdr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evdr.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"EVDR_API\s+[\w \*]+?\b" + n + r"\s*\(", header), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert re.search(r"#define\s+EVDR_SELECT_MAX\s+4096\b", header) and _lib.EVDR_SELECT_MAX == 4096
    assert lib.evdr_version() == 303


def test_candidate_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def score(nq=4, lq=8, np_=64, lp=40, nplanes=1, r=16, ptr=1, cand=1, out=1, out_stride=None, ws=None, wsb=0, p_stride=None):
        # pointers are fake: nothing is dereferenced on the host
        return lib.evdr_maxsim_fwd_candidates(ptr, ptr, None, ptr, ptr, cand, r, 0, out, r if out_stride is None else out_stride, None,
                                              nq, lq, np_, lp, nplanes, lp * 128 if p_stride is None else p_stride, np_ * lp * 128,
                                              None, None, ws, wsb, None)
    assert score(nplanes=4) == L.EVDR_ERR_SHAPE and b"256" in lib.evdr_last_error()
    assert score(nplanes=3) == L.EVDR_ERR_ARG
    assert score(lq=33) == L.EVDR_ERR_SHAPE and b"lq" in lib.evdr_last_error()
    assert score(r=0) == L.EVDR_ERR_ARG and b"r=0" in lib.evdr_last_error()
    assert score(r=4097) == L.EVDR_ERR_ARG and b"r=4097" in lib.evdr_last_error()
    assert score(nq=-1) == L.EVDR_ERR_ARG and score(np_=-1) == L.EVDR_ERR_ARG
    assert score(cand=None) == L.EVDR_ERR_ARG and score(out=None) == L.EVDR_ERR_ARG
    assert score(ptr=None) == L.EVDR_ERR_ARG
    assert score(out_stride=15) == L.EVDR_ERR_ARG and b"out_stride" in lib.evdr_last_error()
    assert score(p_stride=39 * 128) == L.EVDR_ERR_ARG
    assert score(lp=0) == L.EVDR_ERR_SHAPE
    assert score() == L.EVDR_ERR_WORKSPACE
    assert score(ws=1, wsb=16) == L.EVDR_ERR_WORKSPACE
    assert score(nq=0) == L.EVDR_OK
    assert lib.evdr_maxsim_fwd_candidates_workspace(4, 16) >= 3 * 4 * 16 * 4 + 4 * 4
    assert lib.evdr_maxsim_fwd_candidates_workspace(-1, 16) == 0
    assert lib.evdr_maxsim_fwd_candidates_workspace(4, 0) == 0 and lib.evdr_maxsim_fwd_candidates_workspace(4, 4097) == 0


def test_select_topr_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L
    assert lib.evdr_select_topr(1, 4, 100, 100, 0, 0, 1, None) == L.EVDR_ERR_ARG and b"r=0" in lib.evdr_last_error()
    assert lib.evdr_select_topr(1, 4, 100, 100, 0, 4097, 1, None) == L.EVDR_ERR_ARG
    assert lib.evdr_select_topr(1, -1, 100, 100, 0, 8, 1, None) == L.EVDR_ERR_ARG
    assert lib.evdr_select_topr(1, 4, -1, 100, 0, 8, 1, None) == L.EVDR_ERR_ARG
    assert lib.evdr_select_topr(None, 4, 100, 100, 0, 8, 1, None) == L.EVDR_ERR_ARG
    assert lib.evdr_select_topr(1, 4, 100, 100, 0, 8, None, None) == L.EVDR_ERR_ARG
    assert lib.evdr_select_topr(1, 4, 100, 99, 0, 8, 1, None) == L.EVDR_ERR_ARG and b"row_stride" in lib.evdr_last_error()
    assert lib.evdr_select_topr(None, 0, 100, 100, 0, 8, None, None) == L.EVDR_OK


def _corpus(kind, np_=8, lp=40, idx_base=0):
    """A PageCorpus over host tensors: the argument checks of a candidate call come before any device work."""
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
    Q = torch.zeros(3, 8, 128, dtype=torch.bfloat16)
    cand = torch.zeros(3, 16, dtype=torch.int32)
    for call in (lambda c, q, l: c.score_candidates(q, None, l), lambda c, q, l: c.rerank(q, None, l, 5)):
        with pytest.raises(NotImplementedError, match="fp8"):
            call(_corpus("fp8"), Q, cand)
        with pytest.raises(NotImplementedError, match="width-256"):
            call(_corpus("wide"), torch.zeros(3, 8, 256), cand)
        with pytest.raises(NotImplementedError, match="32 tokens"):
            call(_corpus("bf16"), torch.zeros(3, 33, 128, dtype=torch.bfloat16), cand)
        for bad in (cand.long(), cand[:2], cand[0], torch.zeros(3, 16, dtype=torch.int32, device="meta")):
            with pytest.raises(ValueError, match="int32"):
                call(_corpus("bf16"), Q, bad)
        with pytest.raises(ValueError, match="4096"):
            call(_corpus("f32"), Q.float(), torch.zeros(3, 4097, dtype=torch.int32))
        with pytest.raises(ValueError, match="outside"):
            call(_corpus("f32"), Q.float(), torch.zeros(3, 0, dtype=torch.int32))
    for k in (0, 17, 129):                              # k outside 1..min(r, EVDR_TOPK_MAX)
        with pytest.raises(ValueError, match="k="):
            _corpus("bf16").rerank(Q, None, torch.zeros(3, 16 if k < 129 else 200, dtype=torch.int32), k)


def test_two_stage_retriever_refusals():
    import evdr_amd  # noqa: F401
    from evdr_amd.corpus import TwoStageRetriever
    with pytest.raises(ValueError, match="same pages"):
        TwoStageRetriever(_corpus("fp8", np_=9), _corpus("bf16", np_=8))
    with pytest.raises(ValueError, match="same pages"):
        TwoStageRetriever(_corpus("fp8", idx_base=8), _corpus("bf16"))
    with pytest.raises(NotImplementedError, match="exact"):
        TwoStageRetriever(_corpus("bf16"), _corpus("fp8"))
    with pytest.raises(NotImplementedError, match="exact"):
        TwoStageRetriever(_corpus("bf16"), _corpus("wide"))
    ts = TwoStageRetriever(_corpus("fp8", lp=7), _corpus("bf16"))           # page length and kind of the first stage are free
    Q = torch.zeros(3, 8, 128, dtype=torch.bfloat16)
    for k, c in ((0, 64), (129, 512), (10, 9), (10, 4097)):
        with pytest.raises(ValueError, match="outside"):
            ts.search(Q, None, k=k, candidates=c)
    with pytest.raises(NotImplementedError, match="32 tokens"):
        ts.search(torch.zeros(3, 33, 128, dtype=torch.bfloat16), None, k=5, candidates=64)


def test_ops_wrappers_refuse_before_device_work():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.select_topr(torch.zeros(3, 10), 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.maxsim_forward_candidates(torch.zeros(1, 3, 8, 128, dtype=torch.bfloat16), None, torch.zeros(1, 8, 40, 128, dtype=torch.bfloat16),
                                      None, None, torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32),
                                      torch.zeros(3, 4, dtype=torch.int32))


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not available")
def test_bf16_gather_instance_passes_the_ring_audit_and_uses_no_scratch():
    """The new NPL = 1, GATHER instance of maxsim_fwd16s_kernel is in the audited listing beside the fp16 hi/lo one (template
    arguments: QW, NPL, ..., HI, GATHER), passes scratch/audit_ring_isa.py (rule C: no scratch access), and the listing has 30 instances."""
    audit = os.path.join(ROOT, "scratch", "audit_ring_isa.py")
    r = subprocess.run([sys.executable, audit], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and re.match(r"^\d+ instances audited, 0 failing$", lines[-1]), (r.stdout[-1500:], r.stderr[-500:])
    assert int(lines[-1].split()[0]) >= 30
    gather = [ln for ln in lines if re.search(r"maxsim_fwd16s_kernel<.*, false, true>", ln)]
    assert len(gather) == 2 and all(ln.startswith("ok") for ln in gather), gather
    assert any(re.search(r"kernel<1, 1, false, 8, 2,", ln) for ln in gather) and any(re.search(r"kernel<1, 2, false, 4, 2,", ln) for ln in gather)
