"""fp8 (e4m3fn) corpora: exports, C-ABI argument errors, the Python-side refusals that need no device, and the gfx950 listing of
csrc/maxsim_fwd8.hip (ring rules A-F of scratch/audit_ring_isa.py, no scratch, no spills) -- all without a GPU."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "efficient-visual-document-retrieval_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ["evdr_quantize_fp8", "evdr_maxsim_fwd_fp8"]


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_fp8_entries_are_declared_and_exported(lib):
    from evdr_amd import _lib
    header = open(os.path.join(ROOT, "include", "evdr.h")).read()
    for n in NEW:
        assert re.search(r"EVDR_API int " + n + r"\(", header), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert _lib.ABI_VERSION == 303 and lib.evdr_version() == 303


def test_quantize_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def q(x=1, dtype=L.EVDR_F32, groups=4, rpg=8, d=128, x8=1, shift=1):
        return lib.evdr_quantize_fp8(x, dtype, groups, rpg, d, x8, shift, None)
    assert q(dtype=L.EVDR_F16) == L.EVDR_ERR_ARG and b"dtype" in lib.evdr_last_error()
    assert q(dtype=7) == L.EVDR_ERR_ARG
    assert q(groups=-1) == L.EVDR_ERR_ARG and q(rpg=-1) == L.EVDR_ERR_ARG and q(d=-1) == L.EVDR_ERR_ARG
    assert q(d=129) == L.EVDR_ERR_SHAPE and b"width" in lib.evdr_last_error()
    assert q(d=0) == L.EVDR_ERR_SHAPE
    assert q(x=None) == L.EVDR_ERR_ARG and q(x8=None) == L.EVDR_ERR_ARG and q(shift=None) == L.EVDR_ERR_ARG
    assert q(groups=0, x=None, x8=None, shift=None) == L.EVDR_OK          # nothing to do, nothing launched


def test_forward_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def f(nq=4, lq=8, np_=16, lp=40, ptr=1, qs=1, ps=1, out_stride=None, p_stride=None):
        return lib.evdr_maxsim_fwd_fp8(ptr, ptr, None, ptr, ptr, ptr, np_ if out_stride is None else out_stride, nq, lq, np_, lp,
                                       lp * 128 if p_stride is None else p_stride, qs, ps, None, None)
    assert f(nq=-1) == L.EVDR_ERR_ARG and f(lp=-2) == L.EVDR_ERR_ARG
    assert f(lp=70000) == L.EVDR_ERR_SHAPE
    assert f(lq=0) == L.EVDR_ERR_SHAPE
    assert f(ptr=None) == L.EVDR_ERR_ARG and b"null" in lib.evdr_last_error()
    assert f(qs=None) == L.EVDR_ERR_ARG and f(ps=None) == L.EVDR_ERR_ARG
    assert f(out_stride=15) == L.EVDR_ERR_ARG and f(p_stride=40 * 128 - 16) == L.EVDR_ERR_ARG
    assert f(p_stride=40 * 128 + 8) == L.EVDR_ERR_ARG
    assert f(nq=0, ptr=None) == L.EVDR_OK and f(np_=0, ptr=None) == L.EVDR_OK       # empty score matrix


def test_python_refusals_need_no_gpu():
    import torch
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    with pytest.raises(ValueError, match="dtype"):
        PageCorpus.from_tensor(torch.zeros(2, 3, 128), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):           # fp8 planes need their per-page shifts
        PageCorpus(torch.zeros(1, 2, 3, 128).to(torch.float8_e4m3fn), torch.zeros(2, 1, dtype=torch.int32),
                   torch.zeros(2, dtype=torch.int32))
    assert ops.FP8 is torch.float8_e4m3fn


def _fwd8_listing(extra=()):
    from evdr_amd import build as B
    sys.path.insert(0, os.path.join(ROOT, "scratch"))
    import audit_ring_isa as A
    with tempfile.TemporaryDirectory() as tmp:
        lst = os.path.join(tmp, "fwd8.s")
        cmd = [HIPCC] + B.FLAGS + list(extra) + B.EXTRA_FLAGS.get("maxsim_fwd8.hip", []) + [
            "--cuda-device-only", "-S", os.path.join(CSRC, "maxsim_fwd8.hip"), "-o", lst]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        return A, open(lst).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("extra", [(), ("-DEVDR_SENTINEL",)], ids=["product", "sentinel"])
def test_fwd8_listing_passes_the_ring_audit_without_scratch(extra):
    A, text = _fwd8_listing(extra)
    lines = text.splitlines()
    found = 0
    for name, body in A.kernels(lines):
        errs, stats = A.audit(name, body)
        assert not errs, (name, sorted(set(errs)))
        assert stats["mfma"] > 0 and stats["lds_dma"] > 0, (name, stats)
        found += 1
    assert found >= 4
    assert "v_mfma_scale_f32_16x16x128_f8f6f4" in text
    # no scratch and no VGPR spills (SGPR spills of the eight-query instance go to VGPR lanes, never to memory)
    metas = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(metas) == found and all(int(m) == 0 for m in metas), metas
    assert len(spills) == found and all(int(s) == 0 for s in spills), spills


def test_quantiser_uses_no_scratch():
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    from evdr_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        lst = os.path.join(tmp, "q8.s")
        r = subprocess.run([HIPCC] + B.FLAGS + ["--cuda-device-only", "-S", os.path.join(CSRC, "quant8.hip"), "-o", lst],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(lst).read()
    assert "quantize_fp8_kernel" in text
    assert all(int(m) == 0 for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))
