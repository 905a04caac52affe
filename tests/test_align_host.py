"""Token alignment without a GPU: the torch statement of the rule against a naive per-pair loop, `ops.hard_patch`
against the heat map and against the reference's hard-token loop, the C-ABI and Python refusals, and the kernel's compile-time
resources."""
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import v3_patterns as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "efficient-visual-document-retrieval_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NINF = float("-inf")


@pytest.fixture(scope="module")
def lib():
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- the rule, pair by pair and element by element --------------------------------------------------------------------------------
def naive_align(Q, qmask, P, pmask, cand, idx_base):
    Qn, Pn = Q.double().numpy(), P.double().numpy()
    nq, lq, _ = Qn.shape
    npg, lp, _ = Pn.shape
    r = cand.shape[1]
    sim = np.zeros((nq, r, lq), dtype=np.float64)
    patch = np.full((nq, r, lq), -1, dtype=np.int64)
    heat = np.full((nq, r, lp), NINF, dtype=np.float64)
    for q in range(nq):
        q_bad = not np.isfinite(Qn[q]).all()
        for i in range(r):
            p = int(cand[q, i]) - idx_base
            if p < 0 or p >= npg:
                sim[q, i] = NINF
                continue
            valid = [m for m in range(lp) if pmask[p, m]]
            if not valid:
                continue
            if q_bad or any(not np.isfinite(Pn[p, m]).all() for m in valid):
                for n in range(lq):
                    if qmask[q, n]:
                        sim[q, i, n] = math.nan
                heat[q, i] = math.nan
                continue
            for n in range(lq):
                if not qmask[q, n]:
                    continue
                best, at = NINF, -1
                for m in range(lp):
                    v = float(np.dot(Qn[q, n], Pn[p, m])) if pmask[p, m] else -1e4
                    if v > best:
                        best, at = v, m
                sim[q, i, n], patch[q, i, n] = best, at
                for m in valid:
                    heat[q, i, m] = max(heat[q, i, m], float(np.dot(Qn[q, n], Pn[p, m])))
    return sim.astype(np.float32), patch.astype(np.int32), heat.astype(np.float32)


def _hand_made_case():
    g = torch.Generator().manual_seed(11)
    nq, lq, npg, lp, d = 4, 5, 6, 9, 16
    Q = torch.randn(nq, lq, d, generator=g)
    P = torch.randn(npg, lp, d, generator=g)
    qmask = torch.ones(nq, lq, dtype=torch.bool)
    pmask = torch.ones(npg, lp, dtype=torch.bool)
    P[0, 6] = P[0, 2]                                   # duplicate rows: the lower index wins
    P[0, 8] = P[0, 2]
    qmask[0, 3] = False                                 # a masked query token
    pmask[1] = False                                    # an all-masked page
    qmask[2] = False                                    # a query with no valid token
    pmask[2, 5:] = False                                # a ragged page
    pmask[3, [0, 4]] = False                            # masked patches in front of and between valid ones
    P[4, 3, 7] = float("nan")                           # a NaN patch in a valid position
    P[5, 3, 7] = float("nan")                           # ... and in a masked one: no effect
    pmask[5, 3] = False
    return Q, qmask, P, pmask


@pytest.mark.parametrize("idx_base", [0, 100])
def test_reference_equals_the_naive_loop(idx_base):
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    Q, qmask, P, pmask = _hand_made_case()
    b = idx_base
    cand = torch.tensor([[b + 0, b + 0, -1, b + 1, b + 4, b + 5, b + 6],            # duplicates, -1, the page count itself
                         [b + 2, b + 3, b - 1, b + 5, b + 1, b + 4, b + 2],         # one below idx_base
                         [b + 0, b + 1, b + 4, b + 5, b + 3, 10 ** 6, b + 2],       # the query without a valid token
                         [b + 5, b + 4, b + 3, b + 2, b + 1, b + 0, b + 7]], dtype=torch.int32)
    sim, patch, heat = ops.align_reference(Q, qmask, P, pmask, cand, idx_base=b, heat=True)
    assert sim.dtype == torch.float32 and patch.dtype == torch.int32 and heat.dtype == torch.float32
    ws, wp, wh = naive_align(Q, qmask.numpy(), P, pmask.numpy(), cand.numpy(), b)
    np.testing.assert_array_equal(sim.numpy(), ws)
    np.testing.assert_array_equal(patch.numpy(), wp)
    np.testing.assert_array_equal(heat.numpy(), wh)
    two = ops.align_reference(Q, qmask, P, pmask, cand, idx_base=b)
    assert len(two) == 2 and torch.equal(two[1], patch)
    # the hand-made content, spelled out
    assert set(patch[0, 0].tolist()) <= {-1, 0, 1, 2, 3, 4, 5, 7} and patch[0, 0, 3] == -1 and sim[0, 0, 3] == 0     # never 6 or 8
    assert torch.equal(patch[0, 0], patch[0, 1]) and torch.equal(sim[0, 0], sim[0, 1])
    assert (sim[0, 2] == NINF).all() and (patch[0, 2] == -1).all() and (heat[0, 2] == NINF).all()                      # hole
    assert (sim[0, 3] == 0).all() and (patch[0, 3] == -1).all() and (heat[0, 3] == NINF).all()                         # all-masked page
    assert torch.isnan(sim[0, 4][qmask[0]]).all() and sim[0, 4, 3] == 0 and (patch[0, 4] == -1).all() and torch.isnan(heat[0, 4]).all()
    assert torch.isfinite(sim[0, 5]).all() and heat[0, 5, 3] == NINF                                                   # NaN under the mask
    assert (sim[2, 0] == 0).all() and (patch[2] == -1).all() and (heat[2, 0] == NINF).all()                            # no valid token
    assert (sim[1, 2] == NINF).all() and (sim[2, 5] == NINF).all() and (sim[3, 6] == NINF).all() and (sim[0, 6] == NINF).all()


def test_reference_fill_when_every_valid_product_is_below_the_masked_fill():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    Q = torch.zeros(1, 2, 8)
    Q[0, :, 0] = 120.0
    P = torch.zeros(1, 4, 8)
    P[0, :, 0] = -120.0
    pmask = torch.tensor([[True, True, False, True]])
    sim, patch, heat = ops.align_reference(Q, None, P, pmask, torch.zeros(1, 1, dtype=torch.int32), heat=True)
    assert (sim == -1e4).all() and (patch == 2).all()                    # the first masked patch attains the maximum
    assert heat[0, 0].tolist() == [-14400.0, -14400.0, NINF, -14400.0]


def test_hard_patch_is_the_first_maximum_of_the_heat_map():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    g = torch.Generator().manual_seed(5)
    nq, lq, npg, lp, d = 6, 7, 9, 21, 32
    Q = torch.nn.functional.normalize(torch.randn(nq, lq, d, generator=g), dim=-1)
    P = torch.nn.functional.normalize(torch.randn(npg, lp, d, generator=g), dim=-1)
    qmask = torch.rand(nq, lq, generator=g) > 0.2
    qmask[3] = False
    pmask = torch.rand(npg, lp, generator=g) > 0.3
    pmask[4] = False
    P[6, 2, 0] = float("nan")
    pmask[6, 2] = True
    cand = torch.randint(-1, npg + 1, (nq, 8), generator=g, dtype=torch.int32)
    sim, patch, heat = ops.align_reference(Q, qmask, P, pmask, cand, heat=True)
    got = ops.hard_patch(sim, patch)
    assert got.dtype == torch.int32 and tuple(got.shape) == (nq, 8)
    real = torch.isfinite(heat).any(-1)
    want = torch.where(real, torch.nan_to_num(heat, nan=NINF).argmax(-1), torch.full((nq, 8), -1)).to(torch.int32)
    assert torch.equal(got, want)
    assert (got[3] == -1).all() and (got[cand == 4] == -1).all() and (got[cand == 6] == -1).all() and (got[cand == -1] == -1).all()
    assert (got >= 0).sum() > 20                                         # most pairs are real


def test_hard_patch_equals_the_reference_loop_of_select_hard_tokens():
    """tests/v3_patterns.select_hard_tokens picks Ptn[di][argmax(sim.max(0))] per (query, hard page): with distinct pages per list the
    rows it returns are the rows `hard_patch` names."""
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    g = torch.Generator().manual_seed(3)
    nq, lq, npg, lp, d = 5, 6, 12, 33, 128
    Q = torch.nn.functional.normalize(torch.randn(nq, lq, d, generator=g), dim=-1)
    P = torch.nn.functional.normalize(torch.randn(npg, lp, d, generator=g), dim=-1)
    qmask = torch.rand(nq, lq, generator=g) > 0.25
    qmask[:, 0] = True
    pmask = torch.rand(npg, lp, generator=g) > 0.3
    pmask[:, 1] = True
    # the same selection inputs for both sides: any two score blocks give some aux lists
    sc_t, sc_s = torch.randn(nq, npg, generator=g), torch.randn(nq, npg, generator=g)
    k, aux_docs = 6, 3
    rows = V.select_hard_tokens(sc_t, sc_s, Q, qmask, P, pmask, k, aux_docs)                  # (nq * aux_docs, 1, d), l2-normalised
    rank_t = torch.argsort(torch.argsort(sc_t, dim=-1, descending=True), dim=-1)
    rank_s = torch.argsort(torch.argsort(sc_s, dim=-1, descending=True), dim=-1)
    top_i = torch.topk(sc_t, k=k, dim=-1).indices
    aux = top_i.gather(1, torch.topk((rank_t.float() - rank_s.float()).gather(1, top_i).abs(), k=aux_docs, dim=1).indices)
    hp = ops.hard_patch(*ops.align_reference(Q, qmask, P, pmask, aux.to(torch.int32)))
    picked = P[aux.flatten(), hp.flatten().long()]
    picked = (picked / (picked.norm(dim=-1, keepdim=True) + 1e-12)).view(-1, 1, d)
    np.testing.assert_allclose(picked.numpy(), rows.numpy(), atol=1e-6)


def test_hard_patch_exact_ties_go_to_the_lowest_patch():
    import evdr_amd  # noqa: F401
    from evdr_amd import ops
    sim = torch.tensor([[[0.5, 0.9, 0.9, 0.2], [0.9, 0.9, 0.9, 0.0], [NINF, NINF, NINF, NINF], [0.0, 0.0, 0.0, 0.0]]])
    patch = torch.tensor([[[4, 7, 3, 1], [9, -1, 2, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]]], dtype=torch.int32)
    assert ops.hard_patch(sim, patch).tolist() == [[3, 2, -1, -1]]
    # the same through the reference: identical patch rows and identical query tokens
    Q = torch.zeros(1, 3, 4)
    Q[0, :, 0] = 1.0
    P = torch.zeros(1, 6, 4)
    P[0, [1, 4, 5], 0] = 0.75
    s, p_, h = ops.align_reference(Q, None, P, None, torch.zeros(1, 1, dtype=torch.int32), heat=True)
    assert (p_ == 1).all() and ops.hard_patch(s, p_).tolist() == [[1]] and int(h[0, 0].argmax()) == 1


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound(lib):
    from evdr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evdr.h")).read(), flags=re.S)
    assert re.search(r"EVDR_API\s+int\s+evdr_maxsim_align\s*\(", header)
    assert hasattr(lib, "evdr_maxsim_align") and "evdr_maxsim_align" in _lib.SIGNATURES
    assert lib.evdr_version() == 303


def test_align_argument_errors_need_no_gpu(lib):
    from evdr_amd import _lib as L

    def align(nq=4, lq=8, np_=64, lp=40, nplanes=1, r=16, ptr=16, cand=16, sim=16, patch=16, heat=None, p_stride=None):
        # pointers are fake: nothing is dereferenced on the host
        return lib.evdr_maxsim_align(ptr, ptr, None, ptr, ptr, cand, r, 0, sim, patch, heat, nq, lq, np_, lp, nplanes,
                                     lp * 128 if p_stride is None else p_stride, np_ * lp * 128, None, None, None)
    assert align(lq=0) == L.EVDR_ERR_SHAPE and b"lq" in lib.evdr_last_error()
    assert align(lq=33) == L.EVDR_ERR_SHAPE and b"lq" in lib.evdr_last_error()
    assert align(r=0) == L.EVDR_ERR_ARG and b"r=0" in lib.evdr_last_error()
    assert align(r=L.EVDR_SELECT_MAX + 1) == L.EVDR_ERR_ARG and b"r=4097" in lib.evdr_last_error()
    assert align(nplanes=4) == L.EVDR_ERR_SHAPE and b"256" in lib.evdr_last_error()
    assert align(nplanes=3) == L.EVDR_ERR_ARG
    assert align(nq=-1) == L.EVDR_ERR_ARG and align(np_=-1) == L.EVDR_ERR_ARG and align(lp=-1) == L.EVDR_ERR_ARG
    assert align(lq=-1) == L.EVDR_ERR_ARG and align(r=-1) == L.EVDR_ERR_ARG
    assert align(sim=None) == L.EVDR_ERR_ARG and align(patch=None) == L.EVDR_ERR_ARG and align(cand=None) == L.EVDR_ERR_ARG
    assert align(ptr=None) == L.EVDR_ERR_ARG
    assert align(p_stride=39 * 128) == L.EVDR_ERR_ARG and align(p_stride=40 * 128 + 4) == L.EVDR_ERR_ARG
    assert align(ptr=8) == L.EVDR_ERR_ARG and b"aligned" in lib.evdr_last_error()
    assert align(lp=0) == L.EVDR_ERR_SHAPE
    assert align(nq=0) == L.EVDR_OK
    assert align(nq=0, ptr=None, cand=None, sim=None, patch=None) == L.EVDR_OK


def _corpus(kind, np_=8, lp=40, idx_base=0):
    """A PageCorpus over host tensors: the argument checks of an alignment call come before any device work."""
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
    from evdr_amd import ops
    Q = torch.zeros(3, 8, 128, dtype=torch.bfloat16)
    cand = torch.zeros(3, 16, dtype=torch.int32)
    for call in (lambda c, q, l: c.align(q, None, l), lambda c, q, l: c.align(q, None, l, heat=True),
                 lambda c, q, l: c.hard_patches(q, None, l)):
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
        with pytest.raises(RuntimeError, match="GPU only"):               # well-formed arguments: there is no CPU path
            call(_corpus("bf16"), Q, cand)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.maxsim_align(torch.zeros(1, 3, 8, 128, dtype=torch.bfloat16), None, torch.zeros(1, 8, 40, 128, dtype=torch.bfloat16), None,
                         None, torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), cand)


# ---- the kernel's listing ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not available")
def test_alignment_kernels_use_no_scratch_and_spill_nothing():
    from evdr_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        lst = os.path.join(tmp, "align.s")
        cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + B.FLAGS + ["--cuda-device-only", "-S", os.path.join(CSRC, "align.hip"), "-o", lst]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(lst).read()
    meta, cur = {}, {}
    for ln in text.splitlines():
        m = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", ln)
        if m:
            cur[m.group(1)] = m.group(2)
            if len(cur) == 4:
                meta[cur["name"]] = {k: int(v) for k, v in cur.items() if k != "name"}
                cur = {}
    kernels = {k: v for k, v in meta.items() if "align_kernel" in k}
    assert len(kernels) == 2 and len(meta) == 2, sorted(meta)             # the bf16 and the fp16 hi/lo instance, and nothing else
    for name, m in kernels.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert "v_mfma_f32_16x16x32_bf16" in text and "v_mfma_f32_16x16x32_f16" in text
    assert "global_atomic" not in text and "flat_atomic" not in text
