"""The fused pairwise ranking losses, host side (no GPU): the float64 statements of the two rules (ops.pairwise_distill_reference,
ops.lambda_reference) against the reference's fixtures and against today's criterion functions, the opt-in switch on tensors the kernels
do not take, and the argument checks of the three C entry points."""
import ctypes

import numpy as np
import pytest
import torch

import golden_recipes as R
import pair_loss_cases as PC


@pytest.fixture(scope="module")
def mods():
    import evdr_amd  # noqa: F401
    from evdr_amd import criterion, ops
    return criterion, ops


def _lambda_reference_full(ops, s, t, alpha=1.0, eps=1e-6):
    """lambda_reference behind lambda_loss's own sort / gain / discount, gradient scattered back through the order."""
    s_sorted, gain, disc, order = PC.lambda_inputs(s, t)
    loss, g_sorted = ops.lambda_reference(s_sorted, gain, disc, alpha, eps)
    return loss, torch.zeros_like(g_sorted).scatter_(1, order, g_sorted)


def test_reference_statements_reproduce_the_fixtures(mods, golden):
    """On the inputs of the reference's own criterion run (tests/golden/losses.npz): loss and gradient of both losses, with the tolerances of
    test_secondary_losses_match_reference."""
    _crit, ops = mods
    z = golden("losses")
    ss, st, _labels = R.losses_case()
    for name, (loss, grad) in {"pairwise_distillation_loss": ops.pairwise_distill_reference(ss, st),
                               "lambda_loss": _lambda_reference_full(ops, ss, st)}.items():
        assert loss.dtype == torch.float64 and grad.dtype == torch.float64 and tuple(grad.shape) == tuple(ss.shape)
        np.testing.assert_allclose(loss.item(), float(z[name]), rtol=1e-5, err_msg=name)
        np.testing.assert_allclose(grad.numpy(), z[name + "_grad"], atol=1e-6, rtol=1e-4, err_msg=name)


def _f64_cases():
    out = []
    for b, n in ((6, 16), (3, 257)):
        s, t = PC.scores("normal", b, n, seed=1)
        out.append((f"{b}x{n}", s, t))
    s, t = PC.scores("normal", 2, 300, seed=1)
    s[:, 17] = PC.FILL
    s[:, 211] = PC.FILL          # two fill columns of one row meet in a pair
    t[:, 17] = PC.FILL
    t[:, 90] = PC.FILL
    s[1] = t[1]                  # a row with s == t
    out.append(("2x300 fill", s, t))
    return out


@pytest.mark.parametrize("chunk", [128, 7])
def test_reference_statements_equal_todays_functions_in_float64(mods, chunk):
    """float64 autograd of today's criterion functions == the closed forms.  RankNet: both sides are float64 throughout and agree to
    rounding.  lambda_loss keeps two fp32 pieces when it is handed float64 scores: the discount table and its pairwise differences
    (`disc` is built with dtype=torch.float, so every |disc_i - disc_j| is rounded to fp32: up to 2^-24 = 6e-8 relative per weight) and
    the denominator (`upper.sum() + eps` is an fp32 tensor: 8e-9 relative at N = 16).  The rule takes the fp32 table and subtracts
    exactly, so loss and gradient agree to 1e-7 relative, a gradient entry (a signed sum of such terms) to 1e-7 of the largest entry."""
    crit, ops = mods
    assert not crit.fused_pair_losses_enabled()
    for tag, s, t in _f64_cases():
        s64, t64 = s.double(), t.double()
        sg = s64.clone().requires_grad_(True)
        want = crit.pairwise_distillation_loss(sg, t64)
        want.backward()
        loss, grad = ops.pairwise_distill_reference(s64, t64, row_chunk=chunk)
        np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-12, err_msg=tag)
        np.testing.assert_allclose(grad.numpy(), sg.grad.numpy(), rtol=1e-9, atol=1e-16, err_msg=tag)
        sg = s64.clone().requires_grad_(True)
        want = crit.lambda_loss(sg, t64, alpha=1.3, eps=1e-6)
        want.backward()
        s_sorted, gain, disc, order = PC.lambda_inputs(s64, t64)
        loss, g_sorted = ops.lambda_reference(s_sorted, gain, disc, 1.3, 1e-6, row_chunk=chunk)
        grad = torch.zeros_like(g_sorted).scatter_(1, order, g_sorted)
        np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-7, err_msg=tag)
        np.testing.assert_allclose(grad.numpy(), sg.grad.numpy(), rtol=1e-7, atol=1e-7 * sg.grad.abs().max().item(), err_msg=tag)


def test_todays_fp32_functions_sit_on_the_float64_rule(mods):
    """The inputs are sound: fp32 torch on the CPU is within 1e-6 relative of the float64 rule on these shapes, the -1e4 case included."""
    crit, ops = mods
    for tag, s, t in _f64_cases():
        np.testing.assert_allclose(crit.pairwise_distillation_loss(s, t).item(), ops.pairwise_distill_reference(s, t)[0].item(), rtol=1e-6, err_msg=tag)
        np.testing.assert_allclose(crit.lambda_loss(s, t).item(), _lambda_reference_full(ops, s, t)[0].item(), rtol=1e-6, err_msg=tag)


def test_switch_is_off_on_import_and_leaves_cpu_tensors_alone(mods):
    crit, _ops = mods
    assert crit.fused_pair_losses_enabled() is False

    def run(s, t):
        out = []
        for fn in (crit.pairwise_distillation_loss, lambda a, b: crit.lambda_loss(a, b, alpha=0.7, eps=1e-6)):
            sg = s.clone().requires_grad_(True)
            v = fn(sg, t)
            v.backward()
            out += [v.detach(), sg.grad]
        return out

    s, t = PC.scores("fill", 3, 40, seed=2)
    inputs = [(s, t), (s.double(), t.double()), (s[:, :0], t[:, :0]), (s[:0], t[:0])]
    off = [run(a, b) for a, b in inputs]
    crit.enable_fused_pair_losses()
    try:
        assert crit.fused_pair_losses_enabled() is True
        on = [run(a, b) for a, b in inputs]
    finally:
        crit.disable_fused_pair_losses()
    assert crit.fused_pair_losses_enabled() is False
    for x, y in zip(off, on):
        for a, b in zip(x, y):
            assert a.dtype == b.dtype and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0))      # empty shapes give NaN both ways


def test_argument_errors_need_no_gpu():
    """Status codes before anything touches the device (pointers are fake: nothing is dereferenced on the host)."""
    import evdr_amd  # noqa: F401
    from evdr_amd import build, _lib as L
    build.build(verbose=False)
    lib = L.load()
    b, n = 4, 100
    need = lib.evdr_pair_loss_workspace(b, n)
    assert need >= b * 2 * 8 + 4 and need < 4096                     # a partial per (row, 64-column tile) and the ticket; nothing N x N
    big = lib.evdr_pair_loss_workspace(1024, 65535)
    assert 1024 * 1024 * 8 < big < 1024 * 65535                       # the largest shape the issue names is admitted, O(B N / 64)
    assert lib.evdr_pair_loss_workspace(0, 5) == 0 and lib.evdr_pair_loss_workspace(5, 0) == 0
    assert lib.evdr_pair_loss_workspace(65536, 5) == 0 and lib.evdr_pair_loss_workspace(5, (1 << 20) + 1) == 0
    P = 4096                                                          # a fake, 8-byte aligned address
    f = ctypes.c_float

    def pw(ss=P, st=P, b=b, n=n, loss=P, grad=None, ws=P, nbytes=need):
        return lib.evdr_pairwise_distill_fwd_bwd(ss, st, b, n, loss, grad, ws, nbytes, None)

    def lam(ss=P, gain=P, disc=P, b=b, n=n, loss=P, grad=None, ws=P, nbytes=need):
        return lib.evdr_lambda_pairs_fwd_bwd(ss, gain, disc, b, n, f(1.0), f(1e-6), loss, grad, ws, nbytes, None)

    for call in (pw, lam):
        assert call(ss=None) == L.EVDR_ERR_ARG and b"null" in lib.evdr_last_error()
        assert call(loss=None) == L.EVDR_ERR_ARG
        assert call(ws=None) == L.EVDR_ERR_ARG
        assert call(b=0) == L.EVDR_ERR_ARG and call(n=0) == L.EVDR_ERR_ARG and call(b=-1) == L.EVDR_ERR_ARG
        assert call(ws=P + 4) == L.EVDR_ERR_ARG and b"aligned" in lib.evdr_last_error()
        assert call(b=65536, nbytes=1 << 40) == L.EVDR_ERR_SHAPE and b"limits" in lib.evdr_last_error()
        assert call(n=(1 << 20) + 1, nbytes=1 << 40) == L.EVDR_ERR_SHAPE
        assert call(nbytes=need - 1) == L.EVDR_ERR_WORKSPACE and b"too small" in lib.evdr_last_error()
    assert pw(st=None) == L.EVDR_ERR_ARG
    assert lam(gain=None) == L.EVDR_ERR_ARG and lam(disc=None) == L.EVDR_ERR_ARG


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes(mods):
    _crit, ops = mods
    s, t = PC.scores("normal", 2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pairwise_distill(s, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lambda_pairs(*PC.lambda_inputs(s, t)[:3], 1.0, 1e-6)
    for bad_b, bad_n in ((0, 4), (4, 0), (ops.PAIR_MAX_B + 1, 4), (4, ops.PAIR_MAX_N + 1)):
        with pytest.raises(RuntimeError, match="pair_loss_workspace"):
            ops.pair_loss_workspace(bad_b, bad_n, "cpu")


def test_pair_kernels_use_no_scratch():
    """scratch/kres.py over csrc/pairloss.hip: both kernels compile for gfx950 without scratch memory and without VGPR spills (the
    per-lane gradient and fp64 loss partials stay in registers through the unrolled pair loop)."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scratch", "kres.py"), "pairloss.hip"], capture_output=True, text=True,
                       timeout=600, cwd=root)
    rows = [ln for ln in r.stdout.splitlines() if re.match(r"(pairwise_distill|lambda_pairs)_kernel\(", ln)]
    assert r.returncode == 0 and len(rows) == 2, (r.stdout[-1500:], r.stderr[-500:])
    for ln in rows:
        m = re.search(r"VGPR\s+(\d+) AGPR\s+(\d+) spill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", ln)
        assert m and int(m.group(3)) == 0 and int(m.group(4)) == 0 and int(m.group(5)) == 0, ln
