"""The fused pairwise ranking losses on the GPU (csrc/pairloss.hip): both kernels against the float64 statements of their
rules over the tile / wave-quarter edges and the input kinds that stress the range handling, determinism, the autograd plumbing behind
`criterion.enable_fused_pair_losses()`, the O(B * N) memory bound, the reference's own training steps with the switch on, and the limits.

Gates (from the rule and the number formats, not from what the kernels give):
  loss, both losses: rtol 1e-5 -- the project's gate for these losses (tests/test_host_logic.py, tests/test_v3_patterns.py).
  RankNet gradient:  |g - g64| <= 1e-5 G + 1e-4 |g64| with G = 2 / (B N), the largest gradient the rule can produce (N pair terms, each
                     within [-1, 1], times 2 / (B N^2)): a few ulps per term over N terms stay below 1e-6 G, a dropped or doubled tile
                     of 64 terms does not.
  LambdaLoss gradient: atol 1e-5 max|g64|, rtol 1e-4."""
import math

import numpy as np
import pytest
import torch

import golden_recipes as R
import pair_loss_cases as PC
import v3_patterns as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# tile (64 i per workgroup), wave quarters (ceil(N / 4) j per wave: N = 3 leaves a wave idle, 5 and 129 make ragged quarters) and
# multi-workgroup rows; B = 33 puts more rows than one in flight per tile column
SHAPES = [(b, n) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000) for b in (1, 3, 33)] + [(3, 3), (3, 5), (3, 129)]
ALPHA, EPS = 1.3, 1e-6
_CACHE = {}


@pytest.fixture(scope="module")
def mods():
    import evdr_amd  # noqa: F401
    from evdr_amd import criterion, ops
    return criterion, ops


def case(ops, kind, b, n):
    """Inputs on the device and the float64 statements, computed once per (kind, shape) and shared read-only."""
    key = (kind, b, n)
    if key not in _CACHE:
        s, t = (x.to(DEV) for x in PC.scores("normal" if kind == "ties" else kind, b, n))
        s_sorted, gain, disc, order = PC.lambda_inputs(s, t)
        if kind == "ties":                              # (f): equal adjacent gains -- those pairs have weight 0
            gain = gain.clone()
            gain[:, 1::2] = gain[:, 0:gain.shape[1] - gain.shape[1] % 2:2]
        _CACHE[key] = dict(s=s, t=t, s_sorted=s_sorted, gain=gain, disc=disc, order=order,
                           pw=ops.pairwise_distill_reference(s, t) if kind != "ties" else None,
                           lam=ops.lambda_reference(s_sorted, gain, disc, ALPHA, EPS))
    return _CACHE[key]


def ranknet_excess(g, g64, b, n):
    """max over entries of |g - g64| - 1e-4 |g64|, in units of G = 2 / (B N): the gate is 1e-5."""
    return float(((g.double() - g64).abs() - 1e-4 * g64.abs()).max()) / (2.0 / (b * n))


def lambda_excess(g, g64):
    """max over entries of |g - g64| - 1e-4 |g64|, in units of max|g64| (0 where the rule's gradient is all zero and so is g)."""
    scale = float(g64.abs().max())
    worst = float(((g.double() - g64).abs() - 1e-4 * g64.abs()).max())
    return worst / scale if scale > 0 else (0.0 if worst <= 0 else math.inf)


@pytest.mark.parametrize("kind", PC.KINDS)
def test_ranknet_kernel_matches_the_float64_rule(mods, kind):
    _crit, ops = mods
    worst = {"loss_rel": 0.0, "grad_excess_over_G": -math.inf}
    for b, n in SHAPES:
        c = case(ops, kind, b, n)
        loss, grad = ops.pairwise_distill(c["s"], c["t"])
        l64, g64 = c["pw"]
        rel = abs(float(loss) - float(l64)) / abs(float(l64))
        exc = ranknet_excess(grad, g64, b, n)
        worst = {"loss_rel": max(worst["loss_rel"], rel), "grad_excess_over_G": max(worst["grad_excess_over_G"], exc)}
        assert rel <= 1e-5, (kind, b, n, float(loss), float(l64))
        assert exc <= 1e-5, (kind, b, n, exc)
        G = 2.0 / (b * n)
        if kind == "constant":
            np.testing.assert_allclose(float(loss), math.log(2.0), rtol=1e-6, err_msg=f"{b}x{n}")
            assert float(grad.abs().max()) <= 1e-5 * G, (b, n)
        if kind == "same":
            assert float(grad.abs().max()) <= 1e-5 * G, (b, n, float(grad.abs().max()) / G)
    print(f"ranknet {kind}: {worst}")


@pytest.mark.parametrize("kind", PC.KINDS + ("ties",))
def test_lambda_kernel_matches_the_float64_rule(mods, kind):
    _crit, ops = mods
    worst = {"loss_rel": 0.0, "grad_excess_over_max": -math.inf}
    for b, n in SHAPES:
        c = case(ops, kind, b, n)
        loss, grad = ops.lambda_pairs(c["s_sorted"], c["gain"], c["disc"], ALPHA, EPS)
        l64, g64 = c["lam"]
        np.testing.assert_allclose(float(loss), float(l64), rtol=1e-5, atol=0, err_msg=f"{kind} {b}x{n}")
        exc = lambda_excess(grad, g64)
        assert exc <= 1e-5, (kind, b, n, exc)
        if float(l64) != 0.0:
            worst["loss_rel"] = max(worst["loss_rel"], abs(float(loss) - float(l64)) / abs(float(l64)))
        worst["grad_excess_over_max"] = max(worst["grad_excess_over_max"], exc)
        if kind == "constant" or n == 1:                 # no gain differs: every weight is 0
            assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    print(f"lambda {kind}: {worst}")


@pytest.mark.parametrize("kind,b,n", [("normal", 3, 257), ("fill", 33, 1000), ("wide", 5, 65)])
def test_same_bits_every_launch_and_under_row_permutation(mods, kind, b, n):
    _crit, ops = mods
    c = case(ops, kind, b, n)
    perm = torch.randperm(b, generator=torch.Generator().manual_seed(b)).to(DEV)
    ws = ops.pair_loss_workspace(b, n, DEV)                  # one workspace for all launches: every launch leaves the ticket at zero
    rows_of = lambda x, rows: x if rows is None else x[rows].contiguous()
    runs = {"ranknet": lambda rows=None, **k: ops.pairwise_distill(rows_of(c["s"], rows), rows_of(c["t"], rows), **k),
            "lambda": lambda rows=None, **k: ops.lambda_pairs(rows_of(c["s_sorted"], rows), rows_of(c["gain"], rows), c["disc"], ALPHA, EPS, **k)}
    for tag, run in runs.items():
        l0, g0 = run(ws=ws)
        l1, g1 = run(ws=ws)
        assert torch.equal(l0, l1) and torch.equal(g0, g1), tag
        l2, none = run(ws=ws, want_grad=False)
        assert none is None and torch.equal(l0, l2), tag
        l3, g3 = run()                                       # a fresh workspace gives the same bits
        assert torch.equal(l0, l3) and torch.equal(g0, g3), tag
        _lp, gp = run(perm, ws=ws)
        assert torch.equal(gp, g0[perm]), tag
    assert int(ws.view(torch.int32)[-64:].abs().sum()) == 0                       # ticket back at zero


def _grads(fn, s, t):
    sg = s.clone().requires_grad_(True)
    loss = fn(sg, t)
    loss.backward()
    return loss.detach(), sg.grad


def test_autograd_plumbing_agrees_with_the_switch_off_path(mods):
    """The loss lines of mainv2_iter_lipairwise.py and mainv2_iter_lambda.py with the switch on and off, on the same CUDA inputs: upstream
    scaling (0.5 x, 3 x), the scatter through the teacher's order, a non-contiguous student, and a double backward (which re-derives
    the step from the torch form)."""
    crit, _ops = mods
    b, n = 6, 48
    s, t = (x.to(DEV) for x in PC.scores("normal", b, n, seed=5))          # tie-free teacher: tie order belongs to torch.sort
    G = 2.0 / (b * n)
    lipair = lambda a, tt: 1.0 * crit.listwise_distillation_loss(a, tt, k=8, temperature=2.0) + 0.5 * crit.pairwise_distillation_loss(a, tt)
    pair_t = lambda a, tt: crit.pairwise_distillation_loss(a.t().contiguous().t(), tt) * 1.0          # a column-major student
    lam = lambda a, tt: 3.0 * crit.lambda_loss(a, tt, alpha=ALPHA, eps=EPS)

    def second_order(a, tt):
        (g,) = torch.autograd.grad(crit.pairwise_distillation_loss(a, tt) + crit.lambda_loss(a, tt), a, create_graph=True)
        return (g * g).sum()

    assert not crit.fused_pair_losses_enabled()
    off = {k: _grads(f, s, t) for k, f in (("lipair", lipair), ("pair_t", pair_t), ("lam", lam), ("second", second_order))}
    off_pair = _grads(crit.pairwise_distillation_loss, s, t)[1]
    crit.enable_fused_pair_losses()
    try:
        on = {k: _grads(f, s, t) for k, f in (("lipair", lipair), ("pair_t", pair_t), ("lam", lam), ("second", second_order))}
    finally:
        crit.disable_fused_pair_losses()
    for k in off:
        np.testing.assert_allclose(float(on[k][0]), float(off[k][0]), rtol=1e-5, err_msg=k)
    # lipairwise: the listwise part is the same torch code both ways; the pairwise part carries the RankNet gate, times its 0.5
    d = (on["lipair"][1] - off["lipair"][1]).abs()
    assert bool((d <= 0.5 * (1e-5 * G + 1e-4 * off_pair.abs()) + 1e-6 * off["lipair"][1].abs()).all()), float(d.max()) / G
    assert ranknet_excess(on["pair_t"][1], off["pair_t"][1].double(), b, n) <= 1e-5
    assert lambda_excess(on["lam"][1], off["lam"][1].double()) <= 1e-5
    np.testing.assert_allclose(on["second"][1].cpu().numpy(), off["second"][1].cpu().numpy(), rtol=1e-4,
                               atol=1e-5 * float(off["second"][1].abs().max()))


@pytest.mark.parametrize("which", ["ranknet", "lambda"])
def test_memory_stays_linear_in_the_row_length(mods, which):
    """B = 2, N = 4096, forward + backward with the switch on: at most 1 MiB + 64 B N bytes over the baseline (scores, sort outputs,
    gradients, workspace); ONE (B, N, N) fp32 intermediate of the torch form would be 134 MB."""
    crit, _ops = mods
    b, n = 2, 4096
    s, t = (x.to(DEV) for x in PC.scores("normal", b, n, seed=3))
    fn = crit.pairwise_distillation_loss if which == "ranknet" else crit.lambda_loss
    crit.enable_fused_pair_losses()
    try:
        sg = s.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = fn(sg, t)
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
    finally:
        crit.disable_fused_pair_losses()
    assert sg.grad is not None and bool(torch.isfinite(sg.grad).all()) and math.isfinite(float(loss.detach()))
    assert peak - base <= (1 << 20) + 64 * b * n, (peak - base, (1 << 20) + 64 * b * n)


def test_the_reference_steps_hold_with_the_switch_on(mods, golden, monkeypatch):
    """The lambda, lipairwise, pairscore and ranknet steps of the reference's scripts (tests/golden/make_golden_losses_steps.py) with the
    switch on, with the checks and tolerances of test_hip_path_reproduces_the_nine_loss_steps -- and the fused path was the one taken."""
    crit, ops = mods
    calls = {"pairwise": 0, "lambda": 0}
    real_pw, real_lam = ops.pairwise_distill, ops.lambda_pairs
    monkeypatch.setattr(ops, "pairwise_distill", lambda *a, **k: (calls.__setitem__("pairwise", calls["pairwise"] + 1), real_pw(*a, **k))[1])
    monkeypatch.setattr(ops, "lambda_pairs", lambda *a, **k: (calls.__setitem__("lambda", calls["lambda"] + 1), real_lam(*a, **k))[1])
    z = golden("v3_loss_steps")
    case_ = R.v3_case()
    be = V.hip_backend()
    grad_atol = 1e-6
    crit.enable_fused_pair_losses()
    try:
        steps = V.loss_steps(be)
        for tag in ("lambda", "lipairwise", "pairscore", "ranknet"):
            out = V.step_with_loss(be, case_, steps[tag])
            main_key = f"{tag}__total_loss" if f"{tag}__total_loss" in z.files else f"{tag}__loss"
            np.testing.assert_allclose(out["total_loss"], float(z[main_key]), rtol=1e-5, err_msg=tag)
            for k, v in out.items():
                if f"{tag}__{k}" in z.files and k not in ("total_loss",):
                    np.testing.assert_allclose(v, float(z[f"{tag}__{k}"]), rtol=1e-5, err_msg=f"{tag}:{k}")
            g = out["grad"].cpu().numpy()
            want = z[f"{tag}__grad_sample"]
            np.testing.assert_allclose(g[::2, ::2, ::2], want, atol=max(grad_atol, 5e-5 * float(np.abs(want).max())), rtol=1e-5, err_msg=tag)
            np.testing.assert_allclose(np.linalg.norm(g.astype(np.float64)), float(z[f"{tag}__grad_norm"]), rtol=1e-4, err_msg=tag)
            d = np.abs(out["param_after"].cpu().numpy()[::2, ::2, ::2] - z[f"{tag}__param_sample"])
            big = np.abs(want) > 1e-6 * max(1.0, float(np.abs(want).max()) / 1e-2)
            assert d[big].max() <= 2e-6 and d.max() < 2e-3, (tag, d[big].max(), d.max())
    finally:
        crit.disable_fused_pair_losses()
    assert calls == {"pairwise": 3, "lambda": 1}, calls


def test_refused_shapes_raise_before_any_launch(mods):
    _crit, ops = mods
    for b, n in ((ops.PAIR_MAX_B + 1, 1), (1, ops.PAIR_MAX_N + 1)):
        s = torch.zeros(b, n, device=DEV)
        with pytest.raises(RuntimeError, match="launch limits"):
            ops.pairwise_distill(s, s)
        with pytest.raises(RuntimeError, match="launch limits"):
            ops.lambda_pairs(s, s, torch.zeros(n, device=DEV), 1.0, 1e-6)
    s = torch.zeros(2, 8, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        ops.pairwise_distill(s.double(), s.double())
    with pytest.raises(RuntimeError, match="B >= 1 and N >= 1"):
        ops.pairwise_distill(s[:0], s[:0])
    with pytest.raises(RuntimeError, match="pair_loss_workspace"):
        ops.pairwise_distill(s, s, ws=torch.zeros(8, dtype=torch.uint8, device=DEV))
