"""Counterpart of the reference's criterion.py for the north-star loss.

`infonce_distillation_loss` keeps the reference signature (criterion.py:56-68) and runs loss + gradient in
one HIP kernel (evdr_infonce_distill_fwd_bwd): d loss/d score_s = (softmax(s/τ) - onehot(argmax t)) / (τ B),
which feeds the MaxSim backward directly."""
import torch

from . import ops


# Workspaces of the one-launch loss kernel (row losses + the ticket word the last workgroup resets), one per (device, stream, batch
# size): launches on one stream are ordered, so a workspace never serves two launches at once; the reference drives this from a
# single Python thread on one stream (SURVEY §8(b) "Threading / streams").  Inside a stream capture the stateless two-launch form is
# used instead (same bits: a captured graph must not share a ticket word with eager launches).
_LOSS_WS = {}


def _loss_workspace(score_s):
    if not score_s.is_cuda or torch.cuda.is_current_stream_capturing():
        return None
    dev = score_s.device
    key = (dev.index, ops.L.current_stream_handle(dev), int(score_s.shape[0]))
    ws = _LOSS_WS.get(key)
    if ws is None:
        if len(_LOSS_WS) > 16:
            _LOSS_WS.clear()
        ws = _LOSS_WS[key] = ops.infonce_workspace(score_s.shape[0], dev)
    return ws


class _InfoNCEDistill(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score_s, score_t, temperature):
        loss, grad = ops.infonce_distill(score_s, score_t, temperature, want_grad=ctx.needs_input_grad[0],
                                         ws=_loss_workspace(score_s) if score_s.dim() == 2 and score_s.shape[0] > 0 else None)
        if grad is not None:
            ctx.save_for_backward(grad)
            ctx.in_dtype = score_s.dtype
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return (grad * gout).to(ctx.in_dtype), None, None


def infonce_distillation_loss(score_s: torch.Tensor, score_t: torch.Tensor, temperature: float = 0.07) -> torch.Tensor:
    """CE(score_s / temperature, argmax_p score_t), mean over the batch; the teacher is not differentiated."""
    return _InfoNCEDistill.apply(score_s, score_t.detach(), float(temperature))


# ----------------------------------------------------------------------------------------------------
# The other losses of the reference's criterion.py: small (B, N) elementwise / pairwise math that consumes the
# MaxSim kernel's score matrices unchanged.  Plain torch on the scores' device
# (the two pairwise ones optionally fused, below); the gradient w.r.t. score_s then flows into the HIP MaxSim backward.  Signatures and defaults as in the
# reference; the teacher scores are never differentiated.
# ----------------------------------------------------------------------------------------------------
import torch.nn.functional as _F


def infonce_supervised_loss(score_s: torch.Tensor, labels: torch.Tensor, temperature: float = 0.07) -> torch.Tensor:
    """CE(score_s / τ, labels) with explicit top-1 labels (criterion.py:43-53)."""
    return _F.cross_entropy(score_s / temperature, labels)


def score_preserving_loss(score_s: torch.Tensor, score_t: torch.Tensor) -> torch.Tensor:
    """Mean squared error between student and (detached) teacher scores (criterion.py:74-83)."""
    return ((score_s - score_t.detach()) ** 2).mean()


# ---- opt-in fused pairwise ranking losses (csrc/pairloss.hip) -----------------------------------------------------
# `enable_fused_pair_losses()` once -- in the re-export shim of INTEGRATION.md §1 -- and `pairwise_distillation_loss` / `lambda_loss` of
# CUDA fp32 (B, N) student and teacher scores run loss + gradient in ONE HIP launch with O(B * N) memory, instead of broadcast torch expressions over several
# (B, N, N) fp32 tensors that autograd keeps for the backward.  Off (the default) both functions are the torch code below, to the bit;
# on, everything the kernels do not take (CPU tensors, other dtypes, empty shapes, a stream capture, a double backward) still is.
_FUSED_PAIR_LOSSES = False
_PAIR_WS = {}                # (device, stream, B, N) -> ops.pair_loss_workspace: keyed as _LOSS_WS is, for the same reason


def enable_fused_pair_losses() -> None:
    global _FUSED_PAIR_LOSSES
    _FUSED_PAIR_LOSSES = True


def disable_fused_pair_losses() -> None:
    global _FUSED_PAIR_LOSSES
    _FUSED_PAIR_LOSSES = False
    _PAIR_WS.clear()


def fused_pair_losses_enabled() -> bool:
    return _FUSED_PAIR_LOSSES


def _takes_fused_pair_path(score_s, score_t) -> bool:
    return (_FUSED_PAIR_LOSSES and isinstance(score_s, torch.Tensor) and score_s.is_cuda and score_s.dtype == torch.float32
            and score_s.dim() == 2 and score_s.shape[0] >= 1 and score_s.shape[1] >= 1 and isinstance(score_t, torch.Tensor)
            and score_t.device == score_s.device and score_t.shape == score_s.shape and score_t.dtype == torch.float32
            and not torch.cuda.is_current_stream_capturing())


def _pair_workspace(score_s):
    dev = score_s.device
    key = (dev.index, ops.L.current_stream_handle(dev), int(score_s.shape[0]), int(score_s.shape[1]))
    ws = _PAIR_WS.get(key)
    if ws is None:
        if len(_PAIR_WS) > 16:
            _PAIR_WS.clear()
        ws = _PAIR_WS[key] = ops.pair_loss_workspace(score_s.shape[0], score_s.shape[1], dev)
    return ws


def _double_backward(torch_loss, ctx, gout):
    """backward under create_graph=True: the saved gradient is a constant to autograd, so the step is re-derived from the torch form."""
    score_s, score_t = ctx.saved_tensors[:2]
    with torch.enable_grad():
        (g,) = torch.autograd.grad(torch_loss(score_s, score_t, *ctx.extra), score_s, create_graph=True)
    return g * gout


class _PairwiseDistill(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score_s, score_t):
        ss = score_s.contiguous()
        loss, grad = ops.pairwise_distill(ss, score_t.contiguous(), want_grad=ctx.needs_input_grad[0], ws=_pair_workspace(ss))
        ctx.extra = ()
        if grad is not None:
            ctx.save_for_backward(score_s, score_t, grad)
        return loss

    @staticmethod
    def backward(ctx, gout):
        if torch.is_grad_enabled():
            return _double_backward(_pairwise_distillation_torch, ctx, gout), None
        return ctx.saved_tensors[2] * gout, None


class _LambdaLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score_s, score_t, alpha, eps):
        n = score_s.shape[1]
        t_sorted, order = score_t.sort(dim=1, descending=True)
        s_sorted = score_s.gather(1, order)
        disc = 1.0 / torch.log2(torch.arange(1, n + 1, device=score_s.device, dtype=torch.float) + 1.0)
        gain = torch.sigmoid(t_sorted)
        loss, grad_sorted = ops.lambda_pairs(s_sorted, gain.contiguous(), disc, alpha, eps, want_grad=ctx.needs_input_grad[0],
                                             ws=_pair_workspace(s_sorted))
        ctx.extra = (alpha, eps)
        if grad_sorted is not None:
            ctx.save_for_backward(score_s, score_t, torch.empty_like(grad_sorted).scatter_(1, order, grad_sorted))
        return loss

    @staticmethod
    def backward(ctx, gout):
        if torch.is_grad_enabled():
            return _double_backward(_lambda_torch, ctx, gout), None, None, None
        return ctx.saved_tensors[2] * gout, None, None, None


def pairwise_distillation_loss(score_s: torch.Tensor, score_t: torch.Tensor) -> torch.Tensor:
    """RankNet-style: for every ordered page pair (i, j) the student's margin s_i - s_j is a logit whose soft
    target is sigmoid(t_i - t_j); mean BCE over all B*N*N pairs (criterion.py:89-108).  With `enable_fused_pair_losses()` CUDA fp32
    scores take the one-launch HIP kernel."""
    if _takes_fused_pair_path(score_s, score_t):
        return _PairwiseDistill.apply(score_s, score_t.detach())
    return _pairwise_distillation_torch(score_s, score_t)


def _pairwise_distillation_torch(score_s, score_t):
    t = score_t.detach()
    margin_s = score_s[:, :, None] - score_s[:, None, :]
    target = torch.sigmoid(t[:, :, None] - t[:, None, :])
    return _F.binary_cross_entropy_with_logits(margin_s, target)


def listwise_distillation_loss(score_s: torch.Tensor, score_t: torch.Tensor, k: int = 10,
                               temperature: float = 1.0) -> torch.Tensor:
    """Partial cross-entropy over the teacher's top-k pages, scaled by τ² (criterion.py:114-142)."""
    logp_s = torch.log_softmax(score_s / temperature, dim=1)
    p_t = torch.softmax(score_t.detach() / temperature, dim=1)
    top_p, top_i = p_t.topk(k, dim=1)
    return -(top_p * logp_s.gather(1, top_i)).sum(dim=1).mean() * (temperature ** 2)


def lambda_loss(score_s: torch.Tensor, score_t: torch.Tensor, alpha: float = 1.0, eps: float = 1e-6) -> torch.Tensor:
    """LambdaLoss-style pairwise logistic loss in the teacher's ranking order, weighted by
    10 * |Δgain| * |Δdiscount| over the upper-triangular pairs (criterion.py:148-189).  With `enable_fused_pair_losses()` CUDA fp32
    scores keep the sort, gain and discount in torch (O(B * N)) and take the one-launch HIP kernel for the pairs."""
    if _takes_fused_pair_path(score_s, score_t):
        return _LambdaLoss.apply(score_s, score_t.detach(), float(alpha), float(eps))
    return _lambda_torch(score_s, score_t, alpha, eps)


def _lambda_torch(score_s, score_t, alpha, eps):
    t = score_t.detach()
    n = score_s.shape[1]
    t_sorted, order = t.sort(dim=1, descending=True)
    s_sorted = score_s.gather(1, order)
    disc = 1.0 / torch.log2(torch.arange(1, n + 1, device=score_s.device, dtype=torch.float) + 1.0)
    d_disc = (disc[None, :, None] - disc[None, None, :]).abs()
    gain = torch.sigmoid(t_sorted)
    d_gain = (gain[:, :, None] - gain[:, None, :]).abs()
    weight = d_gain * d_disc * 10.0
    pair = -_F.logsigmoid(alpha * (s_sorted[:, :, None] - s_sorted[:, None, :]))
    upper = torch.triu(torch.ones(n, n, device=score_s.device), diagonal=1)
    return (weight * pair * upper).sum() / (upper.sum() + eps)


def ranknce_loss(score_s: torch.Tensor, score_t: torch.Tensor, temperature: float = 1.0,
                 lambda_weight: float = 1.0) -> torch.Tensor:
    """InfoNCE against the teacher's top-1 (position 0 after sorting by the teacher) plus a softplus penalty on
    adjacent student margins weighted by sigmoid of the teacher's adjacent margins (criterion.py:192-226)."""
    t = score_t.detach()
    t_sorted, order = t.sort(dim=1, descending=True)
    s_sorted = score_s.gather(1, order)
    labels = torch.zeros(score_s.shape[0], dtype=torch.long, device=score_s.device)
    nce = _F.cross_entropy(s_sorted / temperature, labels)
    ds = s_sorted[:, :-1] - s_sorted[:, 1:]
    dt = t_sorted[:, :-1] - t_sorted[:, 1:]
    rank = (torch.sigmoid(dt) * _F.softplus(-ds)).mean()
    return nce + lambda_weight * rank
