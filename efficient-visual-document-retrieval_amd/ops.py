"""Thin torch-tensor wrappers over the C ABI (include/evdr.h).  PyTorch is plumbing here: it owns device
memory and the stream; every computation below runs in libevdr.so's HIP kernels on the caller's current
stream, with no synchronisation.  CPU tensors are rejected (there is no CPU path in the product)."""
from __future__ import annotations

from typing import Optional, Tuple

import collections
import weakref

import torch

from . import _lib as L

D = 128                  # width of one column block (the ColPali / ColQwen projection width: every tuned instance)
D_WIDE = 256             # two column blocks: the widest embedding the kernels score (fp16 hi/lo planes x 2 blocks, round 6)


def _require_cuda(*tensors) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "evdr_amd scores on the GPU only (HIP kernels, no CPU fallback): got a tensor on "
                f"{t.device}; move inputs to a cuda device")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")
    if dev is None:
        raise RuntimeError("no tensors given")
    return dev


def _mask_u8(m: Optional[torch.Tensor], shape, dev) -> Optional[torch.Tensor]:
    """mask.bool() as the reference does (evaluator/retrieval.py:179-180); one byte per token."""
    if m is None:
        return None
    if tuple(m.shape) != tuple(shape):
        raise RuntimeError(f"mask shape {tuple(m.shape)} does not match {tuple(shape)}")
    if m.dtype is torch.bool and m.device == dev and m.is_contiguous():
        return m                                        # the usual case, a dozen times per training step: no dispatcher round trips
    return m.to(device=dev).bool().contiguous()


def kernel_width(d: int) -> int:
    """Width the kernels score a d-wide embedding at: 128 (one column block) or 256 (two)."""
    if d <= 0 or d > D_WIDE:
        raise NotImplementedError(f"embedding width {d} unsupported (kernels are built for widths up to {D_WIDE})")
    return D if d <= D else D_WIDE


def pad_width(x: torch.Tensor) -> torch.Tensor:
    """(..., d) -> (..., 128) for d <= 128, (..., 256) for 128 < d <= 256, with zero columns appended (a zero column contributes
    an exact 0 to every dot product, so scores, arg-max and the first d columns of every gradient are those of the narrow
    tensors).  The reference takes any width (evaluator/retrieval.py:173); wider than 256 is not supported here."""
    d = x.shape[-1]
    w = kernel_width(d)
    return x if d == w else torch.nn.functional.pad(x, (0, w - d))


def split_wide(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(..., 256) -> ((4, ..., 128) fp16 planes, absmax word): `split_f32` of the two 128-column blocks under ONE power of two for
    the whole tensor; plane index = 2 * (0 hi | 1 lo) + column block -- the layout evdr_maxsim_fwd_prepared takes as nplanes = 4."""
    if x.shape[-1] != D_WIDE:
        raise RuntimeError(f"split_wide needs rows of width {D_WIDE}")
    lead = tuple(x.shape[:-1])
    blocks = x.float().reshape(-1, 2, D).transpose(0, 1).contiguous()           # (column block, row, 128)
    planes, amax = split_f32(blocks)                                           # (hi | lo, column block, row, 128)
    return planes.view((4,) + lead + (D,)), amax


def workspace(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def pack_pmask(pmask: Optional[torch.Tensor], npages: int, lp: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """(np, lp) byte mask -> (tilemask (np, ceil(lp/32)) int32 bits, pageflags (np,) int32)."""
    lib = L.load()
    ntiles = (lp + 31) // 32
    tilemask = torch.empty((npages, ntiles), dtype=torch.int32, device=dev)
    pageflags = torch.empty((npages,), dtype=torch.int32, device=dev)
    pm = _mask_u8(pmask, (npages, lp), dev)
    with L.on(dev):
        L.check(lib.evdr_pack_pmask(L.ptr(pm), npages, lp, L.ptr(tilemask), L.ptr(pageflags),
                                    L.current_stream_handle(dev)))
    return tilemask, pageflags


def flag_nonfinite(P: torch.Tensor, pmask: Optional[torch.Tensor], pageflags: torch.Tensor) -> None:
    """Set bit 3 of pageflags[p] for every page with a NaN / Inf element in a valid patch (evdr_flag_nonfinite): the
    forward kernels then return NaN for that page, where torch.max would have propagated it (evaluator/retrieval.py:201).
    P (np, lp, 128) fp32 / bf16 / fp16 (the hi plane of fp16 hi/lo planes), dense rows, any page stride."""
    dev = _require_cuda(P, pageflags)
    npg, lp, d = P.shape
    if npg == 0 or lp == 0:
        return
    kind = {torch.float32: L.EVDR_F32, torch.bfloat16: L.EVDR_BF16, torch.float16: L.EVDR_F16}.get(P.dtype)
    if kind is None or d != D or P.stride(2) != 1 or P.stride(1) != D:
        raise RuntimeError("flag_nonfinite needs (np, lp, 128) fp32 / bf16 / fp16 pages with dense rows")
    pm = _mask_u8(pmask, (npg, lp), dev)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_flag_nonfinite(L.ptr(P), kind, L.ptr(pm), npg, lp, int(P.stride(0)), L.ptr(pageflags),
                                        L.current_stream_handle(dev)))


def split_f32(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(..., 128) fp32 -> ((2, ..., 128) fp16 planes hi/lo of x * 2^k, absmax word): hi + lo == x * 2^k to ~2^-22, with
    one power of two k per tensor that the kernels derive from the absmax word (int32 tensor of 1 element holding the
    bits of max|x|; keep it with the planes)."""
    dev = _require_cuda(x)
    if x.shape[-1] != D:
        raise NotImplementedError(f"rows of width {x.shape[-1]}: this entry takes 128-wide rows (129..256 columns: `split_wide`; the scorers pad and split by themselves)")
    lib = L.load()
    xc = x.float().contiguous()
    rows = xc.numel() // D
    planes = torch.empty((2,) + tuple(xc.shape), dtype=torch.float16, device=dev)
    amax = torch.empty((1,), dtype=torch.int32, device=dev)
    with L.on(dev):
        L.check(lib.evdr_split_f32(L.ptr(xc), rows, L.ptr(planes), L.ptr(amax), L.current_stream_handle(dev)))
    return planes, amax


def split_f32_segments(x: torch.Tensor, seg: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """`split_f32` of consecutive groups of `seg` leading entries of x (n, ..., 128) in ONE launch -- the batches of a training
    epoch, known when the epoch starts.  Returns (planes, absmax words): planes (nseg, 2 * seg * rows_per_entry * 128) fp16,
    one row per segment, absmax (nseg,) int32; `segment_planes` cuts out segment s in `split_f32`'s format.  Every segment
    keeps its own absmax word: bit for bit the planes `split_f32(x[s * seg:(s + 1) * seg])` makes."""
    dev = _require_cuda(x)
    if x.shape[-1] != D:
        raise NotImplementedError(f"rows of width {x.shape[-1]}: this entry takes 128-wide rows (129..256 columns: `split_wide`; the scorers pad and split by themselves)")
    xc = x.float().contiguous()
    n = xc.shape[0]
    per = (xc.numel() // D) // max(n, 1)                       # rows per leading entry
    if seg < 1 or seg * per > 2048:
        raise ValueError(f"segments of {seg} x {per} rows: one segment is at most 2048 rows")
    nseg = (n + seg - 1) // seg
    planes = torch.empty((nseg, 2 * seg * per * D), dtype=torch.float16, device=dev)
    amax = torch.empty((max(nseg, 1),), dtype=torch.int32, device=dev)
    if n:
        lib = L.load()
        with L.on(dev):
            for s0 in range(0, nseg, 65535):                       # one launch covers at most 65535 segments (grid limit)
                s1 = min(nseg, s0 + 65535)
                rows = (min(n, s1 * seg) - s0 * seg) * per
                L.check(lib.evdr_split_f32_segments(xc.data_ptr() + s0 * seg * per * D * 4, rows, seg * per, planes[s0:].data_ptr(),
                                                    amax[s0:].data_ptr(), L.current_stream_handle(dev)))
    return planes, amax


def segment_planes(planes: torch.Tensor, amax: torch.Tensor, s: int, shape) -> Tuple[torch.Tensor, torch.Tensor]:
    """Segment s of `split_f32_segments` as ((2,) + shape fp16 planes, its absmax word): views, nothing is copied.  `shape` =
    shape of the fp32 batch (a short last batch has fewer leading entries)."""
    n = 1
    for d in shape:
        n *= int(d)
    return planes[s, : 2 * n].view((2,) + tuple(int(d) for d in shape)), amax[s:s + 1]


def maxsim_forward(Q: torch.Tensor, P: torch.Tensor, qmask: Optional[torch.Tensor], pmask: Optional[torch.Tensor],
                   want_argmax: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """A1 (evaluator/retrieval.py:166-213) through evdr_maxsim_fwd.  bf16 x bf16 inputs are scored as
    they are; anything else is upcast to fp32 like the reference (:176-177) and scored to fp32 accuracy."""
    dev = _require_cuda(Q, P)
    if Q.dim() != 3 or P.dim() != 3 or Q.shape[-1] != P.shape[-1]:
        raise RuntimeError(f"expected Q (Nq,Lq,D) and P (Np,Lp,D), got {tuple(Q.shape)} and {tuple(P.shape)}")
    Q, P = pad_width(Q), pad_width(P)                 # narrower embeddings: zero columns add exact zeros to every dot product
    nq, lq, d = Q.shape
    npg, lp, _ = P.shape
    out = torch.empty((nq, npg), dtype=torch.float32, device=dev)
    arg = torch.empty((nq, npg, lq), dtype=torch.int16, device=dev) if want_argmax else None
    if nq == 0 or npg == 0:
        return out, arg
    if lq == 0 or lp == 0:
        raise RuntimeError(f"zero-length token axis (Lq={lq}, Lp={lp})")
    if lp > 65535 or lq > 65535:
        raise NotImplementedError("token axes longer than 65535 are not supported")
    if d == D_WIDE:
        # 129..256 columns: every dtype is upcast like the reference does (evaluator/retrieval.py:176-177) and scored to fp32
        # accuracy on four planes (fp16 hi/lo x two column blocks), through the prepared entry point
        qp, qa = split_wide(Q)
        pp, pa = split_wide(P)
        tilemask, pageflags = pack_pmask(pmask, npg, lp, dev)
        for cb in (0, 1):
            flag_nonfinite(pp[cb], pmask, pageflags)                          # the hi planes of both column blocks
        return maxsim_forward_prepared(qp, qa, pp, pa, qmask, tilemask, pageflags, want_argmax=want_argmax)
    lib = L.load()
    if Q.dtype == torch.bfloat16 and P.dtype == torch.bfloat16:
        dtype = L.EVDR_BF16
        Qc = Q.contiguous()
        Pc = P if (P.stride(2) == 1 and P.stride(1) == D and P.stride(0) >= lp * D) else P.contiguous()
    else:
        dtype = L.EVDR_F32
        Qc = Q.float().contiguous()
        Pc = P.float().contiguous()
    strides = (L.C.c_int64 * 2)(Qc.stride(0), Pc.stride(0))
    qm = _mask_u8(qmask, (nq, lq), dev)
    pm = _mask_u8(pmask, (npg, lp), dev)
    nbytes = lib.evdr_maxsim_fwd_workspace(nq, lq, npg, lp, dtype)
    ws = workspace(nbytes, dev)
    with L.on(dev):
        L.check(lib.evdr_maxsim_fwd(L.ptr(Qc), L.ptr(Pc), L.ptr(qm), L.ptr(pm), L.ptr(out), L.ptr(arg),
                                    nq, lq, npg, lp, d, dtype, strides, L.ptr(ws), ws.numel(),
                                    L.current_stream_handle(dev)))
    return out, arg


def maxsim_forward_prepared(qplanes: torch.Tensor, qamax: Optional[torch.Tensor], pplanes: torch.Tensor,
                            pamax: Optional[torch.Tensor], qmask: Optional[torch.Tensor], tilemask: torch.Tensor,
                            pageflags: torch.Tensor, want_argmax: bool = False, out: Optional[torch.Tensor] = None,
                            out_col: int = 0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """A1 on PREPARED operands (evdr_maxsim_fwd_prepared): planes from `split_f32` / `l2norm_split` (2 fp16 planes + absmax
    word) or bf16 tensors with a leading plane axis of 1, masks from `pack_pmask`.  Nothing is converted or packed here.
    With `out` (nq, >= out_col + np) given, the scores land in out[:, out_col:out_col+np] (a shard's column block)."""
    dev = _require_cuda(qplanes, pplanes)
    nplanes, nq, lq, _ = qplanes.shape
    _, npg, lp, _ = pplanes.shape
    if (nplanes not in (1, 2, 4) or pplanes.shape[0] != nplanes or (nplanes >= 2) != (qplanes.dtype == torch.float16)
            or pplanes.dtype != qplanes.dtype):
        raise RuntimeError("query and page planes must both be (1, ., ., 128) bf16, both (2, ., ., 128) fp16, or both (4, ., ., 128) "
                           "fp16 (width 256: `split_wide`)")
    if pplanes.stride(3) != 1 or pplanes.stride(2) != D or not qplanes.is_contiguous():
        raise RuntimeError("planes must be dense in their last two dims (queries fully contiguous)")
    if out is None:
        out = torch.empty((nq, npg), dtype=torch.float32, device=dev)
        out_col = 0
    view = out[:, out_col:out_col + npg]
    arg = torch.empty((nq, npg, lq), dtype=torch.int16, device=dev) if want_argmax else None
    if nq == 0 or npg == 0:
        return view, arg
    qm = _mask_u8(qmask, (nq, lq), dev)
    qlist = torch.empty((nq + 1,), dtype=torch.int32, device=dev) if (lq > 32 and qm is not None and not want_argmax) else None
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_maxsim_fwd_prepared(
            L.ptr(qplanes), L.ptr(pplanes), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), view.data_ptr(), out.stride(0),
            L.ptr(arg), nq, lq, npg, lp, nplanes, int(pplanes.stride(1)), int(pplanes.stride(0)), L.ptr(qamax), L.ptr(pamax),
            L.ptr(qlist), L.current_stream_handle(dev)))
    return view, arg


def maxsim_forward_pages(qplanes: torch.Tensor, qamax: Optional[torch.Tensor], pplanes: torch.Tensor, pamax: Optional[torch.Tensor],
                         qmask: Optional[torch.Tensor], tilemask: torch.Tensor, pageflags: torch.Tensor, pages: torch.Tensor,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Scores of every query against the pages ONE list names (evdr_maxsim_fwd_pages): (nq, m) fp32, column i = page pages[i].
    pages (m,) int32 on the planes' device holds LOCAL page indices; an entry outside [0, np) is a hole: a column of -inf, nothing
    read.  Planes as `maxsim_forward_prepared` (one bf16 plane or fp16 hi/lo planes), queries of any length.  With `out`
    (nq, >= m) fp32 given, the scores land in out[:, :m].  No host synchronisation."""
    dev = _require_cuda(qplanes, pplanes)
    if qplanes.dim() != 4 or pplanes.dim() != 4:
        raise RuntimeError("planes must be (planes, rows, tokens, 128)")
    nplanes, nq, lq, _ = qplanes.shape
    _, npg, lp, _ = pplanes.shape
    if nplanes == 4 or pplanes.shape[0] == 4:
        raise NotImplementedError("page-subset scoring does not cover width-256 corpora (four planes)")
    if (nplanes not in (1, 2) or pplanes.shape[0] != nplanes or (nplanes == 2) != (qplanes.dtype == torch.float16)
            or pplanes.dtype != qplanes.dtype):
        raise RuntimeError("query and page planes must both be (1, ., ., 128) bf16 or both (2, ., ., 128) fp16 hi/lo")
    if pplanes.stride(3) != 1 or pplanes.stride(2) != D or not qplanes.is_contiguous():
        raise RuntimeError("planes must be dense in their last two dims (queries fully contiguous)")
    if not isinstance(pages, torch.Tensor) or pages.dim() != 1 or pages.dtype != torch.int32 or pages.device != dev:
        raise ValueError(f"pages must be an (m,) int32 tensor on {dev}; got {tuple(getattr(pages, 'shape', ()))} "
                         f"{getattr(pages, 'dtype', None)} on {getattr(pages, 'device', None)}")
    pages = pages.contiguous()
    m = int(pages.shape[0])
    if out is None:
        out = torch.empty((nq, m), dtype=torch.float32, device=dev)
    elif out.dim() != 2 or out.shape[0] != nq or out.shape[1] < m or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != dev:
        raise RuntimeError("out must be an (nq, >= m) fp32 tensor with unit column stride on the planes' device")
    view = out[:, :m]
    if nq == 0 or m == 0:
        return view
    if npg == 0:                                        # every entry is a hole
        view.fill_(float("-inf"))
        return view
    qm = _mask_u8(qmask, (nq, lq), dev)
    qlist = torch.empty((nq + 1,), dtype=torch.int32, device=dev) if lq > 32 else None
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_maxsim_fwd_pages(
            L.ptr(qplanes), L.ptr(pplanes), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), L.ptr(pages), m, view.data_ptr(),
            out.stride(0) if nq > 1 else max(m, out.shape[1]), nq, lq, npg, lp, nplanes, int(pplanes.stride(1)), int(pplanes.stride(0)),
            L.ptr(qamax), L.ptr(pamax), L.ptr(qlist), L.current_stream_handle(dev)))
    return view


# ---- fp8 (e4m3fn) corpora (include/evdr.h "fp8 corpora") -------------------------------------------------------------
FP8 = torch.float8_e4m3fn


def quantize_fp8(x: torch.Tensor, rows_per_group: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(..., d) with d <= 128 -> ((..., 128) float8_e4m3fn bytes of x * 2^k, (groups,) int32 k): one power of two per group of
    `rows_per_group` consecutive rows (a page: lp rows, a query: lq rows), chosen on the device (evdr_quantize_fp8).  The width is
    padded with zero columns as `pad_width` does; fp32 and bf16 are read as they are, other float dtypes go through fp32."""
    dev = _require_cuda(x)
    d = x.shape[-1]
    if d > D:
        raise NotImplementedError(f"fp8 covers embeddings of width <= {D}; got width {d}")
    if rows_per_group < 1:
        raise ValueError(f"rows_per_group must be >= 1; got {rows_per_group}")
    xc = x if x.dtype in (torch.float32, torch.bfloat16) else x.float()
    xc = xc.contiguous()
    rows = xc.numel() // d if d else 0
    if rows % rows_per_group:
        raise ValueError(f"{rows} rows do not split into groups of {rows_per_group}")
    groups = rows // rows_per_group
    x8 = torch.empty(tuple(x.shape[:-1]) + (D,), dtype=FP8, device=dev)
    shift = torch.empty((groups,), dtype=torch.int32, device=dev)
    if groups == 0:
        return x8, shift
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_quantize_fp8(L.ptr(xc), L.EVDR_BF16 if xc.dtype == torch.bfloat16 else L.EVDR_F32, groups, rows_per_group, d,
                                      L.ptr(x8), L.ptr(shift), L.current_stream_handle(dev)))
    return x8, shift


def maxsim_forward_fp8(q8: torch.Tensor, qshift: torch.Tensor, p8: torch.Tensor, pshift: torch.Tensor, qmask: Optional[torch.Tensor],
                       tilemask: torch.Tensor, pageflags: torch.Tensor, out: Optional[torch.Tensor] = None,
                       out_col: int = 0) -> torch.Tensor:
    """A1 on fp8 operands (evdr_maxsim_fwd_fp8): q8 (nq, lq, 128) / p8 (np, lp, 128) float8_e4m3fn with their per-query / per-page
    shifts from `quantize_fp8`, masks from `pack_pmask`.  With `out` (nq, >= out_col + np) given, the scores land in
    out[:, out_col:out_col+np] (a shard's column block).  Returns that (nq, np) view."""
    dev = _require_cuda(q8, p8)
    if q8.dtype != FP8 or p8.dtype != FP8 or q8.dim() != 3 or p8.dim() != 3 or q8.shape[-1] != D or p8.shape[-1] != D:
        raise RuntimeError("fp8 operands must be (n, l, 128) float8_e4m3fn tensors (ops.quantize_fp8)")
    if p8.stride(2) != 1 or p8.stride(1) != D or not q8.is_contiguous():
        raise RuntimeError("fp8 pages must be dense in their last two dims (queries fully contiguous)")
    nq, lq, _ = q8.shape
    npg, lp, _ = p8.shape
    if tuple(qshift.shape) != (nq,) or tuple(pshift.shape) != (npg,):
        raise RuntimeError("one shift per query and one per page (ops.quantize_fp8)")
    if out is None:
        out = torch.empty((nq, npg), dtype=torch.float32, device=dev)
        out_col = 0
    view = out[:, out_col:out_col + npg]
    if nq == 0 or npg == 0:
        return view
    qm = _mask_u8(qmask, (nq, lq), dev)
    qlist = torch.empty((nq + 1,), dtype=torch.int32, device=dev) if (lq > 32 and qm is not None) else None
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_maxsim_fwd_fp8(L.ptr(q8), L.ptr(p8), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), view.data_ptr(),
                                        out.stride(0), nq, lq, npg, lp, int(p8.stride(0)), L.ptr(qshift), L.ptr(pshift), L.ptr(qlist),
                                        L.current_stream_handle(dev)))
    return view


def maxsim_forward_fp8_pages(q8: torch.Tensor, qshift: torch.Tensor, p8: torch.Tensor, pshift: torch.Tensor,
                             qmask: Optional[torch.Tensor], tilemask: torch.Tensor, pageflags: torch.Tensor, pages: torch.Tensor,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Scores of every query against the pages ONE list names, on fp8 operands (evdr_maxsim_fwd_fp8_pages): (nq, m) fp32, column i =
    page pages[i], the bits `maxsim_forward_fp8` gives that (query, page) for the same query batch.  pages (m,) int32 on the
    corpus's device holds LOCAL page indices in any order (duplicates are each scored); an entry outside [0, np) is a hole: a column
    of -inf, nothing read.  Operands as `maxsim_forward_fp8`, queries of any length.  With `out` (nq, >= m) fp32 given, the scores
    land in out[:, :m].  No host synchronisation."""
    dev = _require_cuda(q8, p8)
    if q8.dtype != FP8 or p8.dtype != FP8 or q8.dim() != 3 or p8.dim() != 3 or q8.shape[-1] != D or p8.shape[-1] != D:
        raise RuntimeError("fp8 operands must be (n, l, 128) float8_e4m3fn tensors (ops.quantize_fp8)")
    if p8.stride(2) != 1 or p8.stride(1) != D or not q8.is_contiguous():
        raise RuntimeError("fp8 pages must be dense in their last two dims (queries fully contiguous)")
    nq, lq, _ = q8.shape
    npg, lp, _ = p8.shape
    if tuple(qshift.shape) != (nq,) or tuple(pshift.shape) != (npg,):
        raise RuntimeError("one shift per query and one per page (ops.quantize_fp8)")
    if not isinstance(pages, torch.Tensor) or pages.dim() != 1 or pages.dtype != torch.int32 or pages.device != dev:
        raise ValueError(f"pages must be an (m,) int32 tensor on {dev}; got {tuple(getattr(pages, 'shape', ()))} "
                         f"{getattr(pages, 'dtype', None)} on {getattr(pages, 'device', None)}")
    pages = pages.contiguous()
    m = int(pages.shape[0])
    if out is None:
        out = torch.empty((nq, m), dtype=torch.float32, device=dev)
    elif out.dim() != 2 or out.shape[0] != nq or out.shape[1] < m or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != dev:
        raise RuntimeError("out must be an (nq, >= m) fp32 tensor with unit column stride on the corpus's device")
    view = out[:, :m]
    if nq == 0 or m == 0:
        return view
    if npg == 0:                                        # every entry is a hole
        view.fill_(float("-inf"))
        return view
    qm = _mask_u8(qmask, (nq, lq), dev)
    qlist = torch.empty((nq + 1,), dtype=torch.int32, device=dev) if lq > 32 else None
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_maxsim_fwd_fp8_pages(
            L.ptr(q8), L.ptr(p8), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), L.ptr(pages), m, view.data_ptr(),
            out.stride(0) if nq > 1 else max(m, out.shape[1]), nq, lq, npg, lp, int(p8.stride(0)), L.ptr(qshift), L.ptr(pshift),
            L.ptr(qlist), L.current_stream_handle(dev)))
    return view


# ---- growable corpus: fused page ingest (include/evdr.h "growable corpus") --------------------------------------------
def corpus_ingest(P: torch.Tensor, pmask: Optional[torch.Tensor], planes: torch.Tensor, tilemask: torch.Tensor, pageflags: torch.Tensor,
                  shift: Optional[torch.Tensor] = None, pamax: Optional[torch.Tensor] = None, first_page: int = 0,
                  dst_pages: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> None:
    """Prepare the pages P (b, lp_src, d) fp32 / bf16 / fp16 IN PLACE in a corpus's storage (evdr_corpus_ingest): ONE launch writes
    planes, tile words, flag words (and fp8 shifts) of pages first_page .. first_page + b, or of the pages dst_pages (b,) int32 names
    (LOCAL indices on the device; an entry outside [0, capacity) is a hole, its page skipped).  planes (nplanes, capacity, lp, 128)
    bf16 (1 plane), fp16 hi/lo (2, with the corpus's absmax word `pamax`) or float8_e4m3fn (1, with `shift` (capacity,)); tilemask
    (capacity, ceil(lp / 32)) and pageflags (capacity,) int32 -- the FULL storage, not the views of the pages filled so far.  status:
    optional (1,) int32, zeroed by the caller; bit 0 = a finite element above the corpus's binade (fp16 hi/lo).  No synchronisation."""
    dev = _require_cuda(P, planes, tilemask, pageflags)
    if P.dim() != 3 or planes.dim() != 4:
        raise RuntimeError(f"expected pages (b, lp_src, d) and planes (planes, capacity, lp, 128); got {tuple(P.shape)} and {tuple(planes.shape)}")
    b, lp_src, d = P.shape
    nplanes, cap, lp, _ = planes.shape
    src = {torch.float32: L.EVDR_F32, torch.bfloat16: L.EVDR_BF16, torch.float16: L.EVDR_F16}.get(P.dtype)
    if src is None:
        raise RuntimeError(f"pages must be fp32, bf16 or fp16; got {P.dtype}")
    kind = L.EVDR_CORPUS_FP8 if planes.dtype == FP8 else {1: L.EVDR_CORPUS_BF16, 2: L.EVDR_CORPUS_F16_HILO}.get(nplanes, L.EVDR_CORPUS_F16_WIDE)
    if planes.stride(3) != 1 or planes.stride(2) != D or not tilemask.is_contiguous() or not pageflags.is_contiguous():
        raise RuntimeError("planes must be dense in their last two dims, tile and flag words contiguous")
    if tuple(tilemask.shape) != (cap, (lp + 31) // 32) or tuple(pageflags.shape) != (cap,) or (shift is not None and tuple(shift.shape) != (cap,)):
        raise RuntimeError("tilemask (capacity, ceil(lp / 32)), pageflags (capacity,) and shift (capacity,) must cover the planes' capacity")
    if dst_pages is not None and (dst_pages.dim() != 1 or dst_pages.dtype != torch.int32 or dst_pages.device != dev or dst_pages.shape[0] != b):
        raise ValueError(f"dst_pages must be a (b,) = ({b},) int32 tensor on {dev}")
    Pc = P.contiguous()
    pm = _mask_u8(pmask, (b, lp_src), dev)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_corpus_ingest(L.ptr(Pc), src, L.ptr(pm), b, lp_src, d, lp_src * d, L.ptr(planes), kind, cap, lp,
                                       int(planes.stride(1)), int(planes.stride(0)), L.ptr(tilemask), L.ptr(pageflags), L.ptr(shift),
                                       L.ptr(pamax), int(first_page), None if dst_pages is None else L.ptr(dst_pages.contiguous()),
                                       L.ptr(status), L.current_stream_handle(dev)))


# ---- pooled corpora: group-mean pooling fused into the ingest (include/evdr.h "pooled corpora") ---------------------
def pool_groups_windows(lp: int, f: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Shared CSR grouping (members (lp,), offsets (ceil(lp / f) + 1,)) int32 on the CPU: row-major windows of `f` consecutive patches;
    the last window is ragged when f does not divide lp."""
    lp, f = int(lp), int(f)
    if lp < 1 or f < 1:
        raise ValueError(f"pool_groups_windows needs lp >= 1 and f >= 1; got lp={lp}, f={f}")
    offsets = torch.arange(0, lp + f, f, dtype=torch.int32).clamp_max(lp)[: (lp + f - 1) // f + 1]
    return torch.arange(lp, dtype=torch.int32), offsets


def pool_groups_grid(rows: int, cols: int, fr: int, fc: int, first: int = 0, extra: str = "own",
                     lp: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Shared CSR grouping (members, offsets) int32 on the CPU: `fr` x `fc` blocks of a row-major `rows` x `cols` patch grid whose
    first patch is patch `first` of the page (ragged blocks at the right and bottom edges).  Patches outside the grid -- [0, first)
    and [first + rows * cols, lp), ColPali's special tokens -- each keep a group of their own (extra="own"; groups in patch order:
    the ones in front, the blocks row-major, the ones behind) or are left out of every group (extra="drop").  lp: patches per page,
    default first + rows * cols (nothing behind the grid)."""
    rows, cols, fr, fc, first = int(rows), int(cols), int(fr), int(fc), int(first)
    lp = first + rows * cols if lp is None else int(lp)
    if min(rows, cols, fr, fc) < 1 or first < 0 or lp < first + rows * cols:
        raise ValueError(f"pool_groups_grid needs rows, cols, fr, fc >= 1, first >= 0 and lp >= first + rows * cols; got "
                         f"rows={rows}, cols={cols}, fr={fr}, fc={fc}, first={first}, lp={lp}")
    if extra not in ("own", "drop"):
        raise ValueError(f"extra must be 'own' or 'drop'; got {extra!r}")
    r, c = torch.arange(rows), torch.arange(cols)
    block = ((r // fr)[:, None] * ((cols + fc - 1) // fc) + (c // fc)[None, :]).flatten()      # block of every grid patch, row-major
    order = torch.argsort(block, stable=True)                                                 # patches block by block, row-major inside
    sizes = torch.bincount(block)
    own = extra == "own"
    front = torch.arange(first if own else 0)
    back = torch.arange(first + rows * cols, lp if own else first + rows * cols)
    members = torch.cat([front, order + first, back]).to(torch.int32)
    counts = torch.cat([torch.ones_like(front), sizes, torch.ones_like(back)])
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(torch.int32)
    return members, offsets


def _check_pool_args(P, pmask, members, offsets) -> Tuple[int, int, int, int, int, bool]:
    """Shapes, dtypes and (shared groupings) the offsets of a pooling call, before any device work: (b, lp_src, d, ls, m, per_page).
    A SHARED grouping is validated here, on the host (offsets[0] == 0, non-decreasing, offsets[-1] <= m); given as device tensors it
    is read back for that, which synchronises -- hand over the CPU tensors `pool_groups_*` return to avoid it.  A PER-PAGE grouping
    is checked for shape and dtype only and never read back: the kernel clamps its offsets into the list, so a bad one can empty
    groups but not leave the arrays."""
    if not isinstance(P, torch.Tensor) or P.dim() != 3:
        raise ValueError(f"pages must be a (b, lp_src, d) tensor; got {tuple(getattr(P, 'shape', ()))}")
    b, lp_src, d = P.shape
    if d > D:
        raise NotImplementedError(f"pooling covers embeddings of width <= {D}, not width-256 corpora; got width {d}")
    if d < 1:
        raise ValueError(f"pages must be a (b, lp_src, d) tensor with d >= 1; got {tuple(P.shape)}")
    if P.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"pooling takes fp32, bf16 or fp16 pages; got {P.dtype}")
    if pmask is not None and (not isinstance(pmask, torch.Tensor) or tuple(pmask.shape) != (b, lp_src)):
        raise ValueError(f"pmask shape {tuple(getattr(pmask, 'shape', ()))} does not match the pages' {(b, lp_src)}")
    for name, t in (("members", members), ("offsets", offsets)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name} must be an int32 or int64 tensor; got {getattr(t, 'dtype', type(t))}")
        if t.is_cuda and P.is_cuda and t.device != P.device:
            raise ValueError(f"{name} on {t.device}, pages on {P.device}")
    if members.dim() != offsets.dim() or members.dim() not in (1, 2):
        raise ValueError(f"members / offsets must be (m,) / (ls + 1,) shared by all pages or (b, m) / (b, ls + 1) per page; got "
                         f"{tuple(members.shape)} / {tuple(offsets.shape)}")
    per_page = members.dim() == 2
    if per_page and (members.shape[0] != b or offsets.shape[0] != b):
        raise ValueError(f"per-page members / offsets need one row per page (b = {b}); got {tuple(members.shape)} / {tuple(offsets.shape)}")
    m, ls = int(members.shape[-1]), int(offsets.shape[-1]) - 1
    if not (1 <= ls <= 65535):
        raise ValueError(f"offsets must hold ls + 1 entries with ls in 1..65535; got {ls + 1}")
    if not per_page:
        off = offsets.cpu().long()
        if int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()) or int(off[-1]) > m:
            raise ValueError(f"offsets must start at 0, be non-decreasing and end at or below the {m} members")
    return int(b), int(lp_src), int(d), ls, m, per_page


def _pool_lists(members: torch.Tensor, offsets: torch.Tensor, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    return (members.to(device=dev, dtype=torch.int32).contiguous(), offsets.to(device=dev, dtype=torch.int32).contiguous())


_SRC_DTYPE = {torch.float32: L.EVDR_F32, torch.bfloat16: L.EVDR_BF16, torch.float16: L.EVDR_F16}


def pool_pages(P: torch.Tensor, pmask: Optional[torch.Tensor], members: torch.Tensor, offsets: torch.Tensor,
               normalize: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Group-mean pooling of every page's patches (evdr_pool_pages, ONE launch): P (n, lp_src, d <= 128) fp32 / bf16 / fp16, pmask
    (n, lp_src) or None, grouping in CSR form -- members int32 patch indices group after group, offsets (ls + 1) -- shared by all
    pages ((m,), (ls + 1,): `pool_groups_windows`, `pool_groups_grid`) or per page ((n, m), (n, ls + 1): clustering labels computed
    elsewhere).  Returns (Pbar (n, ls, d) fp32, pooled_mask (n, ls) bool) by the rule `pool_reference` states, bit for bit: the
    mean of a group's valid members in list order, l2-renormalised unless normalize=False; a group without a valid member is a
    masked token of zeros.  What a trainer initialises a student from (Pbar_raw / pmask_student) and what `PageCorpus.from_pooled`
    stores without materialising it.  Argument validation: `_check_pool_args` (a shared grouping on the device is read back once;
    CPU groupings and per-page groupings never synchronise)."""
    b, lp_src, d, ls, m, per_page = _check_pool_args(P, pmask, members, offsets)
    dev = _require_cuda(P)
    out = torch.empty((b, ls, d), dtype=torch.float32, device=dev)
    mask = torch.empty((b, ls), dtype=torch.bool, device=dev)
    if b == 0:
        return out, mask
    mem, off = _pool_lists(members, offsets, dev)
    Pc = P.contiguous()
    pm = _mask_u8(pmask, (b, lp_src), dev)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_pool_pages(L.ptr(Pc), _SRC_DTYPE[P.dtype], L.ptr(pm), b, lp_src, d, lp_src * d, L.ptr(mem), L.ptr(off), m, ls,
                                    int(per_page), int(bool(normalize)), L.ptr(out), d, L.ptr(mask), L.current_stream_handle(dev)))
    return out, mask


def corpus_pool_ingest(P: torch.Tensor, pmask: Optional[torch.Tensor], members: torch.Tensor, offsets: torch.Tensor, planes: torch.Tensor,
                       tilemask: torch.Tensor, pageflags: torch.Tensor, shift: Optional[torch.Tensor] = None,
                       pamax: Optional[torch.Tensor] = None, first_page: int = 0, dst_pages: Optional[torch.Tensor] = None,
                       status: Optional[torch.Tensor] = None, normalize: bool = True) -> None:
    """`corpus_ingest` of the pooled pages `pool_pages(P, pmask, members, offsets, normalize)` would return, without materialising
    them (evdr_corpus_pool_ingest): ONE launch pools every page and writes its planes, tile words, flag word (and fp8 shift) IN PLACE
    into the corpus's storage -- the bits `corpus_ingest` writes for the pooled page.  planes / tilemask / pageflags / shift / pamax /
    first_page / dst_pages / status as in `corpus_ingest`, with the corpus's page length lp >= ls.  A bf16 corpus takes any source
    dtype here: the pooled value is rounded to bf16.  No synchronisation beyond what `_check_pool_args` says about device groupings."""
    b, lp_src, d, ls, m, per_page = _check_pool_args(P, pmask, members, offsets)
    dev = _require_cuda(P, planes, tilemask, pageflags)
    if planes.dim() != 4:
        raise RuntimeError(f"expected planes (planes, capacity, lp, 128); got {tuple(planes.shape)}")
    nplanes, cap, lp, _ = planes.shape
    kind = L.EVDR_CORPUS_FP8 if planes.dtype == FP8 else {1: L.EVDR_CORPUS_BF16, 2: L.EVDR_CORPUS_F16_HILO}.get(nplanes, L.EVDR_CORPUS_F16_WIDE)
    if planes.stride(3) != 1 or planes.stride(2) != D or not tilemask.is_contiguous() or not pageflags.is_contiguous():
        raise RuntimeError("planes must be dense in their last two dims, tile and flag words contiguous")
    if tuple(tilemask.shape) != (cap, (lp + 31) // 32) or tuple(pageflags.shape) != (cap,) or (shift is not None and tuple(shift.shape) != (cap,)):
        raise RuntimeError("tilemask (capacity, ceil(lp / 32)), pageflags (capacity,) and shift (capacity,) must cover the planes' capacity")
    if dst_pages is not None and (dst_pages.dim() != 1 or dst_pages.dtype != torch.int32 or dst_pages.device != dev or dst_pages.shape[0] != b):
        raise ValueError(f"dst_pages must be a (b,) = ({b},) int32 tensor on {dev}")
    mem, off = _pool_lists(members, offsets, dev)
    Pc = P.contiguous()
    pm = _mask_u8(pmask, (b, lp_src), dev)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_corpus_pool_ingest(L.ptr(Pc), _SRC_DTYPE[P.dtype], L.ptr(pm), b, lp_src, d, lp_src * d, L.ptr(mem), L.ptr(off), m, ls,
                                            int(per_page), int(bool(normalize)), L.ptr(planes), kind, cap, lp, int(planes.stride(1)),
                                            int(planes.stride(0)), L.ptr(tilemask), L.ptr(pageflags), L.ptr(shift), L.ptr(pamax),
                                            int(first_page), None if dst_pages is None else L.ptr(dst_pages.contiguous()), L.ptr(status),
                                            L.current_stream_handle(dev)))


def pool_reference(P: torch.Tensor, pmask: Optional[torch.Tensor], members: torch.Tensor, offsets: torch.Tensor,
                   normalize: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """The pooling rule in plain torch, on CPU or GPU tensors: (Pbar (n, ls, d) fp32, pooled_mask (n, ls) bool).
    Every fp32 operation is one torch call, so each is rounded on its own, in the order the kernel is pinned to:
    - pooled token t of a page starts from +0.0 and adds the group's VALID members (index inside [0, lp_src), mask byte set) one
      after another in list order, then divides by their count; a group without a valid member is a masked token of zeros;
    - normalize=True applies l2_normalize, x / (||x|| + 1e-12), with the sum of squares formed octet by octet (8 consecutive
      columns, ascending, acc = acc + x * x with the product rounded before the add; columns >= d count as zeros) and the 16 octet
      sums combined by a balanced tree of adjacent pairs; square root, + 1e-12 and divide each correctly rounded."""
    n, lp_src, d = P.shape
    dev = P.device
    x = P.float()
    mem, off = members.to(dev).long(), offsets.to(dev).long()
    if mem.dim() == 1:
        mem, off = mem[None].expand(n, -1), off[None].expand(n, -1)
    m, ls = mem.shape[1], off.shape[1] - 1
    beg = off[:, :-1]
    size = off[:, 1:] - beg
    src_ok = torch.ones((n, lp_src), dtype=torch.bool, device=dev) if pmask is None else pmask.to(dev).bool()
    acc = torch.zeros((n, ls, d), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n, ls), dtype=torch.float32, device=dev)
    longest = int(size.max()) if size.numel() else 0
    for j in range(longest if (m and lp_src) else 0):                   # the j-th member of every group at once: list order
        idx = mem.gather(1, (beg + j).clamp(0, m - 1))
        ok = (j < size) & (idx >= 0) & (idx < lp_src)                   # anything else is a hole
        safe = idx.clamp(0, lp_src - 1)
        ok = ok & src_ok.gather(1, safe)
        row = x.gather(1, safe[:, :, None].expand(-1, -1, d))
        acc = torch.where(ok[:, :, None], acc + row, acc)
        cnt = cnt + ok
    mask = cnt > 0
    out = torch.where(mask[:, :, None], acc / cnt.clamp_min(1.0)[:, :, None], acc)
    if normalize:
        w = torch.nn.functional.pad(out, (0, D - d)).view(n, ls, D // 8, 8)
        s = torch.zeros((n, ls, D // 8), dtype=torch.float32, device=dev)
        for j in range(8):                                              # every octet sequentially, ascending
            s = s + w[..., j] * w[..., j]
        while s.shape[-1] > 1:                                          # 0+1, 2+3, ...; then pairs of those
            s = s[..., 0::2] + s[..., 1::2]
        # the correctly rounded fp32 root: taken in fp64 and rounded (exact for sqrt, 53 >= 2 * 24 + 2); an fp32 sqrt of a CPU
        # tensor may go through a vector math library that is accurate to an ulp but not correctly rounded
        norm = s.double().sqrt().float()
        out = out / (norm + torch.tensor(1e-12, dtype=torch.float32, device=dev))
    return out, mask


# ---- token clustering: similarity-grouped per-page lists for the pooling calls (include/evdr.h "token clustering") -----
CLUSTER_MAX_LS = 4096
CLUSTER_MAX_ITERS = 64
_cluster_ws: dict = {}                   # (device, stream) -> the launch's workspace, kept between calls and grown when a call needs more


def _check_cluster_args(P, pmask, ls, factor, iters) -> Tuple[int, int, int, int, int]:
    """Arguments of a clustering call, before any device work: (b, lp_src, d, ls, iters)."""
    if not isinstance(P, torch.Tensor) or P.dim() != 3:
        raise ValueError(f"pages must be a (b, lp_src, d) tensor; got {tuple(getattr(P, 'shape', ()))}")
    b, lp_src, d = P.shape
    if d > D:
        raise NotImplementedError(f"clustering covers embeddings of width <= {D}, not width-256 corpora; got width {d}")
    if d < 1 or not (1 <= lp_src <= 65535):
        raise ValueError(f"pages must be a (b, lp_src, d) tensor with d >= 1 and lp_src in 1..65535; got {tuple(P.shape)}")
    if P.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"clustering takes fp32, bf16 or fp16 pages; got {P.dtype}")
    if pmask is not None and (not isinstance(pmask, torch.Tensor) or tuple(pmask.shape) != (b, lp_src)):
        raise ValueError(f"pmask shape {tuple(getattr(pmask, 'shape', ()))} does not match the pages' {(b, lp_src)}")
    if (ls is None) == (factor is None):
        raise ValueError("exactly one of ls= (groups per page) and factor= (patches per group: ls = ceil(lp_src / factor)) must be given")
    if factor is not None:
        if int(factor) != factor or int(factor) < 1:
            raise ValueError(f"factor must be an integer >= 1; got {factor}")
        ls = (lp_src + int(factor) - 1) // int(factor)
    if int(ls) != ls or not (1 <= int(ls) <= CLUSTER_MAX_LS):
        raise ValueError(f"ls must be an integer in 1..{CLUSTER_MAX_LS}; got {ls}")
    if int(iters) != iters or not (0 <= int(iters) <= CLUSTER_MAX_ITERS):
        raise ValueError(f"iters must be an integer in 0..{CLUSTER_MAX_ITERS}; got {iters}")
    return int(b), int(lp_src), int(d), int(ls), int(iters)


def cluster_pages(P: torch.Tensor, pmask: Optional[torch.Tensor], ls: Optional[int] = None, factor: Optional[int] = None, iters: int = 8,
                  return_labels: bool = False):
    """Similarity grouping of every page's valid patches (evdr_cluster_pages, ONE launch): spherical k-means per page into at most
    `ls` groups -- or `factor` patches per group, ls = ceil(lp_src / factor); exactly one of the two -- from equal windows over the
    valid patches, `iters` iterations of centroid update + assign.  P (n, lp_src, d <= 128) fp32 / bf16 / fp16, pmask (n, lp_src) or
    None.  Returns (members (n, lp_src), offsets (n, ls + 1)[, labels (n, lp_src)]) int32 on the device: the per-page CSR grouping
    `pool_pages`, `corpus_pool_ingest` and `PageCorpus.from_pooled` take, by the rule `cluster_reference` states, bit for bit.
    Never synchronises; the launch's workspace is kept between calls (per device and stream; its size does not depend on n).
    Arguments are checked before any device work."""
    b, lp_src, d, ls, iters = _check_cluster_args(P, pmask, ls, factor, iters)
    dev = _require_cuda(P)
    members = torch.empty((b, lp_src), dtype=torch.int32, device=dev)
    offsets = torch.empty((b, ls + 1), dtype=torch.int32, device=dev)
    labels = torch.empty((b, lp_src), dtype=torch.int32, device=dev) if return_labels else None
    if b:
        lib = L.load()
        stream = L.current_stream_handle(dev)
        need = int(lib.evdr_cluster_pages_workspace(lp_src, ls))
        ws = _cluster_ws.get((dev, stream))
        if ws is None or ws.numel() < need:
            ws = _cluster_ws[(dev, stream)] = workspace(need, dev)
        Pc = P.contiguous()
        pm = _mask_u8(pmask, (b, lp_src), dev)
        with L.on(dev):
            L.check(lib.evdr_cluster_pages(L.ptr(Pc), _SRC_DTYPE[P.dtype], L.ptr(pm), b, lp_src, d, lp_src * d, ls, iters, L.ptr(members),
                                           L.ptr(offsets), L.ptr(labels), L.ptr(ws), ws.numel(), stream))
    return (members, offsets, labels) if return_labels else (members, offsets)


def _cluster_lists(labels: torch.Tensor, ls: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """labels (n, lp_src) in [-1, ls) -> the CSR lists: group after group, ascending patch index inside a group (stable sort), -1 behind."""
    n = labels.shape[0]
    key = torch.where(labels < 0, torch.full_like(labels, ls), labels)
    order = torch.argsort(key, dim=1, stable=True)
    members = torch.where(key.gather(1, order) < ls, order, torch.full_like(order, -1))
    cnt = torch.zeros((n, ls + 1), dtype=torch.int64, device=labels.device).scatter_add_(1, key, torch.ones_like(key))
    offsets = torch.cat([torch.zeros((n, 1), dtype=torch.int64, device=labels.device), cnt[:, :ls].cumsum(1)], dim=1)
    return members.to(torch.int32), offsets.to(torch.int32)


def cluster_reference(P: torch.Tensor, pmask: Optional[torch.Tensor], ls: int, iters: int,
                      history: Optional[list] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The clustering rule in plain torch, on CPU or GPU tensors: (members (n, lp_src), offsets (n, ls + 1), labels
    (n, lp_src)) int32.  Per page, with v_0 < ... < v_{nv-1} its valid patches and g = min(ls, nv) live groups:
    - start: label(v_i) = floor(i * g / nv); masked patches carry -1 throughout;
    - update: the centroid of a live group is `pool_reference(..., normalize=True)` of its current members in ascending patch index;
      a live group without a member keeps the centroid it had;
    - assign: s_j = x . c_j for the raw row x, formed as the pooled norm is -- 8 octet positions added one after another
      (acc = acc + x * c, product rounded first, columns >= d zeros), the 16 octet sums combined by the tree of adjacent pairs --
      then argmax over the live groups with NaN scores set to -inf: the lowest index of the maximum, 0 when nothing exceeds -inf;
    - after `iters` iterations the labels are listed by a stable argsort: group 0's patches ascending, then group 1's, ..., -1 behind.
    history: a list that receives the labels after the start and after every iteration (what a test counts label changes on).
    Pages are taken a few at a time so that the (pages, lp_src, ls, 16) temporaries stay below 256 MiB."""
    b, lp_src, d, ls, iters = _check_cluster_args(P, pmask, ls, None, iters)
    step = max(1, (1 << 26) // (lp_src * ls * (D // 8)))
    if b > step:
        parts, hist = [], []
        for lo in range(0, b, step):
            h = [] if history is not None else None
            parts.append(cluster_reference(P[lo:lo + step], None if pmask is None else pmask[lo:lo + step], ls, iters, h))
            hist.append(h)
        if history is not None:
            history.extend(torch.cat(hs) for hs in zip(*hist))
        return tuple(torch.cat(ts) for ts in zip(*parts))
    dev = P.device
    ok = torch.ones((b, lp_src), dtype=torch.bool, device=dev) if pmask is None else pmask.to(dev).bool()
    nv = ok.sum(1, keepdim=True)
    g = nv.clamp_max(ls)
    rank = ok.long().cumsum(1) - 1
    minus = torch.full((b, lp_src), -1, dtype=torch.int64, device=dev)
    labels = torch.where(ok, rank * g // nv.clamp_min(1), minus)
    if history is not None:
        history.append(labels.to(torch.int32))
    live = torch.arange(ls, device=dev)[None] < g                       # (b, ls)
    x = torch.nn.functional.pad(P.float(), (0, D - d)).view(b, lp_src, 1, D // 8, 8)
    cent = torch.zeros((b, ls, d), dtype=torch.float32, device=dev)
    for _ in range(iters):
        c, has = pool_reference(P, ok, *_cluster_lists(labels, ls), normalize=True)
        cent = torch.where(has[:, :, None], c, cent)
        cp = torch.nn.functional.pad(cent, (0, D - d)).view(b, 1, ls, D // 8, 8)
        s = torch.zeros((b, lp_src, ls, D // 8), dtype=torch.float32, device=dev)
        for j in range(8):                                              # every octet sequentially, ascending
            s = s + x[..., j] * cp[..., j]
        while s.shape[-1] > 1:                                          # 0+1, 2+3, ...; then pairs of those
            s = s[..., 0::2] + s[..., 1::2]
        s = s[..., 0]
        s = torch.where(torch.isnan(s) | ~live[:, None, :], torch.full_like(s, float("-inf")), s)
        labels = torch.where(ok, s.argmax(-1), minus)
        if history is not None:
            history.append(labels.to(torch.int32))
    members, offsets = _cluster_lists(labels, ls)
    return members, offsets, labels.to(torch.int32)


class ScoreRowCache:
    """Device-side (query row -> score row) cache of ONE prepared, frozen page tensor (include/evdr.h "score-row cache";
    evaluator/retrieval.py builds it for the reference's per-step re-scoring of the frozen teacher,
    mainv2_iter_distill_infonce.py:282-283).  Fixed geometry -- `lq` tokens per query, `row_dtype` rows, `npg` pages -- and a fixed
    `capacity` chosen from a byte budget; nothing is evicted, a full cache simply stops storing.  `nbytes` = device memory held."""

    def __init__(self, lq: int, row_dtype: torch.dtype, npg: int, max_bytes: int, dev, hash_mask: int = 0xFFFFFFFFFFFFFFFF):
        self.lq, self.row_dtype, self.npg, self.dev = int(lq), row_dtype, int(npg), dev
        self.row_bytes = self.lq * D * torch.empty((), dtype=row_dtype).element_size()
        per_entry = self.row_bytes + self.lq + 4 * self.npg + 8 + 4 + 4 * 4        # row, mask, scores, hash, k, four table slots
        self.capacity = int(min(max(int(max_bytes) // per_entry, 0), (1 << 30)))
        if self.capacity < 1:
            raise ValueError(f"score-row cache: a budget of {max_bytes} bytes holds no entry of {per_entry} bytes")
        n_slots = 4
        while n_slots < 2 * self.capacity:                # [2, 4) slots per entry: load factor <= 0.5, <= 16 bytes of table per entry
            n_slots *= 2
        self.slots = torch.zeros((n_slots,), dtype=torch.int32, device=dev)
        self.ent_hash = torch.empty((self.capacity,), dtype=torch.int64, device=dev)
        self.ent_k = torch.empty((self.capacity,), dtype=torch.int32, device=dev)
        self.ent_q = torch.empty((self.capacity, self.row_bytes), dtype=torch.uint8, device=dev)
        self.ent_mask = torch.empty((self.capacity, self.lq), dtype=torch.uint8, device=dev)
        self.ent_scores = torch.empty((self.capacity, self.npg), dtype=torch.float32, device=dev)
        self.n_entries = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.count = torch.zeros((1,), dtype=torch.int32, device=dev)              # view of the last call's miss count (its workspace word)
        self._scratch = {}
        self.c = L.EvdrQCache(self.slots.data_ptr(), n_slots, self.ent_hash.data_ptr(), self.ent_k.data_ptr(), self.ent_q.data_ptr(),
                              self.ent_mask.data_ptr(), self.ent_scores.data_ptr(), self.n_entries.data_ptr(), self.capacity,
                              self.row_bytes, self.lq, self.npg, hash_mask)
        self.nbytes = sum(t.numel() * t.element_size() for t in (self.slots, self.ent_hash, self.ent_k, self.ent_q, self.ent_mask, self.ent_scores))

    def scratch(self, nq: int):
        """(workspace, miss-count view) for batches of nq queries: zeroed once, then owned by the library's ticket protocol."""
        s = self._scratch.get(nq)
        if s is None:
            if len(self._scratch) > 8:
                self._scratch.clear()
            nbytes = int(L.load().evdr_qcache_workspace(nq))
            ws = torch.zeros((nbytes,), dtype=torch.uint8, device=self.dev)
            s = self._scratch[nq] = (ws, ws[nbytes - 256:nbytes - 252].view(torch.int32))
        return s

    def accepts(self, Q: torch.Tensor, npg: int) -> bool:
        return (Q.dim() == 3 and Q.shape[1] == self.lq and Q.shape[2] == D and Q.dtype == self.row_dtype and npg == self.npg
                and Q.device == self.dev and 2 <= self.lq <= 32)


def maxsim_forward_cached(cache: ScoreRowCache, Q: torch.Tensor, qplanes: torch.Tensor, qamax: Optional[torch.Tensor], pplanes: torch.Tensor,
                          pamax: Optional[torch.Tensor], qmask: Optional[torch.Tensor], tilemask: torch.Tensor,
                          pageflags: torch.Tensor) -> torch.Tensor:
    """A1 on prepared operands THROUGH the score-row cache (evdr_maxsim_fwd_prepared_cached): lookup + plan -> forward over the
    missing queries only -> exchange, three launches on the current stream behind ONE C call and no host synchronisation (which queries were missing is decided and consumed on the
    device).  Q is the caller's dense (nq, lq, 128) batch -- its bits are the key --, qplanes / qamax its planes as the forward
    takes them.  The result is, bit for bit, what `maxsim_forward_prepared` returns for the same call."""
    dev = _require_cuda(Q, qplanes, pplanes)
    nq, lq, _ = Q.shape
    nplanes, npg, lp, _ = pplanes.shape
    if not cache.accepts(Q, npg) or not Q.is_contiguous():
        raise RuntimeError("maxsim_forward_cached: the batch does not match the cache's geometry")
    out = torch.empty((nq, npg), dtype=torch.float32, device=dev)
    if nq == 0:
        return out
    qm = _mask_u8(qmask, (nq, lq), dev)
    ws, cache.count = cache.scratch(nq)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_maxsim_fwd_prepared_cached(
            L.C.byref(cache.c), L.ptr(Q), L.ptr(qplanes), L.ptr(pplanes), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), L.ptr(out),
            out.stride(0), nq, lp, nplanes, int(pplanes.stride(1)), int(pplanes.stride(0)), L.ptr(qamax), L.ptr(pamax), L.ptr(ws),
            ws.numel(), L.current_stream_handle(dev)))
    return out


def maxsim_backward(g: torch.Tensor, Q: torch.Tensor, qmask: Optional[torch.Tensor], pmask: Optional[torch.Tensor],
                    argmax: torch.Tensor, npg: int, lp: int) -> torch.Tensor:
    """A6: dP (np, lp, 128) fp32 from upstream g (nq, np) and the forward's argmax."""
    dev = _require_cuda(g, Q, argmax)
    nq, lq, d = Q.shape
    if d == D_WIDE:
        # the gather is linear in Q's columns: one launch per 128-column block, same arg-max and weights
        return torch.cat([maxsim_backward(g, Q[..., cb * D:(cb + 1) * D], qmask, pmask, argmax, npg, lp) for cb in (0, 1)], dim=-1)
    lib = L.load()
    gc = g.float().contiguous()
    Qc = Q.float().contiguous()
    qm = _mask_u8(qmask, (nq, lq), dev)
    pm = _mask_u8(pmask, (npg, lp), dev)
    dP = torch.empty((npg, lp, d), dtype=torch.float32, device=dev)
    with L.on(dev):
        L.check(lib.evdr_maxsim_bwd(L.ptr(gc), L.ptr(Qc), L.ptr(qm), L.ptr(pm), L.ptr(argmax), L.ptr(dP),
                                    nq, lq, npg, lp, d, L.current_stream_handle(dev)))
    return dP


def topk(scores: torch.Tensor, k: int, idx_base: int = 0,
         idx_map: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A8: per-row top-k (score desc, index asc), on device.  scores (nq, n) fp32, row-strided allowed.
    idx_map (nq, n) int32: the index each column reports, in any order along the row.  Of equal scores that straddle the cut, the
    lowest reported indices among equal scores are kept -- with or without a map."""
    dev = _require_cuda(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32 or scores.stride(1) != 1:
        raise RuntimeError("scores must be a 2-D fp32 tensor with unit column stride")
    if not (1 <= k <= L.EVDR_TOPK_MAX):
        raise ValueError(f"k={k} outside 1..{L.EVDR_TOPK_MAX}")
    nq, n = scores.shape
    lib = L.load()
    ts = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ti = torch.empty((nq, k), dtype=torch.int32, device=dev)
    im = None
    if idx_map is not None:
        if tuple(idx_map.shape) != (nq, n):
            raise RuntimeError("idx_map must have the shape of scores")
        im = idx_map.to(device=dev, dtype=torch.int32).contiguous()
    row_stride = scores.stride(0) if nq > 1 else max(n, 1)
    wsb = lib.evdr_topk_workspace(nq, n, k)          # > 0: few long rows, ranked by many workgroups in two levels
    ws = workspace(wsb, dev) if wsb else None
    with L.on(dev):
        L.check(lib.evdr_topk(L.ptr(scores), L.ptr(im), nq, n, max(row_stride, n), idx_base, k, L.ptr(ts), L.ptr(ti),
                              L.ptr(ws), wsb, L.current_stream_handle(dev)))
    return ts, ti


# ---- prefiltered top-k on an fp32 corpus (include/evdr.h "prefiltered top-k"; DESIGN.md "Prefiltered fp32 top-k") -----------------
PREFILTER_MAX_LQ = 32


def _check_prefilter_planes(qplanes: torch.Tensor, pplanes: torch.Tensor) -> None:
    if pplanes.dim() != 4 or pplanes.shape[0] == 1 or pplanes.dtype == torch.bfloat16:
        raise ValueError("prefilter: a bf16 corpus (one plane) has no cheaper first stage; the prefilter serves fp32 corpora "
                         "(fp16 hi/lo planes)")
    if pplanes.shape[0] != 2:
        raise NotImplementedError("prefilter: width-256 corpora (four planes) are not covered")
    if qplanes.dim() != 4 or qplanes.shape[0] != 2 or qplanes.dtype != torch.float16 or pplanes.dtype != torch.float16:
        raise RuntimeError("prefilter: query and page planes must both be (2, ., ., 128) fp16 hi/lo planes (`split_f32`)")
    if qplanes.shape[2] > PREFILTER_MAX_LQ:
        raise NotImplementedError(f"prefilter: queries of {qplanes.shape[2]} tokens; at most {PREFILTER_MAX_LQ} are covered")
    if pplanes.stride(3) != 1 or pplanes.stride(2) != D or not qplanes.is_contiguous():
        raise RuntimeError("planes must be dense in their last two dims (queries fully contiguous)")


def prefilter_corpus_bound(pplanes: torch.Tensor, tilemask: torch.Tensor, pageflags: torch.Tensor) -> torch.Tensor:
    """(2,) fp32 on the device: H, L = the largest hi / lo plane row norm over the valid patches of the corpus (scaled units,
    rounded up; pages flagged non-finite excluded) -- evdr_prefilter_corpus_bound."""
    dev = _require_cuda(pplanes, tilemask, pageflags)
    if pplanes.dim() != 4 or pplanes.shape[0] != 2 or pplanes.dtype != torch.float16:
        raise ValueError("prefilter_corpus_bound: fp16 hi/lo page planes (2, np, lp, 128) expected")
    _, npg, lp, _ = pplanes.shape
    bound = torch.empty((2,), dtype=torch.float32, device=dev)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_prefilter_corpus_bound(L.ptr(pplanes), L.ptr(tilemask), L.ptr(pageflags), npg, lp, int(pplanes.stride(1)),
                                                int(pplanes.stride(0)), L.ptr(bound), L.current_stream_handle(dev)))
    return bound


def prefilter_query_bound(qplanes: torch.Tensor, qamax: torch.Tensor, pamax: torch.Tensor, qmask: Optional[torch.Tensor],
                          bound: torch.Tensor) -> torch.Tensor:
    """(nq,) fp32: E_q, the per-query bound on |exact - coarse| score in real units (evdr_prefilter_query_bound)."""
    dev = _require_cuda(qplanes, bound)
    _, nq, lq, _ = qplanes.shape
    if lq > PREFILTER_MAX_LQ:
        raise NotImplementedError(f"prefilter: queries of {lq} tokens; at most {PREFILTER_MAX_LQ} are covered")
    eq = torch.empty((nq,), dtype=torch.float32, device=dev)
    qm = _mask_u8(qmask, (nq, lq), dev)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_prefilter_query_bound(L.ptr(qplanes.contiguous()), L.ptr(qm), nq, lq, L.ptr(qamax), L.ptr(pamax), L.ptr(bound),
                                               L.ptr(eq), L.current_stream_handle(dev)))
    return eq


def maxsim_forward_coarse(qplanes: torch.Tensor, qamax: torch.Tensor, pplanes: torch.Tensor, pamax: torch.Tensor,
                          qmask: Optional[torch.Tensor], tilemask: torch.Tensor, pageflags: torch.Tensor) -> torch.Tensor:
    """(nq, np) coarse scores of the prefilter: the hi planes alone, one fp16 product per k-step (evdr_maxsim_fwd_coarse)."""
    dev = _require_cuda(qplanes, pplanes)
    _check_prefilter_planes(qplanes, pplanes)
    _, nq, lq, _ = qplanes.shape
    _, npg, lp, _ = pplanes.shape
    out = torch.empty((nq, npg), dtype=torch.float32, device=dev)
    if nq == 0 or npg == 0:
        return out
    qm = _mask_u8(qmask, (nq, lq), dev)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_maxsim_fwd_coarse(L.ptr(qplanes), L.ptr(pplanes), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), out.data_ptr(),
                                           npg, nq, lq, npg, lp, int(pplanes.stride(1)), int(pplanes.stride(0)), L.ptr(qamax),
                                           L.ptr(pamax), L.current_stream_handle(dev)))
    return out


def maxsim_topk_prefilter(qplanes: torch.Tensor, qamax: torch.Tensor, pplanes: torch.Tensor, pamax: torch.Tensor,
                          qmask: Optional[torch.Tensor], tilemask: torch.Tensor, pageflags: torch.Tensor, bound: torch.Tensor, k: int,
                          capacity: int, idx_base: int = 0, stats: Optional[torch.Tensor] = None,
                          ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact two-stage top-k (evdr_maxsim_topk_prefilter): the same (scores, indices) as the exhaustive forward + `topk`, bit for
    bit.  stats: optional (nq + 1,) int32 output (per-query candidate counts, -1 = non-finite bound; then the fallback rows).
    ws: optional byte tensor of at least evdr_maxsim_topk_prefilter_workspace bytes (kept by the caller between calls)."""
    dev = _require_cuda(qplanes, pplanes)
    _check_prefilter_planes(qplanes, pplanes)
    if not (1 <= k <= L.EVDR_TOPK_MAX):
        raise ValueError(f"k={k} outside 1..{L.EVDR_TOPK_MAX}")
    if capacity < k:
        raise ValueError(f"prefilter capacity {capacity} < k = {k}")
    _, nq, lq, _ = qplanes.shape
    _, npg, lp, _ = pplanes.shape
    ts = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ti = torch.empty((nq, k), dtype=torch.int32, device=dev)
    if nq == 0:
        return ts, ti
    qm = _mask_u8(qmask, (nq, lq), dev)
    lib = L.load()
    wsb = lib.evdr_maxsim_topk_prefilter_workspace(nq, npg, int(capacity))
    if ws is None or ws.numel() < wsb:
        ws = workspace(wsb, dev)
    if stats is not None and (stats.dtype != torch.int32 or stats.numel() < nq + 1 or not stats.is_contiguous()):
        raise RuntimeError("stats must be a contiguous int32 tensor of nq + 1 entries")
    with L.on(dev):
        L.check(lib.evdr_maxsim_topk_prefilter(
            L.ptr(qplanes), L.ptr(pplanes), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), nq, lq, npg, lp, 2, int(pplanes.stride(1)),
            int(pplanes.stride(0)), L.ptr(qamax), L.ptr(pamax), L.ptr(bound), int(idx_base), int(k), int(capacity), L.ptr(ts), L.ptr(ti),
            L.ptr(stats), L.ptr(ws), ws.numel(), L.current_stream_handle(dev)))
    return ts, ti


# ---- candidate scoring and top-R selection (include/evdr.h "candidate scoring") ------------------------------------------
CANDIDATES_MAX_LQ = 32


def check_candidates(cand: torch.Tensor, nq: int, dev) -> int:
    """`cand` must be (nq, r) int32 on `dev`, 1 <= r <= EVDR_SELECT_MAX; returns r (no device work)."""
    if not isinstance(cand, torch.Tensor) or cand.dim() != 2 or cand.dtype != torch.int32 or cand.shape[0] != nq or cand.device != dev:
        raise ValueError(f"cand must be an (nq, r) = ({nq}, r) int32 tensor on {dev}; got "
                         f"{tuple(cand.shape) if isinstance(cand, torch.Tensor) else type(cand)} "
                         f"{getattr(cand, 'dtype', None)} on {getattr(cand, 'device', None)}")
    r = int(cand.shape[1])
    if not (1 <= r <= L.EVDR_SELECT_MAX):
        raise ValueError(f"r={r} candidates per query outside 1..{L.EVDR_SELECT_MAX}")
    return r


def maxsim_forward_candidates(qplanes: torch.Tensor, qamax: Optional[torch.Tensor], pplanes: torch.Tensor, pamax: Optional[torch.Tensor],
                              qmask: Optional[torch.Tensor], tilemask: torch.Tensor, pageflags: torch.Tensor, cand: torch.Tensor,
                              idx_base: int = 0, want_clean: bool = False, out: Optional[torch.Tensor] = None,
                              ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Scores of query q against the pages cand[q] names (evdr_maxsim_fwd_candidates): ((nq, r) fp32, cleaned lists or None).
    cand (nq, r) int32 holds page indices + idx_base; entries outside [idx_base, idx_base + np) are holes: -inf, nothing read.
    Planes as `maxsim_forward_prepared` (one bf16 plane or fp16 hi/lo planes).  want_clean: also return cand with holes set to -1.
    ws: optional byte tensor of at least evdr_maxsim_fwd_candidates_workspace bytes (kept by the caller between calls)."""
    dev = _require_cuda(qplanes, pplanes)
    if qplanes.dim() != 4 or pplanes.dim() != 4:
        raise RuntimeError("planes must be (planes, rows, tokens, 128)")
    nplanes, nq, lq, _ = qplanes.shape
    _, npg, lp, _ = pplanes.shape
    if nplanes == 4 or pplanes.shape[0] == 4:
        raise NotImplementedError("candidate scoring does not cover width-256 corpora (four planes)")
    if (nplanes not in (1, 2) or pplanes.shape[0] != nplanes or (nplanes == 2) != (qplanes.dtype == torch.float16)
            or pplanes.dtype != qplanes.dtype):
        raise RuntimeError("query and page planes must both be (1, ., ., 128) bf16 or both (2, ., ., 128) fp16 hi/lo")
    if lq > CANDIDATES_MAX_LQ:
        raise NotImplementedError(f"candidate scoring covers queries of at most {CANDIDATES_MAX_LQ} tokens; got {lq}")
    if pplanes.stride(3) != 1 or pplanes.stride(2) != D or not qplanes.is_contiguous():
        raise RuntimeError("planes must be dense in their last two dims (queries fully contiguous)")
    r = check_candidates(cand, nq, dev)
    cand = cand.contiguous()
    if out is None:
        out = torch.empty((nq, r), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (nq, r) or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != dev:
        raise RuntimeError("out must be an (nq, r) fp32 tensor with unit column stride on the planes' device")
    clean = torch.empty((nq, r), dtype=torch.int32, device=dev) if want_clean else None
    if nq == 0:
        return out, clean
    qm = _mask_u8(qmask, (nq, lq), dev)
    lib = L.load()
    wsb = lib.evdr_maxsim_fwd_candidates_workspace(nq, r)
    if ws is None or ws.numel() < wsb or ws.device != dev:
        ws = workspace(wsb, dev)
    with L.on(dev):
        L.check(lib.evdr_maxsim_fwd_candidates(
            L.ptr(qplanes), L.ptr(pplanes), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), L.ptr(cand), r, int(idx_base), L.ptr(out),
            out.stride(0) if nq > 1 else r, L.ptr(clean), nq, lq, npg, lp, nplanes, int(pplanes.stride(1)), int(pplanes.stride(0)),
            L.ptr(qamax), L.ptr(pamax), L.ptr(ws), ws.numel(), L.current_stream_handle(dev)))
    return out, clean


def select_topr(scores: torch.Tensor, r: int, idx_base: int = 0) -> torch.Tensor:
    """(nq, r) int32: per row of `scores` (nq, n) fp32 the r columns with the largest order key (`topk`'s: NaN first), ties at the
    cut towards the lower index, in ASCENDING index order (+ idx_base), padded with -1 when n < r (evdr_select_topr)."""
    dev = _require_cuda(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise RuntimeError("scores must be a 2-D fp32 tensor with unit column stride")
    if not (1 <= r <= L.EVDR_SELECT_MAX):
        raise ValueError(f"r={r} outside 1..{L.EVDR_SELECT_MAX}")
    nq, n = scores.shape
    out = torch.empty((nq, r), dtype=torch.int32, device=dev)
    if nq == 0:
        return out
    row_stride = scores.stride(0) if nq > 1 else max(n, 1)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_select_topr(L.ptr(scores), nq, n, max(row_stride, n), int(idx_base), int(r), L.ptr(out),
                                     L.current_stream_handle(dev)))
    return out


# ---- token alignment: best patch per query token and page heat maps (include/evdr.h "token alignment") ----------------
ALIGN_MAX_LQ = 32


def maxsim_align(qplanes: torch.Tensor, qamax: Optional[torch.Tensor], pplanes: torch.Tensor, pamax: Optional[torch.Tensor],
                 qmask: Optional[torch.Tensor], tilemask: torch.Tensor, pageflags: torch.Tensor, cand: torch.Tensor,
                 idx_base: int = 0, heat: bool = False):
    """The alignment of query q with the pages cand[q] names (evdr_maxsim_align, ONE launch): (sim (nq, r, lq) fp32, patch (nq, r, lq)
    int32[, heat (nq, r, lp) fp32]) by the rule `align_reference` states.  cand (nq, r) int32 holds page indices + idx_base; entries
    outside [idx_base, idx_base + np) are holes: sim = -inf, patch = -1, heat = -inf, nothing read.  Planes as
    `maxsim_forward_candidates` (one bf16 plane or fp16 hi/lo planes), queries of at most 32 tokens.  sim and patch are the same bits
    with and without heat.  No workspace, no host synchronisation."""
    dev = _require_cuda(qplanes, pplanes)
    if qplanes.dim() != 4 or pplanes.dim() != 4:
        raise RuntimeError("planes must be (planes, rows, tokens, 128)")
    nplanes, nq, lq, _ = qplanes.shape
    _, npg, lp, _ = pplanes.shape
    if nplanes == 4 or pplanes.shape[0] == 4:
        raise NotImplementedError("token alignment does not cover width-256 corpora (four planes)")
    if (nplanes not in (1, 2) or pplanes.shape[0] != nplanes or (nplanes == 2) != (qplanes.dtype == torch.float16)
            or pplanes.dtype != qplanes.dtype):
        raise RuntimeError("query and page planes must both be (1, ., ., 128) bf16 or both (2, ., ., 128) fp16 hi/lo")
    if not (1 <= lq <= ALIGN_MAX_LQ):
        raise NotImplementedError(f"token alignment covers queries of 1..{ALIGN_MAX_LQ} tokens; got {lq}")
    if pplanes.stride(3) != 1 or pplanes.stride(2) != D or not qplanes.is_contiguous():
        raise RuntimeError("planes must be dense in their last two dims (queries fully contiguous)")
    r = check_candidates(cand, nq, dev)
    cand = cand.contiguous()
    sim = torch.empty((nq, r, lq), dtype=torch.float32, device=dev)
    patch = torch.empty((nq, r, lq), dtype=torch.int32, device=dev)
    hm = torch.empty((nq, r, lp), dtype=torch.float32, device=dev) if heat else None
    if nq:
        qm = _mask_u8(qmask, (nq, lq), dev)
        lib = L.load()
        with L.on(dev):
            L.check(lib.evdr_maxsim_align(
                L.ptr(qplanes), L.ptr(pplanes), L.ptr(qm), L.ptr(tilemask), L.ptr(pageflags), L.ptr(cand), r, int(idx_base), L.ptr(sim),
                L.ptr(patch), L.ptr(hm), nq, lq, npg, lp, nplanes, int(pplanes.stride(1)), int(pplanes.stride(0)), L.ptr(qamax),
                L.ptr(pamax), L.current_stream_handle(dev)))
    return (sim, patch, hm) if heat else (sim, patch)


def align_reference(Q: torch.Tensor, qmask: Optional[torch.Tensor], P: torch.Tensor, pmask: Optional[torch.Tensor], cand: torch.Tensor,
                    idx_base: int = 0, heat: bool = False):
    """The alignment rule in plain torch, on CPU (or GPU) tensors: (sim (nq, r, lq) fp32, patch (nq, r, lq) int32
    [, heat (nq, r, lp) fp32]); dot products are accumulated in float64 and rounded once.  Q (nq, lq, d), P (np, lp, d) of any float
    dtype, qmask (nq, lq) / pmask (np, lp) or None = all valid, cand (nq, r) integer page indices + idx_base.  For entry (q, i) with
    page p = cand[q, i] - idx_base:
    - p outside [0, np) is a hole: sim = -inf, patch = -1, heat = -inf;
    - a page without a valid patch: sim = 0, patch = -1, heat = -inf (the forward's exact 0);
    - a pair the forward scores NaN -- a NaN / Inf element in a valid patch of p, or in ANY token of q (masked ones included), on a
      page with a valid patch: sim = NaN in every valid token, patch = -1, heat = NaN;
    - otherwise sim[n] = max_m (pmask[p, m] ? Q[q, n] . P[p, m] : -1e4) with patch[n] the FIRST index attaining it, and heat[m] = the
      max over the valid tokens n of Q[q, n] . P[p, m] for a valid patch, -inf for a masked one (-inf everywhere without a valid token);
    - a masked query token always has sim = 0, patch = -1."""
    nq, lq, _ = Q.shape
    npg, lp, _ = P.shape
    dev = Q.device
    r = cand.shape[1]
    qm = torch.ones((nq, lq), dtype=torch.bool, device=dev) if qmask is None else qmask.to(dev).bool()
    pm = torch.ones((npg, lp), dtype=torch.bool, device=dev) if pmask is None else pmask.to(dev).bool()
    Qd, Pd = Q.double(), P.to(dev).double()
    fin_p = torch.isfinite(Pd).all(-1)                                   # (np, lp)
    page_bad = (~fin_p & pm).any(-1)
    has = pm.any(-1)
    q_bad = ~torch.isfinite(Qd).all(-1).all(-1)                          # (nq,)
    ninf = float("-inf")
    sim = torch.full((nq, r, lq), ninf, dtype=torch.float64, device=dev)
    patch = torch.full((nq, r, lq), -1, dtype=torch.int64, device=dev)
    hm = torch.full((nq, r, lp), ninf, dtype=torch.float64, device=dev)
    local = cand.to(dev).long() - int(idx_base)
    for q in range(nq):
        for i in range(r):
            p = int(local[q, i])
            if p < 0 or p >= npg:
                continue
            tv = qm[q]
            if not bool(has[p]):
                sim[q, i] = 0.0
                continue
            if bool(page_bad[p]) or bool(q_bad[q]):
                sim[q, i] = torch.where(tv, torch.full_like(sim[q, i], float("nan")), torch.zeros_like(sim[q, i]))
                hm[q, i] = float("nan")
                continue
            # (lq, lp), every product summed on its own by the same reduction (a matrix product may sum a row differently depending on
            # where it stands, and identical patch rows must tie exactly); only masked rows hold a non-finite element here
            dots = (Qd[q][:, None, :] * torch.nan_to_num(Pd[p], nan=0.0, posinf=0.0, neginf=0.0)[None, :, :]).sum(-1)
            filled = torch.where(pm[p][None, :], dots, torch.full_like(dots, -1e4))
            v, a = filled.max(dim=1), filled.argmax(dim=1)               # argmax: the first index of the maximum
            sim[q, i] = torch.where(tv, v.values, torch.zeros_like(v.values))
            patch[q, i] = torch.where(tv, a, torch.full_like(a, -1))
            if bool(tv.any()):
                col = dots[tv].max(dim=0).values
                hm[q, i] = torch.where(pm[p], col, torch.full_like(col, ninf))
    out = (sim.float(), patch.to(torch.int32))
    return out + (hm.float(),) if heat else out


def hard_patch(sim: torch.Tensor, patch: torch.Tensor) -> torch.Tensor:
    """(nq, r) int32 from an alignment's (sim, patch): the patch of the valid token with the largest sim, the lowest such patch among
    tokens that tie -- the first index of the heat map's maximum (max over patches of max over tokens = max over tokens of max over
    patches), i.e. the hard token of mainv3_iter_liscore_QA_hardtoken.py:413-417, as long as some valid product reaches the masked
    patches' -1e4.  -1 for holes, pages without a valid patch, queries without a valid token and NaN pairs (their patch is -1
    throughout).  Plain torch on the tensors' device, no read-back."""
    ok = patch >= 0
    s = torch.where(ok, sim, torch.full_like(sim, float("-inf")))
    top = s.max(dim=-1, keepdim=True).values
    big = torch.iinfo(torch.int32).max
    pick = torch.where(ok & (s == top), patch, torch.full_like(patch, big)).min(dim=-1).values
    return torch.where(pick == big, torch.full_like(pick, -1), pick).to(torch.int32)


def _order_key(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> int32 keys in evdr_topk's order (csrc/topk.hip): a larger key ranks earlier, -0.0 == +0.0, every NaN is the
    greatest key (NaN scores rank first, like torch.topk)."""
    u = x.contiguous().view(torch.int32)
    key = torch.where(u < 0, u ^ 0x7FFFFFFF, u)
    key = torch.where(u == -2147483648, torch.zeros_like(key), key)
    return torch.where(torch.isnan(x), torch.full_like(key, 2147483647), key)


def topk_with_ties(scores: torch.Tensor, k: int, to_host: bool = False, have=None):
    """`topk` plus what a ranking by another tie rule needs: for every row whose k-th score is shared by columns that did
    NOT make the cut (score desc, index asc keeps the lowest indices), ALL columns that rank at or above the k-th one.

    The reference hands every score to trec_eval (mainv2_iter_distill_infonce.py:311-317), which breaks ties by docid
    DESCENDING; a device cut by index ascending would hand it a different candidate set whenever equal scores straddle
    rank k.  With the extra columns the metric layer sees every candidate that can appear in ANY top-k under ANY tie
    rule, so its result equals the all-pairs evaluation for every cut-off <= k.  Candidates are counted on the kernel's own
    order keys (NaN = greatest, -0 = +0), so a row whose top-k holds NaNs is cut where the kernel cut it.
    Returns (top_scores, top_idx, extra) with extra = {row: (column indices int64, their scores fp32)} as host numpy
    arrays -- empty when no tie is cut.  to_host=True: top_scores / top_idx come back as numpy arrays too, through ONE
    device-to-host copy that also carries the per-row candidate counts (a second copy only when a tie was cut).
    `have` = (top_scores, top_idx) of `topk(scores, k)` when the caller has run it already."""
    ts, ti = have if have is not None else topk(scores, k)
    extra = {}
    nq, n = scores.shape
    count = None
    if nq and n > k:
        key = _order_key(scores)
        kth = _order_key(ts[:, k - 1:k])
        count = (key >= kth).sum(dim=1, dtype=torch.int32)
    if to_host:
        cols = [ts.view(torch.int32), ti] + ([count[:, None]] if count is not None else [])
        host = torch.cat(cols, dim=1).cpu().numpy()                                # the one copy (and the one sync)
        ts_h, ti_h = host[:, :k].view("float32"), host[:, k:2 * k]
        cut = (host[:, 2 * k] > k).nonzero()[0] if count is not None else ()
    else:
        cut = (count > k).nonzero().flatten().cpu().numpy() if count is not None else ()
    if len(cut):
        rows = torch.as_tensor(cut, device=scores.device, dtype=torch.int64)
        sel = key[rows] >= kth[rows]                                               # (m, n)
        rc = sel.nonzero()
        packed = torch.stack([rows[rc[:, 0]].to(torch.int32), rc[:, 1].to(torch.int32),
                              scores[rows][sel].contiguous().view(torch.int32)]).cpu().numpy()
        r_all, c_all, s_all = packed[0], packed[1].astype("int64"), packed[2].view("float32")
        starts = (r_all[1:] != r_all[:-1]).nonzero()[0] + 1                        # nonzero() lists row-major: rows are contiguous runs
        for a, b in zip([0, *starts.tolist()], [*starts.tolist(), len(r_all)]):
            extra[int(r_all[a])] = (c_all[a:b], s_all[a:b])
    return (ts_h, ti_h, extra) if to_host else (ts, ti, extra)


# ---- document-level search: page scores collapsed to documents (include/evdr.h "document-level search") ---------------
DOC_BLOCK = L.EVDR_DOC_BLOCK          # evdr_doc_max: documents per workgroup
DOC_ROWS = L.EVDR_DOC_ROWS            # ... query rows per workgroup
DOC_LONG = L.EVDR_DOC_LONG            # ... pages from which a document takes a wave instead of a lane


def doc_lists(doc_of_page: torch.Tensor, n_docs: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(members (nm,) int32, offsets (n_docs + 1,) int32): the CSR lists of `evdr_doc_max` from one document id per column.  Document d
    owns members[offsets[d] : offsets[d + 1]], its columns in ASCENDING order (a stable sort by document); columns whose id lies
    outside [0, n_docs) -- -1 = "no document" -- are dropped.  Plain torch on the tensor's device (CPU tensors too), no read-back."""
    if not isinstance(doc_of_page, torch.Tensor) or doc_of_page.dim() != 1 or doc_of_page.dtype.is_floating_point or doc_of_page.dtype == torch.bool:
        raise ValueError(f"doc_of_page must be a 1-D integer tensor; got {tuple(getattr(doc_of_page, 'shape', ()))} "
                         f"{getattr(doc_of_page, 'dtype', None)}")
    n_docs = int(n_docs)
    if not (0 <= n_docs <= 2 ** 31 - 1):
        raise ValueError(f"n_docs={n_docs} outside 0..2^31 - 1")
    d = doc_of_page.long()
    cols = ((d >= 0) & (d < n_docs)).nonzero().flatten()
    dd = d[cols]
    order = torch.sort(dd, stable=True).indices
    counts = torch.bincount(dd, minlength=n_docs)[:n_docs]
    offsets = torch.zeros((n_docs + 1,), dtype=torch.int64, device=d.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return cols[order].to(torch.int32).contiguous(), offsets.to(torch.int32)


def _check_doc_block(scores, members, offsets, idx_map):
    dev = _require_cuda(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise RuntimeError("scores must be a 2-D fp32 tensor with unit column stride")
    for name, t in (("members", members), ("offsets", offsets)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-D int32 tensor on {dev}; got {tuple(getattr(t, 'shape', ()))} "
                             f"{getattr(t, 'dtype', None)} on {getattr(t, 'device', None)}")
    if offsets.shape[0] < 1:
        raise ValueError("offsets must hold n_docs + 1 entries")
    nq, n = scores.shape
    if idx_map is not None and (not isinstance(idx_map, torch.Tensor) or tuple(idx_map.shape) != (n,) or idx_map.dtype != torch.int32
                                or idx_map.device != dev or not idx_map.is_contiguous()):
        raise ValueError(f"idx_map must be a contiguous (n,) = ({n},) int32 tensor on {dev}")
    row_stride = max(scores.stride(0) if nq > 1 else n, n, 1)
    return dev, nq, n, int(members.shape[0]), int(offsets.shape[0]) - 1, row_stride


def _doc_out(out, shapes, dev, what):
    if out is None:
        return tuple(torch.empty(s, dtype=dt, device=dev) for s, dt in shapes)
    if len(out) != len(shapes) or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(s) or t.dtype != dt or t.device != dev
                                      or not t.is_contiguous() for t, (s, dt) in zip(out, shapes)):
        raise ValueError(f"out must be {what}, contiguous, on {dev}")
    return tuple(out)


def doc_max(scores: torch.Tensor, members: torch.Tensor, offsets: torch.Tensor, idx_map: Optional[torch.Tensor] = None, idx_base: int = 0,
            out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per (row, document) the best score and the page attaining it (evdr_doc_max, ONE launch): (doc_scores (nq, n_docs) fp32, doc_best
    (nq, n_docs) int32) by the rule `doc_max_reference` states.  scores (nq, n) fp32, row-strided allowed; members / offsets: the CSR
    lists of `doc_lists` (columns of the block; any order inside a document, duplicates and out-of-range holes allowed); a column
    reports (idx_map[col] if idx_map is given else col) + idx_base.  out=(doc_scores, doc_best): preallocated, dense."""
    dev, nq, n, nm, n_docs, row_stride = _check_doc_block(scores, members, offsets, idx_map)
    ds, db = _doc_out(out, (((nq, n_docs), torch.float32), ((nq, n_docs), torch.int32)), dev, "(doc_scores (nq, n_docs) fp32, doc_best (nq, n_docs) int32)")
    if nq and n_docs:
        with L.on(dev):
            L.check(L.load().evdr_doc_max(L.ptr(scores), L.ptr(members), L.ptr(offsets), L.ptr(idx_map), nq, n, row_stride, nm, n_docs,
                                          int(idx_base), L.ptr(ds), n_docs, L.ptr(db), L.current_stream_handle(dev)))
    return ds, db


def doc_topk(scores: torch.Tensor, members: torch.Tensor, offsets: torch.Tensor, k: int, idx_map: Optional[torch.Tensor] = None,
             idx_base: int = 0, out=None, ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The top-k documents of every row of a score block (evdr_doc_topk: `doc_max`, `topk` over the documents, the best pages):
    (top_scores (nq, k) fp32, top_doc (nq, k) int32, top_page (nq, k) int32) by the rule `doc_reference` states -- key descending,
    document id ascending, (-inf, -1, -1) padding.  Operands as `doc_max`.  out=(top_scores, top_doc, top_page): preallocated;
    ws: optional byte tensor of at least evdr_doc_topk_workspace bytes (kept by the caller between calls)."""
    dev, nq, n, nm, n_docs, row_stride = _check_doc_block(scores, members, offsets, idx_map)
    if not (1 <= k <= L.EVDR_TOPK_MAX):
        raise ValueError(f"k={k} outside 1..{L.EVDR_TOPK_MAX}")
    ts, td, tp = _doc_out(out, (((nq, k), torch.float32), ((nq, k), torch.int32), ((nq, k), torch.int32)), dev,
                          "(top_scores (nq, k) fp32, top_doc (nq, k) int32, top_page (nq, k) int32)")
    if nq:
        lib = L.load()
        wsb = lib.evdr_doc_topk_workspace(nq, n_docs)
        if ws is None or ws.numel() < wsb or ws.device != dev:
            ws = workspace(wsb, dev)
        with L.on(dev):
            L.check(lib.evdr_doc_topk(L.ptr(scores), L.ptr(members), L.ptr(offsets), L.ptr(idx_map), nq, n, row_stride, nm, n_docs,
                                      int(idx_base), int(k), L.ptr(ts), L.ptr(td), L.ptr(tp), L.ptr(ws), ws.numel(),
                                      L.current_stream_handle(dev)))
    return ts, td, tp


def collapse_topk(scores: torch.Tensor, page: torch.Tensor, k: int, doc: Optional[torch.Tensor] = None,
                  doc_of_page: Optional[torch.Tensor] = None, idx_base: int = 0, out=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The top-k DISTINCT documents of every row of a list (evdr_collapse_topk, ONE launch) by the rule `collapse_reference` states.
    scores (nq, r) fp32, row-strided allowed; page (nq, r) int32 reported page indices; the document of an entry from EXACTLY one of
    doc (nq, r) int32 -- any non-negative id, negative = hole -- and doc_of_page (np,) int32 with idx_base: doc_of_page[page - idx_base],
    entries outside [idx_base, idx_base + np) are holes.  1 <= r <= 4096, 1 <= k <= 128.  The result does not depend on the order of
    the list.  out=(top_scores, top_doc, top_page): preallocated."""
    if (doc is None) == (doc_of_page is None):
        raise ValueError("collapse_topk takes exactly one of doc= (a document id per entry) and doc_of_page= (a document id per page)")
    dev = _require_cuda(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise RuntimeError("scores must be a 2-D fp32 tensor with unit column stride")
    nq, r = scores.shape
    if not (1 <= r <= L.EVDR_SELECT_MAX):
        raise ValueError(f"r={r} entries per row outside 1..{L.EVDR_SELECT_MAX}")
    if not (1 <= k <= L.EVDR_TOPK_MAX):
        raise ValueError(f"k={k} outside 1..{L.EVDR_TOPK_MAX}")
    for name, t in (("page", page), ("doc", doc)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (nq, r) or t.dtype != torch.int32 or t.device != dev):
            raise ValueError(f"{name} must be an (nq, r) = ({nq}, {r}) int32 tensor on {dev}; got {tuple(getattr(t, 'shape', ()))} "
                             f"{getattr(t, 'dtype', None)} on {getattr(t, 'device', None)}")
    if doc_of_page is not None and (not isinstance(doc_of_page, torch.Tensor) or doc_of_page.dim() != 1 or doc_of_page.dtype != torch.int32
                                    or doc_of_page.device != dev):
        raise ValueError(f"doc_of_page must be a 1-D int32 tensor on {dev}; got {tuple(getattr(doc_of_page, 'shape', ()))} "
                         f"{getattr(doc_of_page, 'dtype', None)} on {getattr(doc_of_page, 'device', None)}")
    ts, td, tp = _doc_out(out, (((nq, k), torch.float32), ((nq, k), torch.int32), ((nq, k), torch.int32)), dev,
                          "(top_scores (nq, k) fp32, top_doc (nq, k) int32, top_page (nq, k) int32)")
    if nq == 0:
        return ts, td, tp
    page = page.contiguous()
    doc = None if doc is None else doc.contiguous()
    npg = 0
    if doc_of_page is not None:
        doc_of_page = doc_of_page.contiguous()
        npg = int(doc_of_page.shape[0])
        if npg == 0:                                     # no page has a document: every entry is a hole (the C call wants a pointer)
            doc_of_page = torch.full((1,), -1, dtype=torch.int32, device=dev)
    with L.on(dev):
        L.check(L.load().evdr_collapse_topk(L.ptr(scores), L.ptr(page), L.ptr(doc), L.ptr(doc_of_page), npg, int(idx_base), nq, r,
                                            max(scores.stride(0) if nq > 1 else r, r), int(k), L.ptr(ts), L.ptr(td), L.ptr(tp),
                                            L.current_stream_handle(dev)))
    return ts, td, tp


_DOC_ABSENT = -2 ** 63


def _key64(scores: torch.Tensor) -> torch.Tensor:
    """fp32 -> evdr_topk's order key as an int64 in 0 .. 2^32 - 1, and -1 for -inf ("absent")."""
    key = _order_key(scores.float()).long() + 2 ** 31
    return torch.where(scores == float("-inf"), torch.full_like(key, -1), key)


def _key64_to_float(key: torch.Tensor) -> torch.Tensor:
    """The float of an order key (csrc/topk.hip, key_to_float): -0.0 has become +0.0, every NaN one NaN."""
    u = torch.where(key >= 2 ** 31, key - 2 ** 31, 2 ** 32 - 1 - key)
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


def _doc_words(key: torch.Tensor, reported: torch.Tensor) -> torch.Tensor:
    """(key, reported page index) -> one int64 whose maximum is the largest key and, among equal keys, the LOWEST reported index
    (compared as unsigned 32-bit): the kernels' (key << 32 | ~reported), shifted by 2^63 to fit a signed word.  key -1 -> absent."""
    return torch.where(key >= 0, (key - 2 ** 31) * 2 ** 32 + (0xFFFFFFFF - (reported & 0xFFFFFFFF)), torch.full_like(key, _DOC_ABSENT))


def _doc_unwords(word: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(key or -1, reported page index as int32 value or -1) of `_doc_words` words."""
    has = word != _DOC_ABSENT
    hi = torch.div(word, 2 ** 32, rounding_mode="floor")
    page = 0xFFFFFFFF - (word - hi * 2 ** 32)
    page = torch.where(page >= 2 ** 31, page - 2 ** 32, page)
    return torch.where(has, hi + 2 ** 31, torch.full_like(hi, -1)), torch.where(has, page, torch.full_like(page, -1))


def _rank_docs(key: torch.Tensor, doc: torch.Tensor, page: torch.Tensor, k: int):
    """Rows of per-document (key, -1 = absent; document id; best page), all (nq, m) int64 -> the first k present documents by (key
    descending, document id ascending), padded with (-inf, -1, -1)."""
    nq, m = key.shape
    dev = key.device
    ts = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev)
    td = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    tp = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    if nq == 0 or m == 0:
        return ts, td, tp
    by_doc = torch.sort(doc, dim=1, stable=True).indices
    by_key = torch.sort(torch.gather(key, 1, by_doc), dim=1, descending=True, stable=True).indices
    order = torch.gather(by_doc, 1, by_key)[:, :k]
    kk = torch.gather(key, 1, order)
    real = kk >= 0
    c = order.shape[1]
    ts[:, :c] = torch.where(real, _key64_to_float(kk.clamp_min(0)), ts[:, :c])
    td[:, :c] = torch.where(real, torch.gather(doc, 1, order), torch.full_like(kk, -1)).to(torch.int32)
    tp[:, :c] = torch.where(real, torch.gather(page, 1, order), torch.full_like(kk, -1)).to(torch.int32)
    return ts, td, tp


def doc_max_reference(scores: torch.Tensor, doc_of_col: torch.Tensor, n_docs: int, reported: Optional[torch.Tensor] = None):
    """The per-document half of the rule in plain torch, on CPU (or GPU) tensors: (doc_scores (nq, n_docs) fp32,
    doc_best (nq, n_docs) int32).  scores (nq, n); doc_of_col (n,) the document of each column, outside [0, n_docs) = none;
    reported (n,) the page index each column reports (default: the column).  A document's score is the float of the largest order
    key -- evdr_topk's: NaN first, -0 = +0 -- among its columns that are not -inf, its best page the lowest reported index (compared
    as unsigned) attaining that key; (-inf, -1) without such a column."""
    nq, n = scores.shape
    dev = scores.device
    n_docs = int(n_docs)
    d = doc_of_col.to(dev).long()
    rep = torch.arange(n, device=dev) if reported is None else reported.to(dev).long()
    member = (d >= 0) & (d < n_docs)
    word = _doc_words(torch.where(member[None, :], _key64(scores), torch.full((1, 1), -1, dtype=torch.int64, device=dev)), rep[None, :])
    best = torch.full((nq, n_docs + 1), _DOC_ABSENT, dtype=torch.int64, device=dev)
    slot = torch.where(member, d, torch.full_like(d, n_docs))[None, :].expand(nq, n)
    best.scatter_reduce_(1, slot, word, "amax", include_self=True)
    key, page = _doc_unwords(best[:, :n_docs])
    ds = torch.where(key >= 0, _key64_to_float(key.clamp_min(0)), torch.full((1, 1), float("-inf"), dtype=torch.float32, device=dev))
    return ds, page.to(torch.int32)


def doc_reference(scores: torch.Tensor, doc_of_col: torch.Tensor, n_docs: int, k: int, reported: Optional[torch.Tensor] = None):
    """The document-search rule in plain torch, block form: (top_scores (nq, k) fp32, top_doc (nq, k) int32, top_page
    (nq, k) int32).  `doc_max_reference` per document, then the documents that are present by key descending, document id ascending,
    cut at k and padded with (-inf, -1, -1).  Scores are the floats of the winning keys: -0.0 comes back as +0.0."""
    ds, db = doc_max_reference(scores, doc_of_col, n_docs, reported)
    nq = scores.shape[0]
    ids = torch.arange(int(n_docs), device=scores.device)[None, :].expand(nq, int(n_docs))
    return _rank_docs(_key64(ds), ids, db.long(), k)


def collapse_reference(scores: torch.Tensor, doc: torch.Tensor, page: torch.Tensor, k: int):
    """The document-search rule in plain torch, list form: scores / doc / page (nq, r), one entry per listed page; a negative doc, or a
    score of -inf, is a hole.  Ids may be sparse.  Same outputs, order and padding as `doc_reference`; the result does not depend
    on the order of the entries."""
    nq, r = scores.shape
    dev = scores.device
    out = [torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev), torch.full((nq, k), -1, dtype=torch.int32, device=dev),
           torch.full((nq, k), -1, dtype=torch.int32, device=dev)]
    key = _key64(scores)
    for q in range(nq):
        dq = doc[q].to(dev).long()
        ids, inv = torch.unique(dq, return_inverse=True)                                # this row's documents, ascending
        word = _doc_words(torch.where(dq >= 0, key[q], torch.full_like(dq, -1)), page[q].to(dev).long())
        best = torch.full((ids.shape[0],), _DOC_ABSENT, dtype=torch.int64, device=dev)
        best.scatter_reduce_(0, inv, word, "amax", include_self=True)
        bk, bp = _doc_unwords(best)
        row = _rank_docs(bk[None], ids[None], bp[None], k)
        for o, x in zip(out, row):
            o[q] = x[0]
    return tuple(out)


def infonce_workspace(b: int, dev) -> torch.Tensor:
    """Workspace of the one-launch loss (`infonce_distill(..., ws=...)`): b per-row losses + the ticket word, ZEROED here.
    The caller owns it: one per object that issues the loss (a FusedStudent), never shared between streams that may run
    concurrently, alive as long as any captured graph holds its address.  Must not be made inside a stream capture (the
    zero fill would only be recorded, and the first replay would find an uninitialised ticket)."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("infonce_workspace() inside a stream capture: allocate the loss workspace before capturing")
    return torch.zeros((int(b) + 1,), dtype=torch.float32, device=dev)


def infonce_distill(score_s: torch.Tensor, score_t: torch.Tensor, temperature: float,
                    want_grad: bool, ws: Optional[torch.Tensor] = None,
                    loss_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """A5 (criterion.py:56-68) + its closed-form gradient in one pass.  Without `ws`: the stateless two-launch form (row
    kernel + mean kernel, scratch allocated per call).  With `ws` = `infonce_workspace(b, dev)` owned by the caller: ONE
    launch (the last workgroup reduces the row losses; same bits) -- the workspace carries a ticket word between calls, so
    it belongs to exactly one issuer.
    `loss_out`: where the scalar goes -- an fp32 scalar on the device, or a PINNED host scalar (hipHostMalloc memory is
    device-accessible under the same address: the kernel's one 4-byte store lands in host memory and a caller that wants
    float(loss) needs no device-to-host copy launch, only an event behind this kernel)."""
    dev = _require_cuda(score_s, score_t)
    if score_s.shape != score_t.shape or score_s.dim() != 2:
        raise RuntimeError("score_s and score_t must be (B, N) and equal-shaped")
    b, n = score_s.shape
    lib = L.load()
    ss = score_s.float().contiguous()
    st = score_t.float().contiguous()
    if loss_out is None:
        loss = torch.empty((), dtype=torch.float32, device=dev)
    else:
        ok = loss_out.dtype == torch.float32 and loss_out.numel() == 1 and (loss_out.device == dev or (not loss_out.is_cuda and loss_out.is_pinned()))
        if not ok:
            raise RuntimeError("infonce_distill: `loss_out` must be one fp32 element on the scores' device or in pinned host memory")
        loss = loss_out
    grad = torch.empty_like(ss) if want_grad else None
    stream = L.current_stream_handle(dev)
    if ws is None:
        row_loss = torch.empty((max(b, 1),), dtype=torch.float32, device=dev)
        with L.on(dev):
            L.check(lib.evdr_infonce_distill_fwd_bwd(L.ptr(ss), L.ptr(st), b, n, float(temperature), L.ptr(loss),
                                                     L.ptr(grad), L.ptr(row_loss), stream))
        return loss, grad
    if ws.dtype != torch.float32 or ws.device != dev or ws.numel() != b + 1 or not ws.is_contiguous():
        raise RuntimeError(f"infonce_distill: `ws` must be infonce_workspace({b}, {dev}) (got {tuple(ws.shape)} {ws.dtype} on {ws.device})")
    with L.on(dev):
        L.check(lib.evdr_infonce_distill_fwd_bwd_ws(L.ptr(ss), L.ptr(st), b, n, float(temperature), L.ptr(loss),
                                                    L.ptr(grad), L.ptr(ws), stream))
    return loss, grad


# ---- the pairwise ranking losses (csrc/pairloss.hip) -------------------------------------------------------------
PAIR_MAX_B, PAIR_MAX_N = 65535, 1 << 20          # launch limits of the two kernels (include/evdr.h)


def _check_pair_shape(who: str, b: int, n: int) -> None:
    if b < 1 or n < 1:
        raise RuntimeError(f"{who}: needs B >= 1 and N >= 1 (got B={b}, N={n})")
    if b > PAIR_MAX_B or n > PAIR_MAX_N:
        raise RuntimeError(f"{who}: shape beyond the launch limits (B={b} > {PAIR_MAX_B} or N={n} > {PAIR_MAX_N})")


def pair_loss_workspace(b: int, n: int, dev) -> torch.Tensor:
    """Workspace of `pairwise_distill` / `lambda_pairs` for (b, n) scores: one fp64 partial per workgroup and a ticket word, ZEROED here;
    O(b * n / 64) bytes.  The ticket makes it stateful: one per (stream, shape), never shared between streams that may run concurrently,
    and not to be made inside a stream capture."""
    _check_pair_shape("pair_loss_workspace", int(b), int(n))
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("pair_loss_workspace() inside a stream capture: allocate the workspace before capturing")
    return torch.zeros((int(L.load().evdr_pair_loss_workspace(int(b), int(n))),), dtype=torch.uint8, device=dev)


def _pair_inputs(who: str, dev, b: int, n: int, ws: Optional[torch.Tensor], *tensors):
    _check_pair_shape(who, b, n)                    # refused shapes raise here, before any allocation or launch
    for x in tensors:
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise RuntimeError(f"{who}: inputs must be contiguous fp32 tensors (got {x.dtype}, contiguous={x.is_contiguous()})")
    if ws is None:
        ws = pair_loss_workspace(b, n, dev)
    elif ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < L.load().evdr_pair_loss_workspace(b, n):
        raise RuntimeError(f"{who}: `ws` must be pair_loss_workspace({b}, {n}, {dev})")
    return ws


def pairwise_distill(score_s: torch.Tensor, score_t: torch.Tensor, want_grad: bool = True,
                     ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """criterion.pairwise_distillation_loss (RankNet) and d loss / d score_s in one launch, O(B * N) memory: the rule of
    `pairwise_distill_reference`.  score_s / score_t (B, N) contiguous fp32 on one cuda device; returns (loss scalar on the device,
    grad (B, N) or None).  `ws`: a `pair_loss_workspace(B, N, dev)` the caller keeps per stream; without it one is made per call."""
    dev = _require_cuda(score_s, score_t)
    if score_s.dim() != 2 or score_s.shape != score_t.shape:
        raise RuntimeError("pairwise_distill: score_s and score_t must be (B, N) and equal-shaped")
    b, n = int(score_s.shape[0]), int(score_s.shape[1])
    ws = _pair_inputs("pairwise_distill", dev, b, n, ws, score_s, score_t)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty_like(score_s) if want_grad else None
    with L.on(dev):
        L.check(L.load().evdr_pairwise_distill_fwd_bwd(L.ptr(score_s), L.ptr(score_t), b, n, L.ptr(loss), L.ptr(grad), L.ptr(ws), ws.numel(),
                                                       L.current_stream_handle(dev)))
    return loss, grad


def lambda_pairs(s_sorted: torch.Tensor, gain: torch.Tensor, disc: torch.Tensor, alpha: float, eps: float, want_grad: bool = True,
                 ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The pair sum of criterion.lambda_loss and its gradient w.r.t. s_sorted in one launch, O(B * N) memory: the rule of
    `lambda_reference`.  s_sorted / gain (B, N) in the teacher's descending order, disc (N), all contiguous fp32 on one cuda device (the
    caller sorts; the kernel does not).  Returns (loss scalar on the device, grad_sorted (B, N) or None)."""
    dev = _require_cuda(s_sorted, gain, disc)
    if s_sorted.dim() != 2 or gain.shape != s_sorted.shape or tuple(disc.shape) != (s_sorted.shape[1],):
        raise RuntimeError("lambda_pairs: s_sorted and gain must be (B, N) and equal-shaped, disc (N)")
    b, n = int(s_sorted.shape[0]), int(s_sorted.shape[1])
    ws = _pair_inputs("lambda_pairs", dev, b, n, ws, s_sorted, gain, disc)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty_like(s_sorted) if want_grad else None
    with L.on(dev):
        L.check(L.load().evdr_lambda_pairs_fwd_bwd(L.ptr(s_sorted), L.ptr(gain), L.ptr(disc), b, n, float(alpha), float(eps), L.ptr(loss),
                                                   L.ptr(grad), L.ptr(ws), ws.numel(), L.current_stream_handle(dev)))
    return loss, grad


def pairwise_distill_reference(score_s: torch.Tensor, score_t: torch.Tensor, row_chunk: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """The RankNet rule in float64 on the inputs' device, `row_chunk` values of i at a time (O(B * row_chunk * N) memory): with
    m_ij = s_i - s_j and y_ij = sigmoid(t_i - t_j),  loss = 1 / (B N^2) sum [ softplus(m_ij) - y_ij m_ij ]  and
    grad[b, i] = 2 / (B N^2) sum_j ( sigmoid(m_ij) - y_ij ).  Returns (loss, grad) in float64."""
    s, t = score_s.detach().double(), score_t.detach().double()
    b, n = s.shape
    loss = s.new_zeros(())
    grad = torch.zeros_like(s)
    for i0 in range(0, n, row_chunk):
        m = s[:, i0:i0 + row_chunk, None] - s[:, None, :]
        y = torch.sigmoid(t[:, i0:i0 + row_chunk, None] - t[:, None, :])
        loss = loss + (torch.nn.functional.softplus(m) - y * m).sum()
        grad[:, i0:i0 + row_chunk] = (torch.sigmoid(m) - y).sum(dim=2)
    pairs = float(b) * float(n) * float(n)
    return loss / pairs, grad * (2.0 / pairs)


def lambda_reference(s_sorted: torch.Tensor, gain: torch.Tensor, disc: torch.Tensor, alpha: float, eps: float,
                     row_chunk: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """The LambdaLoss pair rule in float64 on the inputs' device, `row_chunk` values of i at a time: with
    w_ij = 10 |gain_i - gain_j| |disc_i - disc_j| and D = N (N - 1) / 2 + eps,  loss = 1 / D sum_b sum_{i<j} w_ij softplus(-alpha (s_i - s_j))
    and grad[b, i] = 1 / D [ sum_{j>i} -alpha w_ij sigmoid(-alpha (s_i - s_j)) + sum_{j<i} alpha w_ji sigmoid(-alpha (s_j - s_i)) ].
    Returns (loss, grad w.r.t. s_sorted) in float64."""
    s, g, d = s_sorted.detach().double(), gain.detach().double(), disc.detach().double()
    b, n = s.shape
    idx = torch.arange(n, device=s.device)
    loss = s.new_zeros(())
    grad = torch.zeros_like(s)
    for i0 in range(0, n, row_chunk):
        sl = slice(i0, i0 + row_chunk)
        w = 10.0 * (g[:, sl, None] - g[:, None, :]).abs() * (d[None, sl, None] - d[None, None, :]).abs()
        x = alpha * (s[:, sl, None] - s[:, None, :])
        later = (idx[None, :] > idx[sl, None])[None]                    # j > i
        earlier = (idx[None, :] < idx[sl, None])[None]                  # j < i
        loss = loss + (w * torch.nn.functional.softplus(-x) * later).sum()
        grad[:, sl] = (-alpha * w * torch.sigmoid(-x) * later + alpha * w * torch.sigmoid(x) * earlier).sum(dim=2)
    denom = n * (n - 1) / 2.0 + eps
    return loss / denom, grad / denom


def l2norm_forward(x: torch.Tensor, rowmask: Optional[torch.Tensor], eps: float, want_planes: bool = False):
    """A4 fused with the row mask: y = m*x / (||m*x|| + eps) over the last (128-wide) dim; returns (y, norms), with
    `want_planes` (y, norms, planes, absmax word): the same launch also leaves y as the scorer's fp16 hi/lo planes
    (`l2norm_split`'s format, constant scale 2^14 since |y| <= 1), so that scoring y needs no absmax + split passes."""
    dev = _require_cuda(x)
    if x.shape[-1] != D or x.dtype != torch.float32:
        raise RuntimeError("l2norm kernel needs fp32 rows of width 128")
    lib = L.load()
    xc = x.contiguous()
    rows = xc.numel() // D
    y = torch.empty_like(xc)
    norm = torch.empty(xc.shape[:-1], dtype=torch.float32, device=dev)
    m = _mask_u8(rowmask, xc.shape[:-1], dev)
    if want_planes:
        planes = torch.empty((2,) + tuple(xc.shape), dtype=torch.float16, device=dev)
        amax = torch.empty((1,), dtype=torch.int32, device=dev)
        with L.on(dev):
            L.check(lib.evdr_l2norm_fwd_split(L.ptr(xc), L.ptr(m), rows, D, float(eps), L.ptr(y), L.ptr(norm), L.ptr(planes), L.ptr(amax),
                                              None, 1, L.current_stream_handle(dev)))
        return y, norm, planes, amax
    with L.on(dev):
        L.check(lib.evdr_l2norm_fwd(L.ptr(xc), L.ptr(m), rows, D, float(eps), L.ptr(y), L.ptr(norm),
                                    L.current_stream_handle(dev)))
    return y, norm


# ---- planes that were made together with an fp32 tensor (l2_normalize's output: utils/preprocess_data.py) -----------------
# The reference's step scores Psb = l2_normalize(Pbar * pmask) right after making it (mainv2_iter_distill_infonce.py:279,286):
# the normalise kernel leaves Psb's planes behind here, keyed on the tensor (address, layout, autograd version) and alive
# only as long as the tensor is; the scorer picks them up instead of running absmax + split over Psb again.
_DERIVED: "collections.OrderedDict" = collections.OrderedDict()
_DERIVED_MAX = 8


def tensor_key(t: Optional[torch.Tensor]):
    """Identity of a tensor's CONTENT for the per-tensor caches (derived planes here, prepared pages and query planes in
    evaluator/retrieval.py): storage address, layout and autograd version counter -- any in-place torch write changes it.
    None = not cacheable: tensors made under torch.inference_mode() track no version counter (`t._version` raises for them), so
    nothing is ever remembered for or looked up by such a tensor; the scorer then prepares its operands per call."""
    if t is None or t.is_inference():
        return None
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype, t.device.index, t._version)


def remember_planes(y: torch.Tensor, planes: torch.Tensor, amax: torch.Tensor) -> None:
    key = tensor_key(y)
    if key is None:
        return
    _DERIVED[key] = (weakref.ref(y, lambda _r, key=key: _DERIVED.pop(key, None)), planes, amax)
    while len(_DERIVED) > _DERIVED_MAX:
        _DERIVED.popitem(last=False)


def planes_of(t: torch.Tensor):
    """(planes, absmax word) made together with `t` (same storage, layout and autograd version: any in-place torch write
    since then changes the key), or None."""
    key = tensor_key(t)
    hit = _DERIVED.get(key) if key is not None else None
    if hit is None or hit[0]() is None:
        return None
    return hit[1], hit[2]


def l2norm_split(x: torch.Tensor, rowmask: Optional[torch.Tensor], eps: float,
                 pageflags: Optional[torch.Tensor] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """y = m*x / (||m*x|| + eps) emitted directly as the scorer's fp16 hi/lo planes (see `split_f32`): ((2, ..., 128) fp16,
    absmax word).  One kernel instead of normalise -> absmax -> split, and no fp32 copy of y in HBM.  With `pageflags`
    (x is (np, lp, 128)) non-finite unmasked rows are reported in their page's flag word on the way (`flag_nonfinite`)."""
    dev = _require_cuda(x)
    if x.shape[-1] != D or x.dtype != torch.float32:
        raise RuntimeError("l2norm kernel needs fp32 rows of width 128")
    lib = L.load()
    xc = x.contiguous()
    rows = xc.numel() // D
    if out is not None:                           # (planes, amax) of an earlier call, overwritten
        planes, amax = out
        if planes.shape != (2,) + tuple(xc.shape) or planes.dtype != torch.float16 or not planes.is_contiguous():
            raise RuntimeError("l2norm_split: `out` planes do not match x")
    else:
        planes = torch.empty((2,) + tuple(xc.shape), dtype=torch.float16, device=dev)
        amax = torch.empty((1,), dtype=torch.int32, device=dev)
    m = _mask_u8(rowmask, xc.shape[:-1], dev)
    with L.on(dev):
        L.check(lib.evdr_l2norm_fwd_split(L.ptr(xc), L.ptr(m), rows, D, float(eps), None, None, L.ptr(planes), L.ptr(amax),
                                          L.ptr(pageflags), int(xc.shape[-2]) if pageflags is not None else 1,
                                          L.current_stream_handle(dev)))
    return planes, amax


def l2norm_backward(gy: torch.Tensor, x: torch.Tensor, rowmask: Optional[torch.Tensor], norm: torch.Tensor,
                    eps: float) -> torch.Tensor:
    dev = _require_cuda(gy, x, norm)
    lib = L.load()
    gc, xc = gy.float().contiguous(), x.contiguous()
    rows = xc.numel() // D
    dx = torch.empty_like(xc)
    m = _mask_u8(rowmask, xc.shape[:-1], dev)
    with L.on(dev):
        L.check(lib.evdr_l2norm_bwd(L.ptr(gc), L.ptr(xc), L.ptr(m), L.ptr(norm), rows, D, float(eps), L.ptr(dx),
                                    L.current_stream_handle(dev)))
    return dx


def maxsim_backward_adamw(g: torch.Tensor, Q: torch.Tensor, qmask: Optional[torch.Tensor], pmask: Optional[torch.Tensor],
                          argmax: torch.Tensor, x: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                          lr: float, betas: Tuple[float, float], eps: float, weight_decay: float, step: int,
                          l2_eps: float = 1e-12, state: Optional[torch.Tensor] = None, next_planes=None,
                          pageflags: Optional[torch.Tensor] = None) -> None:
    """A6 + normalise/mask backward + AdamW in one launch, in place on x / exp_avg / exp_avg_sq (fp32, contiguous).
    `state` (see `adamw_state` / `adamw_advance`): bias corrections come from the device-side step counter instead of
    `step` -- what a HIP-graph replay of the step needs.  `next_planes` = (planes, amax) as `l2norm_split` returns them:
    the launch also leaves l2_normalize(pmask * x_new) there for the next forward (and reports non-finite updated rows in
    `pageflags`), so that the next step needs no normalise pass."""
    dev = _require_cuda(g, Q, argmax, x, exp_avg, exp_avg_sq)
    for t in (x, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != x.shape:
            raise RuntimeError("x / exp_avg / exp_avg_sq must be contiguous fp32 tensors of one shape")
    npg, lp, d = x.shape
    nq, lq, _ = Q.shape
    lib = L.load()
    gc, Qc = g.float().contiguous(), Q.float().contiguous()
    qm = _mask_u8(qmask, (nq, lq), dev)
    pm = _mask_u8(pmask, (npg, lp), dev)
    with L.on(dev):
        planes, amax = next_planes if next_planes is not None else (None, None)
        if planes is not None and (planes.shape != (2,) + tuple(x.shape) or planes.dtype != torch.float16 or not planes.is_contiguous()):
            raise RuntimeError("maxsim_backward_adamw: `next_planes` do not match x")
        L.check(lib.evdr_maxsim_bwd_adamw_planes(L.ptr(gc), L.ptr(Qc), L.ptr(qm), L.ptr(pm), L.ptr(argmax), L.ptr(x),
                                                 L.ptr(exp_avg), L.ptr(exp_avg_sq), nq, lq, npg, lp, d, float(lr),
                                                 float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                                                 float(l2_eps), L.ptr(state), L.ptr(planes), L.ptr(amax),
                                                 L.ptr(pageflags) if planes is not None else None,
                                                 L.current_stream_handle(dev)))
    for t in (x, exp_avg, exp_avg_sq):            # written through raw pointers: tell autograd (and version-keyed caches)
        torch.autograd.graph.increment_version(t)


def adamw_step(grad: torch.Tensor, x: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, lr: float,
               betas: Tuple[float, float], eps: float, weight_decay: float, step: int) -> None:
    """torch.optim.AdamW's update of ONE fp32 tensor in one pass (evdr_adamw_step), in place on x / exp_avg / exp_avg_sq;
    `step` counts this update.  All four tensors dense fp32 of one shape on one device."""
    dev = _require_cuda(grad, x, exp_avg, exp_avg_sq)
    for t in (grad, x, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != x.shape:
            raise RuntimeError("adamw_step: grad / x / exp_avg / exp_avg_sq must be contiguous fp32 tensors of one shape")
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_adamw_step(L.ptr(grad), L.ptr(x), L.ptr(exp_avg), L.ptr(exp_avg_sq), x.numel(), float(lr),
                                    float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                                    L.current_stream_handle(dev)))
    for t in (x, exp_avg, exp_avg_sq):
        torch.autograd.graph.increment_version(t)


def adamw_state(dev) -> torch.Tensor:
    """Zeroed device-side AdamW step counter {int64 step; float bc1; float bc2_sqrt} (16 bytes)."""
    return torch.zeros(2, dtype=torch.int64, device=dev)


def adamw_advance(state: torch.Tensor, betas: Tuple[float, float]) -> None:
    """step += 1 and refresh the bias corrections, on the device, on the current stream."""
    dev = _require_cuda(state)
    lib = L.load()
    with L.on(dev):
        L.check(lib.evdr_adamw_advance(L.ptr(state), float(betas[0]), float(betas[1]), L.current_stream_handle(dev)))


def maxsim_backward_q(g: torch.Tensor, P: torch.Tensor, qmask: Optional[torch.Tensor], pmask: Optional[torch.Tensor],
                      argmax: torch.Tensor, nq: int, lq: int) -> torch.Tensor:
    """A6, query side: dQ (nq, lq, 128) fp32 from upstream g (nq, np), the fp32 pages and the forward's argmax.
    Deterministic (per-segment partial sums added in a fixed order, no float atomics)."""
    dev = _require_cuda(g, P, argmax)
    npg, lp, d = P.shape
    if d == D_WIDE:
        return torch.cat([maxsim_backward_q(g, P[..., cb * D:(cb + 1) * D], qmask, pmask, argmax, nq, lq) for cb in (0, 1)], dim=-1)
    lib = L.load()
    gc, Pc = g.float().contiguous(), P.float().contiguous()
    qm = _mask_u8(qmask, (nq, lq), dev)
    pm = _mask_u8(pmask, (npg, lp), dev)
    dQ = torch.empty((nq, lq, d), dtype=torch.float32, device=dev)
    ws = workspace(lib.evdr_maxsim_bwd_q_workspace(nq, lq, npg, lp), dev)
    with L.on(dev):
        L.check(lib.evdr_maxsim_bwd_q(L.ptr(gc), L.ptr(Pc), L.ptr(qm), L.ptr(pm), L.ptr(argmax), L.ptr(dQ), nq, lq, npg, lp, d,
                                      L.ptr(ws), ws.numel(), L.current_stream_handle(dev)))
    return dQ
