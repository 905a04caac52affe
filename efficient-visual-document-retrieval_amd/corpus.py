"""Resident page corpus, per-shard top-k and the multi-GPU merge (SURVEY §8(d),(e); BASELINE.json config 4).

None of this exists in the reference (single process, whole corpus on one device, ranking on the host from a
dict of every score).  MI355X layout: the corpus is stored page-major in HBM as 16-bit planes (1 plane = a bf16
corpus, 2 planes = an fp32 corpus split into fp16 hi/lo), 263 680 B per 1030-patch page and plane, plus 4 B per
32-patch tile of packed mask; it is prepared once and stays resident (100 k pages = 26.4 GB of 288 GB).
Pages shard contiguously over ranks; queries are replicated; each rank scores its shard and keeps k
candidates per query; ONE all-gather of (nq, 2k) int32 words per rank (scores bit-cast next to global page
indices: 0.8 MB per rank at nq = 1024, k = 100) moves them; every rank merges with the same top-k kernel.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import ops


PREFILTER_CAPACITY = 4096          # default candidate capacity per query of topk(..., prefilter=True)


def shard_range(n_pages: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous shard [lo, hi) of rank `rank`: ceil-sized shards, the last ones may be short or empty."""
    per = (n_pages + world - 1) // world
    lo = min(rank * per, n_pages)
    return lo, min(lo + per, n_pages)


class PageSubset:
    """A set of pages of ONE PageCorpus to restrict searches to (`PageCorpus.subset`): `pages` is the strictly ascending (m,) int32
    list of LOCAL page indices on the corpus's device, `m` its length as a host int.  Immutable; valid for the corpus that made it
    only (same pages AND same idx_base: a `shard` view builds its own).  It holds the corpus's identity token, so a corpus allocated
    later at the same address is still another corpus."""

    __slots__ = ("pages", "m", "_identity", "_n_pages", "_idx_base")

    def __init__(self, pages: torch.Tensor, m: int, corpus: "PageCorpus"):
        self.pages = pages
        self.m = int(m)
        self._identity = corpus._identity
        self._n_pages = corpus.n_pages
        self._idx_base = corpus.idx_base

    def __len__(self) -> int:
        return self.m

    def belongs_to(self, corpus: "PageCorpus") -> bool:
        # views of one corpus share its token and idx_base = base + lo, so (token, idx_base, n_pages) names the page range
        return corpus._identity is self._identity and corpus.n_pages == self._n_pages and corpus.idx_base == self._idx_base


class PageDocuments:
    """Which document every page of ONE PageCorpus belongs to (`PageCorpus.documents`), as the document searches take it
    (DESIGN.md §4.13): `doc_of_page` (n_pages,) int32 -- GLOBAL document ids in [0, n_docs), -1 = no document --, the CSR lists
    `members` / `offsets` of `ops.doc_lists` and `n_docs` as a host int.  Built with a `PageSubset`, the lists index the subset's
    COLUMNS and `idx_map` is the subset's page list.  Immutable and tied to the corpus as a `PageSubset` is (identity token, n_pages,
    idx_base): a `shard()` view builds its own from its slice of the global tensor, and after an `append` it is rebuilt."""

    __slots__ = ("doc_of_page", "members", "offsets", "n_docs", "subset", "_identity", "_n_pages", "_idx_base")

    def __init__(self, doc_of_page: torch.Tensor, members: torch.Tensor, offsets: torch.Tensor, n_docs: int, corpus: "PageCorpus",
                 subset: Optional[PageSubset] = None):
        self.doc_of_page = doc_of_page
        self.members = members
        self.offsets = offsets
        self.n_docs = int(n_docs)
        self.subset = subset
        self._identity = corpus._identity
        self._n_pages = corpus.n_pages
        self._idx_base = corpus.idx_base

    @property
    def idx_map(self) -> Optional[torch.Tensor]:
        return None if self.subset is None else self.subset.pages

    def belongs_to(self, corpus: "PageCorpus") -> bool:
        return corpus._identity is self._identity and corpus.n_pages == self._n_pages and corpus.idx_base == self._idx_base


class PageCorpus:
    """One rank's prepared, HBM-resident slice of the page corpus."""

    def __init__(self, planes: torch.Tensor, tilemask: torch.Tensor, pageflags: torch.Tensor, idx_base: int = 0,
                 amax: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None):
        ok = planes.dim() == 4 and planes.shape[-1] == ops.D and (
            (planes.dtype == torch.bfloat16 and planes.shape[0] == 1) or
            (planes.dtype == torch.float16 and planes.shape[0] in (2, 4) and amax is not None) or
            (planes.dtype == ops.FP8 and planes.shape[0] == 1 and shift is not None and tuple(shift.shape) == (planes.shape[1],)))
        if not ok:
            raise RuntimeError("planes must be (1, np, lp, 128) bf16, (2, np, lp, 128) fp16 hi/lo, (4, np, lp, 128) fp16 hi/lo x two "
                               "column blocks (width 256: ops.split_wide), the fp16 forms with their absmax word, or (1, np, lp, 128) "
                               "float8_e4m3fn with its (np,) int32 per-page shifts (ops.quantize_fp8)")
        self.planes = planes
        self.amax = amax                     # absmax word of the fp32 tensor the fp16 planes were split from
        self.shift = shift                   # fp8 corpus: per-page power of two of the e4m3 bytes (ops.quantize_fp8)
        self.fp8 = planes.dtype == ops.FP8
        self.tilemask = tilemask
        self.pageflags = pageflags
        self.idx_base = int(idx_base)
        self.nplanes, self.n_pages, self.lp, _ = planes.shape
        if planes.stride(3) != 1 or planes.stride(2) != ops.D:
            raise RuntimeError("planes must be dense in their last two dims")
        self.p_stride, self.p_plane_stride = int(planes.stride(1)), int(planes.stride(0))
        self.device = planes.device
        self._ws: Optional[torch.Tensor] = None       # (nq, n_pages) score block of topk(), kept between calls (410 MB at 1024 x 100k)
        # bench.py: a list here makes topk() record a HIP-event pair around its MaxSim launch (on the launch stream) and append
        # it -- the scorer's own share of every TIMED step; the launches themselves are the ones every search issues
        self.score_events: Optional[list] = None
        # prefiltered top-k (topk(..., prefilter=True)): the corpus bound H, L -- computed on the first prefiltered call, shared with
        # shard() views (a corpus's bound holds for any subset of its pages) -- the call's workspace, and the last call's statistics
        self._bound_owner: "PageCorpus" = self
        self._pf_bound: Optional[torch.Tensor] = None
        self._pf_ws: Optional[torch.Tensor] = None
        self._pf_stats: Optional[torch.Tensor] = None
        self._cand_ws: Optional[torch.Tensor] = None  # workspace of score_candidates() / rerank(), kept between calls
        self._doc_ws: Optional[torch.Tensor] = None   # workspace of topk_docs(), kept between calls
        self._identity = object()                     # what a PageSubset is tied to; shard() views share their corpus's token
        # growable corpora (`empty`, `from_tensor(capacity=)`): the storage allocated for `capacity` pages, of which
        # the four tensors above view the first n_pages; None = the tensors above are all there is (capacity == n_pages)
        self.capacity = self.n_pages
        self._store: Optional[tuple] = None
        self._amax_word: Optional[int] = None         # the absmax word on the host, once `replace` has had to read it

    @classmethod
    def empty(cls, capacity: int, lp: int, dtype: torch.dtype, device, idx_base: int = 0, absmax: Optional[float] = None) -> "PageCorpus":
        """A corpus with room for `capacity` pages of `lp` patches and none in it yet (n_pages == 0): `append` fills it in place,
        `replace` overwrites pages, and the storage never moves, so `shard()` views and searches in flight stay valid.
        dtype: torch.bfloat16 (one bf16 plane), torch.float32 (fp16 hi/lo planes) or torch.float8_e4m3fn (e4m3 bytes + per-page shifts).
        absmax (torch.float32 only, required there, a finite float > 0): the bound on |x| the corpus is laid out for -- its bits become
        the absmax word, whose exponent fixes the power of two of every page's planes; an appended element of a higher binade is
        refused, elements far below it keep fewer lo-plane bits.  1.0 suits L2-normalised embeddings.
        Sharded use needs no more than this: a rank reserves its index range by capacity, `idx_base = rank * capacity`."""
        if dtype not in (torch.bfloat16, torch.float32, ops.FP8):
            raise ValueError(f"dtype must be torch.bfloat16, torch.float32 or torch.float8_e4m3fn; got {dtype}")
        if int(capacity) < 0 or not (1 <= int(lp) <= 65535):
            raise ValueError(f"capacity must be >= 0 and lp in 1..65535; got capacity={capacity}, lp={lp}")
        word = None
        if dtype == torch.float32:
            if absmax is None:
                raise ValueError("an fp32 corpus needs absmax=: the bound on |x| it is laid out for (1.0 suits L2-normalised embeddings)")
            word = torch.tensor([float(absmax)], dtype=torch.float32)
            if not (bool(torch.isfinite(word)) and float(word) > 0.0):
                raise ValueError(f"absmax must be a finite float > 0 (as fp32); got {absmax}")
            word = word.view(torch.int32)
        elif absmax is not None:
            raise ValueError("absmax= belongs to fp32 corpora (torch.float32): a bf16 corpus is a copy and an fp8 corpus scales per page")
        c = cls._reserve(int(capacity), int(lp), dtype, torch.device(device), idx_base, None if word is None else word.to(device))
        c._amax_word = None if word is None else int(word)
        return c

    @classmethod
    def _reserve(cls, capacity: int, lp: int, dtype: torch.dtype, dev, idx_base: int, amax: Optional[torch.Tensor]) -> "PageCorpus":
        nplanes, pdt = (2, torch.float16) if dtype == torch.float32 else (1, dtype)
        store = (torch.empty((nplanes, capacity, lp, ops.D), dtype=pdt, device=dev),
                 torch.empty((capacity, (lp + 31) // 32), dtype=torch.int32, device=dev),
                 torch.empty((capacity,), dtype=torch.int32, device=dev),
                 torch.empty((capacity,), dtype=torch.int32, device=dev) if dtype == ops.FP8 else None)
        c = cls(store[0][:, :0], store[1][:0], store[2][:0], idx_base, amax, None if store[3] is None else store[3][:0])
        c._store, c.capacity = store, capacity
        return c

    def _publish(self, n_pages: int) -> None:
        """The four views over the first n_pages pages of the storage."""
        planes, tilemask, pageflags, shift = self._store
        self.planes, self.tilemask, self.pageflags = planes[:, :n_pages], tilemask[:n_pages], pageflags[:n_pages]
        self.shift = None if shift is None else shift[:n_pages]
        self.n_pages = n_pages

    def _check_pages_in(self, P: torch.Tensor, pmask: Optional[torch.Tensor]) -> int:
        """Arguments of `append` / `replace` (before any device work); returns b, the number of pages."""
        if self.nplanes == 4:
            raise NotImplementedError("append() and replace() do not cover width-256 corpora")
        if not isinstance(P, torch.Tensor) or P.dim() != 3:
            raise ValueError(f"pages must be a (b, lp_src, d) tensor; got {tuple(getattr(P, 'shape', ()))}")
        b, lp_src, d = P.shape
        if lp_src > self.lp or not (1 <= d <= ops.D):
            raise ValueError(f"pages of {lp_src} patches x {d} columns do not fit a corpus of {self.lp} patches x <= {ops.D} columns")
        if self.nplanes == 1 and not self.fp8:
            if P.dtype != torch.bfloat16:
                raise RuntimeError("bf16 corpus needs bf16 pages (round them explicitly with .bfloat16(), or "
                                   "build the corpus from fp32 to score at fp32 accuracy)")
        elif P.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"an fp32 or fp8 corpus takes fp32, bf16 or fp16 pages; got {P.dtype}")
        if pmask is not None and tuple(pmask.shape) != (b, lp_src):
            raise ValueError(f"pmask shape {tuple(pmask.shape)} does not match the pages' {(b, lp_src)}")
        return int(b)

    def _storage(self) -> tuple:
        return self._store if self._store is not None else (self.planes, self.tilemask, self.pageflags, self.shift)

    def append(self, P: torch.Tensor, pmask: Optional[torch.Tensor] = None) -> int:
        """Add the pages P (b, lp_src <= lp, d <= 128) behind the last one, in place; returns the GLOBAL index of the first new page.
        Shorter pages are padded with masked zero patches, narrower ones with zero columns.  A bf16 corpus takes bf16 pages only; fp32
        and fp8 corpora take fp32, bf16 or fp16.  Capacity and arguments are checked on the host first; then ONE launch
        (evdr_corpus_ingest) on the current stream prepares the pages behind n_pages, and only then are they published (n_pages
        advanced, planes / tilemask / pageflags / shift re-sliced): a search never sees a half-written page, `shard()` views made
        earlier keep their page range, `PageSubset`s made earlier belong to the shorter corpus and must be rebuilt.
        bf16 and fp8 appends never synchronise.  An fp32 append reads one status word back: an element of a higher binade than the
        corpus's absmax raises ValueError, nothing is published and the next append reuses the slots.  The prefilter bound is dropped
        and recomputed by the next prefiltered call.  b = 0 is a no-op."""
        return self._append(P, pmask, self._check_pages_in(P, pmask), self.nplanes == 2)

    def _append(self, P: torch.Tensor, pmask: Optional[torch.Tensor], b: int, check_range: bool) -> int:
        if self.n_pages + b > self.capacity:
            raise ValueError(f"append of {b} pages to {self.n_pages} exceeds the capacity of {self.capacity} (reserve it with "
                             f"PageCorpus.empty or from_tensor(capacity=); a shard() view cannot grow)")
        first = self.idx_base + self.n_pages
        if b == 0:
            return first
        dev = ops._require_cuda(P)
        planes, tilemask, pageflags, shift = self._storage()
        status = torch.zeros((1,), dtype=torch.int32, device=dev) if check_range else None
        ops.corpus_ingest(P, pmask, planes, tilemask, pageflags, shift, self.amax, first_page=self.n_pages, status=status)
        if status is not None and int(status.item()) & 1:
            raise ValueError("append: a finite element lies in a higher binade than the absmax this fp32 corpus is laid out for; "
                             "nothing was added (lay the corpus out for a larger absmax)")
        self._bound_owner._pf_bound = None
        self._publish(self.n_pages + b)
        return first

    def _check_replace_list(self, pages: torch.Tensor, b: int) -> torch.Tensor:
        """The index list of `replace` / `replace_pooled`, validated on the host: (b,) int64 LOCAL indices on the CPU."""
        if not isinstance(pages, torch.Tensor) or pages.dim() != 1 or pages.dtype.is_floating_point or pages.dtype == torch.bool \
                or pages.shape[0] != b:
            raise ValueError(f"pages must be a (b,) = ({b},) integer tensor of global page indices; got "
                             f"{tuple(getattr(pages, 'shape', ()))} {getattr(pages, 'dtype', None)}")
        local = pages.to(device="cpu", dtype=torch.int64) - self.idx_base
        if bool(((local < 0) | (local >= self.n_pages)).any()):
            raise ValueError(f"replace: an index outside this corpus's pages [{self.idx_base}, {self.idx_base + self.n_pages})")
        if torch.unique(local).numel() != b:
            raise ValueError("replace: duplicate page indices")
        return local

    def replace(self, pages: torch.Tensor, P: torch.Tensor, pmask: Optional[torch.Tensor] = None) -> None:
        """Overwrite the pages `pages` names -- (b,) integer GLOBAL indices, on the CPU or the device -- with P (b, lp_src <= lp,
        d <= 128), in place (evdr_corpus_ingest through its destination list).  A set-up step that validates on the host (a device
        list is read back): every index owned by this corpus and below n_pages, no duplicates; for an fp32 corpus also the range of P
        against the absmax word, so that a refused call leaves the corpus bit-unchanged.  n_pages does not change: views and
        `PageSubset`s of the corpus stay valid and see the new content; the prefilter bound is dropped."""
        b = self._check_pages_in(P, pmask)
        local = self._check_replace_list(pages, b)
        if b == 0:
            return
        dev = ops._require_cuda(P)
        if self.nplanes == 2:
            if self._amax_word is None:
                self._amax_word = int(self.amax.item())
            e = (self._amax_word >> 23) & 0xFF
            top = 2.0 ** ((e if e not in (0, 255) else 141) - 126)            # first value above the corpus's binade (evdr_h2_shift)
            a = P.float().abs()
            if a.numel() and float(torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max()) >= top:
                raise ValueError("replace: a finite element lies in a higher binade than the absmax this fp32 corpus is laid out for; "
                                 "nothing was written")
        planes, tilemask, pageflags, shift = self._storage()
        ops.corpus_ingest(P, pmask, planes, tilemask, pageflags, shift, self.amax, dst_pages=local.to(device=dev, dtype=torch.int32))
        self._bound_owner._pf_bound = None

    # ---- pooled corpora -------------------------------------------------------------------------------
    def _check_pooled_in(self, P, pmask, members, offsets) -> int:
        """Arguments of `append_pooled` / `replace_pooled` (before any device work); returns b, the number of pages."""
        if self.nplanes == 4:
            raise NotImplementedError("append_pooled() and replace_pooled() do not cover width-256 corpora")
        b, _lp_src, _d, ls, _m, _per_page = ops._check_pool_args(P, pmask, members, offsets)
        if ls > self.lp:
            raise ValueError(f"pooled pages of {ls} tokens do not fit a corpus of {self.lp} patches")
        return b

    @classmethod
    def from_pooled(cls, P: torch.Tensor, pmask: Optional[torch.Tensor], members: torch.Tensor, offsets: torch.Tensor,
                    dtype: Optional[torch.dtype] = None, normalize: bool = True, idx_base: int = 0, capacity: Optional[int] = None,
                    absmax: Optional[float] = None) -> "PageCorpus":
        """A corpus of the POOLED pages of P (n, lp_src, d <= 128) fp32 / bf16 / fp16: page length ls = the number of groups, token t
        of a page the mean of the valid patches group t names (CSR lists `members`, `offsets`, shared by all pages or one row per
        page: `ops.pool_pages`, `ops.pool_groups_windows`, `ops.pool_groups_grid`), l2-renormalised unless normalize=False.  ONE fused
        launch (evdr_corpus_pool_ingest) pools and prepares every page; the pooled pages are never materialised, and the corpus is
        bit for bit `PageCorpus.empty(...)` + `append(*ops.pool_pages(...))` (bf16: of the pooled values rounded by `.bfloat16()`).
        The first stage of `TwoStageRetriever` over the same pages at 1 / f of the tokens; everything a corpus does works on it.
        dtype: torch.bfloat16, torch.float32 (fp16 hi/lo planes) or torch.float8_e4m3fn; default bf16 for bf16 pages, else float32.
        absmax (torch.float32 only): the bound the planes are laid out for, as in `empty`; defaults to 1.0 when normalize=True (pooled
        tokens are unit vectors) and is required with normalize=False; a pooled element of a higher binade raises ValueError (one
        status word read back; bf16 and fp8 never synchronise).  capacity (>= n): room for `append_pooled` / `append`.
        Groupings are validated as `ops._check_pool_args` says: shared ones on the host (CPU tensors: no synchronisation), per-page
        ones for shape and dtype only -- they are never read back, the kernel clamps their offsets."""
        b, _lp_src, _d, ls, _m, _per_page = ops._check_pool_args(P, pmask, members, offsets)
        if dtype is None:
            dtype = torch.bfloat16 if P.dtype == torch.bfloat16 else torch.float32
        if dtype not in (torch.bfloat16, torch.float32, ops.FP8):
            raise ValueError(f"dtype must be torch.bfloat16, torch.float32 or torch.float8_e4m3fn; got {dtype}")
        if dtype == torch.float32 and absmax is None:
            if not normalize:
                raise ValueError("an fp32 corpus of unnormalised pooled pages needs absmax=: the bound on |x| it is laid out for")
            absmax = 1.0
        capacity = b if capacity is None else int(capacity)
        if capacity < b:
            raise ValueError(f"capacity {capacity} < the {b} pages given")
        if dtype != torch.float32 and absmax is not None:
            raise ValueError("absmax= belongs to fp32 corpora (torch.float32): a bf16 corpus is a copy and an fp8 corpus scales per page")
        dev = ops._require_cuda(P)
        c = cls.empty(capacity, ls, dtype, dev, idx_base, absmax)
        c._append_pooled(P, pmask, members, offsets, normalize, b, "from_pooled")
        return c

    def append_pooled(self, P: torch.Tensor, pmask: Optional[torch.Tensor], members: torch.Tensor, offsets: torch.Tensor,
                      normalize: bool = True) -> int:
        """`append` of the pooled pages of P (`from_pooled`'s rule; ls <= lp, shorter pages are padded with masked zero tokens)
        without materialising them; returns the GLOBAL index of the first new page.  Capacity and arguments are checked on the host
        first, then ONE launch (evdr_corpus_pool_ingest) prepares the pages behind n_pages and only then are they published, exactly
        as `append`: bf16 and fp8 never synchronise, fp32 reads one status word back and raises ValueError -- nothing published, the
        slots reused -- when a pooled element lies above the corpus's binade.  The prefilter bound is dropped.  b = 0 is a no-op."""
        return self._append_pooled(P, pmask, members, offsets, normalize, self._check_pooled_in(P, pmask, members, offsets), "append_pooled")

    def _append_pooled(self, P, pmask, members, offsets, normalize: bool, b: int, who: str) -> int:
        if self.n_pages + b > self.capacity:
            raise ValueError(f"{who} of {b} pages to {self.n_pages} exceeds the capacity of {self.capacity} (reserve it with "
                             f"PageCorpus.empty or from_pooled(capacity=); a shard() view cannot grow)")
        first = self.idx_base + self.n_pages
        if b == 0:
            return first
        dev = ops._require_cuda(P)
        planes, tilemask, pageflags, shift = self._storage()
        status = torch.zeros((1,), dtype=torch.int32, device=dev) if self.nplanes == 2 else None
        ops.corpus_pool_ingest(P, pmask, members, offsets, planes, tilemask, pageflags, shift, self.amax, first_page=self.n_pages,
                               status=status, normalize=normalize)
        if status is not None and int(status.item()) & 1:
            raise ValueError(f"{who}: a finite pooled element lies in a higher binade than the absmax this fp32 corpus is laid out "
                             f"for; nothing was added (lay the corpus out for a larger absmax)")
        self._bound_owner._pf_bound = None
        self._publish(self.n_pages + b)
        return first

    def replace_pooled(self, pages: torch.Tensor, P: torch.Tensor, pmask: Optional[torch.Tensor], members: torch.Tensor,
                       offsets: torch.Tensor, normalize: bool = True) -> None:
        """`replace` of the pages `pages` names ((b,) integer GLOBAL indices) with the pooled pages of P.  A set-up step like
        `replace`: the index list is validated on the host (owned, below n_pages, distinct).  bf16 and fp8 corpora: one fused launch
        through the destination list, no further synchronisation.  An fp32 corpus must stay bit-unchanged when the call is refused,
        so there the pooled pages are made first (`ops.pool_pages`), their range is checked against the absmax word in torch, and
        `replace` writes them -- the same bits as the fused launch.  n_pages does not change; the prefilter bound is dropped."""
        b = self._check_pooled_in(P, pmask, members, offsets)
        local = self._check_replace_list(pages, b)
        if b == 0:
            return
        dev = ops._require_cuda(P)
        if self.nplanes == 2:
            self.replace(pages, *ops.pool_pages(P, pmask, members, offsets, normalize))
            return
        planes, tilemask, pageflags, shift = self._storage()
        ops.corpus_pool_ingest(P, pmask, members, offsets, planes, tilemask, pageflags, shift, self.amax,
                               dst_pages=local.to(device=dev, dtype=torch.int32), normalize=normalize)
        self._bound_owner._pf_bound = None

    # ---- clustered corpora: pooled corpora whose groups are found on the device ------------------------------
    @classmethod
    def from_clustered(cls, P: torch.Tensor, pmask: Optional[torch.Tensor], ls: Optional[int] = None, factor: Optional[int] = None,
                       iters: int = 8, dtype: Optional[torch.dtype] = None, normalize: bool = True, idx_base: int = 0,
                       capacity: Optional[int] = None, absmax: Optional[float] = None, chunk_pages: int = 4096) -> "PageCorpus":
        """`from_pooled` with the groups found by similarity: every page's valid patches are clustered into at most `ls` groups (or
        `factor` patches per group, ls = ceil(lp_src / factor); exactly one of the two) by `ops.cluster_pages` with `iters`
        iterations, and the pooled pages are stored -- bit for bit `from_pooled(P, pmask, *ops.cluster_pages(P, pmask, ...), ...)`.
        The pages are taken `chunk_pages` at a time: one clustering launch and one fused pooling launch per chunk, appended into
        storage reserved once, so the lists never exist for more than a chunk.  dtype / normalize / idx_base / capacity / absmax as in
        `from_pooled`; the sync rule is `append_pooled`'s (bf16 and fp8 never read anything back, fp32 one status word per chunk)."""
        b, _lp_src, _d, ls, iters = ops._check_cluster_args(P, pmask, ls, factor, iters)
        if int(chunk_pages) < 1:
            raise ValueError(f"chunk_pages must be >= 1; got {chunk_pages}")
        if dtype is None:
            dtype = torch.bfloat16 if P.dtype == torch.bfloat16 else torch.float32
        if dtype not in (torch.bfloat16, torch.float32, ops.FP8):
            raise ValueError(f"dtype must be torch.bfloat16, torch.float32 or torch.float8_e4m3fn; got {dtype}")
        if dtype == torch.float32 and absmax is None:
            if not normalize:
                raise ValueError("an fp32 corpus of unnormalised pooled pages needs absmax=: the bound on |x| it is laid out for")
            absmax = 1.0
        capacity = b if capacity is None else int(capacity)
        if capacity < b:
            raise ValueError(f"capacity {capacity} < the {b} pages given")
        if dtype != torch.float32 and absmax is not None:
            raise ValueError("absmax= belongs to fp32 corpora (torch.float32): a bf16 corpus is a copy and an fp8 corpus scales per page")
        dev = ops._require_cuda(P)
        c = cls.empty(capacity, ls, dtype, dev, idx_base, absmax)
        c._append_clustered(P, pmask, ls, iters, normalize, int(chunk_pages), "from_clustered")
        return c

    def append_clustered(self, P: torch.Tensor, pmask: Optional[torch.Tensor], iters: int = 8, normalize: bool = True,
                         chunk_pages: int = 4096) -> int:
        """`append_pooled` of P's pages clustered into ls = this corpus's page length groups (`from_clustered`'s rule); returns the
        GLOBAL index of the first new page.  Capacity and arguments are checked on the host first; the pages are then clustered,
        pooled and published `chunk_pages` at a time, with `append_pooled`'s sync rule."""
        if self.nplanes == 4:
            raise NotImplementedError("append_clustered() does not cover width-256 corpora")
        if self.lp > ops.CLUSTER_MAX_LS:
            raise ValueError(f"append_clustered clusters into ls = lp groups; lp = {self.lp} exceeds {ops.CLUSTER_MAX_LS}")
        _b, _lp_src, _d, ls, iters = ops._check_cluster_args(P, pmask, self.lp, None, iters)
        if int(chunk_pages) < 1:
            raise ValueError(f"chunk_pages must be >= 1; got {chunk_pages}")
        return self._append_clustered(P, pmask, ls, iters, normalize, int(chunk_pages), "append_clustered")

    def _append_clustered(self, P, pmask, ls: int, iters: int, normalize: bool, chunk_pages: int, who: str) -> int:
        b = int(P.shape[0])
        if self.n_pages + b > self.capacity:
            raise ValueError(f"{who} of {b} pages to {self.n_pages} exceeds the capacity of {self.capacity} (reserve it with "
                             f"PageCorpus.empty or from_clustered(capacity=); a shard() view cannot grow)")
        first = self.idx_base + self.n_pages
        if b:
            ops._require_cuda(P)
        for lo in range(0, b, chunk_pages):
            Pc, mc = P[lo:lo + chunk_pages], None if pmask is None else pmask[lo:lo + chunk_pages]
            members, offsets = ops.cluster_pages(Pc, mc, ls=ls, iters=iters)
            self._append_pooled(Pc, mc, members, offsets, normalize, int(Pc.shape[0]), who)
        return first

    @classmethod
    def from_tensor(cls, P: torch.Tensor, pmask: Optional[torch.Tensor] = None, idx_base: int = 0,
                    dtype: Optional[torch.dtype] = None, capacity: Optional[int] = None) -> "PageCorpus":
        """P (np, lp, d): at d = 128 bf16 is kept as one plane and anything else is treated as fp32 and split into fp16 hi/lo; narrower
        embeddings ride on zero columns; 129 <= d <= 256 is kept as four planes (fp16 hi/lo x two column blocks, any input dtype).
        dtype=torch.float8_e4m3fn (opt-in, d <= 128) stores the pages as e4m3 bytes with one power of two per page (ops.quantize_fp8):
        half the bytes of a bf16 corpus, scored by the fp8 MFMA; queries of any float dtype are quantised per call the same way.
        capacity (>= np, d <= 128): the same corpus -- planes, words and absmax word bit for bit -- in storage with room for `capacity`
        pages, for `append` (see `empty`); prepared by one fused launch instead of the passes below."""
        if dtype is not None and dtype != ops.FP8:
            raise ValueError(f"dtype must be None or torch.float8_e4m3fn; got {dtype}")
        if capacity is not None:
            return cls._from_tensor_reserved(P, pmask, idx_base, dtype, int(capacity))
        dev = ops._require_cuda(P)
        npg, lp, _ = P.shape
        if dtype == ops.FP8:
            if P.shape[-1] > ops.D:
                raise NotImplementedError(f"fp8 corpora cover embeddings of width <= {ops.D}; got width {P.shape[-1]}")
            src = ops.pad_width(P if P.dtype in (torch.float32, torch.bfloat16, torch.float16) else P.float()).contiguous()
            tilemask, pageflags = ops.pack_pmask(pmask, npg, lp, dev)
            ops.flag_nonfinite(src, pmask, pageflags)          # on the SOURCE pages: NaN / Inf in a valid patch -> NaN column
            x8, shift = ops.quantize_fp8(src, max(lp, 1))
            return cls(x8[None], tilemask, pageflags, idx_base, shift=shift)
        P = ops.pad_width(P)
        if P.shape[-1] == ops.D_WIDE:
            planes, amax = ops.split_wide(P)
        else:
            planes, amax = (P.contiguous()[None], None) if P.dtype == torch.bfloat16 else ops.split_f32(P)
        tilemask, pageflags = ops.pack_pmask(pmask, npg, lp, dev)
        for hi in range(planes.shape[0] // 2 if planes.shape[0] > 1 else 1):       # the hi plane of every column block
            ops.flag_nonfinite(planes[hi], pmask, pageflags)                       # once per corpus: NaN / Inf pages score NaN (evdr.h)
        return cls(planes, tilemask, pageflags, idx_base, amax)

    @classmethod
    def _from_tensor_reserved(cls, P: torch.Tensor, pmask: Optional[torch.Tensor], idx_base: int, dtype: Optional[torch.dtype],
                              capacity: int) -> "PageCorpus":
        npg, lp, d = P.shape
        if d > ops.D:
            raise NotImplementedError(f"from_tensor(capacity=) does not cover width-256 corpora; got width {d}")
        if capacity < npg:
            raise ValueError(f"capacity {capacity} < the {npg} pages given")
        dev = ops._require_cuda(P)
        kind = ops.FP8 if dtype == ops.FP8 else (torch.bfloat16 if P.dtype == torch.bfloat16 else torch.float32)
        if P.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            P = P.float()
        amax = None
        if kind == torch.float32:
            # the absmax word from_tensor's split derives: bits of max |x| over the FINITE elements (0 when there is none), taken
            # a slab of pages at a time so that the temporaries stay small; no synchronisation
            m = torch.zeros((), dtype=torch.float32, device=dev)
            step = max(1, (1 << 26) // max(lp * d, 1))
            for s in range(0, npg, step):
                a = P[s:s + step].float().abs()
                if a.numel():
                    m = torch.maximum(m, torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max())
            amax = m.reshape(1).view(torch.int32)
        c = cls._reserve(capacity, max(lp, 1), kind, dev, idx_base, amax)
        c._append(P, pmask, c._check_pages_in(P, pmask), False)       # the word was taken from these very pages: nothing to read back
        return c

    def shard(self, lo: int, hi: int) -> "PageCorpus":
        """Pages [lo, hi) of this corpus as a corpus of their own (views, nothing copied)."""
        view = PageCorpus(self.planes[:, lo:hi], self.tilemask[lo:hi], self.pageflags[lo:hi], self.idx_base + lo, self.amax,
                          None if self.shift is None else self.shift[lo:hi])
        view._bound_owner = self._bound_owner
        view._identity = self._identity
        return view

    # ---- page subsets ----------------------------------------------------------------------------------
    def subset(self, allow: Optional[torch.Tensor] = None, pages: Optional[torch.Tensor] = None) -> PageSubset:
        """The pages a search may return, as a `PageSubset` for `score(..., subset=)`, `topk(..., subset=)` and
        `ShardedRetriever.search(..., subset=)` -- exactly one of:
        allow: (n_pages,) bool mask over THIS corpus's pages (True = searchable);
        pages: integer tensor of GLOBAL page indices in any order; duplicates are merged and entries this corpus does not own are
               dropped, so the same global list can be handed to every shard.
        Deleting pages without re-preparing the corpus is `corpus.subset(allow=~deleted)`.
        A set-up step in plain torch (nonzero / unique) that reads the list length back ONCE -- the only host synchronisation of the
        feature; searches with the subset never synchronise.  Width-256 corpora are not covered; an fp8 corpus does not make subsets
        of its own -- it scores a raw list (`score_pages`) and follows the exact corpus's subset as the first stage of
        `TwoStageRetriever.search(..., subset=)`."""
        if (allow is None) == (pages is None):
            raise ValueError("subset() takes exactly one of allow= (bool mask over this corpus's pages) and pages= (global page indices)")
        self._check_subset_kind()
        dev = self.device
        if allow is not None:
            if not isinstance(allow, torch.Tensor) or allow.dtype != torch.bool or tuple(allow.shape) != (self.n_pages,):
                raise ValueError(f"allow must be an (n_pages,) = ({self.n_pages},) bool tensor; got "
                                 f"{tuple(getattr(allow, 'shape', ()))} {getattr(allow, 'dtype', None)}")
            local = allow.to(dev).nonzero().flatten()
        else:
            if not isinstance(pages, torch.Tensor) or pages.dim() != 1 or pages.dtype.is_floating_point or pages.dtype == torch.bool:
                raise ValueError(f"pages must be a 1-D integer tensor of global page indices; got "
                                 f"{tuple(getattr(pages, 'shape', ()))} {getattr(pages, 'dtype', None)}")
            g = pages.to(device=dev, dtype=torch.int64)
            g = g[(g >= self.idx_base) & (g < self.idx_base + self.n_pages)] - self.idx_base
            local = torch.unique(g)                       # sorted ascending, duplicates merged
        local = local.to(torch.int32).contiguous()
        return PageSubset(local, int(local.shape[0]), self)

    def _check_subset_kind(self) -> None:
        if self.fp8:
            raise NotImplementedError("subset(), score(subset=) and topk(subset=) are not available on an fp8 corpus: score a page list "
                                      "with score_pages(), or search with TwoStageRetriever(fp8, exact).search(..., subset=) and the "
                                      "exact corpus's subset")
        if self.nplanes == 4:
            raise NotImplementedError("page subsets do not cover width-256 corpora")

    def _check_subset(self, subset: PageSubset) -> None:
        """Arguments of a subset search (before any device work)."""
        self._check_subset_kind()
        if not isinstance(subset, PageSubset) or not subset.belongs_to(self):
            raise ValueError("this subset was made by another corpus (another tensor, or a view of the same pages with a different "
                             "idx_base): build it with this corpus's subset()")

    def _query_planes(self, Q: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        if self.fp8:                                      # e4m3 bytes + one shift per query, quantised per call (one launch)
            if Q.shape[-1] > ops.D:
                raise NotImplementedError(f"an fp8 corpus holds embeddings of width <= {ops.D}; got queries of width {Q.shape[-1]}")
            return ops.quantize_fp8(Q, max(Q.shape[1], 1))
        if self.nplanes == 4:                             # a 256-wide corpus: queries of 129..256 columns, any dtype
            if ops.kernel_width(Q.shape[-1]) != ops.D_WIDE:
                raise RuntimeError(f"this corpus holds embeddings of width 129..256; got queries of width {Q.shape[-1]}")
            return ops.split_wide(ops.pad_width(Q))
        if Q.shape[-1] != ops.D:
            Q = ops.pad_width(Q)
            if Q.shape[-1] != ops.D:
                raise RuntimeError(f"this corpus holds embeddings of width <= 128; got queries of width {Q.shape[-1]}")
        if self.nplanes == 1:
            if Q.dtype != torch.bfloat16:
                raise RuntimeError("bf16 corpus needs bf16 queries (round them explicitly with .bfloat16(), or "
                                   "build the corpus from fp32 to score at fp32 accuracy)")
            return Q.contiguous()[None], None
        return ops.split_f32(Q)

    def score(self, Q: torch.Tensor, qmask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              out_col: int = 0, qplanes=None, subset: Optional[PageSubset] = None) -> torch.Tensor:
        """(nq, n_pages) fp32 scores of this shard; with `out` given, written into out[:, out_col:out_col+n_pages].
        `qplanes` = (planes, absmax word) of Q from `ops.split_f32`, when the caller has split the batch already (a training
        step scores the same queries against teacher and student).
        subset (`subset()`): (nq, m) scores of the subset's pages only, columns in list order (ascending page index) -- the bits the
        full call gives those columns, at the cost of m pages."""
        if subset is not None:
            self._check_subset(subset)
        dev = ops._require_cuda(Q)
        nq, lq, _ = Q.shape
        if subset is not None:
            if out is None:
                out = torch.empty((nq, subset.m), dtype=torch.float32, device=dev)
                out_col = 0
            view = out[:, out_col:out_col + subset.m]
            if nq == 0 or subset.m == 0:
                return view
            qp, qamax = qplanes if (qplanes is not None and self.nplanes == 2) else self._query_planes(Q)
            return ops.maxsim_forward_pages(qp, qamax, self.planes, self.amax, qmask, self.tilemask, self.pageflags, subset.pages,
                                            out=view)
        if out is None:
            out = torch.empty((nq, self.n_pages), dtype=torch.float32, device=dev)
            out_col = 0
        view = out[:, out_col:out_col + self.n_pages]
        if nq == 0 or self.n_pages == 0:
            return view
        qp, qamax = qplanes if (qplanes is not None and self.nplanes == 2 and not self.fp8) else self._query_planes(Q)
        if self.fp8:
            ops.maxsim_forward_fp8(qp, qamax, self.planes[0], self.shift, qmask, self.tilemask, self.pageflags, out=out, out_col=out_col)
            return view
        ops.maxsim_forward_prepared(qp, qamax, self.planes, self.amax, qmask, self.tilemask, self.pageflags, out=out,
                                    out_col=out_col)
        return view

    def _check_pages(self, pages: torch.Tensor) -> int:
        """Arguments of a raw page-list call (before any device work); returns m, the list length."""
        if self.nplanes == 4:
            raise NotImplementedError("page lists do not cover width-256 corpora")
        if not isinstance(pages, torch.Tensor) or pages.dim() != 1 or pages.dtype != torch.int32 or pages.device != self.device:
            raise ValueError(f"pages must be an (m,) int32 tensor of local page indices on {self.device}; got "
                             f"{tuple(getattr(pages, 'shape', ()))} {getattr(pages, 'dtype', None)} on {getattr(pages, 'device', None)}")
        return int(pages.shape[0])

    def score_pages(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], pages: torch.Tensor,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(nq, m) fp32 scores of the pages the raw list `pages` names: (m,) int32 LOCAL page indices on this corpus's device, in any
        order, duplicates each scored; column i = page pages[i], the bits `score` gives that pair for the same query batch; an entry
        outside [0, n_pages) is a hole: a column of -inf, nothing read.  fp8 corpora (evdr_maxsim_fwd_fp8_pages),
        bf16 and fp32 corpora (evdr_maxsim_fwd_pages, §4.7); not width-256 corpora.  With `out` (nq, >= m) fp32 given, the scores land
        in out[:, :m].  The cost of m pages; no host synchronisation."""
        m = self._check_pages(pages)
        dev = ops._require_cuda(Q)
        nq = Q.shape[0]
        if nq == 0 or m == 0:
            if out is None:
                out = torch.empty((nq, m), dtype=torch.float32, device=dev)
            return out[:, :m]
        qp, qamax = self._query_planes(Q)
        if self.fp8:
            return ops.maxsim_forward_fp8_pages(qp, qamax, self.planes[0], self.shift, qmask, self.tilemask, self.pageflags, pages, out=out)
        return ops.maxsim_forward_pages(qp, qamax, self.planes, self.amax, qmask, self.tilemask, self.pageflags, pages, out=out)

    def _check_prefilter(self, Q: torch.Tensor, k: int, capacity: Optional[int]) -> int:
        """Arguments of a prefiltered call (before any device work); returns the candidate capacity."""
        if not (1 <= k <= L.EVDR_TOPK_MAX):
            raise ValueError(f"k={k} outside 1..{L.EVDR_TOPK_MAX}")
        if self.fp8:
            raise ValueError("prefilter=True is not available on an fp8 corpus: its first stage would need an error bound on the e4m3 "
                             "scores, and fp8 has no exact rerank (score it with prefilter=False)")
        if self.nplanes == 1:
            raise ValueError("prefilter=True needs an fp32 corpus (fp16 hi/lo planes): a bf16 corpus has no cheaper first stage")
        if self.nplanes != 2:
            raise NotImplementedError("prefilter=True does not cover width-256 corpora")
        if Q.dim() != 3 or Q.shape[1] > ops.PREFILTER_MAX_LQ:
            raise NotImplementedError(f"prefilter=True covers queries of at most {ops.PREFILTER_MAX_LQ} tokens; got shape {tuple(Q.shape)}")
        cap = max(k, min(self.n_pages, PREFILTER_CAPACITY)) if capacity is None else int(capacity)
        if cap < k:
            raise ValueError(f"prefilter capacity {cap} < k = {k}")
        return cap

    def prefilter_bound(self) -> torch.Tensor:
        """(2,) fp32 device tensor H, L of the corpus this one is (a view of): computed once, on the first prefiltered call."""
        owner = self._bound_owner
        if owner._pf_bound is None:
            owner._pf_bound = ops.prefilter_corpus_bound(owner.planes, owner.tilemask, owner.pageflags)
        return owner._pf_bound

    def prefilter_stats(self) -> dict:
        """Candidate counts of the last prefiltered `topk` call (reads them back: synchronises).  min / mean / max over the queries
        whose bound was finite, the number of queries scored exhaustively instead (fallback rows) and the capacity used."""
        if self._pf_stats is None:
            raise RuntimeError("prefilter_stats(): no prefiltered topk() call on this corpus yet")
        st, cap = self._pf_stats
        cnt = st[:-1].cpu()
        fin = cnt[cnt >= 0].double()
        return {"queries": int(cnt.numel()), "capacity": int(cap), "fallback_rows": int(st[-1].item()),
                "candidates_min": int(fin.min().item()) if fin.numel() else None,
                "candidates_mean": float(fin.mean().item()) if fin.numel() else None,
                "candidates_max": int(fin.max().item()) if fin.numel() else None}

    def topk(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], k: int, prefilter: bool = False,
             capacity: Optional[int] = None, subset: Optional[PageSubset] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per-query top-k of this shard with GLOBAL page indices (idx_base added): (nq,k) fp32, (nq,k) int32.
        prefilter=True (fp32 corpora, queries of <= 32 tokens): the exact two-stage form -- hi-plane coarse pass, rigorous per-query
        bound, exact rerank of the pages that can still reach the top k (at most `capacity` per query, default
        max(k, min(n_pages, 4096)); a query with more is scored exhaustively) -- with the SAME bits as prefilter=False, no host
        synchronisation; `prefilter_stats()` reports the candidate counts (DESIGN.md "Prefiltered fp32 top-k").
        Two C-ABI calls on the current stream, no sync: evdr_maxsim_fwd_prepared into this corpus's score block (kept between
        calls: 410 MB at 1024 x 100k), then evdr_topk over it (evdr_maxsim_topk is the same two launches behind one call, for C
        callers; tests pin the two forms to the same bits).  With `score_events` set (bench.py) a HIP-event pair is recorded around
        the MaxSim launch -- the ONLY difference between the timed step of the bench and what `ShardedRetriever.search` runs.
        subset (`subset()`): the top-k among the subset's pages only -- the subset forward into the kept score block, evdr_topk over
        its m columns, columns mapped to global indices through the list (ascending, so ties still break towards the lower index);
        (-inf, -1) padding when m < k.  Not with prefilter=True."""
        if subset is not None:
            if prefilter:
                raise ValueError("prefilter=True cannot be combined with a subset (the coarse pass and its bound cover the whole corpus)")
            self._check_subset(subset)
        cap = self._check_prefilter(Q, k, capacity) if prefilter else 0
        dev = ops._require_cuda(Q)
        nq, lq, _ = Q.shape
        if not (1 <= k <= L.EVDR_TOPK_MAX):               # before the early returns: an invalid k never passes silently
            raise ValueError(f"k={k} outside 1..{L.EVDR_TOPK_MAX}")
        if nq == 0:
            return (torch.empty((0, k), dtype=torch.float32, device=dev), torch.empty((0, k), dtype=torch.int32, device=dev))
        if self.n_pages == 0 or (subset is not None and subset.m == 0):
            return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev), torch.full((nq, k), -1, dtype=torch.int32, device=dev))
        qp, qamax = self._query_planes(Q)
        if subset is not None:
            need = nq * subset.m
            if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
                self._ws = torch.empty((need,), dtype=torch.float32, device=dev)
            ws = self._ws[:need].view(nq, subset.m)
            ev = None
            if self.score_events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            ops.maxsim_forward_pages(qp, qamax, self.planes, self.amax, qmask, self.tilemask, self.pageflags, subset.pages, out=ws)
            if ev is not None:
                ev[1].record()
                self.score_events.append(ev)
            ts, col = ops.topk(ws, k)
            # columns -> global indices through the list: (nq, k) words, never an (nq, m) map; padding (-1) stays -1
            gi = subset.pages[col.clamp_min(0).long()] + self.idx_base
            return ts, torch.where(col >= 0, gi, col)
        if prefilter:
            bound = self.prefilter_bound()
            if self._pf_ws is None or self._pf_ws.device != dev:
                self._pf_ws = None
            stats = torch.empty((nq + 1,), dtype=torch.int32, device=dev)
            wsb = L.load().evdr_maxsim_topk_prefilter_workspace(nq, self.n_pages, cap)
            if self._pf_ws is None or self._pf_ws.numel() < wsb:
                self._pf_ws = ops.workspace(wsb, dev)      # kept between calls, like the exhaustive score block
            out = ops.maxsim_topk_prefilter(qp, qamax, self.planes, self.amax, qmask, self.tilemask, self.pageflags, bound, k, cap,
                                            idx_base=self.idx_base, stats=stats, ws=self._pf_ws)
            self._pf_stats = (stats, cap)
            return out
        # the score block is a FLAT buffer that only grows (410 MB at 1024 x 100k): a short last batch, or alternating batch sizes,
        # view its head instead of reallocating it
        need = nq * self.n_pages
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty((need,), dtype=torch.float32, device=dev)
        ws = self._ws[:need].view(nq, self.n_pages)
        ev = None
        if self.score_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if self.fp8:
            ops.maxsim_forward_fp8(qp, qamax, self.planes[0], self.shift, qmask, self.tilemask, self.pageflags, out=ws)
        else:
            ops.maxsim_forward_prepared(qp, qamax, self.planes, self.amax, qmask, self.tilemask, self.pageflags, out=ws)
        if ev is not None:
            ev[1].record()
            self.score_events.append(ev)
        return ops.topk(ws, k, idx_base=self.idx_base)


    # ---- candidate scoring -----------------------------------------------------------------------------
    def _check_candidates(self, Q: torch.Tensor, cand: torch.Tensor, k: Optional[int] = None) -> int:
        """Arguments of a candidate call (before any device work); returns r, the list length."""
        if self.fp8:
            raise NotImplementedError("candidate scoring is not available on an fp8 corpus (rerank on the bf16 / fp32 corpus of the "
                                      "same pages; an fp8 corpus serves as the FIRST stage of TwoStageRetriever)")
        if self.nplanes == 4:
            raise NotImplementedError("candidate scoring does not cover width-256 corpora")
        if Q.dim() != 3 or Q.shape[1] > ops.CANDIDATES_MAX_LQ:
            raise NotImplementedError(f"candidate scoring covers queries of at most {ops.CANDIDATES_MAX_LQ} tokens; got shape "
                                      f"{tuple(Q.shape)}")
        r = ops.check_candidates(cand, Q.shape[0], self.device)
        if k is not None and not (1 <= k <= min(r, L.EVDR_TOPK_MAX)):
            raise ValueError(f"k={k} outside 1..min(r, {L.EVDR_TOPK_MAX}) = 1..{min(r, L.EVDR_TOPK_MAX)}")
        return r

    def _score_candidates(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], cand: torch.Tensor, want_clean: bool):
        dev = ops._require_cuda(Q)
        nq, r = cand.shape
        wsb = L.load().evdr_maxsim_fwd_candidates_workspace(nq, r)
        if self._cand_ws is None or self._cand_ws.numel() < wsb or self._cand_ws.device != dev:
            self._cand_ws = ops.workspace(wsb, dev)       # kept between calls, like the exhaustive score block
        qp, qamax = self._query_planes(Q)
        return ops.maxsim_forward_candidates(qp, qamax, self.planes, self.amax, qmask, self.tilemask, self.pageflags, cand,
                                             idx_base=self.idx_base, want_clean=want_clean, ws=self._cand_ws)

    def score_candidates(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], cand: torch.Tensor) -> torch.Tensor:
        """(nq, r) fp32: the score of query q and page cand[q, i], the bits `score` gives that pair (bf16 pages shorter than 225
        patches: within 1e-4).  cand (nq, r) int32 holds GLOBAL page indices, r <= 4096; an entry this corpus does not
        own (-1, another shard's page, anything else) is a hole: -inf, no memory read.  Duplicates are scored each.  bf16 and fp32
        corpora, queries of at most 32 tokens; no host synchronisation."""
        self._check_candidates(Q, cand)
        return self._score_candidates(Q, qmask, cand, False)[0]

    def rerank(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], cand: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Top-k of each query's candidate list by exact score: ((nq, k) fp32, (nq, k) int32 global indices), score descending, index
        ascending, (-inf, -1) padding when fewer than k entries are real -- the order and padding of `topk`.  The lists may come in
        any order: where equal scores straddle rank k, the lowest reported indices among equal scores are kept, so a list that names
        every page gives `topk`'s answer bit for bit.  `score_candidates` + `ops.topk` over the lists; 1 <= k <= min(r, EVDR_TOPK_MAX)."""
        self._check_candidates(Q, cand, k)
        sc, clean = self._score_candidates(Q, qmask, cand, True)
        return ops.topk(sc, k, idx_map=clean)

    # ---- document-level search ------------------------------------------------------------------------
    def documents(self, doc_of_page: torch.Tensor, n_docs: Optional[int] = None, subset: Optional[PageSubset] = None) -> PageDocuments:
        """The documents of this corpus's pages, as a `PageDocuments` for `topk_docs`, `rerank_docs` and the retrievers' `search_docs`.
        doc_of_page: (n_pages,) int32 on this corpus's device, one GLOBAL document id per page of THIS corpus (a `shard()` view takes
        its slice of the global tensor; a document may span shards), -1 = the page belongs to no document and is never returned.  A
        document's pages may sit anywhere: interleaved, or appended later.  n_docs: ids lie in [0, n_docs); default: the largest id
        + 1 (every rank of a sharded search must pass the same n_docs, so pass it there).  subset: a `PageSubset` of this corpus --
        the lists then index the subset's columns, for `topk_docs(..., subset=)`.
        A set-up step in plain torch that reads the largest id back ONCE; searches with the result never synchronise."""
        if (not isinstance(doc_of_page, torch.Tensor) or doc_of_page.dtype != torch.int32 or tuple(doc_of_page.shape) != (self.n_pages,)
                or doc_of_page.device != self.device):
            raise ValueError(f"doc_of_page must be an (n_pages,) = ({self.n_pages},) int32 tensor on {self.device}; got "
                             f"{tuple(getattr(doc_of_page, 'shape', ()))} {getattr(doc_of_page, 'dtype', None)} on "
                             f"{getattr(doc_of_page, 'device', None)}")
        if subset is not None:
            self._check_subset(subset)
        doc_of_page = doc_of_page.contiguous()
        top = int(doc_of_page.max().item()) if self.n_pages else -1
        if n_docs is None:
            n_docs = top + 1
        n_docs = int(n_docs)
        if n_docs < 0 or top >= n_docs:
            raise ValueError(f"document ids must lie in [0, n_docs) = [0, {n_docs}) (or be -1); the largest id is {top}")
        cols = doc_of_page if subset is None else doc_of_page[subset.pages.long()]
        members, offsets = ops.doc_lists(cols, n_docs)
        return PageDocuments(doc_of_page, members, offsets, n_docs, self, subset)

    def _check_documents(self, docs: PageDocuments, k: int) -> None:
        if not isinstance(docs, PageDocuments) or not docs.belongs_to(self):
            raise ValueError("these documents were made by another corpus, or by this one before it grew (another tensor, another "
                             "idx_base or another n_pages): build them with this corpus's documents()")
        if not (1 <= k <= L.EVDR_TOPK_MAX):
            raise ValueError(f"k={k} outside 1..{L.EVDR_TOPK_MAX}")

    def topk_docs(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], k: int, docs: PageDocuments,
                  subset: Optional[PageSubset] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Per-query top-k DOCUMENTS of this shard: (scores (nq, k) fp32, doc (nq, k) int32 document ids, page (nq, k) int32 GLOBAL index
        of the document's best page).  A document's score is its best page's; among equally good pages the lowest index is reported;
        rows are score descending, document id ascending, padded with (-inf, -1, -1) when fewer than k documents have a page here
        (`ops.doc_reference` states the rule).  Exact: the forward of `topk` into the kept score block, then `ops.doc_topk` over it --
        no host synchronisation.  bf16, fp32, fp8 and width-256 corpora.  subset: the `PageSubset` `docs` was built with
        (`documents(..., subset=)`): only its pages are scored and returned; refused where `topk(subset=)` is."""
        self._check_documents(docs, k)
        if subset is not docs.subset:
            raise ValueError("subset= must be the PageSubset these documents were built with (documents(..., subset=)): their lists index "
                             "its columns")
        if subset is not None:
            self._check_subset(subset)
        dev = ops._require_cuda(Q)
        nq = Q.shape[0]
        n = self.n_pages if subset is None else subset.m
        if nq == 0 or n == 0 or docs.n_docs == 0:
            return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev), torch.full((nq, k), -1, dtype=torch.int32, device=dev),
                    torch.full((nq, k), -1, dtype=torch.int32, device=dev))
        need = nq * n
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty((need,), dtype=torch.float32, device=dev)
        ws = self._ws[:need].view(nq, n)
        self.score(Q, qmask, out=ws, subset=subset)
        wsb = L.load().evdr_doc_topk_workspace(nq, docs.n_docs)
        if self._doc_ws is None or self._doc_ws.numel() < wsb or self._doc_ws.device != dev:
            self._doc_ws = ops.workspace(wsb, dev)        # kept between calls, like the score block
        return ops.doc_topk(ws, docs.members, docs.offsets, k, idx_map=docs.idx_map, idx_base=self.idx_base, ws=self._doc_ws)

    def rerank_docs(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], cand: torch.Tensor, k: int,
                    docs: PageDocuments) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Top-k documents among the pages each query's candidate list names: (scores, doc, page) as `topk_docs`, by exact score.
        `score_candidates`, then `ops.collapse_topk` with this corpus's doc_of_page; entries this corpus does not own and pages without
        a document are holes.  The lists may come in any order and may repeat pages; a list that names every page gives `topk_docs`'s
        answer bit for bit.  Refusals as `rerank`: bf16 and fp32 corpora, queries of at most 32 tokens, 1 <= k <= min(r, 128)."""
        self._check_candidates(Q, cand, k)
        self._check_documents(docs, k)
        sc, clean = self._score_candidates(Q, qmask, cand, True)
        return ops.collapse_topk(sc, clean, k, doc_of_page=docs.doc_of_page, idx_base=self.idx_base)

    # ---- token alignment ------------------------------------------------------------------------------
    def _check_align(self, Q: torch.Tensor, cand: torch.Tensor) -> int:
        """Arguments of an alignment call (before any device work); returns r, the list length."""
        if self.fp8:
            raise NotImplementedError("token alignment is not available on an fp8 corpus (align on the bf16 / fp32 corpus of the same "
                                      "pages)")
        if self.nplanes == 4:
            raise NotImplementedError("token alignment does not cover width-256 corpora")
        if Q.dim() != 3 or not (1 <= Q.shape[1] <= ops.ALIGN_MAX_LQ):
            raise NotImplementedError(f"token alignment covers queries of 1..{ops.ALIGN_MAX_LQ} tokens; got shape {tuple(Q.shape)}")
        return ops.check_candidates(cand, Q.shape[0], self.device)

    def align(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], cand: torch.Tensor, heat: bool = False):
        """Which patches produced a score: (sim (nq, r, lq) fp32, patch (nq, r, lq) int32[, heat (nq, r, lp) fp32]) for query q and the
        pages cand[q] names -- per query token the best patch of the page (the value the score sums, and the first index attaining it)
        and, with heat=True, per patch the best valid query token (a similarity map over the page).  cand (nq, r) int32 holds GLOBAL
        page indices, e.g. the indices `topk` returned, r <= 4096; an entry this corpus does not own is a hole: sim = -inf, patch = -1,
        heat = -inf, no memory read -- so the same lists can go to every `shard()`.  Rules and fill values: `ops.align_reference`.
        bf16 and fp32 corpora (growable, pooled and clustered ones like any other), queries of at most 32 tokens; one launch, no host
        synchronisation."""
        self._check_align(Q, cand)
        ops._require_cuda(Q)
        qp, qamax = self._query_planes(Q)
        return ops.maxsim_align(qp, qamax, self.planes, self.amax, qmask, self.tilemask, self.pageflags, cand, idx_base=self.idx_base,
                                heat=heat)

    def hard_patches(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], cand: torch.Tensor) -> torch.Tensor:
        """(nq, r) int32: for every listed page the patch most similar to any valid query token -- the hard token of
        mainv3_iter_liscore_QA_hardtoken.py:413-417 -- as `ops.hard_patch` of `align`; -1 for holes, pages without a valid patch,
        queries without a valid token and NaN pairs.  Stays on the device."""
        return ops.hard_patch(*self.align(Q, qmask, cand))


# ---- candidate exchange ---------------------------------------------------------------------------
def pack_candidates(scores: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """(nq,k) fp32 + (nq,k) int32 -> one (nq, 2k) int32 message (scores bit-cast), so one collective moves both."""
    return torch.cat([scores.contiguous().view(torch.int32), idx.to(torch.int32)], dim=1).contiguous()


def unpack_candidates(buf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(world, nq, 2k) int32 -> rank-major candidate lists (nq, world*k) scores fp32 and global indices int32."""
    world, nq, two_k = buf.shape
    k = two_k // 2
    sc = buf[:, :, :k].contiguous().view(torch.float32).permute(1, 0, 2).reshape(nq, world * k)
    ix = buf[:, :, k:].permute(1, 0, 2).reshape(nq, world * k)
    return sc.contiguous(), ix.contiguous()


def gather_candidates(scores: torch.Tensor, idx: torch.Tensor, group=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """All-gather every rank's (nq,k) candidates.  backend nccl (= RCCL over xGMI): device tensors go straight
    into ncclAllGather; backend gloo (CPU rehearsal): staged through host memory."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    msg = pack_candidates(scores, idx)
    backend = dist.get_backend(group)
    if backend == "gloo" and msg.is_cuda:
        host = msg.cpu()
        buf = torch.empty((world * host.shape[0], host.shape[1]), dtype=torch.int32)
        dist.all_gather_into_tensor(buf, host, group=group)
        buf = buf.to(msg.device)
    else:
        # output = the ranks' messages concatenated along dim 0 (the layout both RCCL and gloo accept)
        buf = torch.empty((world * msg.shape[0], msg.shape[1]), dtype=torch.int32, device=msg.device)
        dist.all_gather_into_tensor(buf, msg, group=group)
    return unpack_candidates(buf.view(world, msg.shape[0], msg.shape[1]))


def merge_candidates(scores: torch.Tensor, idx: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Candidate lists (nq, m) scores and global indices, columns in any order -> final top-k (score desc, global index asc) with
    the HIP top-k kernel; where equal scores straddle rank k, the lowest reported indices among equal scores are kept."""
    return ops.topk(scores, k, idx_map=idx)


# ---- document candidates: the three-array form of the exchange above -------------------------------
def pack_doc_candidates(scores: torch.Tensor, doc: torch.Tensor, page: torch.Tensor) -> torch.Tensor:
    """(nq,k) fp32 + (nq,k) int32 document ids + (nq,k) int32 pages -> one (nq, 3k) int32 message (scores bit-cast)."""
    return torch.cat([scores.contiguous().view(torch.int32), doc.to(torch.int32), page.to(torch.int32)], dim=1).contiguous()


def unpack_doc_candidates(buf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(world, nq, 3k) int32 -> rank-major lists (nq, world*k): scores fp32, document ids int32, global pages int32."""
    world, nq, three_k = buf.shape
    k = three_k // 3
    parts = [buf[:, :, i * k:(i + 1) * k].permute(1, 0, 2).reshape(nq, world * k).contiguous() for i in range(3)]
    return parts[0].view(torch.float32), parts[1], parts[2]


def gather_doc_candidates(scores: torch.Tensor, doc: torch.Tensor, page: torch.Tensor, group=None):
    """All-gather every rank's (nq,k) document candidates: ONE collective of (nq, 3k) int32 words per rank (as `gather_candidates`)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    msg = pack_doc_candidates(scores, doc, page)
    if dist.get_backend(group) == "gloo" and msg.is_cuda:
        host = msg.cpu()
        buf = torch.empty((world * host.shape[0], host.shape[1]), dtype=torch.int32)
        dist.all_gather_into_tensor(buf, host, group=group)
        buf = buf.to(msg.device)
    else:
        buf = torch.empty((world * msg.shape[0], msg.shape[1]), dtype=torch.int32, device=msg.device)
        dist.all_gather_into_tensor(buf, msg, group=group)
    return unpack_doc_candidates(buf.view(world, msg.shape[0], msg.shape[1]))


def merge_doc_candidates(scores: torch.Tensor, doc: torch.Tensor, page: torch.Tensor, k: int):
    """Document candidate lists (nq, m), entries in any order, a document possibly named by several shards -> the final top-k
    documents (`ops.collapse_topk` with explicit ids: one entry per document, its best page, key desc, document id asc).  Exact
    when every list is a shard's own top-k: a document of the global top k is in the local top k of the rank that owns its best
    page, because every document ranked above it there ranks above it globally too.  m <= EVDR_SELECT_MAX."""
    return ops.collapse_topk(scores, page, k, doc=doc)


def _check_doc_world(world: int, k: int) -> None:
    if world * k > L.EVDR_SELECT_MAX:
        raise ValueError(f"world * k = {world} * {k} = {world * k} document candidates per query exceed {L.EVDR_SELECT_MAX} "
                         f"(the merge holds a query's whole list in one workgroup)")


def tie_candidates(local_scores: torch.Tensor, idx_base: int, kth_scores: torch.Tensor, k: int, group=None):
    """Tie completion across shards (the page-sharded form of `ops.topk_with_ties`): for every query row whose GLOBAL k-th
    score is shared by pages that did not make the merged cut, all pages of ALL shards that rank at or above it --
    {row: (global page indices int64 ascending, scores fp32)} as host numpy arrays, the same on every rank.
    local_scores (nq, n_local): this rank's score block; kth_scores (nq,): the merged top-k's last column.
    One all-reduce of nq int32 counts (always); an object all-gather of the tied triples only when some row is cut.  The
    metric layer then ranks the tied candidates by trec_eval's rule (docid descending) exactly as the reference's all-pairs
    evaluation would (mainv2_iter_distill_infonce.py:311-319)."""
    import numpy as np
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    nq = local_scores.shape[0]
    key = ops._order_key(local_scores) if local_scores.shape[1] else local_scores.new_zeros((nq, 0), dtype=torch.int32)
    kth = ops._order_key(kth_scores.reshape(nq, 1).to(local_scores.device))
    total = (key >= kth).sum(dim=1, dtype=torch.int32)
    if multi:
        if dist.get_backend(group) == "gloo" and total.is_cuda:
            host = total.cpu()
            dist.all_reduce(host, group=group)
            total = host
        else:
            dist.all_reduce(total, group=group)
    cut = (total > k).nonzero().flatten().to(local_scores.device)
    if cut.numel() == 0:
        return {}
    sel = key[cut] >= kth[cut]
    rc = sel.nonzero()
    mine = (cut[rc[:, 0]].cpu().numpy().astype(np.int64), (rc[:, 1] + int(idx_base)).cpu().numpy().astype(np.int64),
            local_scores[cut][sel].float().cpu().numpy())
    parts = [mine]
    if multi:
        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, mine, group=group)
    rows = np.concatenate([p[0] for p in parts])
    cols = np.concatenate([p[1] for p in parts])
    sc = np.concatenate([p[2] for p in parts])
    order = np.lexsort((cols, rows))                                   # by row, then global page index (shards are contiguous)
    rows, cols, sc = rows[order], cols[order], sc[order]
    starts = np.flatnonzero(rows[1:] != rows[:-1]) + 1
    return {int(rows[a]): (cols[a:b], sc[a:b]) for a, b in zip([0, *starts.tolist()], [*starts.tolist(), len(rows)])}


class ShardedRetriever:
    """Late-interaction retrieval over a page-sharded corpus: local MaxSim + top-k, one all-gather, merge."""

    def __init__(self, shard: PageCorpus, group=None):
        self.shard = shard
        self.group = group

    def search(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], k: int = 100, with_ties: bool = False, prefilter: bool = False,
               capacity: Optional[int] = None, subset: Optional[PageSubset] = None):
        """(top_scores, top_idx) of the whole corpus, (score desc, global index asc), identical on every rank.  with_ties=True
        also returns `extra` (see `tie_candidates`): the candidates a metric with another tie rule needs when equal scores
        straddle rank k -- (top_scores, top_idx, extra); it keeps the shard's score block (nq x n_local fp32) for one more pass.
        prefilter / capacity: `PageCorpus.topk`'s exact two-stage form on every shard (not with with_ties).
        subset: this shard's `PageSubset` (every rank builds its own from the same global list, `shard.subset(pages=...)`): the
        shard-local subset top-k, then the same all-gather and merge (not with with_ties, not with prefilter)."""
        import torch.distributed as dist
        if prefilter and with_ties:
            raise ValueError("prefilter=True cannot complete ties (with_ties=True needs the full score block)")
        if subset is not None and with_ties:
            raise ValueError("a subset search cannot complete ties (with_ties=True needs the full score block)")
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1
        if not with_ties:
            # prefilter=True: each shard's top-k is exact, so the merge is too
            ls, li = self.shard.topk(Q, qmask, k, prefilter=prefilter, capacity=capacity, subset=subset)
            if not multi:
                return ls, li
            sc, ix = gather_candidates(ls, li, self.group)
            return merge_candidates(sc, ix, k)
        scores = self.shard.score(Q, qmask)
        if self.shard.n_pages:
            ls, li = ops.topk(scores, min(k, self.shard.n_pages), idx_base=self.shard.idx_base)
            if ls.shape[1] < k:                                        # a shard shorter than k: holes at the end, like evdr_maxsim_topk
                pad = k - ls.shape[1]
                ls = torch.cat([ls, ls.new_full((ls.shape[0], pad), float("-inf"))], dim=1)
                li = torch.cat([li, li.new_full((li.shape[0], pad), -1)], dim=1)
        else:
            ls, li = self.shard.topk(Q, qmask, k)
        ts, ti = merge_candidates(*gather_candidates(ls, li, self.group), k) if multi else (ls, li)
        return ts, ti, tie_candidates(scores, self.shard.idx_base, ts[:, k - 1], k, self.group)

    def search_docs(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], k: int, docs: PageDocuments,
                    subset: Optional[PageSubset] = None):
        """(scores, doc, page) (nq, k) of the whole corpus's top-k DOCUMENTS, identical on every rank: the shard-local `topk_docs`, ONE
        all-gather of an (nq, 3k) int32 message per rank, `merge_doc_candidates`.  docs: this shard's `PageDocuments` (document ids are
        global, the same n_docs on every rank; a document may span shards); subset: the shard's `PageSubset` `docs` was built with.
        Exact.  world * k <= EVDR_SELECT_MAX."""
        import torch.distributed as dist
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1
        if multi:
            _check_doc_world(dist.get_world_size(self.group), k)
        ls, ld, lp = self.shard.topk_docs(Q, qmask, k, docs, subset=subset)
        if not multi:
            return ls, ld, lp
        return merge_doc_candidates(*gather_doc_candidates(ls, ld, lp, self.group), k)

    def rerank(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], cand: torch.Tensor, k: int):
        """Top-k by exact score among the pages `cand` (nq, r) int32 names (GLOBAL indices, the same lists on every rank): each shard
        reranks the entries it owns (`PageCorpus.rerank`), then the all-gather and merge of `search`.  Identical on every rank, and
        independent of the order of the lists: the lowest reported indices among equal scores are kept at the cut."""
        import torch.distributed as dist
        ls, li = self.shard.rerank(Q, qmask, cand, k)
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1
        if not multi:
            return ls, li
        return merge_candidates(*gather_candidates(ls, li, self.group), k)


class TwoStageRetriever:
    """Approximate search in two passes over the same pages: a cheap corpus proposes, the exact one reranks.

    `coarse` is any PageCorpus over the pages of `exact` (same n_pages and idx_base; page length, dtype and kind are free): an fp8
    copy, a pooled corpus made from the same pages (`PageCorpus.from_pooled`: 1 / f of the tokens, so about 1 / f of the first pass;
    DESIGN.md §4.10, scratch/pool_bench.py), or a compressed student corpus.  `exact` is a bf16 or fp32 corpus.  Every returned score is `exact`'s own bits and the
    returned set is the top-k by exact score among the coarse top-`candidates`; nothing is promised about recall against the
    exhaustive ranking -- measure it (scratch/two_stage_bench.py).  With `subset=` both passes run over the subset's pages only
    (scratch/two_stage_subset_bench.py)."""

    def __init__(self, coarse: PageCorpus, exact: PageCorpus, group=None):
        if coarse.n_pages != exact.n_pages or coarse.idx_base != exact.idx_base:
            raise ValueError(f"coarse and exact corpora must hold the same pages: n_pages {coarse.n_pages} vs {exact.n_pages}, "
                             f"idx_base {coarse.idx_base} vs {exact.idx_base}")
        if exact.fp8 or exact.nplanes == 4:
            raise NotImplementedError("the exact corpus of a two-stage search must be a bf16 or fp32 corpus of width <= 128")
        self.coarse = coarse
        self.exact = exact
        self.group = group
        self._ws: Optional[torch.Tensor] = None       # (nq, n_pages) coarse score block, kept between calls
        # scratch/two_stage_bench.py: a list here makes search() record HIP events around its three parts and append the four
        self.part_events: Optional[list] = None

    def search(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], k: int = 100, candidates: int = 1024, Q_coarse: Optional[torch.Tensor] = None,
               subset: Optional[PageSubset] = None):
        """(top_scores (nq, k) fp32, top_idx (nq, k) int32 global): coarse.score -> select_topr(candidates) -> exact.rerank -> (several
        ranks: all-gather and merge; `candidates` is per shard).  k <= candidates <= 4096.  Q_coarse: the queries in the coarse
        corpus's embedding space when it differs from Q's dtype or model (default: Q).  No host synchronisation.
        subset (made by `exact.subset(...)`; each rank passes its own shard's): the search among the subset's m pages only --
        coarse.score_pages over the list (coarse holds the same pages under the same idx_base, so the local indices name the same
        pages in both corpora), select_topr over the (nq, m) block, columns mapped to global indices through the list, exact.rerank.
        Every returned index lies in the subset; (-inf, -1) padding at the end when m < k, in every row when m = 0."""
        import torch.distributed as dist
        if self.coarse.n_pages != self.exact.n_pages:      # reachable since corpora grow: an append to one corpus of the pair only
            raise ValueError(f"coarse and exact corpora no longer hold the same pages: n_pages {self.coarse.n_pages} vs "
                             f"{self.exact.n_pages} (append to both)")
        if subset is not None:
            if not isinstance(subset, PageSubset) or not subset.belongs_to(self.exact):
                raise ValueError("this subset was made by another corpus (another tensor, or a view of the same pages with a different "
                                 "idx_base): build it with the exact corpus's subset()")
            if self.coarse.nplanes == 4:
                raise NotImplementedError("a two-stage search over a subset does not cover a width-256 coarse corpus")
        if not (1 <= k <= L.EVDR_TOPK_MAX):
            raise ValueError(f"k={k} outside 1..{L.EVDR_TOPK_MAX}")
        if not (k <= candidates <= L.EVDR_SELECT_MAX):
            raise ValueError(f"candidates={candidates} outside k..{L.EVDR_SELECT_MAX} = {k}..{L.EVDR_SELECT_MAX}")
        if Q.dim() != 3 or Q.shape[1] > ops.CANDIDATES_MAX_LQ:
            raise NotImplementedError(f"two-stage search covers queries of at most {ops.CANDIDATES_MAX_LQ} tokens; got shape {tuple(Q.shape)}")
        dev = ops._require_cuda(Q)
        nq = Q.shape[0]
        n = self.coarse.n_pages if subset is None else subset.m
        need = nq * n
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty((max(need, 1),), dtype=torch.float32, device=dev)
        block = self._ws[:need].view(nq, n)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.part_events is not None else None
        if ev:
            ev[0].record()
        if subset is None:
            self.coarse.score(Q if Q_coarse is None else Q_coarse, qmask, out=block)
        else:
            self.coarse.score_pages(Q if Q_coarse is None else Q_coarse, qmask, subset.pages, out=block)
        if ev:
            ev[1].record()
        if subset is None:
            cand = ops.select_topr(block, candidates, idx_base=self.exact.idx_base)
        else:
            # columns -> global indices through the list: (nq, candidates) words, never an (nq, m) map; padding (-1) stays -1
            if n:
                col = ops.select_topr(block, candidates)
                cand = torch.where(col >= 0, subset.pages[col.clamp_min(0).long()] + self.exact.idx_base, col)
            else:                                         # an empty subset: every entry is padding, the rerank returns (-inf, -1) rows
                cand = torch.full((nq, candidates), -1, dtype=torch.int32, device=dev)
        if ev:
            ev[2].record()
        ls, li = self.exact.rerank(Q, qmask, cand, k)
        if ev:
            ev[3].record()
            self.part_events.append(ev)
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1
        if not multi:
            return ls, li
        return merge_candidates(*gather_candidates(ls, li, self.group), k)

    def search_docs(self, Q: torch.Tensor, qmask: Optional[torch.Tensor], k: int, candidates: int, docs: PageDocuments,
                    Q_coarse: Optional[torch.Tensor] = None, subset: Optional[PageSubset] = None):
        """(scores, doc, page) (nq, k): the top-k DOCUMENTS among the coarse top-`candidates` PAGES -- the first stage and
        `select_topr` of `search`, then `exact.rerank_docs` (several ranks: the all-gather and merge of
        `ShardedRetriever.search_docs`; `candidates` is per shard).  docs: `exact.documents(...)`.  APPROXIMATE, like `search`: a document
        is found only if its best page is among the candidates, and a document whose best page is not gets the score of its best
        CANDIDATE page; every returned score is `exact`'s own bits.  k <= candidates <= 4096; with candidates = n_pages the answer is
        `exact.topk_docs`'s.  subset (`exact.subset(...)`): both passes over the subset's pages only.  No host synchronisation."""
        import torch.distributed as dist
        if self.coarse.n_pages != self.exact.n_pages:
            raise ValueError(f"coarse and exact corpora no longer hold the same pages: n_pages {self.coarse.n_pages} vs "
                             f"{self.exact.n_pages} (append to both)")
        if subset is not None:
            if not isinstance(subset, PageSubset) or not subset.belongs_to(self.exact):
                raise ValueError("this subset was made by another corpus (another tensor, or a view of the same pages with a different "
                                 "idx_base): build it with the exact corpus's subset()")
            if self.coarse.nplanes == 4:
                raise NotImplementedError("a two-stage search over a subset does not cover a width-256 coarse corpus")
        self.exact._check_documents(docs, k)
        if not (k <= candidates <= L.EVDR_SELECT_MAX):
            raise ValueError(f"candidates={candidates} outside k..{L.EVDR_SELECT_MAX} = {k}..{L.EVDR_SELECT_MAX}")
        if Q.dim() != 3 or Q.shape[1] > ops.CANDIDATES_MAX_LQ:
            raise NotImplementedError(f"two-stage search covers queries of at most {ops.CANDIDATES_MAX_LQ} tokens; got shape {tuple(Q.shape)}")
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1
        if multi:
            _check_doc_world(dist.get_world_size(self.group), k)
        dev = ops._require_cuda(Q)
        nq = Q.shape[0]
        n = self.coarse.n_pages if subset is None else subset.m
        need = nq * n
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty((max(need, 1),), dtype=torch.float32, device=dev)
        block = self._ws[:need].view(nq, n)
        if subset is None:
            self.coarse.score(Q if Q_coarse is None else Q_coarse, qmask, out=block)
            cand = ops.select_topr(block, candidates, idx_base=self.exact.idx_base)
        elif n:
            self.coarse.score_pages(Q if Q_coarse is None else Q_coarse, qmask, subset.pages, out=block)
            col = ops.select_topr(block, candidates)
            cand = torch.where(col >= 0, subset.pages[col.clamp_min(0).long()] + self.exact.idx_base, col)
        else:
            cand = torch.full((nq, candidates), -1, dtype=torch.int32, device=dev)
        ls, ld, lp = self.exact.rerank_docs(Q, qmask, cand, k, docs)
        if not multi:
            return ls, ld, lp
        return merge_doc_candidates(*gather_doc_candidates(ls, ld, lp, self.group), k)
