/*
 * evdr.h -- C ABI of the MI355X-native late-interaction (MaxSim) scorer.
 *
 * The reference (kimjy-st/Efficient-Visual-Document-Retrieval) has no FFI layer: its boundary
 * for this path is a set of Python function signatures in evaluator/retrieval.py.  Each entry
 * point below names the reference interface it replaces (paths relative to the reference root).
 * The Python host shim (efficient-visual-document-retrieval_amd/evaluator/retrieval.py) binds these with
 * ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless it says "host";
 *   - plain pointers and sizes only, no framework types; all functions return an int status
 *     (EVDR_OK == 0) and never throw/abort across the ABI; evdr_last_error() gives the text;
 *   - nothing here allocates, frees or synchronises: scratch memory comes in through
 *     `workspace` (query the size first), work is enqueued on `hip_stream` (a hipStream_t, may
 *     be NULL for the default stream) and the call returns immediately (graph-capture safe);
 *   - THREADING: entry points may be called from several host threads at once, each call on whatever stream it names (the
 *     reference itself drives its scorer from a single Python thread, DataLoader(num_workers=0);
 *     mainv2_iter_distill_infonce.py:269-321).  The library keeps no mutable state between calls except (a) per kernel
 *     instance, the set of devices on which its dynamic-LDS limit has been raised -- an atomic bit set, and raising the limit
 *     twice is harmless.  evdr_last_error(), evdr_last_fwd_kernel() and the two debug overrides at the end of this file are
 *     THREAD-LOCAL: a thread reads and sets its own, no caller can change what another caller's launch does.  Ordering between calls that
 *     touch the same buffers is the caller's (streams / events), as with any HIP launch; workspaces are per call.
 *     tests/cabi/cabi_threads.cpp: eight threads, one kernel family each, first launches racing, bit-equal to serial calls.
 *     Several processes per node (one per GPU: corpus.py / bench.py) are the multi-GPU form;
 *   - D (embedding width) is 128 (ColPali / ColQwen projection width) for every entry point that takes `d`; wider
 *     embeddings (up to 256) are scored through evdr_maxsim_fwd_prepared with nplanes = 4, and their gradients -- linear in the
 *     columns -- by one evdr_maxsim_bwd / evdr_maxsim_bwd_q call per 128-column block (what the Python host shim does);
 *   - masks are one byte per token, 0 = masked (torch.bool storage);
 *   - dtype: EVDR_F32 inputs are scored to fp32 accuracy (fp16 hi/lo planes of the power-of-two-scaled
 *     tensors, 3 MFMA products, error below the rounding noise of an fp32 accumulation); EVDR_BF16
 *     inputs are used as they are (products exact in fp32).
 *
 * Non-finite inputs.  For finite inputs every result below is the reference's to the stated tolerance.  A NaN is handled
 * where the reference's NaN lands (torch.max propagates it, evaluator/retrieval.py:201; the hardware max does not, so the
 * inputs are inspected instead):
 *   - a NaN in a VALID patch of page p (masked patches are replaced by -1e4 before the max and do not count)
 *     -> out[q][p] = NaN for every q;
 *   - a NaN in any token of query q, masked tokens included (NaN * 0 = NaN, :207) -> out[q][p] = NaN for every page p
 *     that has a valid patch (an all-masked page keeps its exact 0);
 *   - +-Inf elements are treated like NaN (torch yields +-Inf or NaN there depending on signs: the one divergence).
 * Pages are inspected when they are prepared: evdr_maxsim_fwd does it per call; for a resident corpus call
 * evdr_flag_nonfinite once after evdr_pack_pmask (evdr_l2norm_fwd_split can report its rows on the way).  Queries are
 * inspected inside the kernel.  argmax entries of NaN pairs are unspecified; evdr_topk ranks NaN first (like torch.topk);
 * the gradient kernels propagate whatever non-finite upstream gradient they are given, positions unspecified.
 * Limitation: for queries longer than 32 tokens, a non-finite element in a MASKED token beyond the first 32 goes unseen
 * if the query has no valid token in that 32-token slice.
 */
#ifndef EVDR_H
#define EVDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The entry points below are the library's ONLY dynamic symbols: libevdr.so is built with -fvisibility=hidden and each of them
 * carries default visibility (tests/test_cabi_exports.py compares `nm -D --defined-only` with this header, both ways). */
#define EVDR_API __attribute__((visibility("default")))

#define EVDR_OK            0
#define EVDR_ERR_ARG       1   /* null pointer / bad enum / negative size            */
#define EVDR_ERR_SHAPE     2   /* unsupported shape (D != 128, Lp > 65535 w/ argmax) */
#define EVDR_ERR_WORKSPACE 3   /* workspace missing or too small                     */
#define EVDR_ERR_HIP       4   /* a HIP runtime call or kernel launch failed         */

#define EVDR_F32  0
#define EVDR_BF16 1
#define EVDR_F16  2            /* evdr_flag_nonfinite: the hi plane of fp16 hi/lo planes; evdr_corpus_ingest: fp16 source pages */

#define EVDR_TOPK_MAX 128      /* k_values max is 100 (evaluator/retrieval.py:223)   */
#define EVDR_SELECT_MAX 4096   /* candidates per query: evdr_select_topr, evdr_maxsim_fwd_candidates */
#define EVDR_DOC_BLOCK 256     /* evdr_doc_max: documents per workgroup                */
#define EVDR_DOC_ROWS  8       /* evdr_doc_max: query rows per workgroup               */
#define EVDR_DOC_LONG  32      /* evdr_doc_max: pages from which a document takes a wave instead of a lane */

EVDR_API int         evdr_version(void);          /* 10000*major + 100*minor + patch */
EVDR_API const char* evdr_last_error(void);       /* host string, thread-local, valid until the next call */

/* ---- corpus preparation (the steps either side of the hot loop; cacheable for a static corpus) ---- */

/* Pack a (np, lp) byte mask into per-32-patch tile words + per-page flags.
 * tilemask: np * ceil(lp/32) uint32 (bit m of word t = pmask[p][32 t + m]);
 * pageflags: np uint32:
 *   bit0 = page has a valid patch  [doc_has_token, evaluator/retrieval.py:192]
 *   bit1 = page has a masked patch [the -1e4 fill takes part in the max, :198]
 *   bit2 = the valid patches are exactly ONE range [va, vb) -- the whole page, a ragged prefix, an image between masked
 *          text tokens (what utils/preprocess_data.py:101 produces), or no patch at all: then va = bits 4..15 (< 4096),
 *          vb = bits 16..31, and the kernels walk / fetch only that range; otherwise (holes) bits 16..31 = index of the
 *          first masked patch and the tile words decide
 *   bit3 = a valid patch holds a NaN / Inf element (set by evdr_flag_nonfinite, never here). */
EVDR_API int evdr_pack_pmask(const uint8_t* pmask, int64_t np, int64_t lp,
                    uint32_t* tilemask, uint32_t* pageflags, void* hip_stream);

/* Split `rows` x 128 fp32 into two fp16 planes hi/lo of x * 2^k, hi + lo == x * 2^k to 2^-22 relative.  k is one
 * power of two per tensor, chosen from its absmax so that the scaled absmax lies in [2^14, 2^15) (no fp16 overflow, and
 * the lo plane of every element that matters is a normal number).  planes: 2 * rows * 128 uint16 (fp16 bits),
 * plane-major.  amax_bits: 1 uint32 on the device = bits of max|x| (the kernels derive k from it; keep it with the
 * planes).  Three fp16 MFMA products lo*hi + hi*lo + hi*hi then give the fp32 dot product to below fp32 rounding noise.
 * Magnitude limit of the scorers: the forward kernels (evdr_maxsim_fwd*, the candidate, page-list and prefilter paths) bring a
 * product sum back with ONE pre-computed factor 2^-(kq + kp), kq / kp = 141 - the biased exponent of each tensor's absmax.  The factor
 * is a subnormal number from kq + kp = 127 on (it is kept, not flushed) and 0 from kq + kp = 150 on -- e.g. both tensors with an absmax
 * below 2^-60 --: fp32 scores then come out as 0 although the true products (about absmax_q * absmax_p) are ordinary fp32 numbers.
 * evdr_maxsim_align scales the sum itself (ldexpf) and has no such limit, so its token sums differ from the candidate scores there. */
EVDR_API int evdr_split_f32(const float* x, int64_t rows, uint16_t* planes, uint32_t* amax_bits, void* hip_stream);

/* evdr_split_f32 of MANY small tensors laid end to end, in one launch: segment s = rows [s * seg_rows, (s + 1) * seg_rows) of
 * x (the last segment may be short; seg_rows <= 2048, at most 65535 segments) -- the batches of a training epoch, whose
 * queries are known when the epoch starts (the reference draws them per step from a DataLoader,
 * mainv2_iter_distill_infonce.py:81).  Every segment keeps ITS OWN absmax word amax_bits[s] and power of two: its planes
 * are bit for bit those of evdr_split_f32 applied to that segment alone.  Segment s's planes are the contiguous
 * (2, rows_s, 128) block at planes + s * 2 * seg_rows * 128 -- what evdr_maxsim_fwd_prepared takes as Q planes.
 * planes: 2 * rows * 128 uint16 (rounded up to whole segments: ceil(rows / seg_rows) * 2 * seg_rows * 128). */
EVDR_API int evdr_split_f32_segments(const float* x, int64_t rows, int64_t seg_rows, uint16_t* planes, uint32_t* amax_bits, void* hip_stream);

/* Report non-finite page content: sets bit 3 of pageflags[p] (made by evdr_pack_pmask) when a valid patch of page p holds a
 * NaN or +-Inf element; the forward kernels then return NaN for that page ("Non-finite inputs" above).  P: (np, lp, 128)
 * of dtype EVDR_F32, EVDR_BF16 or EVDR_F16 (the hi plane of fp16 hi/lo planes), `p_stride` elements between pages.  One
 * read of P; flags are only ever set, re-run evdr_pack_pmask to clear them. */
EVDR_API int evdr_flag_nonfinite(const void* P, int dtype, const uint8_t* pmask, int64_t np, int64_t lp, int64_t p_stride,
                        uint32_t* pageflags, void* hip_stream);

/* ---- A1: score_multi_vector_masked (evaluator/retrieval.py:166-213) ---------------------------------
 * out[q,p] = sum_n qmask[q,n] * has(p) * max_m( Q[q,n,:]·P[p,m,:] if pmask[p,m] else -1e4 )
 * Q (nq,lq,128), P (np,lp,128) of `dtype`, row-major, contiguous in the last two dims;
 * strides_or_null = {q_stride, p_stride} in ELEMENTS between consecutive queries / pages
 * (NULL = dense).  qmask (nq,lq) / pmask (np,lp) bytes; either may be NULL = all valid.
 * out (nq,np) fp32 dense.  argmax_or_null: (nq,np,lq) uint16, first maximal patch index per
 * query token (what torch.max picks, :201) -- needed only for evdr_maxsim_bwd.
 * chunk_p of the reference is a memory knob with no numerical effect and has no counterpart.
 * lq == 1 with dense queries (the single-token "virtual queries" of mainv3_iter_liscore_QA_hardtoken.py:428-434) is
 * scored 32 queries to an MFMA tile internally; shapes and results are those of the general case.
 * Cost note: this entry PREPARES the pages on every call -- it packs pmask, scans P for NaN / Inf (one extra read of
 * all of P: with 1-8 queries per call, where the scorer itself only streams P once, that roughly doubles the call) and,
 * for EVDR_F32, splits P into fp16 planes.  A caller that scores the same pages more than once should prepare them once
 * (evdr_pack_pmask + evdr_flag_nonfinite [+ evdr_split_f32]) and call evdr_maxsim_fwd_prepared. */
EVDR_API size_t evdr_maxsim_fwd_workspace(int64_t nq, int64_t lq, int64_t np, int64_t lp, int dtype);
EVDR_API int evdr_maxsim_fwd(const void* Q, const void* P, const uint8_t* qmask, const uint8_t* pmask,
                    float* out, uint16_t* argmax_or_null,
                    int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t d, int dtype,
                    const int64_t* strides_or_null,
                    void* workspace, size_t workspace_bytes, void* hip_stream);

/* Same computation on a PREPARED (resident) corpus: planes + packed masks made once with
 * evdr_split_f32 / evdr_pack_pmask.  nplanes = 1 (bf16 tensors as they are), 2 (fp16 hi/lo planes of fp32
 * tensors, with the absmax words evdr_split_f32 produced for Q and P; NULL = planes are unscaled) or 4 (embeddings of
 * width 256: the reference takes any width, evaluator/retrieval.py:173 -- the two 128-column blocks of each tensor as fp16 hi/lo
 * planes under ONE absmax word per tensor, plane index = 2 * (0 hi | 1 lo) + column block, i.e. evdr_split_f32 of the tensor
 * rearranged to (column block, row, 128); widths of 129..255 ride on zero columns; one query per wave, six plane products per
 * k-step into one accumulator chain, same accuracy and NaN rules as nplanes = 2; evdr_flag_nonfinite once per hi plane).  Q planes are
 * (nplanes, nq, lq, 128); P planes are nplanes slabs `p_plane_stride` elements apart, each
 * (np, lp, 128) with `p_stride` elements between pages.  out row stride = out_stride floats, so a
 * shard can write its column block of a wider (nq, N) matrix.  This is the bench / retrieval
 * hot path (SURVEY §8(d),(e)).  qlist_ws_or_null: (nq + 1) int32 of scratch, used when lq > 32 to score the later
 * 32-token slices only for the queries that have valid tokens there (query sets are padded to their longest member). */
EVDR_API int evdr_maxsim_fwd_prepared(const uint16_t* Qplanes, const uint16_t* Pplanes,
                             const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                             float* out, int64_t out_stride, uint16_t* argmax_or_null,
                             int64_t nq, int64_t lq, int64_t np, int64_t lp,
                             int nplanes, int64_t p_stride, int64_t p_plane_stride,
                             const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null,
                             int32_t* qlist_ws_or_null, void* hip_stream);

/* The same forward for a device-side SUBSET of the queries: only the queries qsel[0 .. *qsel_count) (ascending indices into the
 * nq rows of Qplanes, both in device memory) are scored and only their rows of `out` are written; workgroups whose queries all lie
 * beyond *qsel_count leave at once.  The count is read on the device: the host needs no synchronisation to know which queries a
 * preceding kernel selected (the score-row cache below).  lq <= 32 and lq != 1-packed layouts only (EVDR_ERR_SHAPE otherwise); no argmax. */
EVDR_API int evdr_maxsim_fwd_prepared_subset(const uint16_t* Qplanes, const uint16_t* Pplanes,
                             const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                             float* out, int64_t out_stride,
                             int64_t nq, int64_t lq, int64_t np, int64_t lp,
                             int nplanes, int64_t p_stride, int64_t p_plane_stride,
                             const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null,
                             const int32_t* qsel, const int32_t* qsel_count, void* hip_stream);

/* ---- search over a page SUBSET: one list of pages shared by the whole query batch ------------------------------------
 * evdr_maxsim_fwd_pages: out[q][i] = the score of query q and page pages[i], i < m.  pages: m LOCAL page indices (into the np pages
 * of Pplanes) in device memory, any order, duplicates allowed and each scored.  An entry outside [0, np) is a HOLE: out[q][i] = -inf
 * for every q, and the entry never becomes an address (nothing is read for it).  Operands as evdr_maxsim_fwd_prepared with nplanes 1
 * (bf16) or 2 (fp16 hi/lo; 4 -> EVDR_ERR_SHAPE), no argmax; every query shape that entry takes: lq = 1 (packed 32 to a tile) and
 * lq > 32 (32-token slices; qlist_ws_or_null, (nq + 1) int32, is REQUIRED then: EVDR_ERR_WORKSPACE).  out: (nq, m) fp32 with row
 * stride out_stride >= m.  The launch has the exhaustive launch's geometry over the m list positions (query groups x chunks of the
 * list, eight waves scoring their own queries), so it costs what m contiguous pages cost.  Scores follow every rule of the exhaustive
 * forward (-1e4 fill, exact 0 of an all-masked page, page-flag / query NaN rules, per-call plane shifts) and are BIT-EQUAL to what
 * evdr_maxsim_fwd_prepared writes for that (query, page) over the whole corpus with the same query batch, at every page length and
 * for both corpus kinds: also where that launch runs the flat ring kernel (bf16 pages shorter than 225 patches), which chains the
 * same products in the same order (tests/test_gpu_subset.py asserts it at 7, 33, 224, 225 and 1030 patches).  nq = 0 or m = 0: EVDR_OK, nothing written; np = 0 with m > 0:
 * EVDR_ERR_SHAPE.  The list is consumed on the device: no allocation, no host synchronisation, graph-capture safe. */
EVDR_API int evdr_maxsim_fwd_pages(const uint16_t* Qplanes, const uint16_t* Pplanes,
                             const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                             const int32_t* pages, int64_t m, float* out, int64_t out_stride,
                             int64_t nq, int64_t lq, int64_t np, int64_t lp,
                             int nplanes, int64_t p_stride, int64_t p_plane_stride,
                             const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null,
                             int32_t* qlist_ws_or_null, void* hip_stream);

/* ---- score-row cache of a FROZEN page tensor (mainv2_iter_distill_infonce.py:282-283) --------------------------------------------
 * The reference's step re-scores the frozen teacher pages for every batch, every epoch, although a query's teacher scores never
 * change ("caching them is a legal, result-identical optimisation").  evdr_maxsim_fwd_prepared_cached is
 * evdr_maxsim_fwd_prepared (no argmax) through a (query row -> score row) cache that lives on the device, for ONE prepared page
 * tensor, without any host synchronisation.  Three launches on `hip_stream`:
 *   lookup + plan   one workgroup per query: 64-bit hash of (query row bits, mask row, plane shift k of the batch), probe of an
 *                   open-addressing table, and -- on a hash match -- a comparison of the FULL stored row and mask, so that a hash
 *                   collision is a miss.  The last workgroup to finish turns the misses, in ascending order, into the query list of
 *                   the forward and, while the cache has room, gives each a fresh entry and enters it into the table;
 *   forward         evdr_maxsim_fwd_prepared_subset over that device-side list (all hits: every workgroup leaves at once);
 *   exchange        rows of hits are copied out of the cache into `out`, rows of stored misses (score row, query row, mask) into it.
 * The plane shift k (evdr_split_f32 scales a batch by one power of two taken from ITS absmax) is part of the key: a query that comes
 * back in a batch with another absmax exponent is scored again, so a cached row always equals, bit for bit, the row
 * evdr_maxsim_fwd_prepared would write for this very call.  Nothing is evicted: a full cache keeps its entries and later misses are
 * just scored.  One cache belongs to one stream order of calls (never two streams at once).
 * Qrows: the batch as the caller holds it, (nq, cache->lq, 128) dense, cache->row_bytes per query (fp32 or bf16) -- its bits are the
 * key; Qplanes / q_amax: the same batch as the forward takes it.  workspace: evdr_qcache_workspace(nq) bytes, ZEROED by the caller
 * before its first use and then left to the library (it carries a ticket word between calls; after a call the int32 at byte offset
 * evdr_qcache_workspace(nq) - 256 holds the number of queries that had to be scored).
 * The struct is plain host memory; all of its pointers are device memory owned by the caller. */
typedef struct EvdrQCache {
    int32_t*  slots;        /* (n_slots) open-addressing table: 0 = empty, else entry index + 1; zero-initialised by the caller */
    int64_t   n_slots;      /* a power of two, >= 2 * capacity                                                                      */
    uint64_t* ent_hash;     /* (capacity)                                                                                         */
    int32_t*  ent_k;        /* (capacity) plane shift the entry was scored with                                                   */
    uint8_t*  ent_q;        /* (capacity, row_bytes) query rows as the caller's dtype holds them                                  */
    uint8_t*  ent_mask;     /* (capacity, lq) mask rows, 0 / 1                                                                     */
    float*    ent_scores;   /* (capacity, np)                                                                                     */
    int32_t*  n_entries;    /* (1) entries handed out so far; zero-initialised by the caller                                      */
    int64_t   capacity, row_bytes, lq, np;
    uint64_t  hash_mask;    /* all ones; tests narrow it (0 = every row collides) to exercise the full-row comparison             */
} EvdrQCache;
EVDR_API size_t evdr_qcache_workspace(int64_t nq);
EVDR_API int evdr_maxsim_fwd_prepared_cached(const EvdrQCache* cache, const void* Qrows, const uint16_t* Qplanes, const uint16_t* Pplanes,
                             const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                             float* out, int64_t out_stride, int64_t nq, int64_t lp,
                             int nplanes, int64_t p_stride, int64_t p_plane_stride,
                             const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null,
                             void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- A6: autograd of A1 w.r.t. P (loss.backward(), mainv2_iter_distill_infonce.py:290) ---------------
 * dP[p,m,:] = sum_{q,n} g[q,p] * qmask[q,n] * has(p) * [m == argmax[q,p,n]] * Q[q,n,:]
 * g (nq,np) fp32; Q (nq,lq,128) fp32; argmax from evdr_maxsim_fwd; dP (np,lp,128) fp32 is
 * OVERWRITTEN (every element written, masked rows get exact zeros). */
EVDR_API int evdr_maxsim_bwd(const float* g, const float* Q, const uint8_t* qmask, const uint8_t* pmask,
                    const uint16_t* argmax, float* dP,
                    int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t d, void* hip_stream);

/* ---- A6, query side: autograd of A1 w.r.t. Q (the reference's function is differentiable in both arguments) ---------
 * dQ[q,n,:] = qmask[q,n] * sum_p g[q,p] * has(p) * P[p, argmax[q,p,n], :]
 * g (nq,np) fp32; P (np,lp,128) fp32 dense; argmax from evdr_maxsim_fwd; dQ (nq,lq,128) fp32 is OVERWRITTEN.
 * Deterministic: with few (query, token) pairs the page range is split over workgroups, whose partial sums go to the
 * workspace and are added in a fixed order (no float atomics) -- the same bits run after run. */
EVDR_API size_t evdr_maxsim_bwd_q_workspace(int64_t nq, int64_t lq, int64_t np, int64_t lp);
EVDR_API int evdr_maxsim_bwd_q(const float* g, const float* P, const uint8_t* qmask, const uint8_t* pmask,
                      const uint16_t* argmax, float* dQ,
                      int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t d,
                      void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- A6 + A4 backward + the optimizer of A7 in ONE launch (mainv2_iter_distill_infonce.py:279,290-291) ---------------
 * Same gather as evdr_maxsim_bwd, but the gradient w.r.t. the normalised pages stays in LDS and the epilogue applies
 * (1) the backward of  y = m x / (||m x|| + l2_eps)  (l2_normalize(Pbar * pmask), utils/preprocess_data.py:8-9) and
 * (2) torch.optim.AdamW's update (decoupled weight decay, bias correction with `step` = 1 for the first update)
 * in place on the raw parameter x (np,lp,128) and its moments exp_avg / exp_avg_sq (same shape, zero-initialised).
 * pmask doubles as the row mask m.  Result-identical to backward() + AdamW.step() of the reference's step.
 * lr / betas / eps / weight_decay are DOUBLES, as Python hands them to torch: the derived constants (1 - lr * weight_decay,
 * 1 - beta, lr / (1 - beta1^step), ...) are formed in double on the host like torch forms them and only then rounded to fp32
 * (1 - float(0.999) would be off by 1.3e-5 relative). */
EVDR_API int evdr_maxsim_bwd_adamw(const float* g, const float* Q, const uint8_t* qmask, const uint8_t* pmask,
                          const uint16_t* argmax, float* x, float* exp_avg, float* exp_avg_sq,
                          int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t d,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                          float l2_eps, const void* adamw_state_or_null, void* hip_stream);
/* The same launch, also emitting the NEXT forward's operands: l2_normalize(m * x_new) of the updated parameter as the fp16
 * hi/lo planes evdr_l2norm_fwd_split would produce from it (next_planes: 2 x np x lp x 128 fp16, next_amax: their absmax
 * word; both or neither), non-finite updated rows reported in pageflags_or_null (np words, bit 3) like there.  A training
 * loop that keeps the planes (mainv2_iter_distill_infonce.py:279 normalises the parameter at the top of EVERY step) saves
 * the separate normalise pass: one read of x and one launch per step. */
EVDR_API int evdr_maxsim_bwd_adamw_planes(const float* g, const float* Q, const uint8_t* qmask, const uint8_t* pmask,
                                 const uint16_t* argmax, float* x, float* exp_avg, float* exp_avg_sq,
                                 int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t d,
                                 double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                                 float l2_eps, const void* adamw_state_or_null,
                                 void* next_planes_or_null, uint32_t* next_amax_or_null, uint32_t* pageflags_or_null,
                                 void* hip_stream);
/* Device-resident step counter for the calls above, so that a whole training step can be captured in a HIP graph and
 * replayed without a scalar from the host: adamw_state = 16 bytes of device memory {int64 step; float bc1; float bc2_sqrt},
 * zero-initialised.  evdr_adamw_advance does step += 1 and refreshes the bias corrections; evdr_maxsim_bwd_adamw with a
 * non-NULL state reads them from there and ignores its `step` argument. */
EVDR_API int evdr_adamw_advance(void* adamw_state, double beta1, double beta2, void* hip_stream);
/* The optimizer of A7 on its own (utils/utils.py:78-80 -> torch.optim.AdamW at torch's default betas / eps, amsgrad off), for
 * callers that keep the reference's autograd step (loss.backward(); opt.step(), mainv2_iter_distill_infonce.py:290-291): one
 * pass over grad, x, exp_avg, exp_avg_sq (n fp32 elements each, 16-byte aligned, dense), in place; `step` >= 1 is the count
 * INCLUDING this update (bias corrections 1 - beta^step).  torch's default (foreach) form makes eight passes. */
EVDR_API int evdr_adamw_step(const float* grad, float* x, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                    double beta2, double eps, double weight_decay, int64_t step, void* hip_stream);

/* ---- A4: l2_normalize (utils/preprocess_data.py:8-9) fused with the page mask, forward and backward -----------------
 * y[r,:] = m_r * x[r,:] / (||m_r * x[r,:]||_2 + eps), m_r = rowmask[r] != 0 (NULL = all ones); rows x 128 fp32.
 * norm_or_null receives ||m_r x_r|| (needed by the backward).  One call replaces the `Pbar * pmask` multiply and
 * the four ATen kernels of l2_normalize on the training step (mainv2_iter_distill_infonce.py:279).
 * Backward: dx = m * ( gy/(n+eps) - (m x) * ((m x).gy) / (n (n+eps)^2) ), with the norm's subgradient 0 at n = 0
 * (what torch autograd yields for x / (x.norm() + eps)). */
EVDR_API int evdr_l2norm_fwd(const float* x, const uint8_t* rowmask_or_null, int64_t rows, int64_t d, float eps,
                    float* y, float* norm_or_null, void* hip_stream);
EVDR_API int evdr_l2norm_bwd(const float* gy, const float* x, const uint8_t* rowmask_or_null, const float* norm,
                    int64_t rows, int64_t d, float eps, float* dx, void* hip_stream);
/* evdr_l2norm_fwd that also (or only: y_or_null = NULL) emits y in evdr_split_f32's format -- fp16 hi/lo planes
 * (2 * rows * 128 uint16) + the absmax word, here the constant bits of 1.0f since |y| <= 1 -- ready for
 * evdr_maxsim_fwd_prepared(nplanes = 2): the normalised student pages of a training step go to the scorer without an
 * fp32 round trip through HBM (mainv2_iter_distill_infonce.py:279-283).  pageflags_or_null (with rows_per_page = lp): a
 * non-finite unmasked row sets bit 3 of its page's flag word on the way (see evdr_flag_nonfinite). */
EVDR_API int evdr_l2norm_fwd_split(const float* x, const uint8_t* rowmask_or_null, int64_t rows, int64_t d, float eps,
                          float* y_or_null, float* norm_or_null, uint16_t* planes, uint32_t* amax_bits,
                          uint32_t* pageflags_or_null, int64_t rows_per_page, void* hip_stream);

/* ---- A8: top-k per query row, replaces the Nq*N .item() loop (mainv2_iter_distill_infonce.py:311-317)
 * scores (nq, n) fp32 with row stride `row_stride`; idx_map_or_null (nq, n) int32 maps a column to
 * the index to report (used when merging per-shard candidate lists), else column + idx_base.
 * Order: score descending, reported index ascending on ties.  When equal scores straddle the cut, the ones with the lowest
 * reported indices among them are kept, whatever the order of the columns (an idx_map need not ascend along the row; entries
 * that report the same index are interchangeable).  k <= EVDR_TOPK_MAX.
 * top_scores/top_idx (nq, k); rows with n < k are padded with (-inf, -1).
 * workspace_or_null (evdr_topk_workspace bytes; 0 = not needed): lets a few long rows be ranked by many workgroups
 * (per-segment candidates, then a merge) instead of one workgroup per row; same result either way. */
EVDR_API size_t evdr_topk_workspace(int64_t nq, int64_t n, int k);
EVDR_API int evdr_topk(const float* scores, const int32_t* idx_map_or_null, int64_t nq, int64_t n,
              int64_t row_stride, int32_t idx_base, int k,
              float* top_scores, int32_t* top_idx,
              void* workspace_or_null, size_t workspace_bytes, void* hip_stream);

/* A1 + A8 in one call on a prepared corpus: scores land in `workspace` (nq*np floats). */
EVDR_API size_t evdr_maxsim_topk_workspace(int64_t nq, int64_t np);
EVDR_API int evdr_maxsim_topk(const uint16_t* Qplanes, const uint16_t* Pplanes,
                     const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                     int64_t nq, int64_t lq, int64_t np, int64_t lp,
                     int nplanes, int64_t p_stride, int64_t p_plane_stride,
                     const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null,
                     int32_t idx_base, int k, float* top_scores, int32_t* top_idx,
                     void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- prefiltered top-k on an fp32 corpus (nplanes = 2): the same answer as evdr_maxsim_topk, bit for bit ---------------------
 * Every page is scored with the hi planes only (one fp16 product per k-step instead of three); a rigorous per-query bound E_q on
 * |exact - coarse| then keeps only the pages that can still reach the top k,
 *     C_q = { p : coarse[q][p] >= (k-th coarse score of q) - 2 E_q }  u  { p : coarse[q][p] is NaN },
 * and those are re-scored with the exhaustive kernel's own fp16 hi/lo arithmetic (same bits per pair) and ranked with evdr_topk's order.
 * A query whose k-th coarse score or E_q is not finite, or whose |C_q| exceeds `capacity`, is scored exhaustively instead (on the device:
 * no host synchronisation anywhere).  Derivation of E_q: csrc/prefilter.hip and DESIGN.md.  lq <= 32; nplanes must be 2.
 *
 * evdr_prefilter_corpus_bound: bound[0] = H, bound[1] = L = the largest |hi| / |lo| plane row norm over the valid patches of the pages
 *   without a non-finite flag (scaled units of the planes, rounded up): a property of the prepared corpus, computed once.  The values
 *   of a corpus are a valid bound for any subset of its pages (a shard).  2 floats of device memory.
 * evdr_prefilter_query_bound: eq[q] = E_q in real units, from the query planes of the call (Qplanes / q_amax as for the forward).
 * evdr_maxsim_fwd_coarse: out[q][p] = the coarse score (hi planes only, otherwise the forward's semantics: -1e4 fill, NaN rules).
 * evdr_maxsim_topk_prefilter: top_scores / top_idx as evdr_maxsim_topk (idx_base added, (-inf, -1) padding when np < k);
 *   capacity >= k candidates per query; stats_or_null: (nq + 1) int32 -- per query |C_q| (-1: non-finite k-th score or E_q), then the
 *   number of queries that fell back to the exhaustive pass.  workspace: evdr_maxsim_topk_prefilter_workspace bytes. */
EVDR_API int evdr_prefilter_corpus_bound(const uint16_t* Pplanes, const uint32_t* tilemask, const uint32_t* pageflags,
                                int64_t np, int64_t lp, int64_t p_stride, int64_t p_plane_stride, float* bound, void* hip_stream);
EVDR_API int evdr_prefilter_query_bound(const uint16_t* Qplanes, const uint8_t* qmask, int64_t nq, int64_t lq,
                               const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null, const float* bound,
                               float* eq, void* hip_stream);
EVDR_API int evdr_maxsim_fwd_coarse(const uint16_t* Qplanes, const uint16_t* Pplanes,
                           const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                           float* out, int64_t out_stride, int64_t nq, int64_t lq, int64_t np, int64_t lp,
                           int64_t p_stride, int64_t p_plane_stride,
                           const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null, void* hip_stream);
EVDR_API size_t evdr_maxsim_topk_prefilter_workspace(int64_t nq, int64_t np, int capacity);
EVDR_API int evdr_maxsim_topk_prefilter(const uint16_t* Qplanes, const uint16_t* Pplanes,
                               const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                               int64_t nq, int64_t lq, int64_t np, int64_t lp,
                               int nplanes, int64_t p_stride, int64_t p_plane_stride,
                               const uint32_t* q_amax, const uint32_t* p_amax, const float* bound,
                               int32_t idx_base, int k, int capacity, float* top_scores, int32_t* top_idx,
                               int32_t* stats_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- candidate scoring and top-R selection: rerank what a first stage proposed ----------------------------------------
 * evdr_maxsim_fwd_candidates: out[q][i] = the score of query q and page cand[q][i] - idx_base, for every entry with
 *   idx_base <= cand[q][i] < idx_base + np.  Any other entry (-1, another shard's page, garbage) is a HOLE: out[q][i] = -inf and no
 *   memory is read for it; holes may sit anywhere in a row, duplicates are allowed and each is scored.  cand: (nq, r) int32, dense;
 *   out: (nq, r) fp32 with row stride out_stride; cand_clean_or_null: (nq, r) int32, receives cand with its holes set to -1 (the
 *   idx_map of an evdr_topk over out).  Operands as evdr_maxsim_fwd_prepared with nplanes 1 (bf16) or 2 (fp16 hi/lo; 4 ->
 *   EVDR_ERR_SHAPE), lq <= 32, 1 <= r <= EVDR_SELECT_MAX.  Scores follow every rule of the exhaustive forward (-1e4 fill, exact 0 of
 *   an all-masked page, page-flag / query NaN rules, per-call plane shifts), and a candidate's score is BIT-EQUAL to what
 *   evdr_maxsim_fwd_prepared writes for that (query, page) in a launch over the whole corpus with the same query batch wherever that
 *   launch runs the staged kernel: fp16 hi/lo planes at every page length, bf16 pages of at least 8 tiles (225 patches).  (Shorter
 *   bf16 pages go through the flat ring kernel there)  Lists and counts are consumed on the device: no host
 *   synchronisation.  workspace: evdr_maxsim_fwd_candidates_workspace(nq, r) bytes.
 * evdr_select_topr: for each row of the (nq, n) fp32 block `scores` (row stride row_stride) the r columns with the largest order key
 *   -- evdr_topk's: NaN ranks first, -0 ties with +0 --, ties at the cut broken towards the lower index, written to top_idx (nq, r) in
 *   ASCENDING index order (+ idx_base) and padded with -1 when n < r.  1 <= r <= EVDR_SELECT_MAX; for r <= EVDR_TOPK_MAX the set is
 *   exactly evdr_topk's. */
EVDR_API size_t evdr_maxsim_fwd_candidates_workspace(int64_t nq, int r);
EVDR_API int evdr_maxsim_fwd_candidates(const uint16_t* Qplanes, const uint16_t* Pplanes,
                               const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                               const int32_t* cand, int r, int32_t idx_base, float* out, int64_t out_stride,
                               int32_t* cand_clean_or_null, int64_t nq, int64_t lq, int64_t np, int64_t lp,
                               int nplanes, int64_t p_stride, int64_t p_plane_stride,
                               const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null,
                               void* workspace, size_t workspace_bytes, void* hip_stream);
EVDR_API int evdr_select_topr(const float* scores, int64_t nq, int64_t n, int64_t row_stride, int32_t idx_base, int r,
                     int32_t* top_idx, void* hip_stream);

/* ---- token alignment: which patches produced a score ------------------------------------------------------------------
 * evdr_maxsim_align: for query q and every page its own list names, the best patch of each query token -- value and index -- and, if
 *   asked, the page's heat map.  cand: (nq, r) int32 GLOBAL page indices, dense, 1 <= r <= EVDR_SELECT_MAX; the page of entry
 *   cand[q][i] is p = cand[q][i] - idx_base, and an entry outside [idx_base, idx_base + np) is a HOLE that never becomes an address
 *   (evdr_maxsim_fwd_candidates' rule); duplicates are each aligned.  Operands as evdr_maxsim_fwd_candidates with nplanes 1 (bf16) or 2
 *   (fp16 hi/lo with the two absmax words; 4 -> EVDR_ERR_SHAPE), 1 <= lq <= 32; planes 16-byte aligned, p_stride and p_plane_stride
 *   multiples of 8.  Outputs, all dense: sim (nq, r, lq) fp32, patch (nq, r, lq) int32, heat_or_null (nq, r, lp) fp32.
 * For a real entry with page p, pmask = the mask evdr_pack_pmask packed:
 *   sim[q][i][n]   = max_m ( pmask[p][m] ? Q[q][n][:] . P[p][m][:] : -1e4 ), the per-token quantity the forward sums, and patch[q][i][n]
 *                    the FIRST index m attaining it (a masked patch attains -1e4 at its own index): the index rule of the arg-max output
 *                    of evdr_maxsim_fwd_prepared, also where every valid product lies below -1e4 (the first masked patch);
 *   heat[q][i][m]  = max over the VALID tokens n of Q[q][n][:] . P[p][m][:] for a valid patch m, -inf for a masked patch, -inf
 *                    everywhere when the query has no valid token.  The first index of its maximum is the hard token of
 *                    mainv3_iter_liscore_QA_hardtoken.py:413-417; it equals patch[] of the valid token with the largest sim.
 * Fill values:
 *   masked query token                       sim = 0, patch = -1;
 *   page without a valid patch               sim = 0, patch = -1 for every token (the forward's exact 0), heat = -inf;
 *   hole                                     sim = -inf, patch = -1, heat = -inf;
 *   a pair the forward scores NaN (page flag bit 3, or a NaN / Inf element in any token of the query, on a page with a valid patch:
 *   "Non-finite inputs" above)               sim = NaN in every valid token, patch = -1, heat = NaN.
 * Order: the products of one (token, patch) pair are chained in one fixed order -- plane products lo x hi, hi x lo, hi x hi (page x
 *   query), the four 32-column steps ascending inside each, fp32 accumulation in the MFMA -- that does not depend on the patch's place
 *   in the page, on the wave that owns its tile or on whether heat is requested, nor on the query mask (a masked token's products are
 *   formed like any other's and only kept out of sim, patch and the heat maximum); fp16 planes are brought back to real units by one
 *   exact power of two per product sum.  So identical patch rows give identical bits (ties are exact and go to the LOWER patch index),
 *   sim and patch are the same bits with and without heat, and every launch repeats the last one's bits.  Bit-equality of sim with the
 *   forward's internal maxima is NOT promised (values agree to fp32 accumulation error; sums over tokens to the score gate of 1e-4).
 * One launch, one workgroup per (query, list position): no atomics, no workspace, no allocation, no host synchronisation,
 *   graph-capture safe.  Status, all BEFORE any HIP call: EVDR_ERR_ARG for negative sizes, r outside 1..EVDR_SELECT_MAX, nplanes other
 *   than 1, 2, 4, null cand / sim / patch (and, with np > 0, null planes or words), bad strides or alignment; EVDR_ERR_SHAPE for
 *   nplanes = 4, lq outside 1..32, lp = 0 with np > 0, nq * r > 2^31 - 1.  nq = 0: EVDR_OK, nothing written.  np = 0: every entry is a hole. */
EVDR_API int evdr_maxsim_align(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask,
                               const uint32_t* tilemask, const uint32_t* pageflags, const int32_t* cand, int64_t r, int32_t idx_base,
                               float* sim, int32_t* patch, float* heat_or_null,
                               int64_t nq, int64_t lq, int64_t np, int64_t lp, int nplanes, int64_t p_stride, int64_t p_plane_stride,
                               const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null, void* hip_stream);

/* ---- document-level search: page scores collapsed to documents ------------------------------------------------------
 * The rule, shared by the three calls.  Scores are compared by evdr_topk's order key (NaN of either sign first, -0 ties with +0); a
 *   score of -inf -- the hole value of the page-list and candidate paths -- means ABSENT.  A document's score is that of the page with
 *   the largest key among its listed pages; among the pages attaining it the one with the LOWEST reported page index is its best
 *   page, whatever order the pages are listed in.  A document with no listed page, or with -inf pages only, is absent: score -inf,
 *   best page -1, and it takes a result slot only as padding.  Result rows: key descending, DOCUMENT id ascending on ties, cut at k,
 *   padded with (-inf, document -1, page -1).  A reported score is the float of the winning key: -0.0 comes back as +0.0, NaN as a NaN.
 * evdr_doc_max: a segmented arg-max over the (nq, n) fp32 block `scores` (row stride row_stride).  members: (nm) int32 COLUMNS of the
 *   block in CSR order -- documents ascending, any order inside a document, duplicates allowed; a value outside [0, n) is a hole that
 *   never becomes an address.  offsets: (n_docs + 1) int32, document d owns members[offsets[d] : offsets[d + 1]] (its start is clamped
 *   to [0, nm] and its end to [start, nm], so no offset becomes an address outside members either).  The index a column reports is
 *   (idx_map_or_null ? idx_map[column] : column) + idx_base, idx_map_or_null: (n) int32 (the list of a page-subset search).
 *   Outputs: doc_scores (nq, n_docs) fp32 with row stride doc_stride, doc_best (nq, n_docs) int32, dense.  ONE launch, no workspace, no
 *   atomics: the same bits on every launch.  A workgroup takes EVDR_DOC_BLOCK documents x EVDR_DOC_ROWS rows; documents of fewer than
 *   EVDR_DOC_LONG pages take a lane each, longer ones a wave each.
 * evdr_collapse_topk: the top k distinct documents of each row of a list.  scores (nq, r) fp32 with row stride row_stride, page (nq, r)
 *   int32 reported page indices, dense; the document of an entry comes from EXACTLY one of doc_or_null (nq, r) int32, dense -- any
 *   non-negative id, sparse ids up to 2^31 - 1 included, a negative id marks a hole -- and doc_of_page_or_null (np) int32 with idx_base:
 *   the document is doc_of_page[page - idx_base], and an entry outside [idx_base, idx_base + np) is a hole that never becomes an
 *   address (evdr_maxsim_fwd_candidates' rule; a negative doc_of_page value is a page without a document, a hole too).  Both or
 *   neither: EVDR_ERR_ARG.  1 <= r <= EVDR_SELECT_MAX, 1 <= k <= EVDR_TOPK_MAX.  top_scores / top_doc / top_page: (nq, k), dense.  One
 *   workgroup per row with the whole list in LDS, no workspace, no atomics; duplicates are harmless and the result does not depend on
 *   the order of the list.
 * evdr_doc_topk: evdr_doc_max into `workspace`, evdr_topk over the (nq, n_docs) block, then the best page of every returned document
 *   and the padding rule -- three launches (four when evdr_topk splits long rows).  workspace: evdr_doc_topk_workspace(nq, n_docs) bytes
 *   (EVDR_ERR_WORKSPACE when missing or smaller).  n_docs = 0: every row is padding.
 * All three: no allocation, no host synchronisation, graph-capture safe.  Status, all BEFORE any HIP call: EVDR_ERR_ARG for negative
 *   sizes, k or r out of range, row_stride < n (evdr_collapse_topk: < r), doc_stride < n_docs, null pointers, both or neither document
 *   forms; EVDR_ERR_SHAPE for nq, n, nm, n_docs or np above 2^31 - 1 or more than 2^31 - 1 workgroups.  nq = 0: EVDR_OK, nothing written. */
EVDR_API int evdr_doc_max(const float* scores, const int32_t* members, const int32_t* offsets, const int32_t* idx_map_or_null,
                          int64_t nq, int64_t n, int64_t row_stride, int64_t nm, int64_t n_docs, int32_t idx_base,
                          float* doc_scores, int64_t doc_stride, int32_t* doc_best, void* hip_stream);
EVDR_API int evdr_collapse_topk(const float* scores, const int32_t* page, const int32_t* doc_or_null,
                                const int32_t* doc_of_page_or_null, int64_t np, int32_t idx_base, int64_t nq, int r,
                                int64_t row_stride, int k, float* top_scores, int32_t* top_doc, int32_t* top_page, void* hip_stream);
EVDR_API size_t evdr_doc_topk_workspace(int64_t nq, int64_t n_docs);
EVDR_API int evdr_doc_topk(const float* scores, const int32_t* members, const int32_t* offsets, const int32_t* idx_map_or_null,
                           int64_t nq, int64_t n, int64_t row_stride, int64_t nm, int64_t n_docs, int32_t idx_base, int k,
                           float* top_scores, int32_t* top_doc, int32_t* top_page, void* workspace, size_t workspace_bytes,
                           void* hip_stream);

/* ---- fp8 corpora: OCP e4m3fn bytes, scored with the block-scaled 16x16x128 MFMA (opt-in) ----------------------------
 * Quantisation (evdr_quantize_fp8).  Each GROUP of rows_per_group rows (one page, or one query) gets its own power of two: k = the largest
 * integer with amax * 2^k <= 448, amax = max |x| over the group's FINITE elements (k = 0 when it has no finite non-zero element).  Each
 * element is stored as the round-to-nearest-even e4m3fn byte of x * 2^k (subnormals included) -- bit for bit torch's
 * (x.float() * 2.0**k).to(torch.float8_e4m3fn), for fp32 and for bf16 inputs --, columns d..127 are zero, a NaN / +-Inf element becomes
 * the NaN byte 0x7F | sign.  x: (groups * rows_per_group, d) dense, d <= 128; x8: (groups * rows_per_group, 128) bytes; shift: (groups)
 * int32 k.  A query's bytes never depend on the other queries of its batch, a page's never on the rest of the corpus.
 * Scores (evdr_maxsim_fwd_fp8).  out[q][p] = sum_t qmask[q,t] * has(p) * max( max_{valid j} deq(Q8[q,t]) . deq(P8[p,j]), -1e4 if p has a
 * masked patch ), deq(x8) = e4m3(x8) * 2^-k: the products are exact in fp32, the sum over the 128 columns is accumulated in fp32 by the
 * MFMA, and each token's max is brought back by ONE exact ldexp with -(k_q + k_p) (no intermediate over- or underflow).  Masks, the
 * -1e4 fill of masked patches, the exact 0 of an all-masked page, out_stride / column blocks and 32-token slices with qlist_ws_or_null
 * ((nq + 1) int32, lq > 32) are those of evdr_maxsim_fwd_prepared.  P8: (np, lp, 128) bytes, p_stride BYTES between pages (a multiple of
 * 16); Q8: (nq, lq, 128) dense; q_shift (nq) / p_shift (np) from evdr_quantize_fp8.  Non-finite inputs as for the other forwards: page
 * flag bit 3 (evdr_flag_nonfinite run on the SOURCE pages before they are quantised) gives a NaN column; a NaN byte in any token of a
 * query, masked tokens included, gives a NaN row on every page with a valid patch.  The same bits from launch to launch; no argmax.
 * Accuracy: the quantisation itself is the approximation (3 mantissa bits: about 2^-4 relative per element); it is NOT a bound on
 * the fp32 scores, and fp8 top-k is not exact against bf16 / fp32 top-k.
 * Scores of a page list (evdr_maxsim_fwd_fp8_pages).  The operands of evdr_maxsim_fwd_fp8 and the list of
 * evdr_maxsim_fwd_pages: pages (m) int32 LOCAL page indices in device memory, shared by the whole query batch, in any order,
 * duplicates allowed and each scored.  out: (nq, m) fp32 with row stride out_stride >= m; out[q][i] = the score of query q and page
 * pages[i] for 0 <= pages[i] < np -- BIT-EQUAL to what evdr_maxsim_fwd_fp8 writes for that (query, page) in a launch over the whole
 * corpus with the same query batch (the instance is chosen from nq and lp alone, never from m) --; any other entry is a HOLE:
 * out[q][i] = -inf for every q, NaN queries included, and the entry never forms an address.  Status, all before any device work:
 * nq = 0 or m = 0 -> EVDR_OK, nothing written, null pointers accepted; np = 0 with m > 0 -> EVDR_ERR_SHAPE; lq > 32 without
 * qlist_ws_or_null ((nq + 1) int32) -> EVDR_ERR_WORKSPACE; null pointers, m < 0, out_stride < m, p_stride not a multiple of 16 or
 * < lp * 128 -> EVDR_ERR_ARG.  No allocation, no host synchronisation, graph-capture safe; the list is consumed on the device. */
EVDR_API int evdr_quantize_fp8(const void* x, int dtype, int64_t groups, int64_t rows_per_group, int64_t d, uint8_t* x8, int32_t* shift,
                               void* hip_stream);
EVDR_API int evdr_maxsim_fwd_fp8(const uint8_t* Q8, const uint8_t* P8, const uint8_t* qmask, const uint32_t* tilemask,
                                 const uint32_t* pageflags, float* out, int64_t out_stride, int64_t nq, int64_t lq, int64_t np, int64_t lp,
                                 int64_t p_stride, const int32_t* q_shift, const int32_t* p_shift, int32_t* qlist_ws_or_null,
                                 void* hip_stream);
EVDR_API int evdr_maxsim_fwd_fp8_pages(const uint8_t* Q8, const uint8_t* P8, const uint8_t* qmask, const uint32_t* tilemask,
                                       const uint32_t* pageflags, const int32_t* pages, int64_t m, float* out, int64_t out_stride,
                                       int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t p_stride,
                                       const int32_t* q_shift, const int32_t* p_shift, int32_t* qlist_ws_or_null, void* hip_stream);

/* ---- growable corpus: pages prepared IN PLACE in a corpus allocated for `capacity` pages -----------------------------
 * evdr_corpus_ingest writes b source pages into a resident corpus whose planes, tile words, flag words (and fp8 shifts) were allocated
 * for `capacity` pages of lp patches: ONE launch, one workgroup per page, ONE read of the source page and its mask bytes, no
 * allocation, no host synchronisation, graph-capture safe.  The searchers are then called with np = the pages filled so far.
 * Source: src (b, lp_src, d_src) of src_dtype EVDR_F32 / EVDR_BF16 / EVDR_F16, dense rows, src_stride ELEMENTS between pages;
 *   pmask_or_null (b, lp_src) bytes.  lp_src <= lp: patches [lp_src, lp) are written as zeros and masked.  d_src <= 128: columns
 *   d_src..127 are zero.  (d_src a multiple of 8 with src and src_stride 16-byte aligned takes 16-byte loads; anything else is read
 *   element by element, same result.)
 * Corpus: planes of `kind` with p_stride elements between pages (p_plane_stride between the hi and lo plane), tilemask
 *   (capacity, ceil(lp / 32)), pageflags (capacity), shift_or_null (capacity), p_amax_or_null (1 word):
 *   EVDR_CORPUS_BF16     one bf16 plane; the source must be EVDR_BF16 and is copied;
 *   EVDR_CORPUS_F16_HILO fp16 hi/lo planes: evdr_split_f32's split of the page, with the power of two taken from the CORPUS's absmax
 *                        word p_amax (required), NOT from the incoming pages -- the kernels read that word only through its exponent;
 *   EVDR_CORPUS_FP8      e4m3 bytes and the page's shift (shift_or_null required), exactly evdr_quantize_fp8's with one group per
 *                        page: the page amax is taken over all rows as given, masked or not;
 *   EVDR_CORPUS_F16_WIDE width-256 corpora (four planes) are not covered: EVDR_ERR_SHAPE.
 *   Every element offset must keep 16-byte alignment: planes 16-byte aligned, p_stride and p_plane_stride multiples of 8 (16 for fp8).
 * Words: the tile words and the flag word of each page are bit for bit evdr_pack_pmask's (bits 0, 1, the one-range encoding of bits 2,
 *   4..15, 16..31), with bit 3 added when a VALID patch holds NaN or +-Inf (evdr_flag_nonfinite's rule).  The workgroup owns its
 *   page: plain stores, no atomics.
 * Destination: pages first_page .. first_page + b - 1, or, with dst_pages_or_null given, page dst_pages[i] for source page i (b int32
 *   LOCAL page indices in device memory; first_page is ignored).  An entry outside [0, capacity) is a HOLE: that source page is
 *   skipped, nothing is written for it and the entry never becomes an address.  Duplicate entries race; keep them distinct.
 * status_or_null (1 word of device memory, EVDR_CORPUS_F16_HILO only; zero it first): bit 0 is set when a FINITE source element has a
 *   larger exponent than the corpus's absmax word, i.e. its scaled value leaves the [2^14, 2^15) window the planes are laid out for
 *   (such an element may overflow the hi plane).  Non-finite elements do not count here: they are what flag bit 3 is for.
 * Status, all BEFORE any HIP call: EVDR_ERR_ARG for a bad dtype / kind, negative sizes, null pointers, a bf16 corpus with a non-bf16
 *   source, an fp16-plane corpus without p_amax, an fp8 corpus without shifts, first_page < 0 or first_page + b > capacity (without a
 *   list), src_stride < lp_src * d_src, p_stride < lp * 128, misaligned strides; EVDR_ERR_SHAPE for lp_src > lp, d_src outside
 *   1..128, lp outside 1..65535 and EVDR_CORPUS_F16_WIDE.  b = 0: EVDR_OK, nothing written, null pointers accepted. */
#define EVDR_CORPUS_BF16     1
#define EVDR_CORPUS_F16_HILO 2
#define EVDR_CORPUS_F16_WIDE 4
#define EVDR_CORPUS_FP8      8
EVDR_API int evdr_corpus_ingest(const void* src, int src_dtype, const uint8_t* pmask_or_null,
                                int64_t b, int64_t lp_src, int64_t d_src, int64_t src_stride,
                                void* planes, int kind, int64_t capacity, int64_t lp, int64_t p_stride, int64_t p_plane_stride,
                                uint32_t* tilemask, uint32_t* pageflags, int32_t* shift_or_null, const uint32_t* p_amax_or_null,
                                int64_t first_page, const int32_t* dst_pages_or_null, uint32_t* status_or_null, void* hip_stream);

/* ---- pooled corpora: group-mean pooling of a page's patches, fused into the ingest -------------------------------------
 * Pooled token t of a page is the mean of the group's VALID members: fp32, starting from +0.0f, members added one after another in list
 * order (round to nearest), divided by their count (correctly rounded).  Valid = index inside [0, lp_src) and mask byte non-zero; any
 * other index is a hole and is skipped before it forms an address.  A group without a valid member gives a MASKED token of zeros;
 * columns >= d_src are zero.  normalize = 1 then applies x / (||x|| + 1e-12) per token with the sum of squares formed in one fixed
 * order: each octet of 8 consecutive columns summed ascending as acc = acc + x * x (multiply and add rounded separately, no FMA), the
 * 16 octet sums combined by a balanced tree of adjacent pairs (0+1, 2+3, ...; then pairs of those); square root and divide correctly
 * rounded.  normalize = 0 stores the means.
 * Grouping (CSR): members = m int32 source patch indices, group after group; offsets = ls + 1 int32, non-decreasing, offsets[0] = 0,
 *   offsets[ls] <= m; group t owns members[offsets[t] : offsets[t + 1]].  per_page = 0: one grouping for all pages; per_page = 1:
 *   members (b, m) and offsets (b, ls + 1), one row per source page.  A patch may sit in no group or in several.  The offsets are the
 *   caller's to get right: on the device they are clamped into [0, m] and made non-decreasing, so a bad list can empty groups but
 *   never leaves the arrays.
 * evdr_corpus_pool_ingest: evdr_corpus_ingest of the pooled pages without materialising them -- source, corpus, words, destination
 *   (first_page or dst_pages_or_null with holes), status word and status codes as there, with ls <= lp (tokens [ls, lp) are masked
 *   zeros).  Planes, tile words, flag word (bit 3: a pooled token holds NaN / +-Inf) and fp8 shift are bit for bit what
 *   evdr_corpus_ingest writes for the pooled page as evdr_pool_pages returns it.  EVDR_CORPUS_BF16 takes any source dtype here: the
 *   pooled fp32 value is rounded to bf16 (nearest even, NaN -> 0x7FC0), the rounding being what the caller asked for by the kind.
 * evdr_pool_pages: the plain destination -- out (b, ls, d_out) fp32 with d_out = d_src or 128 (zero columns behind d_src) and out_mask
 *   (b, ls) bytes (1 = the group has a valid member).
 * Both: ONE launch, one workgroup per page, no allocation, no host synchronisation, graph-capture safe.  Status, all BEFORE any HIP
 *   call: EVDR_ERR_ARG for a bad dtype / kind / flag, negative sizes, null pointers, bad strides; EVDR_ERR_SHAPE for ls outside
 *   1..65535, ls > lp, d_src outside 1..128, d_out neither d_src nor 128, EVDR_CORPUS_F16_WIDE.  b = 0: EVDR_OK, nothing written. */
EVDR_API int evdr_corpus_pool_ingest(const void* src, int src_dtype, const uint8_t* pmask_or_null,
                                     int64_t b, int64_t lp_src, int64_t d_src, int64_t src_stride,
                                     const int32_t* members, const int32_t* offsets, int64_t m, int64_t ls, int per_page, int normalize,
                                     void* planes, int kind, int64_t capacity, int64_t lp, int64_t p_stride, int64_t p_plane_stride,
                                     uint32_t* tilemask, uint32_t* pageflags, int32_t* shift_or_null, const uint32_t* p_amax_or_null,
                                     int64_t first_page, const int32_t* dst_pages_or_null, uint32_t* status_or_null, void* hip_stream);
EVDR_API int evdr_pool_pages(const void* src, int src_dtype, const uint8_t* pmask_or_null,
                             int64_t b, int64_t lp_src, int64_t d_src, int64_t src_stride,
                             const int32_t* members, const int32_t* offsets, int64_t m, int64_t ls, int per_page, int normalize,
                             float* out, int64_t d_out, uint8_t* out_mask, void* hip_stream);

/* ---- token clustering: a page's valid patches grouped by similarity, as the per-page grouping of the pooling calls ----
 * Spherical k-means per page, every page on its own, in ONE launch; the result is the per-page CSR form (per_page = 1, m = lp_src) that
 * evdr_pool_pages and evdr_corpus_pool_ingest take.  The rule, which the kernel follows bit for bit:
 * Per page the valid patches (mask byte non-zero; no mask = all) in ascending index are v_0 < ... < v_{nv-1}; g = min(ls, nv) groups
 *   are live, groups >= g stay empty.  Start: label(v_i) = floor(i * g / nv), equal contiguous windows over the valid patches; a masked
 *   patch has label -1 throughout.  Then `iters` iterations of an update followed by an assign:
 * Update: the centroid of live group j is the pooled token above with normalize = 1 of the group's current members in ascending patch
 *   index -- list-order mean from +0.0f, correctly rounded divide, x / (||x|| + 1e-12) with the octet / pair-tree sum of squares; a
 *   live group that has no member at the moment keeps the centroid it had.
 * Assign: for a valid patch x (the raw row) and every live j, s_j = x . c_j in the order of that norm: each of the 16 octets of 8
 *   consecutive columns summed ascending as acc = acc + x * c from +0.0f (multiply and add rounded separately, no FMA; columns >= d_src
 *   count as zeros), the 16 octet sums combined by the balanced tree of adjacent pairs.  The new label is the lowest j whose s_j is
 *   the maximum of the non-NaN scores (-0.0f equals +0.0f); when no score exceeds -inf the label is 0.
 * After the last assign (no update follows; pooling does that) the labels are emitted: members (b, lp_src) int32 holds group 0's
 *   patches ascending, then group 1's, ...; every slot behind offsets[ls] is -1 (a hole to the pooling calls); offsets (b, ls + 1)
 *   int32 starts at 0 and ends at nv; labels_or_null (b, lp_src) int32.  iters = 0 gives the windows over the valid patches; a fully
 *   masked page gives all-zero offsets.
 * workspace: evdr_cluster_pages_workspace(lp_src, ls) bytes of device memory, 16-byte aligned; it belongs to the launch's grid and does
 *   not grow with b (0 is returned for sizes evdr_cluster_pages refuses).  No allocation, no host synchronisation, no atomics,
 *   graph-capture safe; one workspace per stream that may run the call concurrently.
 * Status, all BEFORE any HIP call: EVDR_ERR_ARG for a bad dtype, negative sizes, null pointers, src_stride < lp_src * d_src, a
 *   workspace that is too small or misaligned; EVDR_ERR_SHAPE for d_src outside 1..128, lp_src outside 1..65535, ls outside 1..4096,
 *   iters outside 0..64.  b = 0: EVDR_OK, nothing written. */
EVDR_API size_t evdr_cluster_pages_workspace(int64_t lp_src, int64_t ls);
EVDR_API int evdr_cluster_pages(const void* src, int src_dtype, const uint8_t* pmask_or_null,
                                int64_t b, int64_t lp_src, int64_t d_src, int64_t src_stride,
                                int64_t ls, int64_t iters, int32_t* members, int32_t* offsets, int32_t* labels_or_null,
                                void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- A5 (+ its gradient): infonce_distillation_loss (criterion.py:56-68) -----------------------------
 * loss = mean_b CE(score_s[b,:]/temperature, argmax_p score_t[b,:]);
 * dscore[b,p] = (softmax(score_s[b,:]/temperature)[p] - [p == target_b]) / (temperature * B).
 * score_s/score_t (b, n) fp32 dense; loss: 1 float -- device memory, or device-accessible pinned host memory (hipHostMalloc:
 * the one 4-byte store then lands on the host and float(loss) needs no copy launch, only an event behind the call);
 * dscore_or_null (b, n);
 * row_loss: b floats of scratch (device). */
EVDR_API int evdr_infonce_distill_fwd_bwd(const float* score_s, const float* score_t, int64_t b, int64_t n,
                                 float temperature, float* loss, float* dscore_or_null,
                                 float* row_loss, void* hip_stream);

/* The same in ONE launch, for a caller that keeps a workspace across calls: `workspace` = (b + 1) 4-byte words of device
 * memory, the last one a ticket counter that is ZERO before the first call and is left zero by every call (the last
 * workgroup to finish reduces the per-row losses in a fixed order, so the loss is the same bits as above).  One workspace
 * per stream that may run the call concurrently. */
EVDR_API int evdr_infonce_distill_fwd_bwd_ws(const float* score_s, const float* score_t, int64_t b, int64_t n,
                                    float temperature, float* loss, float* dscore_or_null,
                                    void* workspace, void* hip_stream);

/* ---- the pairwise ranking losses, each with its gradient in ONE launch and O(b * n) memory (criterion.py:71-103) ----
 * evdr_pairwise_distill_fwd_bwd (pairwise_distillation_loss, RankNet): score_s / score_t (b, n) fp32 dense.  With m_ij = s_i - s_j and
 *   y_ij = sigmoid(t_i - t_j) per row:  loss = 1 / (b n^2) * sum_b sum_i sum_j [ softplus(m_ij) - y_ij m_ij ],
 *   grad[b, i] = 2 / (b n^2) * sum_j ( sigmoid(m_ij) - y_ij ).
 * evdr_lambda_pairs_fwd_bwd (the pair sum of lambda_loss; the caller sorts by the teacher): s_sorted / gain (b, n) fp32 dense, disc (n).
 *   With w_ij = 10 |gain_i - gain_j| |disc_i - disc_j| and D = n (n - 1) / 2 + eps:
 *   loss = 1 / D * sum_b sum_{i<j} w_ij softplus(-alpha (s_i - s_j))     (a sum over the batch, not a mean),
 *   grad[b, i] = 1 / D * [ sum_{j>i} -alpha w_ij sigmoid(-alpha (s_i - s_j)) + sum_{j<i} alpha w_ji sigmoid(-alpha (s_j - s_i)) ].
 * loss: 1 float in device memory; grad_or_null (b, n) fp32.  Every exponential is taken of -|x|: margins of +-1e4 (masked pages), pairs
 *   of two such fill values and rows wider than the range of fp32 exp are ordinary inputs.  No floating-point atomics: the same bits
 *   launch after launch, and a row's gradient depends on that row only (permuting the batch permutes the gradient rows bit for bit).
 * workspace: evdr_pair_loss_workspace(b, n) bytes of device memory, 8-byte aligned (one fp64 partial per workgroup and a ticket word; it
 *   grows with b * n / 64, never with n^2; 0 is returned for shapes the calls refuse).  The ticket word makes the workspace STATEFUL: zero
 *   the whole workspace ONCE before its first use, then leave it to the library (every call leaves the ticket zero again), and give it to
 *   ONE stream at a time -- two launches in flight on one workspace would share the ticket.  Not for use inside a stream capture next to
 *   eager launches on the same workspace.
 * Status, all BEFORE any HIP call: EVDR_ERR_ARG for b < 1, n < 1, a null pointer (grad_or_null excepted) or a misaligned workspace;
 *   EVDR_ERR_SHAPE for b > 65535 or n > 1048576 (the launch grid is (ceil(n / 64), b)); EVDR_ERR_WORKSPACE for a short workspace. */
EVDR_API size_t evdr_pair_loss_workspace(int64_t b, int64_t n);
EVDR_API int evdr_pairwise_distill_fwd_bwd(const float* score_s, const float* score_t, int64_t b, int64_t n, float* loss,
                                           float* grad_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);
EVDR_API int evdr_lambda_pairs_fwd_bwd(const float* s_sorted, const float* gain, const float* disc, int64_t b, int64_t n, float alpha,
                                       float eps, float* loss, float* grad_or_null, void* workspace, size_t workspace_bytes,
                                       void* hip_stream);

/* ---- debug hooks: not part of the drop-in surface (tests and A/B measurements only) -----------------------------------
 * The library reads NO environment variable and takes no pointer from one; everything that changes its behaviour comes in
 * through a call.  Both overrides are THREAD-LOCAL (like evdr_last_error): they apply to the launches the CALLING thread issues
 * after the call and to no other thread's -- no process-wide mutable state (tests/cabi/cabi_threads.cpp: a thread that forces a
 * variant does not change what its neighbours dispatch).
 * evdr_debug_set_fwd_variant: force a forward-kernel family for the calling thread's launches (0 = default dispatch,
 * 1 = flat per-tile ring, 2 = staged kernel without the priority schedule, 10/11 = fp16-plane stage shapes (3 / 4 tiles),
 * 30 = one 8-wave workgroup per CU also for 3-12 queries, 31 = no non-temporal corpus stream, 33 / 34 = non-temporal stream of
 * the fp16-plane forward forced on / off (default: on for >= 128 MiB of planes read by <= 2 query groups), 36 = two queries per wave also
 * for small fp16-plane launches (default: one per wave when 16-query workgroups would number <= 128); all variants compute the same
 * scores -- the test sweep runs each against the oracle); returns the previous value.
 * evdr_debug_set_pages_per_block: pages per workgroup for the calling thread's launches (0 = automatic); returns the previous value.
 * evdr_last_fwd_kernel: host string naming the forward instance the last evdr_maxsim_fwd* / evdr_maxsim_topk call of
 * this thread dispatched (template arguments as in csrc/maxsim_fwd16.hip) -- what bench.py records next to its timing. */
EVDR_API int         evdr_debug_set_fwd_variant(int variant);
EVDR_API int         evdr_debug_set_pages_per_block(int pages);
EVDR_API const char* evdr_last_fwd_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* EVDR_H */
