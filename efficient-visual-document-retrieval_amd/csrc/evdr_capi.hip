// C-ABI entry points (include/evdr.h).  Argument checking + workspace carving + kernel dispatch.
// Nothing here allocates, frees or synchronises (graph-capture safe); errors come back as status codes.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include "evdr_common.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(EVDR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

inline int64_t ntiles_of(int64_t lp) { return (lp + EVDR_TILE_PATCHES - 1) / EVDR_TILE_PATCHES; }

struct FwdWorkspace {
    size_t tilemask_off, pageflags_off, qlist_off, amax_off, qplanes_off, pplanes_off, total;
};

FwdWorkspace carve_fwd(int64_t nq, int64_t lq, int64_t np, int64_t lp, int dtype) {
    FwdWorkspace w{};
    size_t off = 0;
    w.tilemask_off = off;
    off = align_up(off + (size_t)np * ntiles_of(lp) * 4);
    w.pageflags_off = off;
    off = align_up(off + (size_t)np * 4);
    w.qlist_off = off;                                  // later token slices: [0] = count, [1..nq] = compacted query indices
    if (lq > 32) off = align_up(off + (size_t)(nq + 1) * 4);
    w.amax_off = off;                                   // [0] = Q's absmax bits, [1] = P's
    if (dtype == EVDR_F32) off = align_up(off + 2 * sizeof(uint32_t));
    w.qplanes_off = off;
    if (dtype == EVDR_F32) off = align_up(off + (size_t)2 * nq * lq * EVDR_D * 2);
    w.pplanes_off = off;
    if (dtype == EVDR_F32) off = align_up(off + (size_t)2 * np * lp * EVDR_D * 2);
    w.total = off;
    return w;
}

int check_common(int64_t nq, int64_t lq, int64_t np, int64_t lp) {
    if (nq < 0 || lq < 0 || np < 0 || lp < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (nq > INT32_MAX || np > INT32_MAX || lq > 65535 || lp > 65535)
        return fail(EVDR_ERR_SHAPE, "size out of range (nq=%lld lq=%lld np=%lld lp=%lld)", (long long)nq,
                    (long long)lq, (long long)np, (long long)lp);
    if (nq * lq > INT32_MAX) return fail(EVDR_ERR_SHAPE, "nq * lq = %lld exceeds 2^31 - 1 (kernels index (query, token) pairs in 32 bits)",
                                         (long long)(nq * lq));
    return EVDR_OK;
}

// Runs the forward over 32-token slices of the queries (one slice for Lq <= 32).
// Single-token queries (Lq = 1: the "virtual queries" of mainv3_iter_liscore_QA_hardtoken.py:428-434) would leave 31 of
// the 32 token lanes of the MFMA tile empty; dense (nq, 1, 128) rows ARE the layout of ceil(nq/32) queries of 32 tokens,
// so they are scored as such with one output row per token (EvdrFwdParams::per_token): 32x less MFMA work.
int run_fwd(const uint16_t* Qp, int64_t q_stride, int64_t q_plane_stride, const uint16_t* Pp, int64_t p_stride,
            int64_t p_plane_stride, const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
            float* out, int64_t out_stride, uint16_t* argmax, int64_t nq, int64_t lq, int64_t np, int64_t lp,
            int nplanes, const uint32_t* q_amax, const uint32_t* p_amax, int32_t* qlist_ws, hipStream_t stream,
            const int32_t* qsel = nullptr, const int32_t* qsel_count = nullptr, bool allow_pack = true,
            const int32_t* pages = nullptr, int64_t m = 0) {
    const bool pack = allow_pack && (lq == 1 && nq > 1 && q_stride == EVDR_D);
    for (int64_t tok0 = 0; tok0 < lq; tok0 += 32) {
        EvdrFwdParams p{};
        p.Q = Qp;
        p.q_stride = pack ? 32 * EVDR_D : q_stride;
        p.q_plane_stride = q_plane_stride;
        p.P = Pp;
        p.p_stride = p_stride;
        p.p_plane_stride = p_plane_stride;
        p.q_amax = q_amax;
        p.p_amax = p_amax;
        p.qmask = qmask;
        p.tilemask = tilemask;
        p.pageflags = pageflags;
        p.out = out;
        p.out_stride = out_stride;
        p.argmax = argmax;
        p.nq = (int)(pack ? (nq + 31) / 32 : nq);
        p.lq = pack ? 32 : (int)((lq - tok0 < 32) ? (lq - tok0) : 32);
        p.np = (int)np;
        p.lp = (int)lp;
        p.tok0 = (int)tok0;
        p.lq_total = pack ? 32 : (int)lq;
        p.per_token = pack ? nq : 0;
        p.accumulate = tok0 > 0 ? 1 : 0;
        if (tok0 > 0 && qlist_ws && qmask && !argmax) {
            // queries padded to the longest of a set: only those with a valid token in this slice are scored again
            hipError_t eq = evdr_launch_build_qlist(qmask, nq, lq, tok0, qlist_ws + 1, qlist_ws, stream);
            if (eq != hipSuccess) return hip_fail(eq, "build_qlist launch");
            p.qlist = qlist_ws + 1;
            p.qcount = qlist_ws;
        }
        if (qsel != nullptr) {                          // evdr_maxsim_fwd_prepared_subset: one slice, the caller's device-side list
            p.qlist = qsel;
            p.qcount = qsel_count;
        }
        if (pages != nullptr) {                         // evdr_maxsim_fwd_pages: the batch's page list takes the place of the corpus
            p.np = (int)m;
            p.ncorpus = (int)np;
            p.gather = pages;
        }
        hipError_t e = pages != nullptr ? evdr_launch_maxsim_pages16(p, nplanes, stream)
                                        : evdr_launch_maxsim_fwd(p, nplanes, argmax != nullptr, stream);
        if (e != hipSuccess) return hip_fail(e, "maxsim_fwd launch");
    }
    return EVDR_OK;
}

// the coarse pass of the prefilter: hi planes only (maxsim_fwd16.hip, HI instance); single-token queries packed 32 to a tile like run_fwd
int run_coarse(const uint16_t* Qp, const uint16_t* Pp, const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
               float* out, int64_t out_stride, int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t p_stride, int64_t p_plane_stride,
               const uint32_t* q_amax, const uint32_t* p_amax, hipStream_t stream) {
    const bool pack = (lq == 1 && nq > 1);
    EvdrFwdParams p{};
    p.Q = Qp;
    p.q_stride = pack ? 32 * EVDR_D : lq * EVDR_D;
    p.q_plane_stride = nq * lq * EVDR_D;
    p.P = Pp;
    p.p_stride = p_stride;
    p.p_plane_stride = p_plane_stride;
    p.q_amax = q_amax;
    p.p_amax = p_amax;
    p.qmask = qmask;
    p.tilemask = tilemask;
    p.pageflags = pageflags;
    p.out = out;
    p.out_stride = out_stride;
    p.nq = (int)(pack ? (nq + 31) / 32 : nq);
    p.lq = pack ? 32 : (int)lq;
    p.np = (int)np;
    p.lp = (int)lp;
    p.lq_total = pack ? 32 : (int)lq;
    p.per_token = pack ? nq : 0;
    p.inblock_refill = p.nq > 4 ? 1 : 0;
    hipError_t e = evdr_launch_maxsim_coarse16(p, stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "coarse forward launch");
}

// argument checks shared by the coarse-score and prefiltered top-k entries (before any device work)
int check_prefilter(const char* who, int64_t nq, int64_t lq, int64_t np, int64_t lp, int nplanes, int64_t p_stride) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (nplanes != 2)
        return fail(EVDR_ERR_ARG, "%s: nplanes must be 2 (fp16 hi/lo planes of an fp32 corpus; bf16 has no cheaper first stage, width 256 is not covered)", who);
    if (lq > 32) return fail(EVDR_ERR_SHAPE, "%s: lq must be <= 32", who);
    if (np > 0 && lp > 0 && p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "%s: p_stride smaller than a page", who);
    return EVDR_OK;
}

struct PrefilterWorkspace {
    size_t coarse, tkws, eq, tv, ti, rv, ri, fv, fi, gather, gcount, cand, fb, flist, fcount, total;
};

PrefilterWorkspace carve_prefilter(int64_t nq, int64_t np, int64_t cap) {
    PrefilterWorkspace w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes); return o; };
    size_t tk = evdr_topk_workspace(nq, np, EVDR_TOPK_MAX);
    const size_t tk2 = evdr_topk_workspace(nq, cap, EVDR_TOPK_MAX);
    if (tk2 > tk) tk = tk2;
    const size_t kb = (size_t)nq * EVDR_TOPK_MAX * 4;
    w.coarse = take((size_t)nq * np * 4);
    w.tkws = take(tk);
    w.eq = take((size_t)nq * 4);
    w.tv = take(kb); w.ti = take(kb);
    w.rv = take(kb); w.ri = take(kb);
    w.fv = take(kb); w.fi = take(kb);
    w.gather = take((size_t)nq * cap * 4);
    w.gcount = take((size_t)nq * 4);
    w.cand = take((size_t)nq * cap * 4);
    w.fb = take((size_t)nq * 4);
    w.flist = take((size_t)nq * 4);
    w.fcount = take(4);
    w.total = off;
    return w;
}

struct CandWorkspace {
    size_t glist, gpos, gcount, tmp, total;
};

CandWorkspace carve_candidates(int64_t nq, int64_t r) {
    CandWorkspace w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes); return o; };
    w.glist = take((size_t)nq * r * 4);
    w.gpos = take((size_t)nq * r * 4);
    w.gcount = take((size_t)nq * 4);
    w.tmp = take((size_t)nq * r * 4);
    w.total = off;
    return w;
}

}  // namespace

hipError_t evdr_launch_prefilter_corpus_bound(const uint16_t* P, int64_t np, int64_t lp, int64_t p_stride, int64_t p_plane_stride,
                                              const uint32_t* tilemask, const uint32_t* pageflags, float* bound, hipStream_t stream);
hipError_t evdr_launch_prefilter_query_bound(const uint16_t* Q, const uint8_t* qmask, int64_t nq, int64_t lq, const uint32_t* q_amax,
                                             const uint32_t* p_amax, const float* bound, float* eq, int32_t* fcount, hipStream_t stream);
hipError_t evdr_launch_prefilter_select(const float* coarse, int64_t nq, int64_t np, const float* topv, int kc, const float* eq, int cap,
                                        int32_t* gather, int32_t* gcount, float* cand, int32_t* fb, int32_t* flist, int32_t* fcount,
                                        int32_t* stats, hipStream_t stream);
hipError_t evdr_launch_prefilter_merge(const float* rs, const int32_t* ri, const float* fs, const int32_t* fi, const int32_t* fb, int64_t nq,
                                       int k, int32_t idx_base, const int32_t* fcount, float* top_scores, int32_t* top_idx, int32_t* stats,
                                       hipStream_t stream);

extern "C" {

int evdr_version(void) { return EVDR_VERSION_NUM; }

const char* evdr_last_error(void) { return g_err; }

int evdr_debug_set_fwd_variant(int variant) { return evdr_fwd_variant_exchange(variant); }

int evdr_debug_set_pages_per_block(int pages) { return evdr_pages_per_block_exchange(pages < 0 ? 0 : pages); }

const char* evdr_last_fwd_kernel(void) { return evdr_last_fwd_kernel_name(); }

int evdr_pack_pmask(const uint8_t* pmask, int64_t np, int64_t lp, uint32_t* tilemask, uint32_t* pageflags,
                    void* hip_stream) {
    if (int rc = check_common(0, 0, np, lp)) return rc;
    if (!tilemask || !pageflags) return fail(EVDR_ERR_ARG, "evdr_pack_pmask: null output");
    if (np == 0) return EVDR_OK;
    if (lp == 0) return fail(EVDR_ERR_SHAPE, "evdr_pack_pmask: lp == 0");
    hipError_t e = evdr_launch_pack_pmask(pmask, np, lp, tilemask, pageflags, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "pack_pmask launch");
}

int evdr_split_f32(const float* x, int64_t rows, uint16_t* planes, uint32_t* amax_bits, void* hip_stream) {
    if (rows < 0) return fail(EVDR_ERR_ARG, "evdr_split_f32: negative rows");
    if (!amax_bits) return fail(EVDR_ERR_ARG, "evdr_split_f32: null amax_bits");
    if (rows > 0 && (!x || !planes)) return fail(EVDR_ERR_ARG, "evdr_split_f32: null pointer");
    hipError_t e = evdr_launch_split_f32(x, rows, planes, amax_bits, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "split_f32 launch");
}

int evdr_split_f32_segments(const float* x, int64_t rows, int64_t seg_rows, uint16_t* planes, uint32_t* amax_bits, void* hip_stream) {
    if (rows < 0) return fail(EVDR_ERR_ARG, "evdr_split_f32_segments: negative rows");
    if (seg_rows < 1 || seg_rows > 2048) return fail(EVDR_ERR_ARG, "evdr_split_f32_segments: seg_rows outside 1..2048");
    if ((rows + seg_rows - 1) / seg_rows > 65535) return fail(EVDR_ERR_ARG, "evdr_split_f32_segments: more than 65535 segments");
    if (rows > 0 && (!x || !planes || !amax_bits)) return fail(EVDR_ERR_ARG, "evdr_split_f32_segments: null pointer");
    hipError_t e = evdr_launch_split_f32_segments(x, rows, seg_rows, planes, amax_bits, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "split_f32_segments launch");
}

int evdr_flag_nonfinite(const void* P, int dtype, const uint8_t* pmask, int64_t np, int64_t lp, int64_t p_stride,
                        uint32_t* pageflags, void* hip_stream) {
    if (int rc = check_common(0, 0, np, lp)) return rc;
    if (dtype != EVDR_F32 && dtype != EVDR_BF16 && dtype != EVDR_F16) return fail(EVDR_ERR_ARG, "dtype must be EVDR_F32, EVDR_BF16 or EVDR_F16");
    if (np == 0 || lp == 0) return EVDR_OK;
    if (!P || !pageflags) return fail(EVDR_ERR_ARG, "evdr_flag_nonfinite: null pointer");
    if (p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "p_stride smaller than a page");
    hipError_t e = evdr_launch_flag_nonfinite(P, dtype, pmask, np, lp, p_stride, pageflags, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "flag_nonfinite launch");
}

size_t evdr_maxsim_fwd_workspace(int64_t nq, int64_t lq, int64_t np, int64_t lp, int dtype) {
    if (nq < 0 || lq < 0 || np < 0 || lp < 0) return 0;
    return carve_fwd(nq, lq, np, lp, dtype).total;
}

int evdr_maxsim_fwd(const void* Q, const void* P, const uint8_t* qmask, const uint8_t* pmask, float* out,
                    uint16_t* argmax_or_null, int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t d, int dtype,
                    const int64_t* strides_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (d != EVDR_D)
        return fail(EVDR_ERR_SHAPE, "embedding width %lld: this entry takes width 128 (widths up to 256: evdr_maxsim_fwd_prepared with nplanes = 4)", (long long)d);
    if (dtype != EVDR_F32 && dtype != EVDR_BF16) return fail(EVDR_ERR_ARG, "dtype must be EVDR_F32 or EVDR_BF16");
    if (nq == 0 || np == 0) return EVDR_OK;                      // empty score matrix
    if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis (lq=%lld lp=%lld)", (long long)lq, (long long)lp);
    if (!Q || !P || !out) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd: null Q/P/out");
    const int64_t q_stride = strides_or_null ? strides_or_null[0] : lq * EVDR_D;
    const int64_t p_stride = strides_or_null ? strides_or_null[1] : lp * EVDR_D;
    if (q_stride < lq * EVDR_D || p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "strides smaller than a row block");
    const FwdWorkspace w = carve_fwd(nq, lq, np, lp, dtype);
    if (!workspace || workspace_bytes < w.total)
        return fail(EVDR_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", w.total, workspace_bytes);
    hipStream_t stream = (hipStream_t)hip_stream;
    char* ws = (char*)workspace;
    uint32_t* tilemask = (uint32_t*)(ws + w.tilemask_off);
    uint32_t* pageflags = (uint32_t*)(ws + w.pageflags_off);
    hipError_t e = evdr_launch_pack_pmask(pmask, np, lp, tilemask, pageflags, stream);
    if (e != hipSuccess) return hip_fail(e, "pack_pmask launch");
    if (dtype == EVDR_BF16) {
        // NaN / Inf in a valid patch -> page flag bit 3 (one extra read of P; a resident corpus pays it once, evdr_flag_nonfinite)
        if ((e = evdr_launch_flag_nonfinite(P, 1, pmask, np, lp, p_stride, pageflags, stream)) != hipSuccess)
            return hip_fail(e, "flag_nonfinite launch");
        return run_fwd((const uint16_t*)Q, q_stride, 0, (const uint16_t*)P, p_stride, 0, qmask, tilemask, pageflags, out,
                       np, argmax_or_null, nq, lq, np, lp, 1, nullptr, nullptr, lq > 32 ? (int32_t*)(ws + w.qlist_off) : nullptr, stream);
    }
    if (q_stride != lq * EVDR_D || p_stride != lp * EVDR_D)
        return fail(EVDR_ERR_ARG, "fp32 inputs must be dense (make them contiguous before the call)");
    uint16_t* qpl = (uint16_t*)(ws + w.qplanes_off);
    uint16_t* ppl = (uint16_t*)(ws + w.pplanes_off);
    uint32_t* amax = (uint32_t*)(ws + w.amax_off);
    if ((e = evdr_launch_split_f32((const float*)Q, nq * lq, qpl, amax, stream)) != hipSuccess) return hip_fail(e, "split Q");
    if ((e = evdr_launch_split_f32_pages((const float*)P, np * lp, ppl, amax + 1, pmask, lp, pageflags, stream)) != hipSuccess)
        return hip_fail(e, "split P");
    return run_fwd(qpl, lq * EVDR_D, nq * lq * EVDR_D, ppl, lp * EVDR_D, np * lp * EVDR_D, qmask, tilemask, pageflags, out,
                   np, argmax_or_null, nq, lq, np, lp, 2, amax, amax + 1, lq > 32 ? (int32_t*)(ws + w.qlist_off) : nullptr, stream);
}

int evdr_maxsim_fwd_prepared(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask,
                             const uint32_t* tilemask, const uint32_t* pageflags, float* out, int64_t out_stride,
                             uint16_t* argmax_or_null, int64_t nq, int64_t lq, int64_t np, int64_t lp, int nplanes,
                             int64_t p_stride, int64_t p_plane_stride, const uint32_t* q_amax_or_null,
                             const uint32_t* p_amax_or_null, int32_t* qlist_ws_or_null, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (nplanes != 1 && nplanes != 2 && nplanes != 4)
        return fail(EVDR_ERR_ARG, "nplanes must be 1 (bf16), 2 (fp16 hi/lo) or 4 (fp16 hi/lo x two 128-column blocks: width 256)");
    if (nq == 0 || np == 0) return EVDR_OK;
    if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
    if (!Qplanes || !Pplanes || !tilemask || !pageflags || !out) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_prepared: null pointer");
    if (out_stride < np || p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "stride smaller than the row it spans");
    return run_fwd(Qplanes, lq * EVDR_D, nq * lq * EVDR_D, Pplanes, p_stride, p_plane_stride, qmask, tilemask, pageflags, out,
                   out_stride, argmax_or_null, nq, lq, np, lp, nplanes, nplanes >= 2 ? q_amax_or_null : nullptr,
                   nplanes >= 2 ? p_amax_or_null : nullptr, lq > 32 ? qlist_ws_or_null : nullptr, (hipStream_t)hip_stream);
}

int evdr_maxsim_fwd_pages(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask, const uint32_t* tilemask,
                          const uint32_t* pageflags, const int32_t* pages, int64_t m, float* out, int64_t out_stride, int64_t nq,
                          int64_t lq, int64_t np, int64_t lp, int nplanes, int64_t p_stride, int64_t p_plane_stride,
                          const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null, int32_t* qlist_ws_or_null, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (m < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (m > INT32_MAX) return fail(EVDR_ERR_SHAPE, "size out of range (m=%lld)", (long long)m);
    if (nplanes == 4) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_fwd_pages: width-256 corpora (nplanes = 4) are not covered");
    if (nplanes != 1 && nplanes != 2) return fail(EVDR_ERR_ARG, "nplanes must be 1 (bf16) or 2 (fp16 hi/lo)");
    if (nq == 0 || m == 0) return EVDR_OK;
    if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
    if (np == 0) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_fwd_pages: a page list over an empty corpus");
    if (!Qplanes || !Pplanes || !tilemask || !pageflags || !pages || !out) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_pages: null pointer");
    if (out_stride < m || p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "stride smaller than the row it spans");
    if (lq > 32 && !qlist_ws_or_null)
        return fail(EVDR_ERR_WORKSPACE, "evdr_maxsim_fwd_pages: lq > 32 needs the (nq + 1) int32 qlist workspace");
    return run_fwd(Qplanes, lq * EVDR_D, nq * lq * EVDR_D, Pplanes, p_stride, p_plane_stride, qmask, tilemask, pageflags, out,
                   out_stride, nullptr, nq, lq, np, lp, nplanes, nplanes == 2 ? q_amax_or_null : nullptr,
                   nplanes == 2 ? p_amax_or_null : nullptr, lq > 32 ? qlist_ws_or_null : nullptr, (hipStream_t)hip_stream, nullptr, nullptr,
                   true, pages, m);
}

int evdr_quantize_fp8(const void* x, int dtype, int64_t groups, int64_t rows_per_group, int64_t d, uint8_t* x8, int32_t* shift,
                      void* hip_stream) {
    if (dtype != EVDR_F32 && dtype != EVDR_BF16) return fail(EVDR_ERR_ARG, "evdr_quantize_fp8: dtype must be EVDR_F32 or EVDR_BF16");
    if (groups < 0 || rows_per_group < 0 || d < 0) return fail(EVDR_ERR_ARG, "evdr_quantize_fp8: negative size");
    if (d == 0 || d > EVDR_D) return fail(EVDR_ERR_SHAPE, "evdr_quantize_fp8: width %lld outside 1..128", (long long)d);
    if (groups > INT32_MAX || rows_per_group > INT32_MAX / EVDR_D)
        return fail(EVDR_ERR_SHAPE, "evdr_quantize_fp8: groups = %lld, rows_per_group = %lld out of range", (long long)groups,
                    (long long)rows_per_group);
    if (groups == 0) return EVDR_OK;
    if (!shift || (rows_per_group > 0 && (!x || !x8))) return fail(EVDR_ERR_ARG, "evdr_quantize_fp8: null pointer");
    hipError_t e = evdr_launch_quantize_fp8(x, dtype, groups, rows_per_group, d, x8, shift, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "quantize_fp8 launch");
}

int evdr_corpus_ingest(const void* src, int src_dtype, const uint8_t* pmask_or_null, int64_t b, int64_t lp_src, int64_t d_src,
                       int64_t src_stride, void* planes, int kind, int64_t capacity, int64_t lp, int64_t p_stride, int64_t p_plane_stride,
                       uint32_t* tilemask, uint32_t* pageflags, int32_t* shift_or_null, const uint32_t* p_amax_or_null,
                       int64_t first_page, const int32_t* dst_pages_or_null, uint32_t* status_or_null, void* hip_stream) {
    const char* who = "evdr_corpus_ingest";
    if (src_dtype != EVDR_F32 && src_dtype != EVDR_BF16 && src_dtype != EVDR_F16)
        return fail(EVDR_ERR_ARG, "%s: src_dtype must be EVDR_F32, EVDR_BF16 or EVDR_F16", who);
    if (kind == EVDR_CORPUS_F16_WIDE) return fail(EVDR_ERR_SHAPE, "%s: width-256 corpora (four planes) are not covered", who);
    if (kind != EVDR_CORPUS_BF16 && kind != EVDR_CORPUS_F16_HILO && kind != EVDR_CORPUS_FP8)
        return fail(EVDR_ERR_ARG, "%s: kind must be EVDR_CORPUS_BF16, EVDR_CORPUS_F16_HILO or EVDR_CORPUS_FP8", who);
    if (b < 0 || lp_src < 0 || d_src < 0 || capacity < 0 || lp < 0) return fail(EVDR_ERR_ARG, "%s: negative size", who);
    if (b > INT32_MAX || capacity > INT32_MAX)
        return fail(EVDR_ERR_SHAPE, "%s: b = %lld, capacity = %lld out of range", who, (long long)b, (long long)capacity);
    if (lp < 1 || lp > 65535) return fail(EVDR_ERR_SHAPE, "%s: lp = %lld outside 1..65535", who, (long long)lp);
    if (lp_src > lp) return fail(EVDR_ERR_SHAPE, "%s: lp_src = %lld > lp = %lld", who, (long long)lp_src, (long long)lp);
    if (d_src < 1 || d_src > EVDR_D) return fail(EVDR_ERR_SHAPE, "%s: d_src = %lld outside 1..128", who, (long long)d_src);
    if (kind == EVDR_CORPUS_BF16 && src_dtype != EVDR_BF16)
        return fail(EVDR_ERR_ARG, "%s: a bf16 corpus takes bf16 pages (round them explicitly, or keep an fp32 corpus)", who);
    if (kind == EVDR_CORPUS_F16_HILO && !p_amax_or_null)
        return fail(EVDR_ERR_ARG, "%s: an fp16 hi/lo corpus needs its absmax word (p_amax)", who);
    if (kind == EVDR_CORPUS_FP8 && !shift_or_null) return fail(EVDR_ERR_ARG, "%s: an fp8 corpus needs its per-page shifts", who);
    if (!dst_pages_or_null && (first_page < 0 || first_page + b > capacity))
        return fail(EVDR_ERR_ARG, "%s: pages %lld .. %lld do not fit a capacity of %lld", who, (long long)first_page,
                    (long long)(first_page + b), (long long)capacity);
    if (b == 0) return EVDR_OK;
    if (!planes || !tilemask || !pageflags || (lp_src > 0 && !src)) return fail(EVDR_ERR_ARG, "%s: null pointer", who);
    if (src_stride < lp_src * d_src) return fail(EVDR_ERR_ARG, "%s: src_stride smaller than a source page", who);
    const int64_t al = kind == EVDR_CORPUS_FP8 ? 16 : 8;                     // elements per 16 bytes of the planes
    if (p_stride < lp * EVDR_D || p_stride % al || (kind == EVDR_CORPUS_F16_HILO && p_plane_stride % al) ||
        reinterpret_cast<uintptr_t>(planes) % 16)
        return fail(EVDR_ERR_ARG, "%s: p_stride smaller than a page, or planes / strides not 16-byte aligned", who);
    EvdrIngestParams p{};
    p.src = src; p.src_dtype = src_dtype; p.pmask = pmask_or_null; p.b = b; p.src_stride = src_stride;
    p.lp_src = (int)lp_src; p.d_src = (int)d_src;
    p.planes = planes; p.kind = kind; p.lp = (int)lp; p.capacity = capacity; p.p_stride = p_stride; p.p_plane_stride = p_plane_stride;
    p.tilemask = tilemask; p.pageflags = pageflags; p.shift = shift_or_null; p.p_amax = p_amax_or_null;
    p.first_page = first_page; p.dst_pages = dst_pages_or_null; p.status = kind == EVDR_CORPUS_F16_HILO ? status_or_null : nullptr;
    hipError_t e = evdr_launch_corpus_ingest(p, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "corpus_ingest launch");
}

// source pages and grouping of the two pooling calls; 0 = in order
static int check_pool_source(const char* who, const void* src, int src_dtype, int64_t b, int64_t lp_src, int64_t d_src, int64_t src_stride,
                             const int32_t* members, const int32_t* offsets, int64_t m, int64_t ls, int per_page, int normalize) {
    if (src_dtype != EVDR_F32 && src_dtype != EVDR_BF16 && src_dtype != EVDR_F16)
        return fail(EVDR_ERR_ARG, "%s: src_dtype must be EVDR_F32, EVDR_BF16 or EVDR_F16", who);
    if (b < 0 || lp_src < 0 || d_src < 0 || m < 0 || ls < 0) return fail(EVDR_ERR_ARG, "%s: negative size", who);
    if ((per_page != 0 && per_page != 1) || (normalize != 0 && normalize != 1))
        return fail(EVDR_ERR_ARG, "%s: per_page and normalize are flags (0 or 1)", who);
    if (b > INT32_MAX || m > INT32_MAX || lp_src > INT32_MAX / EVDR_D)
        return fail(EVDR_ERR_SHAPE, "%s: b = %lld, m = %lld, lp_src = %lld out of range", who, (long long)b, (long long)m, (long long)lp_src);
    if (ls < 1 || ls > 65535) return fail(EVDR_ERR_SHAPE, "%s: ls = %lld outside 1..65535", who, (long long)ls);
    if (d_src < 1 || d_src > EVDR_D) return fail(EVDR_ERR_SHAPE, "%s: d_src = %lld outside 1..128", who, (long long)d_src);
    if (b == 0) return EVDR_OK;
    if (!offsets || (m > 0 && !members) || (lp_src > 0 && !src)) return fail(EVDR_ERR_ARG, "%s: null pointer", who);
    if (src_stride < lp_src * d_src) return fail(EVDR_ERR_ARG, "%s: src_stride smaller than a source page", who);
    return EVDR_OK;
}

static void fill_pool_source(EvdrPoolParams& q, const void* src, int src_dtype, const uint8_t* pmask, int64_t b, int64_t lp_src,
                             int64_t d_src, int64_t src_stride, const int32_t* members, const int32_t* offsets, int64_t m, int64_t ls,
                             int per_page, int normalize) {
    q.g.src = src; q.g.src_dtype = src_dtype; q.g.pmask = pmask; q.g.b = b; q.g.src_stride = src_stride;
    q.g.lp_src = (int)lp_src; q.g.d_src = (int)d_src;
    q.members = members; q.offsets = offsets; q.m = (int)m; q.ls = (int)ls; q.normalize = normalize;
    q.members_stride = per_page ? m : 0; q.offsets_stride = per_page ? ls + 1 : 0;
}

int evdr_corpus_pool_ingest(const void* src, int src_dtype, const uint8_t* pmask_or_null, int64_t b, int64_t lp_src, int64_t d_src,
                            int64_t src_stride, const int32_t* members, const int32_t* offsets, int64_t m, int64_t ls, int per_page,
                            int normalize, void* planes, int kind, int64_t capacity, int64_t lp, int64_t p_stride, int64_t p_plane_stride,
                            uint32_t* tilemask, uint32_t* pageflags, int32_t* shift_or_null, const uint32_t* p_amax_or_null,
                            int64_t first_page, const int32_t* dst_pages_or_null, uint32_t* status_or_null, void* hip_stream) {
    const char* who = "evdr_corpus_pool_ingest";
    if (kind == EVDR_CORPUS_F16_WIDE) return fail(EVDR_ERR_SHAPE, "%s: width-256 corpora (four planes) are not covered", who);
    if (kind != EVDR_CORPUS_BF16 && kind != EVDR_CORPUS_F16_HILO && kind != EVDR_CORPUS_FP8)
        return fail(EVDR_ERR_ARG, "%s: kind must be EVDR_CORPUS_BF16, EVDR_CORPUS_F16_HILO or EVDR_CORPUS_FP8", who);
    if (capacity < 0 || lp < 0) return fail(EVDR_ERR_ARG, "%s: negative size", who);
    if (int rc = check_pool_source(who, nullptr, src_dtype, 0, lp_src, d_src, src_stride, members, offsets, m, ls, per_page, normalize)) return rc;
    if (b < 0) return fail(EVDR_ERR_ARG, "%s: negative size", who);
    if (b > INT32_MAX || capacity > INT32_MAX)
        return fail(EVDR_ERR_SHAPE, "%s: b = %lld, capacity = %lld out of range", who, (long long)b, (long long)capacity);
    if (lp < 1 || lp > 65535) return fail(EVDR_ERR_SHAPE, "%s: lp = %lld outside 1..65535", who, (long long)lp);
    if (ls > lp) return fail(EVDR_ERR_SHAPE, "%s: ls = %lld > lp = %lld", who, (long long)ls, (long long)lp);
    if (kind == EVDR_CORPUS_F16_HILO && !p_amax_or_null)
        return fail(EVDR_ERR_ARG, "%s: an fp16 hi/lo corpus needs its absmax word (p_amax)", who);
    if (kind == EVDR_CORPUS_FP8 && !shift_or_null) return fail(EVDR_ERR_ARG, "%s: an fp8 corpus needs its per-page shifts", who);
    if (!dst_pages_or_null && (first_page < 0 || first_page + b > capacity))
        return fail(EVDR_ERR_ARG, "%s: pages %lld .. %lld do not fit a capacity of %lld", who, (long long)first_page,
                    (long long)(first_page + b), (long long)capacity);
    if (b == 0) return EVDR_OK;
    if (!planes || !tilemask || !pageflags) return fail(EVDR_ERR_ARG, "%s: null pointer", who);
    if (int rc = check_pool_source(who, src, src_dtype, b, lp_src, d_src, src_stride, members, offsets, m, ls, per_page, normalize)) return rc;
    const int64_t al = kind == EVDR_CORPUS_FP8 ? 16 : 8;                     // elements per 16 bytes of the planes
    if (p_stride < lp * EVDR_D || p_stride % al || (kind == EVDR_CORPUS_F16_HILO && p_plane_stride % al) ||
        reinterpret_cast<uintptr_t>(planes) % 16)
        return fail(EVDR_ERR_ARG, "%s: p_stride smaller than a page, or planes / strides not 16-byte aligned", who);
    EvdrPoolParams q{};
    fill_pool_source(q, src, src_dtype, pmask_or_null, b, lp_src, d_src, src_stride, members, offsets, m, ls, per_page, normalize);
    EvdrIngestParams& p = q.g;
    p.planes = planes; p.kind = kind; p.lp = (int)lp; p.capacity = capacity; p.p_stride = p_stride; p.p_plane_stride = p_plane_stride;
    p.tilemask = tilemask; p.pageflags = pageflags; p.shift = shift_or_null; p.p_amax = p_amax_or_null;
    p.first_page = first_page; p.dst_pages = dst_pages_or_null; p.status = kind == EVDR_CORPUS_F16_HILO ? status_or_null : nullptr;
    hipError_t e = evdr_launch_corpus_pool(q, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "corpus_pool_ingest launch");
}

int evdr_pool_pages(const void* src, int src_dtype, const uint8_t* pmask_or_null, int64_t b, int64_t lp_src, int64_t d_src,
                    int64_t src_stride, const int32_t* members, const int32_t* offsets, int64_t m, int64_t ls, int per_page, int normalize,
                    float* out, int64_t d_out, uint8_t* out_mask, void* hip_stream) {
    const char* who = "evdr_pool_pages";
    if (int rc = check_pool_source(who, src, src_dtype, b, lp_src, d_src, src_stride, members, offsets, m, ls, per_page, normalize)) return rc;
    if (d_out != d_src && d_out != EVDR_D) return fail(EVDR_ERR_SHAPE, "%s: d_out = %lld is neither d_src nor 128", who, (long long)d_out);
    if (b == 0) return EVDR_OK;
    if (!out || !out_mask) return fail(EVDR_ERR_ARG, "%s: null pointer", who);
    EvdrPoolParams q{};
    fill_pool_source(q, src, src_dtype, pmask_or_null, b, lp_src, d_src, src_stride, members, offsets, m, ls, per_page, normalize);
    q.g.kind = EVDR_POOL_PLAIN; q.g.lp = (int)ls; q.g.capacity = b; q.g.first_page = 0;
    q.out = out; q.out_mask = out_mask; q.d_out = (int)d_out;
    hipError_t e = evdr_launch_corpus_pool(q, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "pool_pages launch");
}

static int check_cluster_shape(const char* who, int64_t lp_src, int64_t ls) {
    if (lp_src < 1 || lp_src > 65535) return fail(EVDR_ERR_SHAPE, "%s: lp_src = %lld outside 1..65535", who, (long long)lp_src);
    if (ls < 1 || ls > 4096) return fail(EVDR_ERR_SHAPE, "%s: ls = %lld outside 1..4096", who, (long long)ls);
    return EVDR_OK;
}

size_t evdr_cluster_pages_workspace(int64_t lp_src, int64_t ls) {
    if (lp_src < 1 || lp_src > 65535 || ls < 1 || ls > 4096) return 0;
    return (size_t)EVDR_CLUSTER_GRID * (size_t)evdr_cluster_slice_bytes(lp_src, ls);
}

int evdr_cluster_pages(const void* src, int src_dtype, const uint8_t* pmask_or_null, int64_t b, int64_t lp_src, int64_t d_src,
                       int64_t src_stride, int64_t ls, int64_t iters, int32_t* members, int32_t* offsets, int32_t* labels_or_null,
                       void* workspace, size_t workspace_bytes, void* hip_stream) {
    const char* who = "evdr_cluster_pages";
    if (src_dtype != EVDR_F32 && src_dtype != EVDR_BF16 && src_dtype != EVDR_F16)
        return fail(EVDR_ERR_ARG, "%s: src_dtype must be EVDR_F32, EVDR_BF16 or EVDR_F16", who);
    if (b < 0 || lp_src < 0 || d_src < 0 || ls < 0 || iters < 0) return fail(EVDR_ERR_ARG, "%s: negative size", who);
    if (b > INT32_MAX) return fail(EVDR_ERR_SHAPE, "%s: b = %lld out of range", who, (long long)b);
    if (d_src < 1 || d_src > EVDR_D) return fail(EVDR_ERR_SHAPE, "%s: d_src = %lld outside 1..128", who, (long long)d_src);
    if (int rc = check_cluster_shape(who, lp_src, ls)) return rc;
    if (iters > 64) return fail(EVDR_ERR_SHAPE, "%s: iters = %lld outside 0..64", who, (long long)iters);
    if (b == 0) return EVDR_OK;
    if (!src || !members || !offsets || !workspace) return fail(EVDR_ERR_ARG, "%s: null pointer", who);
    if (src_stride < lp_src * d_src) return fail(EVDR_ERR_ARG, "%s: src_stride smaller than a source page", who);
    if (workspace_bytes < evdr_cluster_pages_workspace(lp_src, ls) || reinterpret_cast<uintptr_t>(workspace) % 16)
        return fail(EVDR_ERR_ARG, "%s: workspace of %zu bytes is smaller than evdr_cluster_pages_workspace's %zu, or not 16-byte aligned", who,
                    workspace_bytes, evdr_cluster_pages_workspace(lp_src, ls));
    EvdrClusterParams p{};
    p.src = src; p.src_dtype = src_dtype; p.pmask = pmask_or_null; p.b = b; p.src_stride = src_stride;
    p.lp_src = (int)lp_src; p.d_src = (int)d_src; p.ls = (int)ls; p.iters = (int)iters;
    p.members = members; p.offsets = offsets; p.labels = labels_or_null;
    p.workspace = workspace; p.slice_bytes = evdr_cluster_slice_bytes(lp_src, ls); p.cent_off = evdr_cluster_label_bytes(lp_src);
    hipError_t e = evdr_launch_cluster_pages(p, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "cluster_pages launch");
}

// 32-token slices of the fp8 forward over the whole corpus (pages == nullptr) or over the batch's page list (pages, m)
static int run_fwd8(const uint8_t* Q8, const uint8_t* P8, const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                    float* out, int64_t out_stride, int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t p_stride,
                    const int32_t* q_shift, const int32_t* p_shift, int32_t* qlist_ws_or_null, hipStream_t stream,
                    const int32_t* pages, int64_t m) {
    for (int64_t tok0 = 0; tok0 < lq; tok0 += 32) {           // 32-token slices, later ones add into out (as run_fwd)
        EvdrFwd8Params p8{};
        EvdrFwdParams& p = p8.g;
        p.Q = reinterpret_cast<const uint16_t*>(Q8);          // bytes: the strides below count bytes
        p.q_stride = lq * EVDR_D;
        p.P = reinterpret_cast<const uint16_t*>(P8);
        p.p_stride = p_stride;
        p.qmask = qmask;
        p.tilemask = tilemask;
        p.pageflags = pageflags;
        p.out = out;
        p.out_stride = out_stride;
        p.nq = (int)nq;
        p.lq = (int)((lq - tok0 < 32) ? (lq - tok0) : 32);
        p.np = (int)np;
        p.lp = (int)lp;
        p.tok0 = (int)tok0;
        p.lq_total = (int)lq;
        p.accumulate = tok0 > 0 ? 1 : 0;
        p8.q_shift = q_shift;
        p8.p_shift = p_shift;
        if (tok0 > 0 && qlist_ws_or_null && qmask) {
            hipError_t eq = evdr_launch_build_qlist(qmask, nq, lq, tok0, qlist_ws_or_null + 1, qlist_ws_or_null, stream);
            if (eq != hipSuccess) return hip_fail(eq, "build_qlist launch");
            p.qlist = qlist_ws_or_null + 1;
            p.qcount = qlist_ws_or_null;
        }
        hipError_t e;
        if (pages != nullptr) {                               // the batch's page list takes the place of the corpus (as run_fwd)
            p.np = (int)m;
            p.ncorpus = (int)np;
            p.gather = pages;
            e = evdr_launch_maxsim_fwd8_pages(p8, stream);    // (notes its instance itself)
        } else {
            evdr_note_fwd_kernel("maxsim_fwd8_kernel");
            e = evdr_launch_maxsim_fwd8(p8, stream);
        }
        if (e != hipSuccess) return hip_fail(e, "maxsim_fwd_fp8 launch");
    }
    return EVDR_OK;
}

int evdr_maxsim_fwd_fp8(const uint8_t* Q8, const uint8_t* P8, const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags,
                        float* out, int64_t out_stride, int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t p_stride,
                        const int32_t* q_shift, const int32_t* p_shift, int32_t* qlist_ws_or_null, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (nq == 0 || np == 0) return EVDR_OK;
    if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
    if (!Q8 || !P8 || !tilemask || !pageflags || !out || !q_shift || !p_shift)
        return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_fp8: null pointer");
    if (out_stride < np || p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "stride smaller than the row it spans");
    if (p_stride % 16) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_fp8: p_stride must be a multiple of 16 bytes");
    return run_fwd8(Q8, P8, qmask, tilemask, pageflags, out, out_stride, nq, lq, np, lp, p_stride, q_shift, p_shift, qlist_ws_or_null,
                    (hipStream_t)hip_stream, nullptr, 0);
}

int evdr_maxsim_fwd_fp8_pages(const uint8_t* Q8, const uint8_t* P8, const uint8_t* qmask, const uint32_t* tilemask,
                              const uint32_t* pageflags, const int32_t* pages, int64_t m, float* out, int64_t out_stride, int64_t nq,
                              int64_t lq, int64_t np, int64_t lp, int64_t p_stride, const int32_t* q_shift, const int32_t* p_shift,
                              int32_t* qlist_ws_or_null, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (m < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (m > INT32_MAX) return fail(EVDR_ERR_SHAPE, "size out of range (m=%lld)", (long long)m);
    if (nq == 0 || m == 0) return EVDR_OK;
    if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
    if (np == 0) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_fwd_fp8_pages: a page list over an empty corpus");
    if (!Q8 || !P8 || !tilemask || !pageflags || !pages || !out || !q_shift || !p_shift)
        return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_fp8_pages: null pointer");
    if (out_stride < m || p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "stride smaller than the row it spans");
    if (p_stride % 16) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_fp8_pages: p_stride must be a multiple of 16 bytes");
    if (lq > 32 && !qlist_ws_or_null)
        return fail(EVDR_ERR_WORKSPACE, "evdr_maxsim_fwd_fp8_pages: lq > 32 needs the (nq + 1) int32 qlist workspace");
    return run_fwd8(Q8, P8, qmask, tilemask, pageflags, out, out_stride, nq, lq, np, lp, p_stride, q_shift, p_shift, qlist_ws_or_null,
                    (hipStream_t)hip_stream, pages, m);
}

int evdr_maxsim_fwd_prepared_subset(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask,
                                    const uint32_t* tilemask, const uint32_t* pageflags, float* out, int64_t out_stride,
                                    int64_t nq, int64_t lq, int64_t np, int64_t lp, int nplanes, int64_t p_stride,
                                    int64_t p_plane_stride, const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null,
                                    const int32_t* qsel, const int32_t* qsel_count, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (nplanes != 1 && nplanes != 2) return fail(EVDR_ERR_ARG, "nplanes must be 1 (bf16) or 2 (fp16 hi/lo)");
    if (nq == 0 || np == 0) return EVDR_OK;
    if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
    if (lq > 32 || (lq == 1 && nq > 1)) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_fwd_prepared_subset: lq must be 2..32 (or one single-token query)");
    if (!Qplanes || !Pplanes || !tilemask || !pageflags || !out || !qsel || !qsel_count)
        return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_prepared_subset: null pointer");
    if (out_stride < np || p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "stride smaller than the row it spans");
    return run_fwd(Qplanes, lq * EVDR_D, nq * lq * EVDR_D, Pplanes, p_stride, p_plane_stride, qmask, tilemask, pageflags, out,
                   out_stride, nullptr, nq, lq, np, lp, nplanes, nplanes == 2 ? q_amax_or_null : nullptr,
                   nplanes == 2 ? p_amax_or_null : nullptr, nullptr, (hipStream_t)hip_stream, qsel, qsel_count);
}

static int check_qcache(const EvdrQCache* c, const char* who) {
    if (!c) return fail(EVDR_ERR_ARG, "%s: null cache", who);
    if (!c->slots || !c->ent_hash || !c->ent_k || !c->ent_q || !c->ent_mask || !c->ent_scores || !c->n_entries)
        return fail(EVDR_ERR_ARG, "%s: null pointer in the cache struct", who);
    if (c->capacity < 1 || c->capacity > INT32_MAX - 2 || c->lq < 1 || c->np < 1 || c->row_bytes < 4 || (c->row_bytes & 3))
        return fail(EVDR_ERR_ARG, "%s: bad cache geometry", who);
    if (c->n_slots < 2 * c->capacity || (c->n_slots & (c->n_slots - 1)) || c->n_slots > INT32_MAX)
        return fail(EVDR_ERR_ARG, "%s: n_slots must be a power of two >= 2 * capacity", who);
    return EVDR_OK;
}

size_t evdr_qcache_workspace(int64_t nq) {
    if (nq < 0) return 0;
    return align_up((size_t)nq * 8) + 2 * align_up((size_t)nq * 4) + 256;      // hashes | hit | qsel | {miss count, ticket}
}

int evdr_maxsim_fwd_prepared_cached(const EvdrQCache* cache, const void* Qrows, const uint16_t* Qplanes, const uint16_t* Pplanes,
                                    const uint8_t* qmask, const uint32_t* tilemask, const uint32_t* pageflags, float* out,
                                    int64_t out_stride, int64_t nq, int64_t lp, int nplanes, int64_t p_stride, int64_t p_plane_stride,
                                    const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null, void* workspace,
                                    size_t workspace_bytes, void* hip_stream) {
    if (int rc = check_qcache(cache, "evdr_maxsim_fwd_prepared_cached")) return rc;
    const int64_t lq = cache->lq, np = cache->np;
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (nplanes != 1 && nplanes != 2) return fail(EVDR_ERR_ARG, "nplanes must be 1 (bf16) or 2 (fp16 hi/lo)");
    if (nq == 0) return EVDR_OK;
    if (lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
    if (lq > 32 || lq < 2) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_fwd_prepared_cached: the cache's lq must be 2..32");
    if (!Qrows || !Qplanes || !Pplanes || !tilemask || !pageflags || !out) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_prepared_cached: null pointer");
    if (out_stride < np || p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "stride smaller than the row it spans");
    if (!workspace || workspace_bytes < evdr_qcache_workspace(nq))
        return fail(EVDR_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", evdr_qcache_workspace(nq), workspace_bytes);
    hipStream_t stream = (hipStream_t)hip_stream;
    char* ws = (char*)workspace;
    uint64_t* hashes = (uint64_t*)ws;
    int32_t* hit = (int32_t*)(ws + align_up((size_t)nq * 8));
    int32_t* qsel = (int32_t*)(ws + align_up((size_t)nq * 8) + align_up((size_t)nq * 4));
    int32_t* count = (int32_t*)(ws + align_up((size_t)nq * 8) + 2 * align_up((size_t)nq * 4));
    uint32_t* ticket = (uint32_t*)(count + 1);
    const uint32_t* qa = nplanes == 2 ? q_amax_or_null : nullptr;
    hipError_t e = evdr_launch_qcache_lookup_plan(*cache, Qrows, qmask, qa, nq, hashes, hit, qsel, count, ticket, stream);
    if (e != hipSuccess) return hip_fail(e, "qcache_lookup_plan launch");
    if (int rc = run_fwd(Qplanes, lq * EVDR_D, nq * lq * EVDR_D, Pplanes, p_stride, p_plane_stride, qmask, tilemask, pageflags, out,
                         out_stride, nullptr, nq, lq, np, lp, nplanes, qa, nplanes == 2 ? p_amax_or_null : nullptr, nullptr, stream,
                         qsel, count))
        return rc;
    e = evdr_launch_qcache_exchange(*cache, Qrows, qmask, nq, hit, out, out_stride, stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "qcache_exchange launch");
}

int evdr_maxsim_bwd(const float* g, const float* Q, const uint8_t* qmask, const uint8_t* pmask, const uint16_t* argmax,
                    float* dP, int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t d, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (d != EVDR_D) return fail(EVDR_ERR_SHAPE, "embedding width %lld unsupported", (long long)d);
    if (np == 0 || lp == 0) return EVDR_OK;
    if (!dP) return fail(EVDR_ERR_ARG, "evdr_maxsim_bwd: null dP");
    if (nq > 0 && lq > 0 && (!g || !Q || !argmax)) return fail(EVDR_ERR_ARG, "evdr_maxsim_bwd: null g/Q/argmax");
    hipError_t e = evdr_launch_maxsim_bwd(g, Q, qmask, pmask, argmax, dP, nq, lq, np, lp, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "maxsim_bwd launch");
}

size_t evdr_maxsim_bwd_q_workspace(int64_t nq, int64_t lq, int64_t np, int64_t lp) {
    if (nq < 0 || lq < 0 || np < 0 || lp < 0) return 0;
    return align_up((size_t)np * ntiles_of(lp) * 4) + align_up((size_t)np * 4) +
           align_up((size_t)evdr_bwd_q_segments(nq * lq, np) * nq * lq * EVDR_D * sizeof(float));
}

int evdr_maxsim_bwd_q(const float* g, const float* P, const uint8_t* qmask, const uint8_t* pmask, const uint16_t* argmax,
                      float* dQ, int64_t nq, int64_t lq, int64_t np, int64_t lp, int64_t d, void* workspace,
                      size_t workspace_bytes, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (d != EVDR_D) return fail(EVDR_ERR_SHAPE, "embedding width %lld unsupported", (long long)d);
    if (nq == 0 || lq == 0) return EVDR_OK;
    if (!dQ) return fail(EVDR_ERR_ARG, "evdr_maxsim_bwd_q: null dQ");
    if (np > 0 && (!g || !P || !argmax)) return fail(EVDR_ERR_ARG, "evdr_maxsim_bwd_q: null g/P/argmax");
    if (np > 0 && lp == 0) return fail(EVDR_ERR_SHAPE, "lp == 0");
    if (!workspace || workspace_bytes < evdr_maxsim_bwd_q_workspace(nq, lq, np, lp))
        return fail(EVDR_ERR_WORKSPACE, "workspace too small: need %zu bytes", evdr_maxsim_bwd_q_workspace(nq, lq, np, lp));
    hipStream_t stream = (hipStream_t)hip_stream;
    uint32_t* tilemask = (uint32_t*)workspace;
    uint32_t* pageflags = (uint32_t*)((char*)workspace + align_up((size_t)np * ntiles_of(lp) * 4));
    hipError_t e = hipSuccess;
    if (np > 0 && (e = evdr_launch_pack_pmask(pmask, np, lp, tilemask, pageflags, stream)) != hipSuccess)
        return hip_fail(e, "pack_pmask launch");
    float* partials = (float*)((char*)workspace + align_up((size_t)np * ntiles_of(lp) * 4) + align_up((size_t)np * 4));
    e = evdr_launch_maxsim_bwd_q(g, P, qmask, pageflags, argmax, dQ, partials, nq, lq, np, lp, stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "maxsim_bwd_q launch");
}

int evdr_maxsim_bwd_adamw(const float* g, const float* Q, const uint8_t* qmask, const uint8_t* pmask, const uint16_t* argmax,
                          float* x, float* exp_avg, float* exp_avg_sq, int64_t nq, int64_t lq, int64_t np, int64_t lp,
                          int64_t d, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                          float l2_eps, const void* adamw_state_or_null, void* hip_stream) {
    return evdr_maxsim_bwd_adamw_planes(g, Q, qmask, pmask, argmax, x, exp_avg, exp_avg_sq, nq, lq, np, lp, d, lr, beta1, beta2,
                                        eps, weight_decay, step, l2_eps, adamw_state_or_null, nullptr, nullptr, nullptr,
                                        hip_stream);
}

int evdr_maxsim_bwd_adamw_planes(const float* g, const float* Q, const uint8_t* qmask, const uint8_t* pmask,
                                 const uint16_t* argmax, float* x, float* exp_avg, float* exp_avg_sq, int64_t nq, int64_t lq,
                                 int64_t np, int64_t lp, int64_t d, double lr, double beta1, double beta2, double eps,
                                 double weight_decay, int64_t step, float l2_eps, const void* adamw_state_or_null,
                                 void* next_planes_or_null, uint32_t* next_amax_or_null, uint32_t* pageflags_or_null,
                                 void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (d != EVDR_D) return fail(EVDR_ERR_SHAPE, "embedding width %lld unsupported", (long long)d);
    if (!adamw_state_or_null && step < 1) return fail(EVDR_ERR_ARG, "step must be >= 1 (1 for the first update)");
    if (np == 0 || lp == 0) return EVDR_OK;
    if (!x || !exp_avg || !exp_avg_sq) return fail(EVDR_ERR_ARG, "evdr_maxsim_bwd_adamw: null parameter/state");
    if (nq > 0 && lq > 0 && (!g || !Q || !argmax)) return fail(EVDR_ERR_ARG, "evdr_maxsim_bwd_adamw: null g/Q/argmax");
    if (next_planes_or_null && !next_amax_or_null) return fail(EVDR_ERR_ARG, "evdr_maxsim_bwd_adamw_planes: planes without their absmax word");
    const double bc1 = 1.0 - pow(beta1, (double)(step < 1 ? 1 : step));
    const double bc2 = 1.0 - pow(beta2, (double)(step < 1 ? 1 : step));
    hipError_t e = evdr_launch_maxsim_bwd_adamw(g, Q, qmask, pmask, argmax, x, exp_avg, exp_avg_sq, nq, lq, np, lp, lr, beta1,
                                                beta2, eps, weight_decay, bc1, sqrt(bc2), l2_eps,
                                                adamw_state_or_null, next_planes_or_null, next_amax_or_null,
                                                pageflags_or_null, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "maxsim_bwd_adamw launch");
}

int evdr_adamw_step(const float* grad, float* x, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                    double beta2, double eps, double weight_decay, int64_t step, void* hip_stream) {
    if (n < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (n == 0) return EVDR_OK;
    if (!grad || !x || !exp_avg || !exp_avg_sq) return fail(EVDR_ERR_ARG, "evdr_adamw_step: null pointer");
    if (((uintptr_t)grad | (uintptr_t)x | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
        return fail(EVDR_ERR_ARG, "evdr_adamw_step: tensors must be 16-byte aligned");
    const double bc1 = 1.0 - pow(beta1, (double)(step < 1 ? 1 : step));
    const double bc2 = 1.0 - pow(beta2, (double)(step < 1 ? 1 : step));
    hipError_t e = evdr_launch_adamw(grad, x, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, sqrt(bc2),
                                     (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "adamw launch");
}

int evdr_adamw_advance(void* adamw_state, double beta1, double beta2, void* hip_stream) {
    if (!adamw_state) return fail(EVDR_ERR_ARG, "evdr_adamw_advance: null state");
    hipError_t e = evdr_launch_adamw_advance(adamw_state, beta1, beta2, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "adamw_advance launch");
}

int evdr_l2norm_fwd(const float* x, const uint8_t* rowmask_or_null, int64_t rows, int64_t d, float eps, float* y,
                    float* norm_or_null, void* hip_stream) {
    if (rows < 0) return fail(EVDR_ERR_ARG, "negative rows");
    if (d != EVDR_D) return fail(EVDR_ERR_SHAPE, "embedding width %lld unsupported", (long long)d);
    if (rows == 0) return EVDR_OK;
    if (!x || !y) return fail(EVDR_ERR_ARG, "evdr_l2norm_fwd: null pointer");
    hipError_t e = evdr_launch_l2norm_fwd(x, rowmask_or_null, rows, eps, y, norm_or_null, nullptr, nullptr, nullptr, 1,
                                          (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "l2norm_fwd launch");
}

int evdr_l2norm_fwd_split(const float* x, const uint8_t* rowmask_or_null, int64_t rows, int64_t d, float eps, float* y_or_null,
                          float* norm_or_null, uint16_t* planes, uint32_t* amax_bits, uint32_t* pageflags_or_null,
                          int64_t rows_per_page, void* hip_stream) {
    if (pageflags_or_null && rows_per_page < 1) return fail(EVDR_ERR_ARG, "evdr_l2norm_fwd_split: rows_per_page must be >= 1");
    if (rows < 0) return fail(EVDR_ERR_ARG, "negative rows");
    if (d != EVDR_D) return fail(EVDR_ERR_SHAPE, "embedding width %lld unsupported", (long long)d);
    if (!amax_bits) return fail(EVDR_ERR_ARG, "evdr_l2norm_fwd_split: null amax_bits");
    if (rows == 0) return EVDR_OK;
    if (!x || !planes) return fail(EVDR_ERR_ARG, "evdr_l2norm_fwd_split: null pointer");
    hipError_t e = evdr_launch_l2norm_fwd(x, rowmask_or_null, rows, eps, y_or_null, norm_or_null, planes, amax_bits,
                                          pageflags_or_null, rows_per_page, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "l2norm_fwd_split launch");
}

int evdr_l2norm_bwd(const float* gy, const float* x, const uint8_t* rowmask_or_null, const float* norm, int64_t rows,
                    int64_t d, float eps, float* dx, void* hip_stream) {
    if (rows < 0) return fail(EVDR_ERR_ARG, "negative rows");
    if (d != EVDR_D) return fail(EVDR_ERR_SHAPE, "embedding width %lld unsupported", (long long)d);
    if (rows == 0) return EVDR_OK;
    if (!gy || !x || !norm || !dx) return fail(EVDR_ERR_ARG, "evdr_l2norm_bwd: null pointer");
    hipError_t e = evdr_launch_l2norm_bwd(gy, x, rowmask_or_null, norm, rows, eps, dx, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "l2norm_bwd launch");
}

size_t evdr_topk_workspace(int64_t nq, int64_t n, int k) {
    if (nq <= 0 || n <= 0 || k < 1) return 0;
    const int nseg = evdr_topk_segments(nq, n);
    return nseg == 1 ? 0 : align_up((size_t)nq * nseg * k * 8);
}

int evdr_topk(const float* scores, const int32_t* idx_map_or_null, int64_t nq, int64_t n, int64_t row_stride,
              int32_t idx_base, int k, float* top_scores, int32_t* top_idx, void* workspace_or_null, size_t workspace_bytes,
              void* hip_stream) {
    if (nq < 0 || n < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (k < 1 || k > EVDR_TOPK_MAX) return fail(EVDR_ERR_ARG, "k=%d outside 1..%d", k, EVDR_TOPK_MAX);
    if (nq == 0) return EVDR_OK;
    if (!top_scores || !top_idx || (n > 0 && !scores)) return fail(EVDR_ERR_ARG, "evdr_topk: null pointer");
    if (row_stride < n) return fail(EVDR_ERR_ARG, "row_stride < n");
    if (workspace_or_null && workspace_bytes < evdr_topk_workspace(nq, n, k)) workspace_or_null = nullptr;   // too small: one level
    hipError_t e = evdr_launch_topk(scores, idx_map_or_null, nq, n, row_stride, idx_base, k, top_scores, top_idx,
                                    workspace_or_null, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "topk launch");
}

size_t evdr_maxsim_topk_workspace(int64_t nq, int64_t np) {
    if (nq < 0 || np < 0) return 0;
    return align_up((size_t)nq * np * sizeof(float)) + evdr_topk_workspace(nq, np, EVDR_TOPK_MAX);
}

int evdr_maxsim_topk(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask, const uint32_t* tilemask,
                     const uint32_t* pageflags, int64_t nq, int64_t lq, int64_t np, int64_t lp, int nplanes,
                     int64_t p_stride, int64_t p_plane_stride, const uint32_t* q_amax_or_null,
                     const uint32_t* p_amax_or_null, int32_t idx_base, int k, float* top_scores,
                     int32_t* top_idx, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!workspace || workspace_bytes < evdr_maxsim_topk_workspace(nq, np))
        return fail(EVDR_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu",
                    evdr_maxsim_topk_workspace(nq, np), workspace_bytes);
    float* scores = (float*)workspace;
    int rc = evdr_maxsim_fwd_prepared(Qplanes, Pplanes, qmask, tilemask, pageflags, scores, np, nullptr, nq, lq, np, lp,
                                      nplanes, p_stride, p_plane_stride, q_amax_or_null, p_amax_or_null, nullptr, hip_stream);
    if (rc != EVDR_OK) return rc;
    char* tkws = (char*)workspace + align_up((size_t)nq * np * sizeof(float));
    return evdr_topk(scores, nullptr, nq, np, np, idx_base, k, top_scores, top_idx, tkws, evdr_topk_workspace(nq, np, EVDR_TOPK_MAX),
                     hip_stream);
}

int evdr_prefilter_corpus_bound(const uint16_t* Pplanes, const uint32_t* tilemask, const uint32_t* pageflags, int64_t np, int64_t lp,
                                int64_t p_stride, int64_t p_plane_stride, float* bound, void* hip_stream) {
    if (int rc = check_common(0, 0, np, lp)) return rc;
    if (!bound) return fail(EVDR_ERR_ARG, "evdr_prefilter_corpus_bound: null bound");
    if (np > 0 && lp > 0) {
        if (!Pplanes || !tilemask || !pageflags) return fail(EVDR_ERR_ARG, "evdr_prefilter_corpus_bound: null pointer");
        if (p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "evdr_prefilter_corpus_bound: p_stride smaller than a page");
    }
    hipError_t e = evdr_launch_prefilter_corpus_bound(Pplanes, np, lp, p_stride, p_plane_stride, tilemask, pageflags, bound,
                                                      (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "prefilter corpus bound launch");
}

int evdr_prefilter_query_bound(const uint16_t* Qplanes, const uint8_t* qmask, int64_t nq, int64_t lq, const uint32_t* q_amax_or_null,
                               const uint32_t* p_amax_or_null, const float* bound, float* eq, void* hip_stream) {
    if (int rc = check_common(nq, lq, 0, 0)) return rc;
    if (lq > 32) return fail(EVDR_ERR_SHAPE, "evdr_prefilter_query_bound: lq must be <= 32");
    if (nq == 0) return EVDR_OK;
    if (!Qplanes || !bound || !eq) return fail(EVDR_ERR_ARG, "evdr_prefilter_query_bound: null pointer");
    hipError_t e = evdr_launch_prefilter_query_bound(Qplanes, qmask, nq, lq, q_amax_or_null, p_amax_or_null, bound, eq, nullptr,
                                                     (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "prefilter query bound launch");
}

int evdr_maxsim_fwd_coarse(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask, const uint32_t* tilemask,
                           const uint32_t* pageflags, float* out, int64_t out_stride, int64_t nq, int64_t lq, int64_t np, int64_t lp,
                           int64_t p_stride, int64_t p_plane_stride, const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null,
                           void* hip_stream) {
    if (int rc = check_prefilter("evdr_maxsim_fwd_coarse", nq, lq, np, lp, 2, p_stride)) return rc;
    if (nq == 0 || np == 0) return EVDR_OK;
    if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
    if (!Qplanes || !Pplanes || !tilemask || !pageflags || !out) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_coarse: null pointer");
    if (out_stride < np) return fail(EVDR_ERR_ARG, "out_stride < np");
    return run_coarse(Qplanes, Pplanes, qmask, tilemask, pageflags, out, out_stride, nq, lq, np, lp, p_stride, p_plane_stride,
                      q_amax_or_null, p_amax_or_null, (hipStream_t)hip_stream);
}

size_t evdr_maxsim_topk_prefilter_workspace(int64_t nq, int64_t np, int capacity) {
    if (nq < 0 || np < 0 || capacity < 1) return 0;
    return carve_prefilter(nq, np, capacity).total;
}

int evdr_maxsim_topk_prefilter(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask, const uint32_t* tilemask,
                               const uint32_t* pageflags, int64_t nq, int64_t lq, int64_t np, int64_t lp, int nplanes,
                               int64_t p_stride, int64_t p_plane_stride, const uint32_t* q_amax, const uint32_t* p_amax,
                               const float* bound, int32_t idx_base, int k, int capacity, float* top_scores, int32_t* top_idx,
                               int32_t* stats_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = check_prefilter("evdr_maxsim_topk_prefilter", nq, lq, np, lp, nplanes, p_stride)) return rc;
    if (k < 1 || k > EVDR_TOPK_MAX) return fail(EVDR_ERR_ARG, "k=%d outside 1..%d", k, EVDR_TOPK_MAX);
    if (capacity < k) return fail(EVDR_ERR_ARG, "capacity %d < k = %d", capacity, k);
    if (nq > 0 && (int64_t)capacity * nq > INT32_MAX) return fail(EVDR_ERR_SHAPE, "capacity * nq exceeds 2^31 - 1");
    if (nq == 0) return EVDR_OK;
    if (!top_scores || !top_idx) return fail(EVDR_ERR_ARG, "evdr_maxsim_topk_prefilter: null output");
    if (np == 0) return evdr_topk(nullptr, nullptr, nq, 0, 0, idx_base, k, top_scores, top_idx, nullptr, 0, hip_stream);
    if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
    if (!Qplanes || !Pplanes || !tilemask || !pageflags || !q_amax || !p_amax || !bound)
        return fail(EVDR_ERR_ARG, "evdr_maxsim_topk_prefilter: null pointer");
    const PrefilterWorkspace w = carve_prefilter(nq, np, capacity);
    if (!workspace || workspace_bytes < w.total)
        return fail(EVDR_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", w.total, workspace_bytes);
    hipStream_t stream = (hipStream_t)hip_stream;
    char* ws = (char*)workspace;
    float* coarse = (float*)(ws + w.coarse);
    void* tkws = ws + w.tkws;
    const size_t tkb = w.eq - w.tkws;
    float* eq = (float*)(ws + w.eq);
    int32_t* fcount = (int32_t*)(ws + w.fcount);
    int32_t* flist = (int32_t*)(ws + w.flist);
    int32_t* fb = (int32_t*)(ws + w.fb);
    int32_t* gather = (int32_t*)(ws + w.gather);
    int32_t* gcount = (int32_t*)(ws + w.gcount);
    float* cand = (float*)(ws + w.cand);
    const int kc = (int)(np < k ? np : k);                  // the k-th coarse score exists only in a corpus of >= k pages
    // 1. coarse pass, 2. E_q (and the fallback count reset), 3. the k-th coarse score, 4. candidate lists / fallback list
    int rc = run_coarse(Qplanes, Pplanes, qmask, tilemask, pageflags, coarse, np, nq, lq, np, lp, p_stride, p_plane_stride, q_amax, p_amax,
                        stream);
    if (rc != EVDR_OK) return rc;
    hipError_t e = evdr_launch_prefilter_query_bound(Qplanes, qmask, nq, lq, q_amax, p_amax, bound, eq, fcount, stream);
    if (e != hipSuccess) return hip_fail(e, "prefilter query bound launch");
    if ((rc = evdr_topk(coarse, nullptr, nq, np, np, 0, kc, (float*)(ws + w.tv), (int32_t*)(ws + w.ti), tkws, tkb, hip_stream)) != EVDR_OK)
        return rc;
    e = evdr_launch_prefilter_select(coarse, nq, np, (const float*)(ws + w.tv), kc, eq, capacity, gather, gcount, cand, fb, flist, fcount,
                                     stats_or_null, stream);
    if (e != hipSuccess) return hip_fail(e, "prefilter select launch");
    // 5. exact rerank of every list (the exhaustive launch's arithmetic), 6. its top-k, reported as corpus pages through the list
    {
        EvdrFwdParams p{};
        p.Q = Qplanes;
        p.q_stride = lq * EVDR_D;
        p.q_plane_stride = nq * lq * EVDR_D;
        p.P = Pplanes;
        p.p_stride = p_stride;
        p.p_plane_stride = p_plane_stride;
        p.q_amax = q_amax;
        p.p_amax = p_amax;
        p.qmask = qmask;
        p.tilemask = tilemask;
        p.pageflags = pageflags;
        p.out = cand;
        p.out_stride = capacity;
        p.nq = (int)nq;
        p.lq = (int)lq;
        p.np = capacity;
        p.lp = (int)lp;
        p.lq_total = (int)lq;
        p.inblock_refill = 1;
        p.gather = gather;
        p.gcount = gcount;
        if ((e = evdr_launch_maxsim_gather16(p, stream)) != hipSuccess) return hip_fail(e, "prefilter rerank launch");
    }
    if ((rc = evdr_topk(cand, gather, nq, capacity, capacity, 0, k, (float*)(ws + w.rv), (int32_t*)(ws + w.ri), tkws, tkb, hip_stream)) != EVDR_OK)
        return rc;
    // 7. fallback rows: the exhaustive exact forward over the device-side list (into the coarse block), 8. their top-k
    if ((rc = run_fwd(Qplanes, lq * EVDR_D, nq * lq * EVDR_D, Pplanes, p_stride, p_plane_stride, qmask, tilemask, pageflags, coarse, np,
                      nullptr, nq, lq, np, lp, 2, q_amax, p_amax, nullptr, stream, flist, fcount, false)) != EVDR_OK)
        return rc;
    if ((rc = evdr_topk(coarse, nullptr, nq, np, np, idx_base, k, (float*)(ws + w.fv), (int32_t*)(ws + w.fi), tkws, tkb, hip_stream)) != EVDR_OK)
        return rc;
    // 9. by row
    e = evdr_launch_prefilter_merge((const float*)(ws + w.rv), (const int32_t*)(ws + w.ri), (const float*)(ws + w.fv), (const int32_t*)(ws + w.fi),
                                    fb, nq, k, idx_base, fcount, top_scores, top_idx, stats_or_null, stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "prefilter merge launch");
}

size_t evdr_maxsim_fwd_candidates_workspace(int64_t nq, int r) {
    if (nq < 0 || r < 1 || r > EVDR_SELECT_MAX) return 0;
    return carve_candidates(nq, r).total;
}

int evdr_maxsim_fwd_candidates(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask, const uint32_t* tilemask,
                               const uint32_t* pageflags, const int32_t* cand, int r, int32_t idx_base, float* out, int64_t out_stride,
                               int32_t* cand_clean_or_null, int64_t nq, int64_t lq, int64_t np, int64_t lp, int nplanes, int64_t p_stride,
                               int64_t p_plane_stride, const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null, void* workspace,
                               size_t workspace_bytes, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (nplanes == 4) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_fwd_candidates: width-256 corpora (nplanes = 4) are not covered");
    if (nplanes != 1 && nplanes != 2) return fail(EVDR_ERR_ARG, "nplanes must be 1 (bf16) or 2 (fp16 hi/lo)");
    if (lq > 32) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_fwd_candidates: lq must be <= 32");
    if (r < 1 || r > EVDR_SELECT_MAX) return fail(EVDR_ERR_ARG, "r=%d outside 1..%d", r, EVDR_SELECT_MAX);
    if (nq * r > INT32_MAX) return fail(EVDR_ERR_SHAPE, "nq * r exceeds 2^31 - 1");
    if (nq == 0) return EVDR_OK;
    if (!cand || !out) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_candidates: null cand/out");
    if (out_stride < r) return fail(EVDR_ERR_ARG, "out_stride < r");
    if (np > 0) {
        if (lq == 0 || lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
        if (!Qplanes || !Pplanes || !tilemask || !pageflags) return fail(EVDR_ERR_ARG, "evdr_maxsim_fwd_candidates: null pointer");
        if (p_stride < lp * EVDR_D) return fail(EVDR_ERR_ARG, "p_stride smaller than a page");
    }
    const CandWorkspace w = carve_candidates(nq, r);
    if (!workspace || workspace_bytes < w.total)
        return fail(EVDR_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", w.total, workspace_bytes);
    hipStream_t stream = (hipStream_t)hip_stream;
    char* ws = (char*)workspace;
    int32_t* glist = (int32_t*)(ws + w.glist);
    int32_t* gpos = (int32_t*)(ws + w.gpos);
    int32_t* gcount = (int32_t*)(ws + w.gcount);
    float* tmp = (float*)(ws + w.tmp);
    // 1. lists with holes -> compacted local pages, their list positions and counts; -inf into the holes
    hipError_t e = evdr_launch_cand_compact(cand, nq, r, idx_base, np, glist, gpos, gcount, out, out_stride, cand_clean_or_null, stream);
    if (e != hipSuccess) return hip_fail(e, "candidate compaction launch");
    if (np == 0) return EVDR_OK;                                // every entry is a hole
    // 2. the exhaustive staged kernel's arithmetic over each query's list, 3. scores back to their list positions
    EvdrFwdParams p{};
    p.Q = Qplanes;
    p.q_stride = lq * EVDR_D;
    p.q_plane_stride = nq * lq * EVDR_D;
    p.P = Pplanes;
    p.p_stride = p_stride;
    p.p_plane_stride = p_plane_stride;
    p.q_amax = nplanes == 2 ? q_amax_or_null : nullptr;
    p.p_amax = nplanes == 2 ? p_amax_or_null : nullptr;
    p.qmask = qmask;
    p.tilemask = tilemask;
    p.pageflags = pageflags;
    p.out = tmp;
    p.out_stride = r;
    p.nq = (int)nq;
    p.lq = (int)lq;
    p.np = r;
    p.lp = (int)lp;
    p.lq_total = (int)lq;
    p.inblock_refill = 1;
    p.gather = glist;
    p.gcount = gcount;
    // List chunks map to XCDs round-robin (block_work): the automatic choice (64 positions per workgroup) would give a list of 128 two
    // chunks, i.e. work for two of the eight XCDs.  Here: the smallest multiple of 8 chunks of at most 64 positions each
    // (a pages-per-block override of the calling thread, evdr_debug_set_pages_per_block, is left in charge).
    const int nch = 8 * ((r + 8 * 64 - 1) / (8 * 64));
    const int prev = evdr_pages_per_block_exchange((r + nch - 1) / nch);
    if (prev > 0) evdr_pages_per_block_exchange(prev);
    e = nplanes == 2 ? evdr_launch_maxsim_gather16(p, stream) : evdr_launch_maxsim_gather16_bf16(p, stream);
    if (prev <= 0) evdr_pages_per_block_exchange(prev);
    if (e != hipSuccess) return hip_fail(e, "candidate scoring launch");
    e = evdr_launch_cand_scatter(tmp, gpos, gcount, nq, r, out, out_stride, stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "candidate scatter launch");
}

int evdr_select_topr(const float* scores, int64_t nq, int64_t n, int64_t row_stride, int32_t idx_base, int r, int32_t* top_idx,
                     void* hip_stream) {
    if (nq < 0 || n < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (r < 1 || r > EVDR_SELECT_MAX) return fail(EVDR_ERR_ARG, "r=%d outside 1..%d", r, EVDR_SELECT_MAX);
    if (nq > INT32_MAX || n > INT32_MAX) return fail(EVDR_ERR_SHAPE, "size out of range (nq=%lld n=%lld)", (long long)nq, (long long)n);
    if (nq == 0) return EVDR_OK;
    if (!top_idx || (n > 0 && !scores)) return fail(EVDR_ERR_ARG, "evdr_select_topr: null pointer");
    if (row_stride < n) return fail(EVDR_ERR_ARG, "row_stride < n");
    hipError_t e = evdr_launch_select_topr(scores, nq, n, row_stride, idx_base, r, top_idx, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "select_topr launch");
}

int evdr_maxsim_align(const uint16_t* Qplanes, const uint16_t* Pplanes, const uint8_t* qmask, const uint32_t* tilemask,
                      const uint32_t* pageflags, const int32_t* cand, int64_t r, int32_t idx_base, float* sim, int32_t* patch,
                      float* heat_or_null, int64_t nq, int64_t lq, int64_t np, int64_t lp, int nplanes, int64_t p_stride,
                      int64_t p_plane_stride, const uint32_t* q_amax_or_null, const uint32_t* p_amax_or_null, void* hip_stream) {
    if (int rc = check_common(nq, lq, np, lp)) return rc;
    if (r < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (nplanes == 4) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_align: width-256 corpora (nplanes = 4) are not covered");
    if (nplanes != 1 && nplanes != 2) return fail(EVDR_ERR_ARG, "nplanes must be 1 (bf16) or 2 (fp16 hi/lo)");
    if (lq < 1 || lq > 32) return fail(EVDR_ERR_SHAPE, "evdr_maxsim_align: lq = %lld outside 1..32", (long long)lq);
    if (r < 1 || r > EVDR_SELECT_MAX) return fail(EVDR_ERR_ARG, "r=%lld outside 1..%d", (long long)r, EVDR_SELECT_MAX);
    if (nq * r > INT32_MAX) return fail(EVDR_ERR_SHAPE, "nq * r exceeds 2^31 - 1");
    if (nq == 0) return EVDR_OK;
    if (!cand || !sim || !patch) return fail(EVDR_ERR_ARG, "evdr_maxsim_align: null cand/sim/patch");
    if (np > 0) {
        if (lp == 0) return fail(EVDR_ERR_SHAPE, "zero-length token axis");
        if (!Qplanes || !Pplanes || !tilemask || !pageflags) return fail(EVDR_ERR_ARG, "evdr_maxsim_align: null pointer");
        // the fragments are 16-byte loads
        if (p_stride < lp * EVDR_D || p_stride % 8 != 0 || (nplanes == 2 && p_plane_stride % 8 != 0) ||
            ((uintptr_t)Qplanes | (uintptr_t)Pplanes) % 16 != 0)
            return fail(EVDR_ERR_ARG, "evdr_maxsim_align: p_stride smaller than a page, or planes / strides not 16-byte aligned");
    }
    hipError_t e = evdr_launch_maxsim_align(Qplanes, Pplanes, qmask, tilemask, pageflags, cand, (int)r, idx_base, sim, patch, heat_or_null,
                                            nq, (int)lq, np, (int)lp, nplanes, p_stride, p_plane_stride, q_amax_or_null, p_amax_or_null,
                                            (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "token alignment launch");
}

// ---- document-level search (csrc/docs.hip) -------------------------------------------------------------------------------------------
namespace {
int check_doc_max(const char* who, const float* scores, const int32_t* members, const int32_t* offsets, int64_t nq, int64_t n,
                  int64_t row_stride, int64_t nm, int64_t n_docs) {
    if (nq < 0 || n < 0 || nm < 0 || n_docs < 0) return fail(EVDR_ERR_ARG, "%s: negative size", who);
    if (nq > INT32_MAX || n > INT32_MAX || nm > INT32_MAX || n_docs > INT32_MAX)
        return fail(EVDR_ERR_SHAPE, "%s: size out of range (nq=%lld n=%lld nm=%lld n_docs=%lld)", who, (long long)nq, (long long)n,
                    (long long)nm, (long long)n_docs);
    const int64_t wgs = ((n_docs + EVDR_DOC_BLOCK - 1) / EVDR_DOC_BLOCK) * ((nq + EVDR_DOC_ROWS - 1) / EVDR_DOC_ROWS);
    if (wgs > INT32_MAX) return fail(EVDR_ERR_SHAPE, "%s: %lld workgroups exceed 2^31 - 1", who, (long long)wgs);
    if (nq == 0) return EVDR_OK;
    if ((n > 0 && !scores) || (nm > 0 && !members) || (n_docs > 0 && !offsets)) return fail(EVDR_ERR_ARG, "%s: null pointer", who);
    if (row_stride < n) return fail(EVDR_ERR_ARG, "%s: row_stride < n", who);
    return EVDR_OK;
}
}  // namespace

int evdr_doc_max(const float* scores, const int32_t* members, const int32_t* offsets, const int32_t* idx_map_or_null, int64_t nq,
                 int64_t n, int64_t row_stride, int64_t nm, int64_t n_docs, int32_t idx_base, float* doc_scores, int64_t doc_stride,
                 int32_t* doc_best, void* hip_stream) {
    if (int rc = check_doc_max("evdr_doc_max", scores, members, offsets, nq, n, row_stride, nm, n_docs)) return rc;
    if (nq == 0) return EVDR_OK;
    if (n_docs > 0 && (!doc_scores || !doc_best)) return fail(EVDR_ERR_ARG, "evdr_doc_max: null output");
    if (doc_stride < n_docs) return fail(EVDR_ERR_ARG, "evdr_doc_max: doc_stride < n_docs");
    hipError_t e = evdr_launch_doc_max(scores, members, offsets, idx_map_or_null, nq, n, row_stride, nm, n_docs, idx_base, doc_scores,
                                       doc_stride, doc_best, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "doc_max launch");
}

int evdr_collapse_topk(const float* scores, const int32_t* page, const int32_t* doc_or_null, const int32_t* doc_of_page_or_null,
                       int64_t np, int32_t idx_base, int64_t nq, int r, int64_t row_stride, int k, float* top_scores,
                       int32_t* top_doc, int32_t* top_page, void* hip_stream) {
    if (nq < 0 || np < 0) return fail(EVDR_ERR_ARG, "evdr_collapse_topk: negative size");
    if (r < 1 || r > EVDR_SELECT_MAX) return fail(EVDR_ERR_ARG, "evdr_collapse_topk: r=%d outside 1..%d", r, EVDR_SELECT_MAX);
    if (k < 1 || k > EVDR_TOPK_MAX) return fail(EVDR_ERR_ARG, "evdr_collapse_topk: k=%d outside 1..%d", k, EVDR_TOPK_MAX);
    if (nq > INT32_MAX || np > INT32_MAX)
        return fail(EVDR_ERR_SHAPE, "evdr_collapse_topk: size out of range (nq=%lld np=%lld)", (long long)nq, (long long)np);
    const bool by_page = doc_of_page_or_null != nullptr;
    if ((doc_or_null != nullptr) == by_page)
        return fail(EVDR_ERR_ARG, "evdr_collapse_topk: give exactly one of doc and doc_of_page (%s)", by_page ? "both given" : "neither given");
    if (nq == 0) return EVDR_OK;
    if (!scores || !page || !top_scores || !top_doc || !top_page) return fail(EVDR_ERR_ARG, "evdr_collapse_topk: null pointer");
    if (row_stride < r) return fail(EVDR_ERR_ARG, "evdr_collapse_topk: row_stride < r");
    hipError_t e = evdr_launch_collapse_topk(scores, page, doc_or_null, doc_of_page_or_null, np, idx_base, nq, r, row_stride, k, top_scores,
                                             top_doc, top_page, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "collapse_topk launch");
}

size_t evdr_doc_topk_workspace(int64_t nq, int64_t n_docs) {
    if (nq <= 0 || n_docs <= 0) return 0;
    return 2 * align_up((size_t)nq * n_docs * 4) + evdr_topk_workspace(nq, n_docs, EVDR_TOPK_MAX);
}

int evdr_doc_topk(const float* scores, const int32_t* members, const int32_t* offsets, const int32_t* idx_map_or_null, int64_t nq,
                  int64_t n, int64_t row_stride, int64_t nm, int64_t n_docs, int32_t idx_base, int k, float* top_scores,
                  int32_t* top_doc, int32_t* top_page, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = check_doc_max("evdr_doc_topk", scores, members, offsets, nq, n, row_stride, nm, n_docs)) return rc;
    if (k < 1 || k > EVDR_TOPK_MAX) return fail(EVDR_ERR_ARG, "evdr_doc_topk: k=%d outside 1..%d", k, EVDR_TOPK_MAX);
    if (nq == 0) return EVDR_OK;
    if (!top_scores || !top_doc || !top_page) return fail(EVDR_ERR_ARG, "evdr_doc_topk: null output");
    const size_t need = evdr_doc_topk_workspace(nq, n_docs);
    if (need && (!workspace || workspace_bytes < need))
        return fail(EVDR_ERR_WORKSPACE, "evdr_doc_topk: workspace too small: need %zu bytes, got %zu", need, workspace ? workspace_bytes : (size_t)0);
    const size_t blk = align_up((size_t)nq * n_docs * 4);
    float* ds = (float*)workspace;
    int32_t* db = n_docs ? (int32_t*)((char*)workspace + blk) : nullptr;
    void* tkws = n_docs ? (char*)workspace + 2 * blk : nullptr;
    hipStream_t stream = (hipStream_t)hip_stream;
    hipError_t e = evdr_launch_doc_max(scores, members, offsets, idx_map_or_null, nq, n, row_stride, nm, n_docs, idx_base, ds, n_docs, db, stream);
    if (e != hipSuccess) return hip_fail(e, "doc_max launch");
    if (int rc = evdr_topk(n_docs ? ds : nullptr, nullptr, nq, n_docs, n_docs, 0, k, top_scores, top_doc, tkws,
                           evdr_topk_workspace(nq, n_docs, EVDR_TOPK_MAX), hip_stream))
        return rc;
    e = evdr_launch_doc_finish(top_scores, top_doc, top_page, db, nq, n_docs, k, stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "doc_topk finish launch");
}

int evdr_infonce_distill_fwd_bwd(const float* score_s, const float* score_t, int64_t b, int64_t n, float temperature,
                                 float* loss, float* dscore_or_null, float* row_loss, void* hip_stream) {
    if (b < 0 || n < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (!(temperature > 0.f)) return fail(EVDR_ERR_ARG, "temperature must be > 0");
    if (b == 0 || n == 0) return fail(EVDR_ERR_SHAPE, "empty score matrix (b=%lld n=%lld)", (long long)b, (long long)n);
    if (!score_s || !score_t || !loss || !row_loss) return fail(EVDR_ERR_ARG, "evdr_infonce_distill_fwd_bwd: null pointer");
    hipError_t e = evdr_launch_infonce(score_s, score_t, b, n, temperature, loss, dscore_or_null, row_loss,
                                       (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "infonce launch");
}

int evdr_infonce_distill_fwd_bwd_ws(const float* score_s, const float* score_t, int64_t b, int64_t n, float temperature,
                                    float* loss, float* dscore_or_null, void* workspace, void* hip_stream) {
    if (b < 0 || n < 0) return fail(EVDR_ERR_ARG, "negative size");
    if (!(temperature > 0.f)) return fail(EVDR_ERR_ARG, "temperature must be > 0");
    if (b == 0 || n == 0) return fail(EVDR_ERR_SHAPE, "empty score matrix (b=%lld n=%lld)", (long long)b, (long long)n);
    if (!score_s || !score_t || !loss || !workspace) return fail(EVDR_ERR_ARG, "evdr_infonce_distill_fwd_bwd_ws: null pointer");
    hipError_t e = evdr_launch_infonce_ws(score_s, score_t, b, n, temperature, loss, dscore_or_null, (float*)workspace,
                                          (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "infonce launch");
}

// ---- the pairwise ranking losses (csrc/pairloss.hip): workspace = one fp64 partial per workgroup | ticket word
namespace {
inline size_t pair_partials_bytes(int64_t b, int64_t n) { return align_up((size_t)b * (size_t)((n + EVDR_PAIR_TILE - 1) / EVDR_PAIR_TILE) * 8); }

int check_pair_loss(const char* who, int64_t b, int64_t n, const void* in0, const void* in1, const void* in2, const float* loss,
                    const void* workspace, size_t workspace_bytes) {
    if (b < 1 || n < 1) return fail(EVDR_ERR_ARG, "%s: b and n must be >= 1 (b=%lld n=%lld)", who, (long long)b, (long long)n);
    if (!in0 || !in1 || !in2 || !loss || !workspace) return fail(EVDR_ERR_ARG, "%s: null pointer", who);
    if (b > EVDR_PAIR_MAX_B || n > EVDR_PAIR_MAX_N)
        return fail(EVDR_ERR_SHAPE, "%s: shape beyond the launch limits (b=%lld > %d or n=%lld > %d)", who, (long long)b, EVDR_PAIR_MAX_B,
                    (long long)n, EVDR_PAIR_MAX_N);
    if (((uintptr_t)workspace & 7u) != 0) return fail(EVDR_ERR_ARG, "%s: workspace must be 8-byte aligned", who);
    const size_t need = evdr_pair_loss_workspace(b, n);
    if (workspace_bytes < need) return fail(EVDR_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", who, need, workspace_bytes);
    return EVDR_OK;
}
}  // namespace

size_t evdr_pair_loss_workspace(int64_t b, int64_t n) {
    if (b < 1 || n < 1 || b > EVDR_PAIR_MAX_B || n > EVDR_PAIR_MAX_N) return 0;
    return pair_partials_bytes(b, n) + 256;
}

int evdr_pairwise_distill_fwd_bwd(const float* score_s, const float* score_t, int64_t b, int64_t n, float* loss, float* grad_or_null,
                                  void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = check_pair_loss("evdr_pairwise_distill_fwd_bwd", b, n, score_s, score_t, score_s, loss, workspace, workspace_bytes)) return rc;
    unsigned int* ticket = (unsigned int*)((char*)workspace + pair_partials_bytes(b, n));
    hipError_t e = evdr_launch_pairwise_distill(score_s, score_t, b, n, loss, grad_or_null, (double*)workspace, ticket, (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "pairwise_distill launch");
}

int evdr_lambda_pairs_fwd_bwd(const float* s_sorted, const float* gain, const float* disc, int64_t b, int64_t n, float alpha, float eps,
                              float* loss, float* grad_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (int rc = check_pair_loss("evdr_lambda_pairs_fwd_bwd", b, n, s_sorted, gain, disc, loss, workspace, workspace_bytes)) return rc;
    unsigned int* ticket = (unsigned int*)((char*)workspace + pair_partials_bytes(b, n));
    hipError_t e = evdr_launch_lambda_pairs(s_sorted, gain, disc, b, n, alpha, eps, loss, grad_or_null, (double*)workspace, ticket,
                                            (hipStream_t)hip_stream);
    return e == hipSuccess ? EVDR_OK : hip_fail(e, "lambda_pairs launch");
}

}  // extern "C"
