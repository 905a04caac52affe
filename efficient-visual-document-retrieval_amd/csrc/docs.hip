// Document-level search: page scores collapsed to documents, entirely on the device.
//
// evdr_doc_max       a segmented arg-max over a (nq, n) score block: per (query row, document) the largest order key among the
//                    document's listed columns and the LOWEST reported page index attaining it.
// evdr_collapse_topk the top-k DISTINCT documents of a per-query list of (score, page[, document]) entries: the candidate and the
//                    shard-merge form.
// evdr_doc_topk      evdr_doc_max into the workspace, evdr_topk over the (nq, n_docs) block, and a small gather of the best pages.
//
// Every comparison is an INTEGER comparison of one packed word, (order key << 32) | ~reported index: the maximum of such words is
// the best score and, among equal scores, the lowest reported index -- whatever order the members arrive in.  No float compare,
// no atomics of any kind, no workspace (evdr_doc_max, evdr_collapse_topk): the same bits on every launch.
//
// evdr_doc_max geometry.  A 256-thread workgroup owns EVDR_DOC_BLOCK = 256 consecutive documents and EVDR_DOC_ROWS = 8 query rows:
// the member lists of its documents are read once for 8 rows of scores (eight independent loads in flight per lane), and the
// rest of the row blocks find them in the L2 (400 KB of members for 100 k pages).  Documents shorter than EVDR_DOC_LONG = 32
// pages -- the usual case: PDFs, decks -- take one LANE each (neighbouring lanes read neighbouring stretches of `members` and of
// the score rows, so a wave's loads fall into a few cache lines that stay in the L1 for the next iterations); longer documents
// are listed in the LDS and taken by one WAVE each, 64 members per step with unit-stride reads of `members`, and a 6-step
// butterfly of the packed words.  Lanes never wait for a 5000-page neighbour, and a long document keeps 64 lanes busy.
// Nothing is read through an index that was not checked: offsets are clamped to [0, nm], members outside [0, n) are holes.
//
// evdr_collapse_topk geometry.  One 256-thread workgroup per row, the whole list (<= EVDR_SELECT_MAX = 4096 entries) in 48 KB of
// LDS as 96-bit records.  Two bitonic sorts: by (document asc, key desc, page asc) -- the first record of every run of equal
// documents is that document's winner --, then the winners by (key desc, document asc).  Sorting makes the result independent
// of the order of the list; duplicates are equal records.  Ids may be sparse and as large as 2^31 - 1: they are only compared.
#include "evdr_common.h"

namespace {

constexpr int DM_THREADS = 256;
constexpr int DM_WAVES = DM_THREADS / 64;
constexpr uint32_t KEY_NINF = 0x007FFFFFu;           // order_key(-inf): "absent"
static_assert(EVDR_DOC_BLOCK == DM_THREADS, "one lane per document of the block");

// evdr_topk's order (csrc/topk.hip, order_key / key_to_float): the two must stay the same function
__device__ __forceinline__ uint32_t order_key(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;   // NaN of either sign ranks first (integer test: the build assumes no NaNs)
    if (u == 0x80000000u) u = 0u;                              // -0.0 ties with +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_to_float(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __builtin_bit_cast(float, u);
}

__device__ __forceinline__ unsigned long long umax64(unsigned long long x, unsigned long long y) { return x > y ? x : y; }

__global__ void __launch_bounds__(DM_THREADS) doc_max_kernel(const float* __restrict__ scores, const int32_t* __restrict__ members,
                                                            const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ idx_map, int64_t nq, int64_t n,
                                                            int64_t row_stride, int64_t nm, int64_t n_docs, int32_t idx_base,
                                                            int64_t ndb, float* __restrict__ doc_scores, int64_t doc_stride,
                                                            int32_t* __restrict__ doc_best) {
    __shared__ int32_t long_list[EVDR_DOC_BLOCK];
    __shared__ uint32_t wave_cnt[DM_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t d0 = (int64_t)(blockIdx.x % ndb) * EVDR_DOC_BLOCK;
    const int64_t q0 = (int64_t)(blockIdx.x / ndb) * EVDR_DOC_ROWS;

    // rows past nq read the last row again (a valid address) and are never written
    const float* row0 = scores + q0 * row_stride;
    const int rlast = (int)min((int64_t)EVDR_DOC_ROWS, nq - q0) - 1;

    auto clamp_off = [&](int64_t d, int64_t& lo, int64_t& hi) {
        lo = min(max((int64_t)offsets[d], (int64_t)0), nm);
        hi = min(max((int64_t)offsets[d + 1], lo), nm);
    };
    // one member into the running words of the 8 rows
    auto take = [&](int32_t col, unsigned long long (&best)[EVDR_DOC_ROWS]) {
        if ((uint32_t)col >= (uint32_t)n) return;                                   // hole: never an address
        const uint32_t rep = (uint32_t)((idx_map ? idx_map[col] : col) + idx_base);
        const uint32_t low = 0xFFFFFFFFu - rep;
        float f[EVDR_DOC_ROWS];
#pragma unroll
        for (int r = 0; r < EVDR_DOC_ROWS; ++r) f[r] = row0[min(r, rlast) * row_stride + col];
#pragma unroll
        for (int r = 0; r < EVDR_DOC_ROWS; ++r) {
            const uint32_t key = order_key(f[r]);
            const unsigned long long w = key == KEY_NINF ? 0ull : (((unsigned long long)key << 32) | low);
            best[r] = umax64(best[r], w);
        }
    };
    auto store = [&](int64_t d, int r, unsigned long long w) {
        if (q0 + r >= nq) return;
        doc_scores[(q0 + r) * doc_stride + d] = w ? key_to_float((uint32_t)(w >> 32)) : -__builtin_inff();
        doc_best[(q0 + r) * n_docs + d] = w ? (int32_t)(0xFFFFFFFFu - (uint32_t)w) : -1;
    };

    // ---- short documents: one lane each
    const int64_t d = d0 + tid;
    int64_t lo = 0, hi = 0;
    if (d < n_docs) clamp_off(d, lo, hi);
    const bool is_long = hi - lo >= EVDR_DOC_LONG;
    if (d < n_docs && !is_long) {
        unsigned long long best[EVDR_DOC_ROWS];
#pragma unroll
        for (int r = 0; r < EVDR_DOC_ROWS; ++r) best[r] = 0ull;
        for (int64_t i = lo; i < hi; ++i) take(members[i], best);
#pragma unroll
        for (int r = 0; r < EVDR_DOC_ROWS; ++r) store(d, r, best[r]);
    }

    // ---- long documents: listed in block order, one wave each
    const unsigned long long bal = __ballot(is_long);
    if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < DM_WAVES; ++w) {
        if (w < wv) before += wave_cnt[w];
        total += wave_cnt[w];
    }
    if (is_long) long_list[before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    for (uint32_t j = wv; j < total; j += DM_WAVES) {
        const int64_t dl = d0 + long_list[j];
        int64_t llo, lhi;
        clamp_off(dl, llo, lhi);
        unsigned long long best[EVDR_DOC_ROWS];
#pragma unroll
        for (int r = 0; r < EVDR_DOC_ROWS; ++r) best[r] = 0ull;
        for (int64_t i = llo + lane; i < lhi; i += 64) take(members[i], best);
#pragma unroll
        for (int r = 0; r < EVDR_DOC_ROWS; ++r) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) best[r] = umax64(best[r], (unsigned long long)__shfl_xor(best[r], off));
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < EVDR_DOC_ROWS; ++r) store(dl, r, best[r]);
        }
    }
}

// ---- top-k distinct documents of a list --------------------------------------------------------------------------------------------
constexpr int CT_THREADS = 256;

__global__ void __launch_bounds__(CT_THREADS) collapse_topk_kernel(const float* __restrict__ scores, const int32_t* __restrict__ page,
                                                                  const int32_t* __restrict__ doc,
                                                                  const int32_t* __restrict__ doc_of_page, int64_t np,
                                                                  int32_t idx_base, int r, int npad, int64_t row_stride, int k,
                                                                  float* __restrict__ top_scores, int32_t* __restrict__ top_doc,
                                                                  int32_t* __restrict__ top_page) {
    __shared__ unsigned long long a[EVDR_SELECT_MAX];    // sort word, descending
    __shared__ uint32_t b[EVDR_SELECT_MAX];              // its low 32 bits: ~page

    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    // records: (~document, key, ~page); a hole, or an entry scored -inf, is the all-zero record, which sorts below every real one
    for (int i = tid; i < npad; i += CT_THREADS) {
        unsigned long long aw = 0ull;
        uint32_t bw = 0u;
        if (i < r) {
            const int32_t pg = page[row * r + i];
            int32_t dc = -1;
            if (doc) {
                dc = doc[row * r + i];
            } else {
                const int64_t p = (int64_t)pg - (int64_t)idx_base;
                if (p >= 0 && p < np) dc = doc_of_page[p];                          // outside: a hole that never becomes an address
            }
            const uint32_t key = order_key(scores[row * row_stride + i]);
            if (dc >= 0 && key != KEY_NINF) {
                aw = ((unsigned long long)(~(uint32_t)dc) << 32) | key;
                bw = ~(uint32_t)pg;
            }
        }
        a[i] = aw;
        b[i] = bw;
    }
    __syncthreads();

    auto sort_desc = [&]() {
        for (int size = 2; size <= npad; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < npad / 2; t += CT_THREADS) {
                    const int lo = 2 * t - (t & (stride - 1));
                    const int hi = lo + stride;
                    const bool desc = ((lo & size) == 0);
                    const unsigned long long x = a[lo], y = a[hi];
                    const uint32_t px = b[lo], py = b[hi];
                    const bool less = x < y || (x == y && px < py);
                    if (less == desc) { a[lo] = y; a[hi] = x; b[lo] = py; b[hi] = px; }
                }
                __syncthreads();
            }
        }
    };
    sort_desc();                                         // document ascending, key descending, page ascending

    // the first record of a run of equal documents is the document's winner: (key, ~document, ~page); everything else -> zero
    uint32_t win = 0u;                                   // bit j: record tid + j * CT_THREADS (npad / CT_THREADS <= 16 of them)
    for (int i = tid, j = 0; i < npad; i += CT_THREADS, ++j) {
        const unsigned long long x = a[i];
        if (x != 0ull && (i == 0 || (uint32_t)(a[i - 1] >> 32) != (uint32_t)(x >> 32))) win |= 1u << j;
    }
    __syncthreads();
    for (int i = tid, j = 0; i < npad; i += CT_THREADS, ++j) {
        const unsigned long long x = a[i];
        const bool w = (win >> j) & 1u;
        a[i] = w ? ((x << 32) | (x >> 32)) : 0ull;
        if (!w) b[i] = 0u;
    }
    __syncthreads();
    sort_desc();                                         // key descending, document ascending

    for (int j = tid; j < k; j += CT_THREADS) {
        const unsigned long long x = a[j];
        const bool real = x != 0ull;                     // a winner's key is above KEY_NINF > 0
        top_scores[row * k + j] = real ? key_to_float((uint32_t)(x >> 32)) : -__builtin_inff();
        top_doc[row * k + j] = real ? (int32_t)(~(uint32_t)x) : -1;
        top_page[row * k + j] = real ? (int32_t)(~b[j]) : -1;
    }
}

// evdr_doc_topk's last step: top_doc holds evdr_topk's columns (document ids, -1 padding); absent documents (-inf) become padding
__global__ void __launch_bounds__(256) doc_finish_kernel(const float* __restrict__ top_scores, int32_t* __restrict__ top_doc,
                                                        int32_t* __restrict__ top_page, const int32_t* __restrict__ doc_best,
                                                        int64_t n_docs, int k, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int32_t dc = top_doc[i];
    const bool real = dc >= 0 && dc < n_docs && order_key(top_scores[i]) != KEY_NINF;
    top_page[i] = real ? doc_best[(i / k) * n_docs + dc] : -1;
    if (!real) top_doc[i] = -1;
}

}  // namespace

hipError_t evdr_launch_doc_max(const float* scores, const int32_t* members, const int32_t* offsets, const int32_t* idx_map, int64_t nq,
                               int64_t n, int64_t row_stride, int64_t nm, int64_t n_docs, int32_t idx_base, float* doc_scores,
                               int64_t doc_stride, int32_t* doc_best, hipStream_t stream) {
    if (nq == 0 || n_docs == 0) return hipSuccess;
    const int64_t ndb = (n_docs + EVDR_DOC_BLOCK - 1) / EVDR_DOC_BLOCK, nrb = (nq + EVDR_DOC_ROWS - 1) / EVDR_DOC_ROWS;
    hipLaunchKernelGGL(doc_max_kernel, dim3((unsigned)(ndb * nrb)), dim3(DM_THREADS), 0, stream, scores, members, offsets, idx_map, nq, n,
                       row_stride, nm, n_docs, idx_base, ndb, doc_scores, doc_stride, doc_best);
    return hipGetLastError();
}

hipError_t evdr_launch_collapse_topk(const float* scores, const int32_t* page, const int32_t* doc, const int32_t* doc_of_page, int64_t np,
                                     int32_t idx_base, int64_t nq, int r, int64_t row_stride, int k, float* top_scores,
                                     int32_t* top_doc, int32_t* top_page, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    int npad = 2;
    while (npad < r || npad < k) npad <<= 1;             // <= EVDR_SELECT_MAX: r and k are (both are powers of two at their limits)
    hipLaunchKernelGGL(collapse_topk_kernel, dim3((unsigned)nq), dim3(CT_THREADS), 0, stream, scores, page, doc, doc_of_page, np,
                       idx_base, r, npad, row_stride, k, top_scores, top_doc, top_page);
    return hipGetLastError();
}

hipError_t evdr_launch_doc_finish(const float* top_scores, int32_t* top_doc, int32_t* top_page, const int32_t* doc_best, int64_t nq,
                                  int64_t n_docs, int k, hipStream_t stream) {
    const int64_t total = nq * k;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(doc_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, top_scores, top_doc, top_page,
                       doc_best, n_docs, k, total);
    return hipGetLastError();
}
