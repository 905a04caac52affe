// Exact two-stage top-k on an fp32 corpus (fp16 hi/lo planes): bounds, candidate selection and the merge of
// evdr_maxsim_topk_prefilter (include/evdr.h).  The scoring launches themselves are instances of maxsim_fwd16s_kernel
// (maxsim_fwd16.hip): the coarse pass (hi plane only) and the gathered exact rerank.
//
// The rule ("Prefiltered fp32 top-k").  Per query q: s~_p = coarse score (hi . hi only), s_p = exact score, E_q a
// bound with |s_p - s~_p| <= E_q for every page whose scores are not NaN, t~_q the k-th coarse score in top-k order.  Then
//     C_q = { p : s~_p >= t~_q - 2 E_q }  u  { p : s~_p is NaN }
// holds the exhaustive exact top-k, ties included: the k coarse leaders have s >= t~ - E, so the k-th exact score T >= t~ - E, and every
// page with s >= T has s~ >= T - E >= t~ - 2 E.  NaN scores come from page flags and query tokens only and are NaN in both passes.
// A query whose t~ or E is not finite, or whose |C_q| exceeds the capacity, is scored exhaustively instead (the fallback list).
//
// The bound, in the scaled units of the planes (x * 2^k; scores come back by the exact factor 2^-(kq + kp)).  Per (token t, patch j):
//   exact  = fl( sum of 384 products q_lo.p_hi, q_hi.p_lo, q_hi.p_hi )   coarse = fl( sum of 128 products q_hi.p_hi )
// fp16 x fp16 products are exact in fp32; each chain is taken to round at most once per product added (the MFMA's internal order
// is not documented), so |chain - exact sum| <= g_n * sum |terms|, g_n = n u / (1 - n u), u = 2^-24.  With a = |q_hi,t|,
// b = |q_lo,t|, H = max_j |p_hi,j|, L = max_j |p_lo,j| over the VALID patches of non-NaN pages (Cauchy-Schwarz):
//   |exact - coarse| <= a L + b H + g_384 (a H + a L + b H) + g_128 a H                      =: e_t
//   |exact|, |coarse| <= (1 + g_384) (a H + a L + b H)                                       =: n_t
// The max over patches is 1-Lipschitz and the -1e4 of masked patches joins both maxima identically, so e_t carries through it;
// |max| <= n_t as well (the -1e4 wins only when every valid product is below -1e4, i.e. n_t > 1e4).  Masked tokens add exact zeros
// in both passes.  The fp32 sum over the 32 token lanes rounds at most 31 times in each pass:
//   E_q = 2^-(kq + kp) * ( sum_t e_t + 2 g_31 sum_t n_t ) + 1e-37          (the last term: fp32 underflow of the rescaled maxima)
// Norms are sums of squares of fp16 values in fp64 (exact), square roots rounded up; E_q is evaluated in fp64 and rounded up to
// fp32; the threshold t~ - 2 E is formed in fp64 and lowered by a relative 2^-50.
#include "evdr_common.h"

namespace {

constexpr double kU = 1.0 / 16777216.0;                 // fp32 unit roundoff 2^-24
__device__ __forceinline__ double gam(int n) { return n * kU / (1.0 - n * kU); }

__device__ __forceinline__ bool nan_bits(float f) { return (__builtin_bit_cast(uint32_t, f) & 0x7FFFFFFFu) > 0x7F800000u; }
__device__ __forceinline__ bool finite_bits(float f) { return (__builtin_bit_cast(uint32_t, f) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool finite_d(double d) {
    return (__builtin_bit_cast(uint64_t, d) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// fp64 -> fp32, rounded toward +inf (non-negative inputs; NaN / Inf stay what they are)
__device__ __forceinline__ float up_f32(double d) {
    if (!finite_d(d)) return (float)d;
    float f = (float)d;
    if ((double)f < d) f = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + 1u);
    return f;
}

// square root of a sum of squares, upward: the fp64 sqrt is within one ulp, a relative 2^-50 covers it
__device__ __forceinline__ double norm_up(double ss) { return __builtin_sqrt(ss) * (1.0 + 0x1p-50); }

__device__ __forceinline__ double sq16(uint16_t h) {
    const double v = (double)__builtin_bit_cast(_Float16, h);
    return v * v;
}

// ---- corpus: H = max |p_hi,j|, L = max |p_lo,j| over valid patches of pages without a non-finite flag ---------------------
__global__ void bound_init_kernel(uint32_t* hl) {
    if (threadIdx.x < 2) hl[threadIdx.x] = 0u;
}

// 16 lanes per patch row (8 dims of each plane per lane), grid-stride over the np * lp rows
__global__ void __launch_bounds__(256) corpus_bound_kernel(const uint16_t* __restrict__ P, int64_t np, int64_t lp, int64_t p_stride,
                                                           int64_t p_plane_stride, const uint32_t* __restrict__ tilemask,
                                                           const uint32_t* __restrict__ pageflags, uint32_t* hl) {
    const int sub = threadIdx.x & 15;
    const int64_t rows = np * lp;
    const int64_t ntiles = (lp + EVDR_TILE_PATCHES - 1) / EVDR_TILE_PATCHES;
    float hmax = 0.f, lmax = 0.f;                       // non-negative: the bit patterns order like the values
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; r < rows; r += ((int64_t)gridDim.x * blockDim.x) >> 4) {
        const int64_t page = r / lp, m = r - page * lp;
        const bool valid = ((tilemask[page * ntiles + (m >> 5)] >> (m & 31)) & 1u) && !(pageflags[page] & 8u);
        if (!valid) continue;                           // (uniform over the 16 lanes of the row)
        const uint16_t* h = P + page * p_stride + m * EVDR_D + sub * 8;
        const uint16_t* l = h + p_plane_stride;
        double sh = 0.0, sl = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) { sh += sq16(h[i]); sl += sq16(l[i]); }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) { sh += __shfl_xor(sh, off, 16); sl += __shfl_xor(sl, off, 16); }
        hmax = __builtin_fmaxf(hmax, up_f32(norm_up(sh)));
        lmax = __builtin_fmaxf(lmax, up_f32(norm_up(sl)));
    }
    for (int off = 32; off > 0; off >>= 1) {
        hmax = __builtin_fmaxf(hmax, __shfl_xor(hmax, off));
        lmax = __builtin_fmaxf(lmax, __shfl_xor(lmax, off));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(hl, __builtin_bit_cast(uint32_t, hmax));
        atomicMax(hl + 1, __builtin_bit_cast(uint32_t, lmax));
    }
}

// ---- per query: E_q in real units ---------------------------------------------------------------------------------------------
// 32 lanes per query (lane = token), 8 queries per 256-thread workgroup.  Also zeroes the fallback count of the call.
__global__ void __launch_bounds__(256) query_bound_kernel(const uint16_t* __restrict__ Q, const uint8_t* __restrict__ qmask, int64_t nq,
                                                          int64_t lq, const uint32_t* q_amax, const uint32_t* p_amax,
                                                          const float* __restrict__ bound, float* __restrict__ eq, int32_t* fcount) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && fcount != nullptr) *fcount = 0;
    const int t = threadIdx.x & 31;
    const int64_t q = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    double e = 0.0, n = 0.0;
    if (q < nq && t < lq && (qmask == nullptr || qmask[q * lq + t] != 0)) {
        const uint16_t* h = Q + (q * lq + t) * EVDR_D;
        const uint16_t* l = h + nq * lq * EVDR_D;
        double sh = 0.0, sl = 0.0;
        for (int i = 0; i < EVDR_D; ++i) { sh += sq16(h[i]); sl += sq16(l[i]); }
        const double a = norm_up(sh), b = norm_up(sl);
        const double H = bound[0], L = bound[1];
        const double cross = a * H + a * L + b * H;
        e = a * L + b * H + gam(384) * cross + gam(128) * a * H;
        n = (1.0 + gam(384)) * cross;
    }
    for (int off = 16; off > 0; off >>= 1) { e += __shfl_xor(e, off, 32); n += __shfl_xor(n, off, 32); }
    if (q < nq && t == 0) {
        const int kq = q_amax ? evdr_h2_shift(*q_amax) : 0;
        const int kp = p_amax ? evdr_h2_shift(*p_amax) : 0;
        const double inv = __builtin_ldexp(1.0, -(kq + kp));
        eq[q] = up_f32((inv * (e + 2.0 * gam(31) * n) + 1e-37) * (1.0 + 0x1p-40));
    }
}

// ---- per query: candidate list (ascending page order), count, fallback list ------------------------------------------------
constexpr int SEL_THREADS = 256;

__global__ void __launch_bounds__(SEL_THREADS) select_kernel(const float* __restrict__ coarse, int64_t np, const float* __restrict__ topv,
                                                             int kc, const float* __restrict__ eq, int cap, int32_t* __restrict__ gather,
                                                             int32_t* __restrict__ gcount, float* __restrict__ cand,
                                                             int32_t* __restrict__ fb, int32_t* __restrict__ flist, int32_t* fcount,
                                                             int32_t* __restrict__ stats) {
    __shared__ uint32_t wave_cnt[SEL_THREADS / 64];
    __shared__ uint32_t sh_total;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = coarse + q * np;
    const float tau = topv[q * kc + kc - 1];
    const float E = eq[q];
    const bool ok = finite_bits(tau) && finite_bits(E);
    double thr = (double)tau - 2.0 * (double)E;
    thr -= __builtin_fabs(thr) * 0x1p-50 + 1e-300;
    auto is_cand = [&](float s) { return nan_bits(s) || (double)s >= thr; };

    uint32_t cnt = 0;
    if (ok)
        for (int64_t i = tid; i < np; i += SEL_THREADS) cnt += is_cand(row[i]) ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) wave_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < SEL_THREADS / 64; ++w) tot += wave_cnt[w];
        sh_total = tot;
    }
    __syncthreads();
    const uint32_t total = sh_total;
    const bool fallback = !ok || total > (uint32_t)cap;
    int32_t* g = gather + q * cap;
    float* c = cand + q * cap;
    if (tid == 0) {
        gcount[q] = fallback ? 0 : (int32_t)total;
        fb[q] = fallback ? 1 : 0;
        if (stats != nullptr) stats[q] = ok ? (int32_t)min(total, (uint32_t)INT32_MAX) : -1;
        if (fallback) flist[atomicAdd(fcount, 1)] = (int32_t)q;
    }
    const int64_t filled = fallback ? 0 : total;
    // unused list positions: never scored, never selected ahead of a real score
    for (int64_t i = filled + tid; i < cap; i += SEL_THREADS) {
        g[i] = -1;
        c[i] = -__builtin_inff();
    }
    if (fallback) return;
    // ordered compaction, 256 pages per round
    uint32_t base = 0;
    for (int64_t i0 = 0; i0 < np; i0 += SEL_THREADS) {
        const int64_t i = i0 + tid;
        const bool m = i < np && is_cand(row[i]);
        const unsigned long long bal = __ballot(m);
        const uint32_t before = (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
        __syncthreads();                                 // wave_cnt of the previous round has been read
        if (lane == 0) wave_cnt[wave] = (uint32_t)__builtin_popcountll(bal);
        __syncthreads();
        uint32_t off = base, round = 0;
        for (int w = 0; w < SEL_THREADS / 64; ++w) {
            const uint32_t v = wave_cnt[w];
            if (w < wave) off += v;
            round += v;
        }
        if (m) g[off + before] = (int32_t)i;
        base += round;
    }
}

// ---- per query: the rerank's top-k or the fallback's, by row -------------------------------------------------------------------
__global__ void merge_kernel(const float* __restrict__ rs, const int32_t* __restrict__ ri, const float* __restrict__ fs,
                             const int32_t* __restrict__ fi, const int32_t* __restrict__ fb, int64_t nq, int k, int32_t idx_base,
                             const int32_t* fcount, float* __restrict__ top_scores, int32_t* __restrict__ top_idx, int32_t* stats) {
    const int64_t q = blockIdx.x;
    const bool f = fb[q] != 0;
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        const int64_t o = q * k + i;
        if (f) {
            top_scores[o] = fs[o];
            top_idx[o] = fi[o];
        } else {
            top_scores[o] = rs[o];
            top_idx[o] = ri[o] < 0 ? -1 : ri[o] + idx_base;
        }
    }
    if (q == 0 && threadIdx.x == 0 && stats != nullptr) stats[nq] = *fcount;
}

}  // namespace

hipError_t evdr_launch_prefilter_corpus_bound(const uint16_t* P, int64_t np, int64_t lp, int64_t p_stride, int64_t p_plane_stride,
                                              const uint32_t* tilemask, const uint32_t* pageflags, float* bound, hipStream_t stream) {
    hipLaunchKernelGGL(bound_init_kernel, dim3(1), dim3(64), 0, stream, (uint32_t*)bound);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int64_t rows = np * lp;
    if (rows == 0) return hipSuccess;
    int64_t blocks = (rows + 15) / 16;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(corpus_bound_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, P, np, lp, p_stride, p_plane_stride, tilemask,
                       pageflags, (uint32_t*)bound);
    return hipGetLastError();
}

hipError_t evdr_launch_prefilter_query_bound(const uint16_t* Q, const uint8_t* qmask, int64_t nq, int64_t lq, const uint32_t* q_amax,
                                             const uint32_t* p_amax, const float* bound, float* eq, int32_t* fcount, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(query_bound_kernel, dim3((unsigned)((nq + 7) / 8)), dim3(256), 0, stream, Q, qmask, nq, lq, q_amax, p_amax, bound,
                       eq, fcount);
    return hipGetLastError();
}

hipError_t evdr_launch_prefilter_select(const float* coarse, int64_t nq, int64_t np, const float* topv, int kc, const float* eq, int cap,
                                        int32_t* gather, int32_t* gcount, float* cand, int32_t* fb, int32_t* flist, int32_t* fcount,
                                        int32_t* stats, hipStream_t stream) {
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)nq), dim3(SEL_THREADS), 0, stream, coarse, np, topv, kc, eq, cap, gather, gcount, cand,
                       fb, flist, fcount, stats);
    return hipGetLastError();
}

hipError_t evdr_launch_prefilter_merge(const float* rs, const int32_t* ri, const float* fs, const int32_t* fi, const int32_t* fb, int64_t nq,
                                       int k, int32_t idx_base, const int32_t* fcount, float* top_scores, int32_t* top_idx, int32_t* stats,
                                       hipStream_t stream) {
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)nq), dim3(128), 0, stream, rs, ri, fs, fi, fb, nq, k, idx_base, fcount, top_scores,
                       top_idx, stats);
    return hipGetLastError();
}
