// Candidate scoring and top-R selection (include/evdr.h "candidate scoring").
//
// evdr_maxsim_fwd_candidates scores query q against the pages its own list names.  The scoring launch is the GATHER instance of
// maxsim_fwd16s_kernel (maxsim_fwd16.hip), which walks a COMPACTED list of corpus pages with a device-side count per query.  The two
// kernels here sit on either side of it:
//   cand_compact_kernel   (nq, r) lists with holes -> compacted local page numbers + their list positions + counts; writes -inf
//                         into the holes of the output and, if asked, the cleaned lists (holes = -1)
//   cand_scatter_kernel   the rerank's scores (compacted order) back to their list positions
// A hole is any entry outside [idx_base, idx_base + np): it is never turned into an address.
//
// evdr_select_topr: per row of an (nq, n) fp32 block the r columns with the largest order key (evdr_topk's key: NaN first, -0 == +0),
// ties at the cut towards the lower index, written in ASCENDING index order.  One 256-thread workgroup per row: the radix select of
// csrc/topk.hip (11 + 11 + 10 bits) finds the r-th key and how many of its equals belong to the set, then an ordered compaction writes
// the set: each wave owns a contiguous quarter of the row, counts its members first, and walks the quarter a second time with
// ballot / popcount offsets -- no barrier inside the walk.
#include "evdr_common.h"

namespace {

constexpr int CD_THREADS = 256;

__global__ void __launch_bounds__(CD_THREADS) cand_compact_kernel(const int32_t* __restrict__ cand, int r, int32_t idx_base, int64_t np,
                                                                  int32_t* __restrict__ glist, int32_t* __restrict__ gpos,
                                                                  int32_t* __restrict__ gcount, float* __restrict__ out, int64_t out_stride,
                                                                  int32_t* __restrict__ clean) {
    __shared__ uint32_t wave_cnt[CD_THREADS / 64];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* row = cand + q * r;
    int32_t* g = glist + q * r;
    int32_t* gp = gpos + q * r;
    uint32_t base = 0;
    for (int i0 = 0; i0 < r; i0 += CD_THREADS) {
        const int i = i0 + tid;
        const int32_t c = i < r ? row[i] : -1;
        const int64_t local = (int64_t)c - (int64_t)idx_base;
        const bool m = i < r && local >= 0 && local < np;
        if (i < r) {
            if (!m) out[q * out_stride + i] = -__builtin_inff();
            if (clean != nullptr) clean[q * r + i] = m ? c : -1;
        }
        const unsigned long long bal = __ballot(m);
        const uint32_t before = (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
        __syncthreads();                                 // wave_cnt of the previous round has been read
        if (lane == 0) wave_cnt[wave] = (uint32_t)__builtin_popcountll(bal);
        __syncthreads();
        uint32_t off = base, round = 0;
        for (int w = 0; w < CD_THREADS / 64; ++w) {
            const uint32_t v = wave_cnt[w];
            if (w < wave) off += v;
            round += v;
        }
        if (m) {
            g[off + before] = (int32_t)local;
            gp[off + before] = i;
        }
        base += round;
    }
    if (tid == 0) gcount[q] = (int32_t)base;
}

__global__ void __launch_bounds__(CD_THREADS) cand_scatter_kernel(const float* __restrict__ tmp, const int32_t* __restrict__ gpos,
                                                                  const int32_t* __restrict__ gcount, int r, float* __restrict__ out,
                                                                  int64_t out_stride) {
    const int64_t q = blockIdx.x;
    const int n = min(gcount[q], r);
    for (int j = threadIdx.x; j < n; j += CD_THREADS) out[q * out_stride + gpos[q * r + j]] = tmp[q * r + j];
}

// ---- top-R selection ---------------------------------------------------------------------------------------------------------
constexpr int SR_THREADS = 256;
constexpr int SR_BINS = 2048;
constexpr int SR_BPT = SR_BINS / SR_THREADS;

__device__ __forceinline__ uint32_t order_key(float f) {          // csrc/topk.hip's key
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(SR_THREADS) select_topr_kernel(const float* __restrict__ scores, int64_t n, int64_t row_stride,
                                                                 int32_t idx_base, int r, int32_t* __restrict__ out) {
    __shared__ uint32_t hist[SR_BINS];
    __shared__ uint32_t suf[SR_THREADS + 1];
    __shared__ uint32_t sh_prefix, sh_need;
    __shared__ uint32_t wgt[SR_THREADS / 64], weq[SR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = scores + (int64_t)blockIdx.x * row_stride;
    int32_t* o = out + (int64_t)blockIdx.x * r;
    if (n <= r) {                                        // the whole row, then holes
        for (int i = tid; i < r; i += SR_THREADS) o[i] = i < n ? (int32_t)i + idx_base : -1;
        return;
    }
    if (tid == 0) { sh_prefix = 0; sh_need = (uint32_t)r; }
    __syncthreads();
    // ---- the r-th largest key T, and how many elements == T belong to the set (radix select, most significant digit first)
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = (pass == 0) ? 21 : (pass == 1 ? 10 : 0);
        const int bits = (pass == 2) ? 10 : 11;
        const uint32_t dmask = (1u << bits) - 1u;
#pragma unroll
        for (int b = 0; b < SR_BPT; ++b) hist[tid * SR_BPT + b] = 0;
        __syncthreads();
        const uint32_t prefix = sh_prefix;
        const uint32_t himask = (pass == 0) ? 0u : (0xFFFFFFFFu << (shift + bits));
        // every thread runs the same number of rounds (wave-level votes below); four loads in flight per thread and round
        for (int64_t i0 = 0; i0 < n; i0 += 4 * SR_THREADS) {
            float f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = i0 + u * SR_THREADS + tid;
                f[u] = i < n ? row[i] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = i0 + u * SR_THREADS + tid;
                const uint32_t key = order_key(f[u]);
                const uint32_t d = (key >> shift) & dmask;
                bool mine = i < n && ((key & himask) == prefix);
                if (pass == 0) {
                    // the first digit (sign, exponent, two mantissa bits) is the same for almost every score of a row: count the few
                    // distinct digits per wave, one atomic each (as csrc/topk.hip); what is left after 3 rounds goes one by one
                    unsigned long long todo = __ballot(mine);
                    for (int it = 0; it < 3 && todo != 0ull; ++it) {
                        const int leader = __ffsll((long long)todo) - 1;
                        const uint32_t dl = (uint32_t)__builtin_amdgcn_readlane((int)d, leader);
                        const unsigned long long same = __ballot(mine && d == dl);
                        if (lane == leader) atomicAdd(&hist[dl], (uint32_t)__popcll(same));
                        todo &= ~same;
                        mine = mine && d != dl;
                    }
                }
                if (mine) atomicAdd(&hist[d], 1u);
            }
        }
        __syncthreads();
        uint32_t own = 0;
#pragma unroll
        for (int b = 0; b < SR_BPT; ++b) own += hist[tid * SR_BPT + b];
        suf[tid] = own;                                  // -> suf[t] = count of digits >= SR_BPT * t
        if (tid == 0) suf[SR_THREADS] = 0;
        __syncthreads();
        for (int off = 1; off < SR_THREADS; off <<= 1) {
            const uint32_t add = (tid + off < SR_THREADS) ? suf[tid + off] : 0u;
            __syncthreads();
            suf[tid] += add;
            __syncthreads();
        }
        const uint32_t need = sh_need;
        if (suf[tid] >= need && suf[tid + 1] < need) {    // exactly one thread: the wanted digit is one of its bins
            uint32_t above = suf[tid + 1];
            for (int b = SR_BPT - 1; b >= 0; --b) {
                const uint32_t cnt = hist[tid * SR_BPT + b];
                if (above + cnt >= need) {
                    sh_prefix = prefix | ((uint32_t)(tid * SR_BPT + b) << shift);
                    sh_need = need - above;
                    break;
                }
                above += cnt;
            }
        }
        __syncthreads();
    }
    const uint32_t T = sh_prefix;
    const uint32_t need_eq = sh_need;                    // the first need_eq elements == T in index order are in
    // ---- ordered compaction: wave w owns columns [w * seg, (w + 1) * seg)
    const int64_t seg = ((n + SR_THREADS - 1) / SR_THREADS) * 64;
    const int64_t lo = min(n, (int64_t)wave * seg), hi = min(n, lo + seg);
    uint32_t cgt = 0, ceq = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) {
        const uint32_t key = order_key(row[i]);
        cgt += key > T ? 1u : 0u;
        ceq += key == T ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) { cgt += __shfl_xor(cgt, off); ceq += __shfl_xor(ceq, off); }
    if (lane == 0) { wgt[wave] = cgt; weq[wave] = ceq; }
    __syncthreads();
    uint32_t bgt = 0, beq = 0;
    for (int w = 0; w < wave; ++w) { bgt += wgt[w]; beq += weq[w]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        const uint32_t key = i < hi ? order_key(row[i]) : 0u;
        const bool gt = i < hi && key > T, eq = i < hi && key == T;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        const uint32_t gb = bgt + (uint32_t)__builtin_popcountll(bg & below);
        const uint32_t eb = beq + (uint32_t)__builtin_popcountll(be & below);
        if (gt || (eq && eb < need_eq)) {
            const uint32_t pos = gb + min(eb, need_eq);  // members in front of this one: < r by construction
            if (pos < (uint32_t)r) o[pos] = (int32_t)i + idx_base;
        }
        bgt += (uint32_t)__builtin_popcountll(bg);
        beq += (uint32_t)__builtin_popcountll(be);
    }
}

}  // namespace

hipError_t evdr_launch_cand_compact(const int32_t* cand, int64_t nq, int r, int32_t idx_base, int64_t np, int32_t* glist, int32_t* gpos,
                                    int32_t* gcount, float* out, int64_t out_stride, int32_t* cand_clean, hipStream_t stream) {
    hipLaunchKernelGGL(cand_compact_kernel, dim3((unsigned)nq), dim3(CD_THREADS), 0, stream, cand, r, idx_base, np, glist, gpos, gcount,
                       out, out_stride, cand_clean);
    return hipGetLastError();
}

hipError_t evdr_launch_cand_scatter(const float* tmp, const int32_t* gpos, const int32_t* gcount, int64_t nq, int r, float* out,
                                    int64_t out_stride, hipStream_t stream) {
    hipLaunchKernelGGL(cand_scatter_kernel, dim3((unsigned)nq), dim3(CD_THREADS), 0, stream, tmp, gpos, gcount, r, out, out_stride);
    return hipGetLastError();
}

hipError_t evdr_launch_select_topr(const float* scores, int64_t nq, int64_t n, int64_t row_stride, int32_t idx_base, int r,
                                   int32_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(select_topr_kernel, dim3((unsigned)nq), dim3(SR_THREADS), 0, stream, scores, n, row_stride, idx_base, r, out);
    return hipGetLastError();
}
