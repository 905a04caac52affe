// Token alignment (include/evdr.h "token alignment"): for query q and the pages ITS list names, the best patch of every
// query token (value and first index) and, if asked, the page's heat map (per patch, the best valid query token).
//
// One workgroup of four waves per (query, list position).  The query's <= 32 token rows are resident as the MFMA A operand (two
// 16-row blocks x four k-steps of 32 columns, per plane); the page is walked in tiles of 16 patches, wave w taking tiles w, w + 4, ...,
// whose rows go straight from global memory into the B operand with one 16-byte load per lane, plane and k-step: every patch is read
// once per pair, there is nothing to share through LDS.  Fragment maps of v_mfma_f32_16x16x32 (cdna_hip_programming.md §3), lane l,
// c = l & 15, g = l >> 4:
//   A[row c][k = 8g + j]   = token (16t + c) of the query, dims 32s + 8g + j     (t = token block, s = k-step)
//   B[k = 8g + j][col c]   = patch (16T + c) of the page, dims 32s + 8g + j      (T = tile)
//   C/D[row 4g + reg][col c] -> the lane holds, for patch 16T + c, the tokens 16t + 4g + reg, reg = 0..3
// so a lane owns ONE patch of a tile and eight tokens.  Per tile: the tile-mask bit of the lane's patch decides whether its eight
// products may replace the lane's running (max, index) pairs -- tiles ascend, so a strict > keeps the first index --, and the column
// maximum over the valid tokens (registers, then the four lane groups) is the patch's heat value, stored by the wave that owns the
// tile.  After the walk the eight pairs are reduced over the 16 lanes of a row group, then over the four waves through 1 KiB of LDS;
// ties go to the lower patch index at every level.  Products of one (token, patch) pair are chained in ONE order -- planes lo x hi,
// hi x lo, hi x hi (page x query; a bf16 corpus has the one product), k-steps ascending inside each -- whatever the tile, the wave or
// the outputs asked for.  No atomics, no workspace, plain stores: the same bits launch after launch.
#include <type_traits>

#include "evdr_common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4v;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4v;

namespace {

constexpr int AL_WAVES = 4;
constexpr int AL_THREADS = AL_WAVES * 64;

struct AlignParams {
    const uint16_t* Q;          // (nplanes, nq, lq, 128) dense
    int64_t q_plane_stride;
    const uint16_t* P;          // nplanes slabs of (np, lp, 128), p_stride elements between pages
    int64_t p_stride, p_plane_stride;
    const uint32_t* q_amax;     // fp16 hi/lo planes: absmax words (null = unscaled)
    const uint32_t* p_amax;
    const uint8_t* qmask;       // (nq, lq) or null
    const uint32_t* tilemask;   // (np, ceil(lp / 32))
    const uint32_t* pageflags;  // (np)
    const int32_t* cand;        // (nq, r) GLOBAL page indices
    int32_t idx_base;
    int r, lq, lp;
    int64_t np;
    float* sim;                 // (nq, r, lq)
    int32_t* patch;             // (nq, r, lq)
    float* heat;                // (nq, r, lp) or null
};

__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

__device__ __forceinline__ float opaque_nan() {
    float v = __builtin_bit_cast(float, 0x7FC00000u);
    asm volatile("" : "+v"(v));                        // the optimiser must not reason about it (-fno-honor-nans)
    return v;
}

__device__ __forceinline__ f32x4v mfma16(const bf16x8& a, const bf16x8& b, const f32x4v& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4v mfma16(const f16x8& a, const f16x8& b, const f32x4v& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// exponent field all ones in any 16-bit element (maxsim_fwd16.hip: frag_exp_carry); integer only
template <typename F>
__device__ __forceinline__ uint32_t exp_carry(const F& v) {
    constexpr uint32_t M = std::is_same<F, bf16x8>::value ? 0x7F807F80u : 0x7C007C00u;
    constexpr uint32_t U = std::is_same<F, bf16x8>::value ? 0x00800080u : 0x04000400u;
    const u32x4v w = __builtin_bit_cast(u32x4v, v);
    return ((w[0] & M) + U) | ((w[1] & M) + U) | ((w[2] & M) + U) | ((w[3] & M) + U);
}

// every output of a pair that is not walked: sim / patch of the valid and of the masked tokens, one value for the whole heat row
__device__ __forceinline__ void fill_pair(const AlignParams& p, int64_t pair, uint32_t qvalid, float sim_valid, float heat_all) {
    const int tid = threadIdx.x;
    if (tid < p.lq) {
        p.sim[pair * p.lq + tid] = ((qvalid >> tid) & 1u) ? sim_valid : 0.f;
        p.patch[pair * p.lq + tid] = -1;
    }
    if (p.heat != nullptr)
        for (int m = tid; m < p.lp; m += AL_THREADS) p.heat[pair * p.lp + m] = heat_all;
}

template <int NPL>
__global__ void __launch_bounds__(AL_THREADS) align_kernel(const AlignParams p) {
    using frag = typename std::conditional<NPL == 2, f16x8, bf16x8>::type;
    // plane products (page plane, query plane), smaller magnitude first: the forward's order
    constexpr int NPROD = NPL == 1 ? 1 : 3;
    constexpr int PP[3] = {NPL - 1, 0, 0};
    constexpr int PQ[3] = {0, NPL - 1, 0};
    __shared__ float s_val[AL_WAVES][32];
    __shared__ int s_idx[AL_WAVES][32];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int64_t pair = blockIdx.x;                    // = q * r + i
    const int64_t q = pair / p.r;

    // ---- the list entry: a hole never becomes an address
    const int64_t local = (int64_t)p.cand[pair] - (int64_t)p.idx_base;
    if (local < 0 || local >= p.np) {
        if (tid < p.lq) {
            p.sim[pair * p.lq + tid] = neg_inf();
            p.patch[pair * p.lq + tid] = -1;
        }
        if (p.heat != nullptr)
            for (int m = tid; m < p.lp; m += AL_THREADS) p.heat[pair * p.lp + m] = neg_inf();
        return;
    }
    const uint32_t pf = p.pageflags[local];

    // ---- the query: valid-token word, fragments, non-finite tokens (all wave-uniform in the end)
    uint32_t qvalid;
    {
        const bool v = lane < p.lq && (p.qmask == nullptr || p.qmask[q * p.lq + lane] != 0);
        qvalid = (uint32_t)__ballot(v);
    }
    frag aq[NPL][2][4];
    const bool two_blocks = p.lq > 16;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = 16 * t + c;
            const uint16_t* src = p.Q + (int64_t)pl * p.q_plane_stride + (q * p.lq + min(row, p.lq - 1)) * EVDR_D + 8 * g;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                frag v = *reinterpret_cast<const frag*>(src + 32 * s);
                if (row >= p.lq) v = frag{0, 0, 0, 0, 0, 0, 0, 0};
                aq[pl][t][s] = v;
            }
        }
    bool qbad;
    {
        uint32_t carry = 0u;                            // the hi plane: NaN and Inf survive the split there
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < 4; ++s) carry |= exp_carry(aq[0][t][s]);
        qbad = __ballot((carry & 0x80008000u) != 0u) != 0ull;
    }

    // ---- pairs that are not walked (the forward's rules, in its order)
    if (!(pf & 1u) || qvalid == 0u) {                   // no valid patch: the exact 0; no valid token: nothing to align
        const bool nan_pair = (pf & 1u) && ((pf & 8u) || qbad);
        fill_pair(p, pair, qvalid, 0.f, nan_pair ? opaque_nan() : neg_inf());
        return;
    }
    if ((pf & 8u) || qbad) {                            // a pair the forward scores NaN
        const float nan = opaque_nan();
        fill_pair(p, pair, qvalid, nan, nan);
        return;
    }

    // fp16 planes carry x * 2^k: one exact power of two brings a product sum back.  It is applied to the sum with ldexpf, not as a
    // factor: 2^-(kq + kp) itself is subnormal from kq + kp = 127 on and 0 from 150 on (both absmax below 2^-60, say), where the
    // products are still ordinary fp32 numbers; away from underflow the two are the same operation, bit for bit
    int kback = 0;
    if constexpr (NPL == 2) {
        const int kq = p.q_amax ? evdr_h2_shift(*p.q_amax) : 0;
        const int kp = p.p_amax ? evdr_h2_shift(*p.p_amax) : 0;
        kback = -(kq + kp);
    }

    // ---- the walk
    const int ntiles = (p.lp + 15) >> 4;
    const int nwords = (p.lp + 31) >> 5;
    const uint16_t* page = p.P + local * p.p_stride + 8 * g;
    const uint32_t* words = p.tilemask + local * nwords;
    float* heat = p.heat != nullptr ? p.heat + pair * p.lp : nullptr;
    uint32_t tokbits[2];                                // the lane's tokens 16t + 4g + reg
#pragma unroll
    for (int t = 0; t < 2; ++t) tokbits[t] = (qvalid >> (16 * t + 4 * g)) & 0xFu;

    float best[2][4];
    int bidx[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) { best[t][reg] = neg_inf(); bidx[t][reg] = 0x7FFFFFFF; }

    auto load_tile = [&](frag (&b)[NPL][4], int T) {
        const int row = min(16 * T + c, p.lp - 1);      // rows behind the page end are clamped (and masked below)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                b[pl][s] = *reinterpret_cast<const frag*>(page + (int64_t)pl * p.p_plane_stride + (int64_t)row * EVDR_D + 32 * s);
    };
    auto tile_bits = [&](int T) -> uint32_t {           // wave-uniform: the 16 mask bits of tile T
        return (words[T >> 1] >> (16 * (T & 1))) & 0xFFFFu;
    };

    frag b[NPL][4];
    int T = wave;
    if (T < ntiles) load_tile(b, T);
    while (T < ntiles) {
        const int Tn = T + AL_WAVES;
        frag bn[NPL][4];
        if (Tn < ntiles) load_tile(bn, Tn);             // the next tile's rows are on their way while this one is multiplied
        const uint32_t bits = __builtin_amdgcn_readfirstlane(tile_bits(T));
        const int m = 16 * T + c;
        const bool pvalid = ((bits >> c) & 1u) != 0u && m < p.lp;
        float h = neg_inf();
        if (bits != 0u) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t == 1 && !two_blocks) break;
                f32x4v acc = {0, 0, 0, 0};
#pragma unroll
                for (int pr = 0; pr < NPROD; ++pr)
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = mfma16(aq[PQ[pr]][t][s], b[PP[pr]][s], acc);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const float v = NPL == 2 ? __builtin_ldexpf(acc[reg], kback) : acc[reg];
                    const bool take = pvalid && v > best[t][reg];
                    best[t][reg] = take ? v : best[t][reg];
                    bidx[t][reg] = take ? m : bidx[t][reg];
                    if ((tokbits[t] >> reg) & 1u) h = __builtin_fmaxf(h, v);
                }
            }
        }
        if (heat != nullptr) {
            // the four lane groups hold the same patch: group maximum, then one store per patch
            h = __builtin_fmaxf(h, __shfl_xor(h, 16));
            h = __builtin_fmaxf(h, __shfl_xor(h, 32));
            if (g == 0 && m < p.lp) heat[m] = pvalid ? h : neg_inf();
        }
        if (Tn < ntiles) {
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
                for (int s = 0; s < 4; ++s) b[pl][s] = bn[pl][s];
        }
        T = Tn;
    }

    // ---- (max, first index) over the 16 lanes of a row group, then over the waves
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float v = best[t][reg];
            int bi = bidx[t][reg];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const float ov = __shfl_xor(v, off);
                const int oi = __shfl_xor(bi, off);
                const bool tb = (ov > v) || (ov == v && oi < bi);
                v = tb ? ov : v;
                bi = tb ? oi : bi;
            }
            if (c == 0) {
                s_val[wave][16 * t + 4 * g + reg] = v;
                s_idx[wave][16 * t + 4 * g + reg] = bi;
            }
        }
    __syncthreads();
    if (tid < p.lq) {
        float v = s_val[0][tid];
        int bi = s_idx[0][tid];
#pragma unroll
        for (int w = 1; w < AL_WAVES; ++w) {
            const float ov = s_val[w][tid];
            const int oi = s_idx[w][tid];
            const bool tb = (ov > v) || (ov == v && oi < bi);
            v = tb ? ov : v;
            bi = tb ? oi : bi;
        }
        if (pf & 2u) {                                  // the masked patches' -1e4 takes part in the max, at its first index
            const int fm = (pf & 4u) ? (((pf >> 4) & 0xFFFu) > 0u ? 0 : (int)(pf >> 16)) : (int)(pf >> 16);
            const bool tb = (-1e4f > v) || (-1e4f == v && fm < bi);
            v = tb ? -1e4f : v;
            bi = tb ? fm : bi;
        }
        const bool tv = ((qvalid >> tid) & 1u) != 0u;
        p.sim[pair * p.lq + tid] = tv ? v : 0.f;
        p.patch[pair * p.lq + tid] = tv ? bi : -1;
    }
}

}  // namespace

hipError_t evdr_launch_maxsim_align(const uint16_t* Q, const uint16_t* P, const uint8_t* qmask, const uint32_t* tilemask,
                                    const uint32_t* pageflags, const int32_t* cand, int r, int32_t idx_base, float* sim, int32_t* patch,
                                    float* heat, int64_t nq, int lq, int64_t np, int lp, int nplanes, int64_t p_stride,
                                    int64_t p_plane_stride, const uint32_t* q_amax, const uint32_t* p_amax, hipStream_t stream) {
    AlignParams a{};
    a.Q = Q;
    a.q_plane_stride = nq * lq * EVDR_D;
    a.P = P;
    a.p_stride = p_stride;
    a.p_plane_stride = p_plane_stride;
    a.q_amax = nplanes == 2 ? q_amax : nullptr;
    a.p_amax = nplanes == 2 ? p_amax : nullptr;
    a.qmask = qmask;
    a.tilemask = tilemask;
    a.pageflags = pageflags;
    a.cand = cand;
    a.idx_base = idx_base;
    a.r = r;
    a.lq = lq;
    a.lp = lp;
    a.np = np;
    a.sim = sim;
    a.patch = patch;
    a.heat = heat;
    const dim3 grid((unsigned)(nq * r));                // pair = q * r + i (one dimension: nq may exceed a grid's y limit)
    if (nplanes == 2) hipLaunchKernelGGL(align_kernel<2>, grid, dim3(AL_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(align_kernel<1>, grid, dim3(AL_THREADS), 0, stream, a);
    return hipGetLastError();
}
