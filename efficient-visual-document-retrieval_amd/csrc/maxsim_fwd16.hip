// MaxSim forward on the 16x16x32 MFMA shape: bf16 inputs (retrieval hot path) and fp32 inputs as fp16 hi/lo planes.
//
// Mapping: see the header of maxsim_fwd.hip (queries resident as the MFMA B operand, token on the lane, LDS-DMA ring,
// XOR-swizzled conflict-free A reads, XCD-aware block map, fast path for all-valid tiles).  Why this shape: under
// MFMA-dense load on real data MI355X is power-limited, and a register-only MFMA loop sustains 1.90 PFLOP/s with
// 16x16x32 against 1.81 with 32x32x16 (scratch/probe/mfma_peak.hip).  The 16-patch granularity also trims the tail of
// a 1030-patch page (65 x 16 = 1040 rows instead of 33 x 32 = 1056).
//
// Fragment maps (cdna_hip_programming.md §3), lane l: c = l & 15, g = l >> 4
//   A[row c][k = 8g + j]   = patch (16u + c) of the tile, dims 32s + 8g + j      (u = 16-patch half, s = k-step)
//   B[k = 8g + j][col c]   = token (16t + c) of the query, dims 32s + 8g + j      (t = token half)
//   C/D[row 4g + reg][col c] -> lane holds, for token 16t + c, the patches 16u + 4g + reg, reg = 0..3
#include <stdio.h>
#include <type_traits>

#include "maxsim_device.h"

typedef __attribute__((ext_vector_type(4))) float f32x4v;

namespace {

using namespace evdr;
constexpr int TILE_BYTES = kTileBytes;

// Queries q0 .. q0 + QW - 1 of a wave: themselves, or -- in a later 32-token slice of long queries -- entries of the
// compacted list of queries that HAVE a valid token in the slice (p.qlist / p.qcount, built by build_qlist_kernel), so
// that the slice costs in proportion to the long queries, not to all of them.
template <int QW>
__device__ __forceinline__ void resolve_queries(const EvdrFwdParams& p, int q0, int (&qreal)[QW]) {
    const int n = p.qlist ? __builtin_amdgcn_readfirstlane(*p.qcount) : p.nq;
#pragma unroll
    for (int j = 0; j < QW; ++j) {
        const int qv = q0 + j;
        int q = -1;
        if (qv < n) q = p.qlist ? __builtin_amdgcn_readfirstlane(p.qlist[qv]) : qv;
        qreal[j] = q;
    }
}


// ---- non-finite inputs (include/evdr.h, "non-finite inputs") ------------------------------------------------------------
// v_max3_f32 drops NaNs where torch.max propagates them (evaluator/retrieval.py:201), and the hot loop has no room for a
// NaN-propagating max.  So non-finite INPUTS are detected instead -- pages at preparation time (page flag bit 3), queries
// here, once per wave, on the resident fragments -- and the page epilogue returns NaN for every (query, page) pair that
// involves one, which is where the reference's NaN lands: a NaN in a valid patch poisons its page's column, a NaN in ANY
// token of a query (masked ones included: NaN * 0 = NaN, :207) poisons the row on every page that has a valid patch.
// Exponent test on the 16-bit elements (bf16: 0x7F80, fp16: 0x7C00); all integer, the build assumes no NaNs in float compares.
// Per 32-bit word holding two elements: (w & exponent fields) + (one unit of each field) carries into bit 15 / bit 31
// exactly when a field is all ones; the words of a fragment are OR-ed and tested once (3 VALU per word).
template <typename F>
__device__ __forceinline__ uint32_t frag_exp_carry(const F& v) {
    constexpr uint32_t M = std::is_same<F, bf16x8>::value ? 0x7F807F80u : 0x7C007C00u;
    constexpr uint32_t U = std::is_same<F, bf16x8>::value ? 0x00800080u : 0x04000400u;
    typedef __attribute__((ext_vector_type(4))) uint32_t u32x4v;
    const u32x4v w = __builtin_bit_cast(u32x4v, v);
    return ((w[0] & M) + U) | ((w[1] & M) + U) | ((w[2] & M) + U) | ((w[3] & M) + U);
}
// 32 token bits of one query of the wave (bit n = token n holds a non-finite element), wave-uniform
__device__ __forceinline__ uint32_t token_bad_bits(bool bad_t0, bool bad_t1) {
    const unsigned long long b0 = __ballot(bad_t0), b1 = __ballot(bad_t1);     // lane = 16 g + c holds token 16 t + c
    const uint32_t f0 = (uint32_t)((b0 | (b0 >> 16) | (b0 >> 32) | (b0 >> 48)) & 0xFFFFull);
    const uint32_t f1 = (uint32_t)((b1 | (b1 >> 16) | (b1 >> 32) | (b1 >> 48)) & 0xFFFFull);
    return f0 | (f1 << 16);
}
__device__ __forceinline__ float opaque_nan() {
    float v = __builtin_bit_cast(float, 0x7FC00000u);
    asm volatile("" : "+v"(v));                        // the optimiser must not reason about it (-fno-honor-nans)
    return v;
}

// Flat per-tile schedule: WAVES waves per workgroup, ST 32-patch tiles per ring stage, NSTAGE ring slots over the
// block's flat tile stream (stages ignore page boundaries).  Used for short pages (< 8 tiles, e.g. the compressed
// student pages); long pages take maxsim_fwd16s_kernel below.
template <int QW, int WAVES, int ST, int NSTAGE>
__global__ void __launch_bounds__(WAVES * 64, 2) maxsim_fwd16_kernel(const EvdrFwdParams p) {
    constexpr int STAGE_BYTES = ST * TILE_BYTES;
    constexpr int G = ST * 8 / WAVES;                           // LDS-DMA pieces per wave per stage
    static_assert((ST * 8) % WAVES == 0 && NSTAGE >= 2, "bad ring geometry");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15;
    const int g = lane >> 4;

    const BlockWork bw = block_work(p);
    if (!bw.valid) return;
    const int qg = bw.qg, pg0 = bw.pg0, npages = bw.npages;
    // a launch over a device-side query list (later token slices, evdr_maxsim_fwd_prepared_subset): a workgroup whose queries all lie
    // beyond the list has nothing to score and nothing to fetch (workgroup-uniform: before any barrier)
    if (p.qlist != nullptr && qg * WAVES * QW >= __builtin_amdgcn_readfirstlane(*p.qcount)) return;
    const int total_tiles = npages * p.ntiles;
    const int nstages = (total_tiles + ST - 1) / ST;

    // ---- resident query fragments: bq[j][t][s]
    const int q0 = (qg * WAVES + wave) * QW;
    int qreal[QW];                                        // wave-uniform: the queries of this wave, -1 = none
    resolve_queries<QW>(p, q0, qreal);
    bool active = qreal[0] >= 0;
    bf16x8 bq[QW][2][4];
    float qwt[QW][2];
#pragma unroll
    for (int j = 0; j < QW; ++j) {
        const int q = qreal[j];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int tok = 16 * t + c;
            const bool ok = (q >= 0) && (tok < p.lq);
            const int64_t row = (int64_t)q * p.q_stride + (int64_t)(p.tok0 + tok) * EVDR_D + g * 8;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (ok) v = *reinterpret_cast<const bf16x8*>(p.Q + row + s * 32);
                bq[j][t][s] = v;
            }
            float w = 0.f;
            if (ok) w = (p.qmask == nullptr || p.qmask[(int64_t)q * p.lq_total + p.tok0 + tok] != 0) ? 1.f : 0.f;
            qwt[j][t] = w;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t qbad[QW];                                    // wave-uniform: tokens of query j with a NaN / Inf element
#pragma unroll
    for (int j = 0; j < QW; ++j) {
        uint32_t c0 = 0u, c1 = 0u;
#pragma unroll
        for (int s = 0; s < 4; ++s) { c0 |= frag_exp_carry(bq[j][0][s]); c1 |= frag_exp_carry(bq[j][1][s]); }
        qbad[j] = token_bad_bits((c0 & 0x80008000u) != 0u, (c1 & 0x80008000u) != 0u);
    }
    if (p.accumulate && p.argmax == nullptr) {
        // a later 32-token slice of long queries (queries padded to the longest of a set: most have no valid token here):
        // a wave whose queries add nothing skips its MFMA work, a workgroup without any such query leaves at once
        // (not when the argmax is wanted: that is defined for masked query tokens too)
        float any = 0.f;
#pragma unroll
        for (int j = 0; j < QW; ++j) any += qwt[j][0] + qwt[j][1];
        active = active && (__ballot(any != 0.f) != 0ull);
        // workgroup-wide OR through the first word of the (not yet used) ring: the fp16 instances own all 160 KiB of LDS as
        // dynamic memory, a static flag (__syncthreads_or) would push them over the limit
        volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(smem);
        if (threadIdx.x == 0) *flag = 0u;
        __syncthreads();
        if (active && lane == 0) *flag = 1u;
        __syncthreads();
        const bool wg_active = *flag != 0u;
        __syncthreads();
        if (!wg_active) return;
    }

    const uint32_t smem_base = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
    auto issue_stage = [&](int s, int slot) {
        const uint32_t sbase = smem_base + slot * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int pc = wave * G + i;
            const int tis = pc >> 3, piece = pc & 7;
            int t = s * ST + tis;
            t = min(t, total_tiles - 1);
            const int pgi = t / p.ntiles;
            const int tip = t - pgi * p.ntiles;
            const int rit = piece * 4 + (lane >> 4);
            const int row = min(tip * EVDR_TILE_PATCHES + rit, p.lp - 1);
            const int csrc = (lane & 15) ^ (rit & 15);
            const uint16_t* src = p.P + (int64_t)(pg0 + pgi) * p.p_stride + (int64_t)row * EVDR_D + csrc * 8;
            lds_dma_16B(src, __builtin_amdgcn_readfirstlane(sbase + tis * TILE_BYTES + piece * 1024));
        }
    };

    typedef const __attribute__((address_space(4))) uint32_t* cptr_t;
    cptr_t tilemask_c = (cptr_t)(uintptr_t)p.tilemask;
    cptr_t pageflags_c = (cptr_t)(uintptr_t)p.pageflags;

    float run[QW][2];
    int pgi = 0, tip = 0;
    uint32_t pflags = pageflags_c[pg0];
    auto reset_run = [&]() {
#pragma unroll
        for (int j = 0; j < QW; ++j) run[j][0] = run[j][1] = (pflags & 2u) ? -1e4f : neg_inf();
    };
    reset_run();

    // A fragment address: row (16u + c) * 256 + ((4s + g) ^ c) * 16   (row & 15 == c for both halves)
    const int a_lane_off = c * (EVDR_D * 2);
    const int gx = g ^ c;      // (4s + g) ^ c == (4s) ^ (g ^ c): 4s and g (< 4) share no bits, so 4s + g == 4s ^ g

#pragma unroll
    for (int i = 0; i < NSTAGE - 1; ++i)
        if (i < nstages) issue_stage(i, i);
    int slot = 0;
    for (int s = 0; s < nstages; ++s) {
        // stage s has landed once only the younger stages' pieces (NSTAGE-2 of them in steady state) remain
#if defined(EVDR_RING_FAULT) && EVDR_RING_FAULT == 2
        // WAR control of the sentinel instrument (never shipped): the refill of the slot stage s-1 was read from, issued BEFORE the
        // hand-over, i.e. while slower waves may still be reading it
        if (s + NSTAGE - 1 < nstages) issue_stage(s + NSTAGE - 1, slot == 0 ? NSTAGE - 1 : slot - 1);
#endif
        // (waits + barrier as one statement: ring_barrier, maxsim_device.h)
        if (NSTAGE >= 3 && s + 1 < nstages) {
            if (NSTAGE >= 4 && s + 2 < nstages) ring_barrier<2 * G>(); else ring_barrier<G>();
        } else {
            ring_barrier<0>();
        }
#if !(defined(EVDR_RING_FAULT) && EVDR_RING_FAULT == 2)
        if (s + NSTAGE - 1 < nstages) issue_stage(s + NSTAGE - 1, slot == 0 ? NSTAGE - 1 : slot - 1);
#endif
        const char* sbase = smem + slot * STAGE_BYTES;
        if (active) {
#pragma unroll
            for (int tis = 0; tis < ST; ++tis) {
                if (s * ST + tis < total_tiles) {
                    const int page = pg0 + pgi;
                    const uint32_t tm = tilemask_c[(int64_t)page * p.ntiles + tip];
                    if (tm != 0u) {
                        const char* tb = sbase + tis * TILE_BYTES + a_lane_off;
                        const bool hi_live = (tm >> 16) != 0u;            // wave-uniform: skip an all-masked 16-patch half
                        bf16x8 a[2][4];
#pragma unroll
                        for (int s4 = 0; s4 < 4; ++s4) a[0][s4] = *reinterpret_cast<const bf16x8*>(tb + (((4 * s4) ^ gx) << 4));
                        if (hi_live) {
#pragma unroll
                            for (int s4 = 0; s4 < 4; ++s4)
                                a[1][s4] = *reinterpret_cast<const bf16x8*>(tb + 16 * EVDR_D * 2 + (((4 * s4) ^ gx) << 4));
                        }
                        if (tm == 0xFFFFFFFFu) {
#pragma unroll
                            for (int j = 0; j < QW; ++j) {
#pragma unroll
                                for (int t = 0; t < 2; ++t) {
                                    f32x4v acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
                                    for (int s4 = 0; s4 < 4; ++s4) {
                                        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][s4], bq[j][t][s4], acc0, 0, 0, 0);
                                        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][s4], bq[j][t][s4], acc1, 0, 0, 0);
                                    }
                                    float m = run[j][t];
                                    m = __builtin_fmaxf(__builtin_fmaxf(m, acc0[0]), acc0[1]);
                                    m = __builtin_fmaxf(__builtin_fmaxf(m, acc0[2]), acc0[3]);
                                    m = __builtin_fmaxf(__builtin_fmaxf(m, acc1[0]), acc1[1]);
                                    m = __builtin_fmaxf(__builtin_fmaxf(m, acc1[2]), acc1[3]);
                                    run[j][t] = m;
                                }
                            }
                        } else {
                            uint32_t mybits = tm >> (4 * g);
                            asm volatile("" : "+v"(mybits));
#pragma unroll
                            for (int j = 0; j < QW; ++j) {
#pragma unroll
                                for (int t = 0; t < 2; ++t) {
                                    f32x4v acc0 = {0, 0, 0, 0};
#pragma unroll
                                    for (int s4 = 0; s4 < 4; ++s4)
                                        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][s4], bq[j][t][s4], acc0, 0, 0, 0);
                                    float m = run[j][t];
#pragma unroll
                                    for (int i = 0; i < 4; ++i) m = __builtin_fmaxf(m, ((mybits >> i) & 1u) ? acc0[i] : neg_inf());
                                    if (hi_live) {
                                        f32x4v acc1 = {0, 0, 0, 0};
#pragma unroll
                                        for (int s4 = 0; s4 < 4; ++s4)
                                            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][s4], bq[j][t][s4], acc1, 0, 0, 0);
#pragma unroll
                                        for (int i = 0; i < 4; ++i)
                                            m = __builtin_fmaxf(m, ((mybits >> (16 + i)) & 1u) ? acc1[i] : neg_inf());
                                    }
                                    run[j][t] = m;
                                }
                            }
                        }
                    }
                    if (++tip == p.ntiles) {
                        const float has = (pflags & 1u) ? 1.f : 0.f;
#pragma unroll
                        for (int j = 0; j < QW; ++j) {
                            float cs = 0.f;
#pragma unroll
                            for (int t = 0; t < 2; ++t) {
                                cs += xgroup_max(run[j][t]) * has * qwt[j][t];
                            }
                            cs = row16_sum(cs);
                            if ((pflags & 1u) && ((pflags & 8u) || qbad[j] != 0u)) cs = opaque_nan();
                            if (lane == 0 && qreal[j] >= 0) {
                                float* o = p.out + (int64_t)qreal[j] * p.out_stride + page;
                                if (p.accumulate) atomicAdd(o, cs);
                                else *o = cs;
                            }
                        }
                        tip = 0;
                        ++pgi;
                        if (pgi < npages) pflags = pageflags_c[pg0 + pgi];
                        reset_run();
                    }
                }
            }
        }
        slot = (slot == NSTAGE - 1) ? 0 : slot + 1;
    }
}



// ---- page-aligned stages, straight-line fast stage ---------------------------------------------------------------
// Ring stages are aligned to pages: a page of T tiles is ceil(T/ST) stages, the last one short -- or, when T = k*ST + 1,
// k stages whose last one carries the extra tile in a ring slot of ST + 1 tiles (a 1030-patch page = 3 stages of 8 full
// tiles + 1 stage of 8 full tiles and the 6-patch tail tile).  A stage whose ST tiles are all valid and belong
// to one page -- 32 of the 33 tiles of such a page -- runs as ONE basic block: 2*ST half-tile steps x 2*QW chains per
// wave with no branch, no scalar load and no wait other than the LDS counters in between, so the compiler overlaps
// every epilogue and every ds_read with MFMAs of the following chains (the per-tile schedule lost ~28 % of the
// matrix pipe to the gaps between tiles).  A partial FIRST tile rides inside the same block (HEAD instance, bf16); in other
// partially valid stages runs of full tiles go through a rolled per-tile loop and only partial tiles take the per-half path.
// Tile masks of pages whose valid patches form one range (flag bit 2) are derived from the range, such pages are walked
// only over the stages that hold a valid patch and only those tiles are fetched; mask words are read for pages with holes.
// WAVES = 8: one workgroup per CU; WAVES = 4: two independent workgroups per CU (3-12 queries per launch).
// NT: the corpus stream uses the non-temporal policy (launches in which every page is read by exactly one workgroup).
//
// NPL = 1: bf16 inputs, one product per k-step.
// NPL = 2: fp32 inputs as two fp16 planes hi/lo of x * 2^k (k per tensor from its absmax, evdr_h2_shift): three plane
//          products lo*hi + hi*lo + hi*hi per k-step reproduce the fp32 dot product to ~2^-22 relative, below the
//          rounding noise of an fp32 accumulation; scores are rescaled by 2^-(kq + kp) at the page end, where the -1e4 of
//          masked patches (evaluator/retrieval.py:185,198) joins the max in real units.
// ARGMAX: also writes, per (query, page, token), the first patch index attaining the max (what torch.max returns and
//          autograd routes the gradient to).
// DIAG instantiation: s_memtime stamps around the segments of a wave's life, summed per wave and written to p.dbg
// ([block][wave][8] cycles: total, prologue, barrier wait, top-of-stage refill, fast block, generic stage / tail tile,
// page finish, control work in front of the barrier).  Its fences forbid overlaps the real kernel has: read SHARES, never its run time.
__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
template <int NPL> struct FragOf { using type = bf16x8; };
template <> struct FragOf<2> { using type = f16x8; };
__device__ __forceinline__ f32x4v mfma16(const bf16x8& a, const bf16x8& b, const f32x4v& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4v mfma16(const f16x8& a, const f16x8& b, const f32x4v& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// (value, index) reduction over the four lane groups {l, l^16, l^32, l^48}: larger value wins, equal values -> lower index
__device__ __forceinline__ void xgroup_argmax(float& v, int& idx) {
    {
        float a = v, b = v, ia = __builtin_bit_cast(float, idx), ib = ia;
        swap16(a, b);
        swap16(ia, ib);
        const int xa = __builtin_bit_cast(int, ia), xb = __builtin_bit_cast(int, ib);
        const bool tb = (b > a) || (b == a && xb < xa);
        v = tb ? b : a;
        idx = tb ? xb : xa;
    }
    {
        float a = v, b = v, ia = __builtin_bit_cast(float, idx), ib = ia;
        swap32(a, b);
        swap32(ia, ib);
        const int xa = __builtin_bit_cast(int, ia), xb = __builtin_bit_cast(int, ib);
        const bool tb = (b > a) || (b == a && xb < xa);
        v = tb ? b : a;
        idx = tb ? xb : xa;
    }
}

// NCB = 2 (round 6): embeddings of width 256 as TWO 128-column blocks per value plane -- the memory / LDS / register layout simply has
//          NPL * NCB planes of (., ., 128) (plane index = value plane * NCB + column block), and a dot product is the sum of the
//          per-block plane products into ONE accumulator chain (the max over patches needs the whole 256-wide product, so the blocks
//          cannot be scored apart).  fp16 hi/lo planes only (bf16 inputs of that width are upcast like the reference does,
//          evaluator/retrieval.py:176-177), one query per wave (128 VGPRs of query fragments), 1-tile stages (4 planes = 32 KiB a tile).
//
// HI (prefiltered top-k, csrc/prefilter.hip): the COARSE pass over an fp32 corpus -- the hi plane of fp16 hi/lo planes only, one
//          fp16 product per k-step (NPL = 1 arithmetic, the bf16 instance's bytes and ring), with the NPL = 2 semantics otherwise: scaled
//          units, the -1e4 of masked patches deferred to the page end, rescaling by 2^-(kq + kp), page flags and query NaN detection.
// GATHER:  the exact RERANK of the prefilter: workgroup b scores ONE query (p.nq query groups of one) against ITS candidate list
//          p.gather[q * p.np + i], i < p.gcount[q] (corpus page indices; p.np = list capacity), writing out[q * out_stride + i].  The
//          per-pair arithmetic is the instance's own, so a candidate's score is the exhaustive launch's bits for that pair (one query
//          per wave and two give the same bits: tests/test_gpu_random_sweep.py variant 36).  Only wave 0 scores; the others share the
//          ring's fetch work.
// PAGES:   search over a page SUBSET (evdr_maxsim_fwd_pages): ONE list p.gather[i], i < p.np, shared by the whole batch (corpus page
//          indices; p.np = list length, p.ncorpus = pages of the corpus), in the exhaustive launch's geometry -- query groups x chunks of
//          list positions, every wave scoring its own QW queries -- writing out[q * out_stride + i].  An entry outside [0, p.ncorpus) is
//          a hole: it is treated as a page without any valid patch (nothing fetched, its index clamped wherever one is formed) and its
//          column is -inf.  The per-pair arithmetic is the instance's own.  The body (maxsim_fwd16s_body.inc) is shared by two kernel
//          templates, maxsim_fwd16s_kernel and maxsim_fwd16s_pages_kernel, so that the former's template argument lists stay what they were.
template <int QW, int NPL, bool ARGMAX, int ST, int NSTAGE, bool DIAG = false, bool BAL = false, int OCC = 2, int WAVES = 8, bool NT = false, int NCB = 1,
          bool HI = false, bool GATHER = false>
__global__ void __launch_bounds__(WAVES * 64, OCC) maxsim_fwd16s_kernel(const EvdrFwdParams p) {
    constexpr bool PAGES = false;
#include "maxsim_fwd16s_body.inc"
}

// page-subset instances (PAGES): eight waves, the priority schedule, 8-tile stages on bf16 planes / 4-tile stages on fp16 hi/lo planes
template <int QW, int NPL, int ST>
__global__ void __launch_bounds__(8 * 64, 2) maxsim_fwd16s_pages_kernel(const EvdrFwdParams p) {
    constexpr bool PAGES = true, ARGMAX = false, DIAG = false, BAL = true, NT = false, HI = false, GATHER = false;
    constexpr int NSTAGE = 2, WAVES = 8, NCB = 1;
#include "maxsim_fwd16s_body.inc"
}

template <int QW, int NPL, int ST>
hipError_t launch16s_pages(const EvdrFwdParams& pin, hipStream_t stream) {
    EvdrFwdParams p = pin;
    constexpr int LDS = 2 * (ST + 1) * NPL * TILE_BYTES;
    auto kern = maxsim_fwd16s_pages_kernel<QW, NPL, ST>;
    static std::atomic<uint64_t> attr_devs{0};
    if (hipError_t e = evdr_ensure_dyn_lds((const void*)kern, LDS, attr_devs); e != hipSuccess) return e;
    const int64_t blocks = evdr_set_geometry(p, 8 * QW, LDS <= 80 * 1024 ? 2 : 1);      // p.np = list length: chunks of list positions
    static const char* const name = [] {
        static char buf[64];
        snprintf(buf, sizeof(buf), "maxsim_fwd16s_pages_kernel<%d,%d,%d>pages", QW, NPL, ST);
        return (const char*)buf;
    }();
    evdr_note_fwd_kernel(name);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(8 * 64), LDS, stream, p);
    return hipGetLastError();
}

template <int QW, int NPL, bool ARGMAX, int ST, int NSTAGE, bool DIAG = false, bool BAL = false, int OCC = 2, int WAVES = 8, bool NT = false, int NCB = 1,
          bool HI = false, bool GATHER = false>
hipError_t launch16s(const EvdrFwdParams& pin, hipStream_t stream) {
    EvdrFwdParams p = pin;
    constexpr int LDS = NSTAGE * (ST + 1) * NPL * NCB * TILE_BYTES;
    auto kern = maxsim_fwd16s_kernel<QW, NPL, ARGMAX, ST, NSTAGE, DIAG, BAL, OCC, WAVES, NT, NCB, HI, GATHER>;
    static std::atomic<uint64_t> attr_devs{0};
    if (hipError_t e = evdr_ensure_dyn_lds((const void*)kern, LDS, attr_devs); e != hipSuccess) return e;
    // (the rerank: one query per workgroup)
    const int64_t blocks = evdr_set_geometry(p, GATHER ? 1 : WAVES * QW, LDS <= 80 * 1024 ? 2 : 1);      // two workgroups share a CU's 160 KiB, or one owns it
    static const char* const name = [] {
        static char buf[96];
        snprintf(buf, sizeof(buf), "maxsim_fwd16s_kernel<%d,%d,%s,%d,%d,%s,%s,%d,%d,%s>%s", QW, NPL, ARGMAX ? "true" : "false", ST, NSTAGE,
                 DIAG ? "true" : "false", BAL ? "true" : "false", OCC, WAVES, NT ? "true" : "false",
                 NCB == 2 ? "x2cols" : (HI ? "hi" : (GATHER ? "gather" : "")));
        return (const char*)buf;
    }();
    evdr_note_fwd_kernel(name);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(WAVES * 64), LDS, stream, p);
    return hipGetLastError();
}

template <int QW, int WAVES, int ST, int NSTAGE>
hipError_t launch16(const EvdrFwdParams& pin, hipStream_t stream) {
    EvdrFwdParams p = pin;
    constexpr int LDS = NSTAGE * ST * TILE_BYTES;
    auto kern = maxsim_fwd16_kernel<QW, WAVES, ST, NSTAGE>;
    static std::atomic<uint64_t> attr_devs{0};
    if (hipError_t e = evdr_ensure_dyn_lds((const void*)kern, LDS, attr_devs); e != hipSuccess) return e;
    const int64_t blocks = evdr_set_geometry(p, WAVES * QW);
    static const char* const name = [] {
        static char buf[64];
        snprintf(buf, sizeof(buf), "maxsim_fwd16_kernel<%d,%d,%d,%d>", QW, WAVES, ST, NSTAGE);
        return (const char*)buf;
    }();
    evdr_note_fwd_kernel(name);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(WAVES * 64), LDS, stream, p);
    return hipGetLastError();
}

}  // namespace

// NPL = 1 without argmax (retrieval / eval): geom 0 (default) = page-aligned 8-tile stages with the self-balancing priority
// schedule (maxsim_fwd16s_kernel) for pages of >= 8 tiles, the flat per-tile ring (maxsim_fwd16_kernel) for shorter
// pages; geom 1 forces the flat kernel, geom 2 the staged kernel without the priority schedule (evdr_debug_set_fwd_variant:
// the test sweep runs every instance against the oracle); 50/51 are the stamped diagnostic instances of the experiment build.  Argmax and fp16 hi/lo planes (nplanes = 2): the staged kernel for every
// page length.
#ifdef EVDR_EXPERIMENT
static unsigned long long* g_dbg_buffer = nullptr;
unsigned long long* evdr_experiment_dbg_buffer() { return g_dbg_buffer; }
extern "C" EVDR_API void evdr_experiment_set_dbg_buffer(void* dev_ptr) { g_dbg_buffer = (unsigned long long*)dev_ptr; }
#endif

hipError_t evdr_launch_maxsim_fwd16(const EvdrFwdParams& p, int qw, int waves, int nplanes, bool want_argmax, int geom, hipStream_t stream) {
    const int ntiles = (p.lp + EVDR_TILE_PATCHES - 1) / EVDR_TILE_PATCHES;
#ifdef EVDR_EXPERIMENT
    if (geom == 52 && nplanes == 2 && want_argmax && qw == 2) {      // stamped student-forward instance (scratch/diag_student.py)
        EvdrFwdParams pd = p;
        pd.dbg = evdr_experiment_dbg_buffer();
        return launch16s<2, 2, true, 3, 2, true, true>(pd, stream);
    }
    if (geom == 53 && nplanes == 2 && !want_argmax && qw == 2) {     // stamped teacher-forward instance (scratch/diag_teacher.py)
        EvdrFwdParams pd = p;
        pd.dbg = evdr_experiment_dbg_buffer();
        return launch16s<2, 2, false, 4, 2, true, true>(pd, stream);
    }
#endif
    if (nplanes == 4) {
        // 256-wide embeddings as fp16 hi/lo planes x two 128-column blocks (NCB = 2): one query per wave, 1-tile stages
        return want_argmax ? launch16s<1, 2, true, 1, 2, false, true, 2, 8, false, 2>(p, stream)
                           : launch16s<1, 2, false, 1, 2, false, true, 2, 8, false, 2>(p, stream);
    }
    if (nplanes == 2) {
#ifdef EVDR_EXPERIMENT
        // variant 12 (experiment build): the student forward as TWO independent 4-wave workgroups per CU (1-tile stages, 64 KiB of
        // ring each) instead of one 8-wave workgroup -- VERDICT round 3, item 5 (profiles/r04_experiments.txt)
        if (geom == 12 && want_argmax && qw == 2) return launch16s<2, 2, true, 1, 2, false, false, 2, 4>(p, stream);
        if (geom == 13 && want_argmax && qw == 2) return launch16s<1, 2, true, 1, 2, false, false, 2, 4>(p, stream);
#endif
        // 16-KiB tiles: 4-tile stages (2 x 5 x 16 KiB = all 160 KiB of LDS) or 3-tile stages, whichever sends fewer FULL tiles
        // through the per-tile path: a stage runs as the straight-line block only if all its tiles are full, and a lone
        // tail tile rides in the previous stage.  1030 patches = 33 tiles: 8 x 4 + tail; 206 patches = 7 tiles: 2 x 3 + tail
        // (with 4-tile stages the second stage -- tiles 4, 5 and the 14-patch tail -- would be generic).
        auto generic_full_tiles = [&](int st) {
            const bool partial = (p.lp % EVDR_TILE_PATCHES) != 0;
            const int r = ntiles % st;
            if (r == 1 && ntiles > st) return partial ? 0 : 1;
            if (r == 0) return partial ? st - 1 : 0;
            return partial ? r - 1 : r;
        };
        const bool st3 = geom == 10 || (geom != 11 && generic_full_tiles(3) < generic_full_tiles(4));   // 10 / 11: A/B force
        if (st3) {
            if (want_argmax) return qw == 2 ? launch16s<2, 2, true, 3, 2, false, true>(p, stream) : launch16s<1, 2, true, 3, 2, false, true>(p, stream);
            return qw == 2 ? launch16s<2, 2, false, 3, 2, false, true>(p, stream) : launch16s<1, 2, false, 3, 2, false, true>(p, stream);
        }
        if (want_argmax) return qw == 2 ? launch16s<2, 2, true, 4, 2, false, true>(p, stream) : launch16s<1, 2, true, 4, 2, false, true>(p, stream);
        // Non-temporal corpus stream for a LARGE corpus read by at most two query groups (the frozen teacher of a training step:
        // 32 queries x 500 x 1030 patches = 264 MB of planes, more than half of the 256-MiB Infinity Cache).  Such a stream gains
        // nothing from the cache (each step evicts its own head before coming round) and, on the default policy, evicts what runs
        // between two passes: the student's parameters, moments and planes, which the student forward and the update kernel
        // re-read a few hundred microseconds later.  Measured inside the fused step (scratch/nt_teacher_ab.py, interleaved, same
        // process): update kernel 86.5 -> 78.7 us, student forward 76.4 -> 74.2, teacher forward unchanged (the two workgroups
        // that share a page chunk still meet in the XCD's L2), step 0.456 -> 0.442 ms; same bits.  geom 33 / 34 force it on / off.
        const int64_t corpus_bytes = (int64_t)p.np * p.lp * EVDR_D * 2 * 2;
        const int qgroups = (p.nq + 8 * qw - 1) / (8 * qw);
        const bool nt2 = geom == 33 || (geom != 34 && qgroups <= 2 && corpus_bytes >= ((int64_t)128 << 20) && !p.per_token);
        if (nt2) return qw == 2 ? launch16s<2, 2, false, 4, 2, false, true, 2, 8, true>(p, stream) : launch16s<1, 2, false, 4, 2, false, true, 2, 8, true>(p, stream);
        return qw == 2 ? launch16s<2, 2, false, 4, 2, false, true>(p, stream) : launch16s<1, 2, false, 4, 2, false, true>(p, stream);
    }
    if (want_argmax) return qw == 2 ? launch16s<2, 1, true, 8, 2, false, true>(p, stream) : launch16s<1, 1, true, 8, 2, false, true>(p, stream);
#ifdef EVDR_EXPERIMENT
    // stamped diagnostic instances (scratch/diag_stamps.py): compiled only into the experiment build (libevdr_exp.so), the
    // stamp buffer comes in through evdr_experiment_set_dbg_buffer
    if ((geom == 50 || geom == 51) && ntiles >= 8 && qw == 4) {
        EvdrFwdParams pd = p;
        pd.dbg = evdr_experiment_dbg_buffer();
        return geom == 50 ? launch16s<4, 1, false, 8, 2, true, false>(pd, stream) : launch16s<4, 1, false, 8, 2, true, true>(pd, stream);
    }
#endif
    if (geom == 2 && ntiles >= 8 && qw == 4) return launch16s<4, 1, false, 8, 2, false, false>(p, stream);   // A/B: no priority schedule
#ifdef EVDR_EXPERIMENT
    // variant 60 (experiment build only): 32 queries per workgroup as FOUR waves of eight -- one wave per SIMD with 512 registers,
    // the query fragments pinned to the AGPR half and read from there by the MFMAs -- instead of eight waves of four: half the LDS
    // fragment reads per FLOP.  Measured (profiles/r04_experiments.txt): bit-identical scores, 16 % SLOWER at 1024 x 20 000
    // (111.8 ms against 96.5; 23 % slower with dependent chains): with one wave per SIMD nothing covers a wave's own waits
    // (fragment reads, LDS-DMA issue, MFMA-result latency), and hipcc's schedule leaves those in the open.  Not shipped.
    if (qw == 8 && waves == 4 && ntiles >= 8) return launch16s<8, 1, false, 8, 2, false, false, 1, 4>(p, stream);
#endif
    // launches of ONE query group (<= 8 queries here): every page is read by exactly one workgroup, exactly once -> the corpus
    // stream uses the non-temporal policy (NT instances; geom 31 = A/B without it)
    const bool nt = geom != 31;
    if (waves == 4 && geom != 1) {                        // two independent 4-wave workgroups per CU, 4-tile stages, 2 or 3 queries per wave
        if (qw == 3) return launch16s<3, 1, false, 4, 2, false, false, 2, 4, true>(p, stream);
        if (qw == 1) return launch16s<1, 1, false, 4, 2, false, false, 2, 4, true>(p, stream);
        return nt ? launch16s<2, 1, false, 4, 2, false, false, 2, 4, true>(p, stream) : launch16s<2, 1, false, 4, 2, false, false, 2, 4>(p, stream);
    }
    if ((geom != 1 && ntiles >= 8) || p.per_token) {
        if (qw == 4) return launch16s<4, 1, false, 8, 2, false, true>(p, stream);
        if (qw == 3) return launch16s<3, 1, false, 8, 2, false, true>(p, stream);
        if (qw == 2) return launch16s<2, 1, false, 8, 2, false, true>(p, stream);
        if (nt && p.nq <= 8 && !p.per_token) return launch16s<1, 1, false, 8, 2, false, true, 2, 8, true>(p, stream);
        return launch16s<1, 1, false, 8, 2, false, true>(p, stream);
    }
    if (qw >= 3) return launch16<4, 8, 4, 3>(p, stream);
    if (qw == 2) return launch16<2, 8, 4, 3>(p, stream);
    return launch16<1, 8, 4, 3>(p, stream);
}

// Prefiltered top-k (csrc/prefilter.hip).  Coarse pass: the hi plane of an fp32 corpus on the bf16 headline geometry (8-tile stages,
// four queries per wave: one fp16 plane has the bf16 plane's bytes and MFMA rate).  Rerank: the fp16 hi/lo instance of one query per
// wave (the exhaustive launch's own arithmetic) over per-query candidate lists.
hipError_t evdr_launch_maxsim_coarse16(const EvdrFwdParams& p, hipStream_t stream) {
    return launch16s<4, 1, false, 8, 2, false, true, 2, 8, false, 1, true>(p, stream);
}

hipError_t evdr_launch_maxsim_gather16(const EvdrFwdParams& p, hipStream_t stream) {
    return launch16s<1, 2, false, 4, 2, false, true, 2, 8, false, 1, false, true>(p, stream);
}

// Candidate scoring on a bf16 corpus (csrc/candidates.hip): the bf16 staged instance of one query per wave (8-tile stages, the
// exhaustive staged launch's own arithmetic per pair) over per-query candidate lists.
hipError_t evdr_launch_maxsim_gather16_bf16(const EvdrFwdParams& p, hipStream_t stream) {
    return launch16s<1, 1, false, 8, 2, false, true, 2, 8, false, 1, false, true>(p, stream);
}

// Search over a page subset (evdr_maxsim_fwd_pages): p.gather = the batch's list of p.np corpus pages, p.ncorpus = pages of the corpus.
// bf16: one query per wave up to 8 queries, four above; fp16 hi/lo: one up to 8 queries, two above.  The exhaustive launch may pick
// another number of queries per wave for the same batch: the bits per (query, page) pair do not depend on it.
hipError_t evdr_launch_maxsim_pages16(const EvdrFwdParams& pin, int nplanes, hipStream_t stream) {
    EvdrFwdParams p = pin;
    p.inblock_refill = p.nq > 4 ? 1 : 0;                  // as the exhaustive launch (maxsim_fwd.hip)
    if (nplanes == 2) return p.nq > 8 ? launch16s_pages<2, 2, 4>(p, stream) : launch16s_pages<1, 2, 4>(p, stream);
    return p.nq > 8 ? launch16s_pages<4, 1, 8>(p, stream) : launch16s_pages<1, 1, 8>(p, stream);
}
