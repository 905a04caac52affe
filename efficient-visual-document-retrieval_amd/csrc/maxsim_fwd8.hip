// MaxSim forward on an fp8 (OCP e4m3fn) corpus: the block-scaled 16x16x128 MFMA with neutral scales, one instruction per
// 16 patches x 16 tokens x the whole 128-wide row (include/evdr.h "fp8 corpora").
//
// Operands: bytes of x * 2^k per group (csrc/quant8.hip), k per page and per query.  e4m3 x e4m3 products are exact in fp32;
// scores are max-folded in scaled units and brought back by 2^-(kq + kp) with ONE v_ldexp per (query, page, token) at the page
// end, where the -1e4 of masked patches (evaluator/retrieval.py:198) joins the max in real units -- as the fp16-plane path does.
//
// Fragment maps, lane l: c = l & 15, g = l >> 4
//   A[row c][k in group g]  = bytes 32g .. 32g + 31 of patch (16u + c) of the tile      (u = 16-patch half)
//   B[k in group g][col c]  = bytes 32g .. 32g + 31 of token (16t + c) of the query     (t = token half)
//   C/D[row 4g + reg][col c] -> lane holds, for token 16t + c, the patches 16u + 4g + reg, reg = 0..3
// Both operands take the SAME 32 byte positions of their row in the same register order, so whatever K order the hardware
// assigns inside a lane's 32 bytes, it assigns it to A and B alike and it cancels out of the dot product (tests/test_gpu_fp8.py
// checks the three maps with exact small-integer data and asymmetric pages).
//
// LDS: a 32-patch tile is 32 rows x 128 B = 4 KiB.  A fragment is two ds_read_b128 (logical 16-B chunks 2g and 2g + 1 of the
// lane's row); chunk q of row r is stored at chunk q ^ ((r >> 1) & 5).  Over every 16-lane group of ds_read_b128 the 16 lanes
// then hit 16 distinct 16-B slots of the 256-B bank row: conflict-free (the 8 rows of a group's lanes with the same parity pair
// up with 8 distinct chunk indices).  The LDS image stays lane-linear for the DMA; the XOR moves to the source address.
//
// Schedule: page-aligned ring stages of ST tiles (a page of T tiles is ceil(T / ST) stages; when T = k * ST + 1 the last stage
// carries the extra tile), NSTAGE slots, every wave issues G pieces of 1 KiB per stage (pieces past the stage's tiles re-read
// its last tile into the unused end of the slot: the count per stage is fixed, as ring_barrier<N> needs).  A stage whose first
// ST - 1 tiles are all valid runs as one straight-line block (the last tile folds through its mask word, so the partial tail
// tile of a 1030-patch page rides in it); other stages take the per-tile masked fold.
#include "maxsim_device.h"

typedef __attribute__((ext_vector_type(4))) float f32x4v;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

namespace {

using namespace evdr;
constexpr int TILE8_BYTES = EVDR_TILE_PATCHES * EVDR_D;     // 4 KiB: one 32-patch tile of fp8 rows
constexpr int WAVES8 = 8;

__device__ __forceinline__ f32x4v mfma8(const i32x8& a, const i32x8& b, const f32x4v& c) {
    // cbsz = blgp = 0: A and B are e4m3; E8M0 scales 127 = 2^0 for both (op_sel 0)
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}

// the queries of a wave (maxsim_fwd16.hip's resolve_queries: themselves, or entries of the later-slice query list)
template <int QW>
__device__ __forceinline__ void resolve_queries8(const EvdrFwdParams& p, int q0, int (&qreal)[QW]) {
    const int n = p.qlist ? __builtin_amdgcn_readfirstlane(*p.qcount) : p.nq;
#pragma unroll
    for (int j = 0; j < QW; ++j) {
        const int qv = q0 + j;
        int q = -1;
        if (qv < n) q = p.qlist ? __builtin_amdgcn_readfirstlane(p.qlist[qv]) : qv;
        qreal[j] = q;
    }
}

// a NaN byte of e4m3fn is S.1111.111 (the format has no infinities; the quantiser maps NaN and +-Inf to it):
// (b & 0x7F) + 1 carries into bit 7 exactly for 0x7F, and never across a byte
__device__ __forceinline__ uint32_t frag_nan_bytes(const i32x8& v) {
    uint32_t acc = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc |= ((uint32_t)v[i] & 0x7F7F7F7Fu) + 0x01010101u;
    return acc & 0x80808080u;
}
__device__ __forceinline__ uint32_t token_bad_bits8(bool bad_t0, bool bad_t1) {
    const unsigned long long b0 = __ballot(bad_t0), b1 = __ballot(bad_t1);     // lane = 16 g + c holds token 16 t + c
    const uint32_t f0 = (uint32_t)((b0 | (b0 >> 16) | (b0 >> 32) | (b0 >> 48)) & 0xFFFFull);
    const uint32_t f1 = (uint32_t)((b1 | (b1 >> 16) | (b1 >> 32) | (b1 >> 48)) & 0xFFFFull);
    return f0 | (f1 << 16);
}
__device__ __forceinline__ float opaque_nan8() {
    float v = __builtin_bit_cast(float, 0x7FC00000u);
    asm volatile("" : "+v"(v));                        // the optimiser must not reason about it (-fno-honor-nans)
    return v;
}

__device__ __forceinline__ i32x8 read_frag(const char* row_base, int off0, int off1) {
    const i32x4 lo = *reinterpret_cast<const i32x4*>(row_base + off0);
    const i32x4 hi = *reinterpret_cast<const i32x4*>(row_base + off1);
    return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int QW, int ST, int NSTAGE>
__global__ void __launch_bounds__(WAVES8 * 64, 1) maxsim_fwd8_kernel(const EvdrFwd8Params p8) {
    constexpr int G = (4 * (ST + 1) + WAVES8 - 1) / WAVES8;     // LDS-DMA pieces per wave per stage (slot: up to ST + 1 tiles)
    constexpr int SLOT_BYTES = G * WAVES8 * 1024;
    static_assert(NSTAGE >= 3 && ST >= 2, "bad ring geometry");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const EvdrFwdParams& p = p8.g;
    const uint8_t* Q8 = reinterpret_cast<const uint8_t*>(p.Q);
    const uint8_t* P8 = reinterpret_cast<const uint8_t*>(p.P);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15;
    const int g = lane >> 4;

    const BlockWork bw = block_work(p);
    if (!bw.valid) return;
    const int qg = bw.qg, pg0 = bw.pg0, npages = bw.npages;
    if (p.qlist != nullptr && qg * WAVES8 * QW >= __builtin_amdgcn_readfirstlane(*p.qcount)) return;
    const int T = p.ntiles;
    const int spp = (T > ST && T % ST == 1) ? T / ST : (T + ST - 1) / ST;      // stages per page
    const int nstages = npages * spp;

    typedef const __attribute__((address_space(4))) uint32_t* cptr_t;
    typedef const __attribute__((address_space(4))) int32_t* ciptr_t;
    cptr_t tilemask_c = (cptr_t)(uintptr_t)p.tilemask;
    cptr_t pageflags_c = (cptr_t)(uintptr_t)p.pageflags;
    ciptr_t qshift_c = (ciptr_t)(uintptr_t)p8.q_shift;
    ciptr_t pshift_c = (ciptr_t)(uintptr_t)p8.p_shift;

    // ---- resident query fragments: bq[j][t], 8 VGPRs each
    const int q0 = (qg * WAVES8 + wave) * QW;
    int qreal[QW];
    resolve_queries8<QW>(p, q0, qreal);
    bool active = qreal[0] >= 0;
    i32x8 bq[QW][2];
    float qwt[QW][2];
    int kq[QW];
#pragma unroll
    for (int j = 0; j < QW; ++j) {
        const int q = qreal[j];
        kq[j] = q >= 0 ? qshift_c[q] : 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int tok = 16 * t + c;
            const bool ok = (q >= 0) && (tok < p.lq);
            const uint8_t* row = Q8 + (int64_t)q * p.q_stride + (int64_t)(p.tok0 + tok) * EVDR_D + g * 32;
            i32x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
            if (ok) {
                lo = *reinterpret_cast<const i32x4*>(row);
                hi = *reinterpret_cast<const i32x4*>(row + 16);
            }
            bq[j][t] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            float w = 0.f;
            if (ok) w = (p.qmask == nullptr || p.qmask[(int64_t)q * p.lq_total + p.tok0 + tok] != 0) ? 1.f : 0.f;
            qwt[j][t] = w;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t qbad = 0u;                                   // wave-uniform: bit j = a token of query j holds a NaN byte
#pragma unroll
    for (int j = 0; j < QW; ++j)
        if (token_bad_bits8(frag_nan_bytes(bq[j][0]) != 0u, frag_nan_bytes(bq[j][1]) != 0u) != 0u) qbad |= 1u << j;
    if (p.accumulate) {
        // a later 32-token slice: a wave whose queries add nothing skips its MFMA work, a workgroup without any such query leaves
        float any = 0.f;
#pragma unroll
        for (int j = 0; j < QW; ++j) any += qwt[j][0] + qwt[j][1];
        active = active && (__ballot(any != 0.f) != 0ull);
        volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(smem);
        if (threadIdx.x == 0) *flag = 0u;
        __syncthreads();
        if (active && lane == 0) *flag = 1u;
        __syncthreads();
        const bool wg_active = *flag != 0u;
        __syncthreads();
        if (!wg_active) return;
    }

    // ---- ring
    const uint32_t smem_base = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
    auto issue_stage = [&](int s, int slot) {
        const int pgi = s / spp;
        const int sip = s - pgi * spp;
        const int t0 = sip * ST;
        const int tcount = (sip == spp - 1) ? T - t0 : ST;
        const uint8_t* pbase = P8 + (int64_t)(pg0 + pgi) * p.p_stride;
        const uint32_t sbase = smem_base + slot * SLOT_BYTES;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int pc = wave * G + i;                           // piece of the slot: tile pc >> 2, rows 8 (pc & 3) .. + 7
            const int tis = min(pc >> 2, tcount - 1);
            const int r = 8 * (pc & 3) + (lane >> 3);
            const int row = min((t0 + tis) * EVDR_TILE_PATCHES + r, p.lp - 1);
            const int chunk = (lane & 7) ^ ((r >> 1) & 5);
            lds_dma_16B(pbase + (int64_t)row * EVDR_D + chunk * 16, __builtin_amdgcn_readfirstlane(sbase + pc * 1024));
        }
    };

    // A fragment of half u: row (16u + c) * 128, chunks (2g) ^ f and (2g + 1) ^ f, f = (c >> 1) & 5
    const int fsw = (c >> 1) & 5;
    const int off0 = c * EVDR_D + (((2 * g) ^ fsw) << 4);
    const int off1 = c * EVDR_D + (((2 * g + 1) ^ fsw) << 4);

    float run[QW][2];
#pragma unroll
    for (int j = 0; j < QW; ++j) run[j][0] = run[j][1] = neg_inf();

    auto fold_full = [&](const i32x8& a0, const i32x8& a1) {
#pragma unroll
        for (int j = 0; j < QW; ++j) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f32x4v z = {0, 0, 0, 0};
                const f32x4v acc0 = mfma8(a0, bq[j][t], z);
                const f32x4v acc1 = mfma8(a1, bq[j][t], z);
                float m = run[j][t];
                m = __builtin_fmaxf(__builtin_fmaxf(m, acc0[0]), acc0[1]);
                m = __builtin_fmaxf(__builtin_fmaxf(m, acc0[2]), acc0[3]);
                m = __builtin_fmaxf(__builtin_fmaxf(m, acc1[0]), acc1[1]);
                m = __builtin_fmaxf(__builtin_fmaxf(m, acc1[2]), acc1[3]);
                run[j][t] = m;
            }
        }
    };
    auto fold_masked = [&](const i32x8& a0, const i32x8& a1, uint32_t tm) {       // tm != 0, wave-uniform
        const bool hi_live = (tm >> 16) != 0u;
        uint32_t mybits = tm >> (4 * g);
        asm volatile("" : "+v"(mybits));
#pragma unroll
        for (int j = 0; j < QW; ++j) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f32x4v z = {0, 0, 0, 0};
                const f32x4v acc0 = mfma8(a0, bq[j][t], z);
                float m = run[j][t];
#pragma unroll
                for (int i = 0; i < 4; ++i) m = __builtin_fmaxf(m, ((mybits >> i) & 1u) ? acc0[i] : neg_inf());
                if (hi_live) {
                    const f32x4v acc1 = mfma8(a1, bq[j][t], z);
#pragma unroll
                    for (int i = 0; i < 4; ++i) m = __builtin_fmaxf(m, ((mybits >> (16 + i)) & 1u) ? acc1[i] : neg_inf());
                }
                run[j][t] = m;
            }
        }
    };
    auto fold_tile = [&](const char* tb, uint32_t tm) {           // one tile through its mask word (tm != 0)
        const i32x8 a0 = read_frag(tb, off0, off1);
        i32x8 a1 = {0, 0, 0, 0, 0, 0, 0, 0};
        if ((tm >> 16) != 0u) a1 = read_frag(tb + 16 * EVDR_D, off0, off1);
        fold_masked(a0, a1, tm);
    };

#pragma unroll
    for (int i = 0; i < NSTAGE - 1; ++i)
        if (i < nstages) issue_stage(i, i);
    const uint32_t last_word = (p.lp & 31) ? ((1u << (p.lp & 31)) - 1u) : 0xFFFFFFFFu;    // mask of the last tile of a page
    int slot = 0, pgi = 0, sip = 0;
    uint32_t pflags = pageflags_c[pg0];
    int kp = pshift_c[pg0];
    for (int s = 0; s < nstages; ++s) {
        // stage s has landed once only the younger stages' pieces remain (waits + barrier as one statement: ring_barrier)
        if (NSTAGE >= 4 && s + 2 < nstages) ring_barrier<2 * G>();
        else if (s + 1 < nstages) ring_barrier<G>();
        else ring_barrier<0>();
        if (s + NSTAGE - 1 < nstages) issue_stage(s + NSTAGE - 1, slot == 0 ? NSTAGE - 1 : slot - 1);
        const int page = pg0 + pgi;
        if (active) {
            const char* sb = smem + slot * SLOT_BYTES;
            const int t0 = sip * ST;
            const int tcount = (sip == spp - 1) ? T - t0 : ST;
            const bool dense = (pflags & 2u) == 0u;               // no masked patch: tile words follow from lp
            auto tword = [&](int ti) -> uint32_t {
                if (dense) return ti == T - 1 ? last_word : 0xFFFFFFFFu;
                return tilemask_c[(int64_t)page * T + ti];
            };
            bool fast = tcount >= ST;
            if (fast && !dense) {
#pragma unroll
                for (int i = 0; i < ST - 1; ++i) fast = fast && (tword(t0 + i) == 0xFFFFFFFFu);
            }
            if (fast) {
                // ST - 1 full tiles, each tile's fragments read while the previous tile's MFMAs run
                i32x8 a0 = read_frag(sb, off0, off1), a1 = read_frag(sb + 16 * EVDR_D, off0, off1);
#pragma unroll 1
                for (int i = 0; i < ST - 1; ++i) {
                    const char* nb = sb + (i + 1) * TILE8_BYTES;
                    const i32x8 n0 = read_frag(nb, off0, off1), n1 = read_frag(nb + 16 * EVDR_D, off0, off1);
                    fold_full(a0, a1);
                    a0 = n0;
                    a1 = n1;
                }
                const uint32_t tm = tword(t0 + ST - 1);             // the last tile of the block: through its mask word
                if (tm != 0u) fold_masked(a0, a1, tm);
                if (tcount > ST) {                                 // the extra tile of a page of k * ST + 1 tiles
                    const uint32_t tx = tword(t0 + ST);
                    if (tx != 0u) fold_tile(sb + ST * TILE8_BYTES, tx);
                }
            } else {
                for (int i = 0; i < tcount; ++i) {
                    const uint32_t tm = tword(t0 + i);
                    if (tm != 0u) fold_tile(sb + i * TILE8_BYTES, tm);
                }
            }
            if (sip == spp - 1) {
                const float has = (pflags & 1u) ? 1.f : 0.f;
                const float fill = (pflags & 2u) ? -1e4f : neg_inf();
#pragma unroll
                for (int j = 0; j < QW; ++j) {
                    const int e = -(kq[j] + kp);                   // one exact rescale: no intermediate over- or underflow
                    float cs = 0.f;
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        float v = __builtin_amdgcn_ldexpf(xgroup_max(run[j][t]), e);
                        v = __builtin_fmaxf(v, fill);
                        cs += v * has * qwt[j][t];
                        run[j][t] = neg_inf();
                    }
                    cs = row16_sum(cs);
                    if ((pflags & 1u) && ((pflags & 8u) || ((qbad >> j) & 1u))) cs = opaque_nan8();
                    if (lane == 0 && qreal[j] >= 0) {
                        float* o = p.out + (int64_t)qreal[j] * p.out_stride + page;
                        if (p.accumulate) atomicAdd(o, cs);
                        else *o = cs;
                    }
                }
            }
        }
        if (++sip == spp) {
            sip = 0;
            if (++pgi < npages) {
                pflags = pageflags_c[pg0 + pgi];
                kp = pshift_c[pg0 + pgi];
            }
        }
        slot = (slot == NSTAGE - 1) ? 0 : slot + 1;
    }
}

template <int QW, int ST, int NSTAGE>
hipError_t launch_fwd8(EvdrFwd8Params p8, hipStream_t stream) {
    constexpr int G = (4 * (ST + 1) + WAVES8 - 1) / WAVES8;
    constexpr int LDS = NSTAGE * G * WAVES8 * 1024;
    static_assert(LDS <= 160 * 1024, "ring exceeds the LDS");
    const int64_t grid = evdr_set_geometry(p8.g, WAVES8 * QW);
    static std::atomic<uint64_t> lds_done{0};
    const void* kern = reinterpret_cast<const void*>(&maxsim_fwd8_kernel<QW, ST, NSTAGE>);
    hipError_t e = evdr_ensure_dyn_lds(kern, LDS, lds_done);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((maxsim_fwd8_kernel<QW, ST, NSTAGE>), dim3((unsigned)grid), dim3(WAVES8 * 64), LDS, stream, p8);
    return hipGetLastError();
}

}  // namespace

hipError_t evdr_launch_maxsim_fwd8(const EvdrFwd8Params& p8_in, hipStream_t stream) {
    EvdrFwd8Params p8 = p8_in;
    p8.g.ntiles = (p8.g.lp + EVDR_TILE_PATCHES - 1) / EVDR_TILE_PATCHES;
    // queries per wave: 8 for large batches (the headline regime), fewer when the batch would leave most waves without a query.
    // Pages of >= 8 tiles: 11-tile stages (a 1030-patch page of 33 tiles = 3 stages); shorter pages: 2-tile stages, at most four
    // queries per wave (eight do not fit that instance's registers).
    const int nq = p8.g.nq;
    if (p8.g.ntiles >= 8) {
        if (nq > 256) return launch_fwd8<8, 11, 3>(p8, stream);
        if (nq > 8) return launch_fwd8<4, 11, 3>(p8, stream);
        return launch_fwd8<1, 11, 3>(p8, stream);
    }
    if (nq > 8) return launch_fwd8<4, 2, 4>(p8, stream);
    return launch_fwd8<1, 2, 4>(p8, stream);
}
