// Fused group-mean page pooling: a page's patches pooled by a group list WHILE the page is ingested.
//
// One workgroup per destination page, as corpus_ingest_kernel (csrc/ingest.hip), whose helpers this file shares: pooled token t of a
// page is the fp32 mean of the group's valid members, added in list order from +0.0f, optionally renormalised by x / (||x|| + 1e-12)
// with the sum of squares formed in ONE fixed order (8-column octets summed sequentially, the 16 octet sums combined by a balanced
// tree of adjacent pairs), so that the bits depend neither on the destination kind nor on the thread layout.  The pooled page is then
// written in the corpus's kind with exactly the bits the ingest kernel would write for it -- or, for the plain destination, as fp32
// rows and mask bytes.  A team of 16 threads (8 for fp8) covers one pooled token, each thread the columns of one 16-byte store; the
// members of a group are gathered with 16-byte loads, 4 (2) of them in flight per thread; the tree is 4 (3) xor-shuffles inside the
// team.  HBM-bound: every source patch is read once (twice for fp8: the page's amax has to be known before a byte can be written,
// and the second read of <= 0.5 MB comes from cache).  LDS holds the reductions only; no atomics on the page's words.
#include "ingest_device.h"

namespace {

constexpr int kThreads = 256;

// separately rounded fp32 operations: no contraction of a multiply and an add into an FMA, whatever -ffp-contract says
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// fp32 bits -> the bits of the nearest bf16 (ties to even) in the high half, NaN -> the canonical quiet NaN: torch's .bfloat16()
__device__ __forceinline__ uint32_t bf16_rne_bits(uint32_t b) {
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC00000u;
    return (b + 0x7FFFu + ((b >> 16) & 1u)) & 0xFFFF0000u;
}

// SRC: dtype of the source pages; KIND: EVDR_CORPUS_BF16 / _F16_HILO / _FP8 or EVDR_POOL_PLAIN; VEC: 16-byte loads (and, for the
// plain destination, 16-byte stores).  A thread handles CH consecutive columns of one pooled token and keeps UN member loads in flight.
template <int SRC, int KIND, bool VEC>
__global__ void __launch_bounds__(kThreads) corpus_pool_ingest_kernel(const EvdrPoolParams q) {
    constexpr int CH = KIND == EVDR_CORPUS_FP8 ? 16 : 8;
    constexpr int CPR = EVDR_D / CH;                                  // threads per pooled token: the team
    constexpr int UN = KIND == EVDR_CORPUS_FP8 ? 2 : 4;
    constexpr int EB = SRC == EVDR_F32 ? 4 : 2;                      // bytes per source element
    __shared__ uint32_t red[7][kThreads / 64];

    const EvdrIngestParams& p = q.g;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t sp = blockIdx.x;                                    // source page
    // the destination is checked BEFORE it forms an address: an entry outside [0, capacity) is a hole, its page is skipped
    const int64_t dst = p.dst_pages ? (int64_t)p.dst_pages[sp] : p.first_page + sp;
    if (dst < 0 || dst >= p.capacity) return;                         // uniform over the workgroup: nobody waits at a barrier below
    const int lp = p.lp, ls = q.ls, lp_src = p.lp_src, d_src = p.d_src, m = q.m;
    const char* src = reinterpret_cast<const char*>(p.src) + sp * p.src_stride * EB;
    const uint8_t* mrow = p.pmask ? p.pmask + sp * lp_src : nullptr;
    const int32_t* mem = q.members + sp * q.members_stride;
    const int32_t* offs = q.offsets + sp * q.offsets_stride;

    // a member counts when its index is a patch of the page (anything else is a hole, never an address) and its mask byte is set
    auto valid = [&](int idx) { return (unsigned)idx < (unsigned)lp_src && (mrow == nullptr || mrow[idx] != 0); };
    // the list range of group t, clamped into [0, m] and made non-decreasing: offsets nobody validated (the per-page form) can
    // empty a group, never leave the list
    auto group_range = [&](int t, int& beg, int& end) {
        beg = min(max(offs[t], 0), m);
        end = min(max(offs[t + 1], beg), m);
    };

    // ---- pooled mask: a token is valid when its group has a valid member.  One token per lane, a ballot per wave gives two tile
    // words; their quantities for the flag word as pack_pmask_kernel; tokens [ls, lp) are masked
    uint32_t first_masked = 0xFFFFu, first_valid = 0xFFFFu, end_valid = 0u, nvalid = 0u;
    const int ntiles = (lp + EVDR_TILE_PATCHES - 1) / EVDR_TILE_PATCHES;
    for (int base = wv * 64; base < ntiles * 32; base += kThreads) {
        const int t = base + lane;
        bool ok = false;
        if (t < ls) {
            int beg, end;
            group_range(t, beg, end);
            for (int j = beg; j < end && !ok; ++j) ok = valid(mem[j]);
        }
        const uint64_t bal = __ballot(ok);
        if constexpr (KIND == EVDR_POOL_PLAIN) {
            if (t < ls) q.out_mask[dst * ls + t] = ok ? 1 : 0;
        } else if ((lane & 31) == 0 && (t >> 5) < ntiles) {
            const int tile = t >> 5, left = lp - t;                   // left >= 1 patches of the page in this tile
            const uint32_t w = (uint32_t)(bal >> lane), inrange = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
            p.tilemask[dst * ntiles + tile] = w;
            nvalid += (uint32_t)__builtin_popcount(w);
            if (w) {
                first_valid = min(first_valid, (uint32_t)(t + __builtin_ctz(w)));
                end_valid = max(end_valid, (uint32_t)(t + 32 - __builtin_clz(w)));
            }
            const uint32_t masked = inrange & ~w;
            if (masked) first_masked = min(first_masked, (uint32_t)(t + __builtin_ctz(masked)));
        }
    }

    // ---- one piece (CH columns) of pooled token u / CPR as fp32 bit patterns; the whole team of the token is here together
    auto pool_piece = [&](int u, uint32_t* v) {
        const int row = u / CPR, col = (u % CPR) * CH;
        float acc[CH];
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] = 0.0f;
        int cnt = 0;
        if (row < ls) {
            int beg, end;
            group_range(row, beg, end);
            for (int j = beg; j < end; j += UN) {
                uint32_t w[UN][CH];
                bool ok[UN];
#pragma unroll
                for (int k = 0; k < UN; ++k) {
                    const int idx = j + k < end ? mem[j + k] : -1;
                    ok[k] = valid(idx);
                    if (ok[k]) {
                        const char* r = src + (int64_t)idx * d_src * EB;
#pragma unroll
                        for (int o = 0; o < CH / 8; ++o) load_oct<SRC, VEC>(r, col + 8 * o, d_src, w[k] + 8 * o);
                    } else {
#pragma unroll
                        for (int e = 0; e < CH; ++e) w[k][e] = 0u;
                    }
                }
#pragma unroll
                for (int k = 0; k < UN; ++k) {                        // list order
                    if (ok[k]) {
#pragma unroll
                        for (int e = 0; e < CH; ++e) acc[e] = add_rn(acc[e], __builtin_bit_cast(float, w[k][e]));
                        ++cnt;
                    }
                }
            }
        }
        if (cnt > 0) {
            const float c = (float)cnt;
#pragma unroll
            for (int e = 0; e < CH; ++e) acc[e] = acc[e] / c;         // correctly rounded (the compiler's default for HIP)
        }
        if (q.normalize) {
            float s[CH / 8];
#pragma unroll
            for (int o = 0; o < CH / 8; ++o) {
                s[o] = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) s[o] = add_rn(s[o], mul_rn(acc[8 * o + j], acc[8 * o + j]));
            }
            float t = s[0];
            if constexpr (CH == 16) t = add_rn(s[0], s[1]);           // the tree's first level inside the thread
#pragma unroll
            for (int o = 1; o < CPR; o <<= 1) t = add_rn(t, __shfl_xor(t, o));    // adjacent pairs, then pairs of those: the same bits in every lane
            const float den = add_rn(__builtin_sqrtf(t), 1e-12f);
#pragma unroll
            for (int e = 0; e < CH; ++e) acc[e] = acc[e] / den;
        }
#pragma unroll
        for (int e = 0; e < CH; ++e) v[e] = __builtin_bit_cast(uint32_t, acc[e]);
    };

    // ---- fp8: the pooled page's amax over all its tokens (the masked ones are zero), then its shift
    int k8 = 0;
    if constexpr (KIND == EVDR_CORPUS_FP8) {
        uint32_t mx = 0u;
        const int total = ls * CPR;
        for (int u = tid; u < total; u += kThreads) {
            uint32_t v[CH];
            pool_piece(u, v);
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const uint32_t b = v[e] & 0x7FFFFFFFu;
                if (b < 0x7F800000u) mx = max(mx, b);                // finite elements only: NaN / Inf never move amax
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        if (lane == 0) red[6][wv] = mx;
        __syncthreads();
        mx = max(max(red[6][0], red[6][1]), max(red[6][2], red[6][3]));
        k8 = fp8_shift(mx);
    }

    // ---- the page
    int k2 = 0;
    if constexpr (KIND == EVDR_CORPUS_F16_HILO) k2 = evdr_h2_shift(*p.p_amax);
    bool bad = false;                                                 // a pooled token holds NaN / +-Inf (a masked one is all zero)
    uint32_t amax = 0u;                                               // fp16 hi/lo: |x| bits of the largest finite element seen
    {
        const int total = lp * CPR;
        for (int u = tid; u < total; u += kThreads) {
            const int row = u / CPR, col = (u % CPR) * CH;
            uint32_t v[CH];
            pool_piece(u, v);
            if constexpr (KIND == EVDR_POOL_PLAIN) {
                float* o = q.out + (dst * ls + row) * q.d_out + col;
                if constexpr (VEC) {
                    if (col < q.d_out) {
                        *reinterpret_cast<uint4*>(o) = make_uint4(v[0], v[1], v[2], v[3]);
                        *reinterpret_cast<uint4*>(o + 4) = make_uint4(v[4], v[5], v[6], v[7]);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < CH; ++e)
                        if (col + e < q.d_out) o[e] = __builtin_bit_cast(float, v[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    const uint32_t b = v[e] & 0x7FFFFFFFu;
                    if (b >= 0x7F800000u) bad = true;
                    else if constexpr (KIND == EVDR_CORPUS_F16_HILO) amax = max(amax, b);
                    if constexpr (KIND == EVDR_CORPUS_BF16) v[e] = bf16_rne_bits(v[e]);
                }
                store_piece<KIND>(p.planes, dst * p.p_stride + (int64_t)row * EVDR_D + col, p.p_plane_stride, v, k2, k8);
            }
        }
    }
    if constexpr (KIND == EVDR_POOL_PLAIN) return;

    // ---- the page's words: plain stores by the one thread that holds the workgroup's reductions
    uint32_t badw = bad ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        first_masked = min(first_masked, (uint32_t)__shfl_xor((int)first_masked, off));
        first_valid = min(first_valid, (uint32_t)__shfl_xor((int)first_valid, off));
        end_valid = max(end_valid, (uint32_t)__shfl_xor((int)end_valid, off));
        nvalid += (uint32_t)__shfl_xor((int)nvalid, off);
        badw |= (uint32_t)__shfl_xor((int)badw, off);
        amax = max(amax, (uint32_t)__shfl_xor((int)amax, off));
    }
    if (lane == 0) {
        red[0][wv] = first_masked;
        red[1][wv] = first_valid;
        red[2][wv] = end_valid;
        red[3][wv] = nvalid;
        red[4][wv] = badw;
        red[5][wv] = amax;
    }
    __syncthreads();
    if (tid == 0) {
        first_masked = min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3]));
        first_valid = min(min(red[1][0], red[1][1]), min(red[1][2], red[1][3]));
        end_valid = max(max(red[2][0], red[2][1]), max(red[2][2], red[2][3]));
        nvalid = red[3][0] + red[3][1] + red[3][2] + red[3][3];
        badw = red[4][0] | red[4][1] | red[4][2] | red[4][3];
        amax = max(max(red[5][0], red[5][1]), max(red[5][2], red[5][3]));
        p.pageflags[dst] = page_flag_word(nvalid, first_masked, first_valid, end_valid, badw);
        if constexpr (KIND == EVDR_CORPUS_FP8) p.shift[dst] = k8;
        if constexpr (KIND == EVDR_CORPUS_F16_HILO) {
            // a finite pooled element whose scaled exponent passes 2^15 leaves the window evdr_h2_shift promises (corpus_ingest_kernel)
            if (p.status != nullptr && (int)(amax >> 23) + k2 > 141) atomicOr(p.status, 1u);
        }
    }
}

template <int SRC, int KIND>
hipError_t launch(const EvdrPoolParams& p, bool vec, hipStream_t stream) {
    if (vec) hipLaunchKernelGGL((corpus_pool_ingest_kernel<SRC, KIND, true>), dim3((unsigned)p.g.b), dim3(kThreads), 0, stream, p);
    else hipLaunchKernelGGL((corpus_pool_ingest_kernel<SRC, KIND, false>), dim3((unsigned)p.g.b), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

template <int KIND>
hipError_t launch_src(const EvdrPoolParams& p, bool vec, hipStream_t stream) {
    if (p.g.src_dtype == EVDR_F32) return launch<EVDR_F32, KIND>(p, vec, stream);
    if (p.g.src_dtype == EVDR_BF16) return launch<EVDR_BF16, KIND>(p, vec, stream);
    return launch<EVDR_F16, KIND>(p, vec, stream);
}

}  // namespace

// arguments are the caller's to check (evdr_corpus_pool_ingest / evdr_pool_pages do): kinds and dtypes valid, b >= 1
hipError_t evdr_launch_corpus_pool(const EvdrPoolParams& p, hipStream_t stream) {
    const int64_t eb = p.g.src_dtype == EVDR_F32 ? 4 : 2;
    bool vec = p.g.d_src % 8 == 0 && reinterpret_cast<uintptr_t>(p.g.src) % 16 == 0 && (p.g.src_stride * eb) % 16 == 0;
    if (p.g.kind == EVDR_POOL_PLAIN) return launch_src<EVDR_POOL_PLAIN>(p, vec && reinterpret_cast<uintptr_t>(p.out) % 16 == 0, stream);
    if (p.g.kind == EVDR_CORPUS_BF16) return launch_src<EVDR_CORPUS_BF16>(p, vec, stream);
    if (p.g.kind == EVDR_CORPUS_F16_HILO) return launch_src<EVDR_CORPUS_F16_HILO>(p, vec, stream);
    return launch_src<EVDR_CORPUS_FP8>(p, vec, stream);
}
