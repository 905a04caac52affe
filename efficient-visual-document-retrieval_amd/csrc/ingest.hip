// Fused page ingest: pages written IN PLACE into a corpus allocated for `capacity` pages (include/evdr.h "growable corpus").
//
// One workgroup per destination page.  From ONE read of the source page and its mask bytes it writes everything the searchers
// need for that page: the 32-patch tile words and the flag word of pack_pmask_kernel (bit 3 by the rule of evdr_flag_nonfinite),
// and the page's planes in the corpus's kind -- a bf16 copy, the fp16 hi/lo split of split_h2_kernel under the CORPUS's absmax word,
// or the e4m3 bytes and the page's shift of quantize_fp8_kernel (a first pass over the page finds its amax; the second read of its
// <= 0.5 MB comes from cache).  HBM-bound byte work: 16-byte loads and stores, several loads in flight per thread (absmax_kernel in
// prep.hip has the measurement), no LDS beyond the reductions, no atomics on the flags (the workgroup owns its page).
#include "ingest_device.h"

namespace {

constexpr int kThreads = 256;

// SRC: dtype of the source pages; KIND: EVDR_CORPUS_*; a thread handles CH consecutive columns of one patch at a time (what one
// 16-byte store of the corpus's element type holds) and keeps UN such pieces in flight.
template <int SRC, int KIND, bool VEC>
__global__ void __launch_bounds__(kThreads) corpus_ingest_kernel(const EvdrIngestParams p) {
    constexpr int CH = KIND == EVDR_CORPUS_FP8 ? 16 : 8;
    constexpr int CPR = EVDR_D / CH;                                  // pieces per patch
    constexpr int UN = KIND == EVDR_CORPUS_FP8 ? 2 : 4;
    constexpr int EB = SRC == EVDR_F32 ? 4 : 2;                      // bytes per source element
    __shared__ uint32_t red[7][kThreads / 64];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t sp = blockIdx.x;                                    // source page
    // the destination is checked BEFORE it forms an address: an entry outside [0, capacity) is a hole, its page is skipped
    const int64_t dst = p.dst_pages ? (int64_t)p.dst_pages[sp] : p.first_page + sp;
    if (dst < 0 || dst >= p.capacity) return;                         // uniform over the workgroup: nobody waits at a barrier below
    const int lp = p.lp, lp_src = p.lp_src, d_src = p.d_src;
    const char* src = reinterpret_cast<const char*>(p.src) + sp * p.src_stride * EB;
    const uint8_t* mrow = p.pmask ? p.pmask + sp * lp_src : nullptr;

    // ---- mask: tile words and the quantities of the flag word, as pack_pmask_kernel; patches [lp_src, lp) are masked
    uint32_t first_masked = 0xFFFFu, first_valid = 0xFFFFu, end_valid = 0u, nvalid = 0u;
    const int ntiles = (lp + EVDR_TILE_PATCHES - 1) / EVDR_TILE_PATCHES;
    for (int t = tid; t < ntiles; t += kThreads) {
        uint32_t w = 0, inrange = 0;
        const int base = t * 32;
#pragma unroll 8
        for (int m = 0; m < 32; ++m) {
            const int i = base + m;
            if (i < lp) {
                inrange |= 1u << m;
                if (i < lp_src && (mrow == nullptr || mrow[i] != 0)) w |= 1u << m;
            }
        }
        p.tilemask[dst * ntiles + t] = w;
        nvalid += (uint32_t)__builtin_popcount(w);
        if (w) {
            first_valid = min(first_valid, (uint32_t)(base + __builtin_ctz(w)));
            end_valid = max(end_valid, (uint32_t)(base + 32 - __builtin_clz(w)));
        }
        const uint32_t masked = inrange & ~w;
        if (masked) first_masked = min(first_masked, (uint32_t)(base + __builtin_ctz(masked)));
    }

    auto load_piece = [&](uint32_t* v, int u) {
        const int row = u / CPR, col = (u % CPR) * CH;
        if (row < lp_src) {
            const char* r = src + (int64_t)row * d_src * EB;
#pragma unroll
            for (int o = 0; o < CH / 8; ++o) load_oct<SRC, VEC>(r, col + 8 * o, d_src, v + 8 * o);
        } else {
#pragma unroll
            for (int e = 0; e < CH; ++e) v[e] = 0u;
        }
    };

    // ---- fp8: the page's amax over all its rows as given, masked or not (quantize_fp8_kernel), then its shift
    int k8 = 0;
    if constexpr (KIND == EVDR_CORPUS_FP8) {
        uint32_t m = 0u;
        auto fold = [&](const uint32_t* v) {
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const uint32_t b = v[e] & 0x7FFFFFFFu;
                if (b < 0x7F800000u) m = max(m, b);                  // finite elements only: NaN / Inf never move amax
            }
        };
        const int total = lp_src * CPR;
        int u = tid;
        for (; u + (UN - 1) * kThreads < total; u += UN * kThreads) {
            uint32_t v[UN][CH];
#pragma unroll
            for (int j = 0; j < UN; ++j) load_piece(v[j], u + j * kThreads);
#pragma unroll
            for (int j = 0; j < UN; ++j) fold(v[j]);
        }
        for (; u < total; u += kThreads) {
            uint32_t v[CH];
            load_piece(v, u);
            fold(v);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
        if (lane == 0) red[6][wv] = m;
        __syncthreads();
        m = max(max(red[6][0], red[6][1]), max(red[6][2], red[6][3]));
        k8 = fp8_shift(m);
    }

    // ---- planes
    const int k2 = KIND == EVDR_CORPUS_F16_HILO ? evdr_h2_shift(*p.p_amax) : 0;
    bool bad = false;                                                 // a VALID patch holds NaN / +-Inf (evdr_flag_nonfinite)
    uint32_t amax = 0u;                                               // fp16 hi/lo: |x| bits of the largest finite element seen
    auto emit = [&](const uint32_t* v, int u) {
        const int row = u / CPR, col = (u % CPR) * CH;
        bool nonfinite = false;
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const uint32_t b = v[e] & 0x7FFFFFFFu;
            if (b >= 0x7F800000u) nonfinite = true;
            else if constexpr (KIND == EVDR_CORPUS_F16_HILO) amax = max(amax, b);
        }
        // rare path; only a source row can be non-finite (row < lp_src), the zero rows behind it are masked anyway
        if (nonfinite && !bad) bad = mrow == nullptr || mrow[row] != 0;
        const int64_t off = dst * p.p_stride + (int64_t)row * EVDR_D + col;
        store_piece<KIND>(p.planes, off, p.p_plane_stride, v, k2, k8);    // bf16 kind: SRC is bf16, v holds the elements' own bits
    };
    {
        const int total = lp * CPR;
        int u = tid;
        for (; u + (UN - 1) * kThreads < total; u += UN * kThreads) {
            uint32_t v[UN][CH];
#pragma unroll
            for (int j = 0; j < UN; ++j) load_piece(v[j], u + j * kThreads);
#pragma unroll
            for (int j = 0; j < UN; ++j) emit(v[j], u + j * kThreads);
        }
        for (; u < total; u += kThreads) {
            uint32_t v[CH];
            load_piece(v, u);
            emit(v, u);
        }
    }

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
        const uint32_t f = page_flag_word(nvalid, first_masked, first_valid, end_valid, badw);
        p.pageflags[dst] = f;
        if constexpr (KIND == EVDR_CORPUS_FP8) p.shift[dst] = k8;
        if constexpr (KIND == EVDR_CORPUS_F16_HILO) {
            // a finite element whose scaled exponent passes 2^15 leaves the window evdr_h2_shift promises: for a normal absmax word
            // that is an exponent field larger than the word's
            if (p.status != nullptr && (int)(amax >> 23) + k2 > 141) atomicOr(p.status, 1u);
        }
    }
}

template <int SRC, int KIND>
hipError_t launch(const EvdrIngestParams& p, bool vec, hipStream_t stream) {
    if (vec) hipLaunchKernelGGL((corpus_ingest_kernel<SRC, KIND, true>), dim3((unsigned)p.b), dim3(kThreads), 0, stream, p);
    else hipLaunchKernelGGL((corpus_ingest_kernel<SRC, KIND, false>), dim3((unsigned)p.b), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

template <int KIND>
hipError_t launch_src(const EvdrIngestParams& p, bool vec, hipStream_t stream) {
    if (p.src_dtype == EVDR_F32) return launch<EVDR_F32, KIND>(p, vec, stream);
    if (p.src_dtype == EVDR_BF16) return launch<EVDR_BF16, KIND>(p, vec, stream);
    return launch<EVDR_F16, KIND>(p, vec, stream);
}

}  // namespace

// arguments are the caller's to check (evdr_corpus_ingest does): kinds and dtypes valid, a bf16 corpus fed bf16 only, b >= 1
hipError_t evdr_launch_corpus_ingest(const EvdrIngestParams& p, hipStream_t stream) {
    const int64_t eb = p.src_dtype == EVDR_F32 ? 4 : 2;
    const bool vec = p.d_src % 8 == 0 && reinterpret_cast<uintptr_t>(p.src) % 16 == 0 && (p.src_stride * eb) % 16 == 0;
    if (p.kind == EVDR_CORPUS_BF16) return launch<EVDR_BF16, EVDR_CORPUS_BF16>(p, vec, stream);
    if (p.kind == EVDR_CORPUS_F16_HILO) return launch_src<EVDR_CORPUS_F16_HILO>(p, vec, stream);
    return launch_src<EVDR_CORPUS_FP8>(p, vec, stream);
}
