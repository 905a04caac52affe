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
//
// Two kernel templates share the body (maxsim_fwd8_body.inc): maxsim_fwd8_kernel over the whole corpus and maxsim_fwd8_pages_kernel
// over ONE page list shared by the batch (evdr_maxsim_fwd_fp8_pages).
#include <stdio.h>

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
    constexpr bool PAGES = false;
#include "maxsim_fwd8_body.inc"
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

// page-list instances (evdr_maxsim_fwd_fp8_pages): p.g.gather = ONE list of p.g.np corpus pages shared by the whole batch,
// p.g.ncorpus = pages of the corpus, in the exhaustive launch's geometry over the list positions -- query groups x chunks of list
// positions, every wave scoring its own QW queries -- writing out[q * out_stride + i].  The body is shared with
// maxsim_fwd8_kernel, whose symbols and instruction streams stay what they were; the per-pair arithmetic is the instance's own.
template <int QW, int ST, int NSTAGE>
__global__ void __launch_bounds__(WAVES8 * 64, 1) maxsim_fwd8_pages_kernel(const EvdrFwd8Params p8) {
    constexpr bool PAGES = true;
#include "maxsim_fwd8_body.inc"
}

template <int QW, int ST, int NSTAGE>
hipError_t launch_fwd8_pages(EvdrFwd8Params p8, hipStream_t stream) {
    constexpr int G = (4 * (ST + 1) + WAVES8 - 1) / WAVES8;
    constexpr int LDS = NSTAGE * G * WAVES8 * 1024;
    static_assert(LDS <= 160 * 1024, "ring exceeds the LDS");
    const int64_t grid = evdr_set_geometry(p8.g, WAVES8 * QW);         // p.np = list length: chunks of list positions
    static std::atomic<uint64_t> lds_done{0};
    const void* kern = reinterpret_cast<const void*>(&maxsim_fwd8_pages_kernel<QW, ST, NSTAGE>);
    hipError_t e = evdr_ensure_dyn_lds(kern, LDS, lds_done);
    if (e != hipSuccess) return e;
    static const char* const name = [] {
        static char buf[64];
        snprintf(buf, sizeof(buf), "maxsim_fwd8_pages_kernel<%d,%d,%d>", QW, ST, NSTAGE);
        return (const char*)buf;
    }();
    evdr_note_fwd_kernel(name);
    hipLaunchKernelGGL((maxsim_fwd8_pages_kernel<QW, ST, NSTAGE>), dim3((unsigned)grid), dim3(WAVES8 * 64), LDS, stream, p8);
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

// The page-list form: the instance is chosen by evdr_launch_maxsim_fwd8's rule from nq and ntiles (NOT from the list length), so a
// page-list launch and an exhaustive launch of one query batch chain the same MFMAs and the same fold per (query, page, token).
hipError_t evdr_launch_maxsim_fwd8_pages(const EvdrFwd8Params& p8_in, hipStream_t stream) {
    EvdrFwd8Params p8 = p8_in;
    p8.g.ntiles = (p8.g.lp + EVDR_TILE_PATCHES - 1) / EVDR_TILE_PATCHES;
    const int nq = p8.g.nq;
    if (p8.g.ntiles >= 8) {
        if (nq > 256) return launch_fwd8_pages<8, 11, 3>(p8, stream);
        if (nq > 8) return launch_fwd8_pages<4, 11, 3>(p8, stream);
        return launch_fwd8_pages<1, 11, 3>(p8, stream);
    }
    if (nq > 8) return launch_fwd8_pages<4, 2, 4>(p8, stream);
    return launch_fwd8_pages<1, 2, 4>(p8, stream);
}
