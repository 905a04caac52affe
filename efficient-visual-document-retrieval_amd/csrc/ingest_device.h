// Device helpers shared by csrc/ingest.hip (pages copied in place) and csrc/pool.hip (pages pooled in place): how a source octet is
// read, how a piece of a page is written in each corpus kind, and how a page's flag word is put together.  One definition each, so
// that a pooled page has bit for bit the planes and words the ingest kernel writes for the same values.
#pragma once
#include "evdr_common.h"
#include "quant8_device.h"

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

__device__ __forceinline__ uint32_t f16_to_f32_bits(uint32_t h) {
    const float f = (float)__builtin_bit_cast(_Float16, (uint16_t)h);      // exact
    return __builtin_bit_cast(uint32_t, f);
}

// Eight consecutive source elements, columns [col, col + 8) of the row at `row`, as fp32 bit patterns (bf16 and fp16 convert
// exactly); columns >= d_src read as zero.  VEC: d_src is a multiple of 8 and every row is 16-byte aligned, so an octet lies
// wholly inside or wholly outside the row and is fetched by one (two for fp32) 16-byte load.
template <int SRC, bool VEC>
__device__ __forceinline__ void load_oct(const char* row, int col, int d_src, uint32_t* v) {
    if constexpr (VEC) {
        if (col >= d_src) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0u;
            return;
        }
        if constexpr (SRC == EVDR_F32) {
            const uint4 a = *reinterpret_cast<const uint4*>(row + (int64_t)col * 4);
            const uint4 b = *reinterpret_cast<const uint4*>(row + (int64_t)col * 4 + 16);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
            v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
            const uint4 a = *reinterpret_cast<const uint4*>(row + (int64_t)col * 2);
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (SRC == EVDR_BF16) {
                    v[2 * j] = w[j] << 16;
                    v[2 * j + 1] = w[j] & 0xFFFF0000u;
                } else {
                    v[2 * j] = f16_to_f32_bits(w[j] & 0xFFFFu);
                    v[2 * j + 1] = f16_to_f32_bits(w[j] >> 16);
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = col + j;
            uint32_t b = 0u;
            if (c < d_src) {
                if constexpr (SRC == EVDR_F32) b = reinterpret_cast<const uint32_t*>(row)[c];
                else if constexpr (SRC == EVDR_BF16) b = (uint32_t)reinterpret_cast<const uint16_t*>(row)[c] << 16;
                else b = f16_to_f32_bits(reinterpret_cast<const uint16_t*>(row)[c]);
            }
            v[j] = b;
        }
    }
}

// One 16-byte store's worth of a page (8 columns, 16 for fp8) at element offset `off` of the planes, from fp32 bit patterns:
// EVDR_CORPUS_BF16: v holds bf16 values (their bits in the high halves); EVDR_CORPUS_F16_HILO: split_h2_kernel's arithmetic under
// the shift k2 of the corpus's absmax word; EVDR_CORPUS_FP8: quantize_fp8_kernel's bytes under the page's shift k8.
template <int KIND>
__device__ __forceinline__ void store_piece(void* planes, int64_t off, int64_t p_plane_stride, const uint32_t* v, int k2, int k8) {
    if constexpr (KIND == EVDR_CORPUS_BF16) {
        uint4 o;
        o.x = (v[0] >> 16) | (v[1] & 0xFFFF0000u);
        o.y = (v[2] >> 16) | (v[3] & 0xFFFF0000u);
        o.z = (v[4] >> 16) | (v[5] & 0xFFFF0000u);
        o.w = (v[6] >> 16) | (v[7] & 0xFFFF0000u);
        *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(planes) + off) = o;
    } else if constexpr (KIND == EVDR_CORPUS_F16_HILO) {
        f16x8 a, b;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = __builtin_ldexpf(__builtin_bit_cast(float, v[j]), k2);    // exact
            const _Float16 h = (_Float16)f;                                            // RNE
            a[j] = h;
            b[j] = (_Float16)(f - (float)h);                                           // the difference is exact in fp32
        }
        _Float16* hi = reinterpret_cast<_Float16*>(planes) + off;
        *reinterpret_cast<f16x8*>(hi) = a;
        *reinterpret_cast<f16x8*>(hi + p_plane_stride) = b;
    } else {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            w[q] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[q] |= e4m3_byte(v[4 * q + e], k8) << (8 * e);
        }
        *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(planes) + off) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// The flag word of pack_pmask_kernel from the page's mask quantities (first_masked / first_valid = 0xFFFF when there is none), with
// bit 3 by the rule of evdr_flag_nonfinite.
__device__ __forceinline__ uint32_t page_flag_word(uint32_t nvalid, uint32_t first_masked, uint32_t first_valid, uint32_t end_valid,
                                                   uint32_t bad) {
    uint32_t f = (nvalid ? 1u : 0u);
    if (first_masked != 0xFFFFu) f |= 2u;
    const uint32_t va = nvalid ? first_valid : 0u, vb = nvalid ? end_valid : 0u;           // the one-range encoding of pack_pmask_kernel
    if (nvalid == vb - va && va < 4096u) f |= 4u | (va << 4) | (vb << 16);
    else f |= (first_masked == 0xFFFFu ? 0u : first_masked) << 16;
    if (bad) f |= 8u;
    return f;
}
