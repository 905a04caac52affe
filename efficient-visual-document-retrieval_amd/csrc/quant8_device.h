// Device helpers of the e4m3fn quantiser, shared by csrc/quant8.hip (whole tensors) and csrc/ingest.hip (pages written in place).
#pragma once
#include <stdint.h>

// k from the bits of a finite, non-negative amax; integer arithmetic only (subnormal amax included)
__device__ __forceinline__ int fp8_shift(uint32_t amax_bits) {
    if (amax_bits == 0u) return 0;
    const uint32_t e8 = amax_bits >> 23, mant = amax_bits & 0x7FFFFFu;
    int e;                          // amax = m * 2^e, m in [1, 2)
    bool small_m;                   // m <= 1.75, i.e. 448 = 1.75 * 2^8 is reached at 2^(8 - e)
    if (e8 == 0u) {
        const int msb = 31 - __builtin_clz(mant);
        e = msb - 149;
        small_m = 4ull * mant <= (7ull << msb);
    } else {
        e = (int)e8 - 127;
        small_m = mant <= 0x600000u;
    }
    return small_m ? 8 - e : 7 - e;
}

__device__ __forceinline__ uint32_t e4m3_byte(uint32_t xbits, int k) {
    const uint32_t sign = xbits & 0x80000000u;
    if ((xbits & 0x7F800000u) == 0x7F800000u) return 0x7Fu | (sign >> 24);          // NaN / +-Inf -> NaN
    uint32_t f = __builtin_bit_cast(uint32_t, __builtin_amdgcn_ldexpf(__builtin_bit_cast(float, xbits), k)) ^ sign;
    uint32_t r;
    if (f >= (1087u << 20)) {                       // >= 464: NaN (not reached: |x| 2^k <= 448)
        r = 0x7Fu;
    } else if (f < (121u << 23)) {                  // below 2^-6: e4m3 subnormal, rounded by an fp32 addition (RNE)
        const uint32_t denorm = 141u << 23;
        const float t = __builtin_bit_cast(float, f) + __builtin_bit_cast(float, denorm);
        r = (__builtin_bit_cast(uint32_t, t) - denorm) & 0xFFu;
    } else {
        const uint32_t odd = (f >> 20) & 1u;
        f += (uint32_t)(7 - 127) * (1u << 23) + 0x7FFFFu;
        f += odd;
        r = (f >> 20) & 0xFFu;
    }
    return r | (sign >> 24);
}
