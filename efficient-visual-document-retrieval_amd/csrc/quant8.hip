// fp32 / bf16 -> OCP e4m3fn bytes with one power-of-two shift per group of rows (include/evdr.h "fp8 corpora").
//
// Group = one page or one query.  k = the largest integer with amax * 2^k <= 448 (the e4m3fn maximum), amax = max |x| over the
// group's FINITE elements (k = 0 when there is no finite non-zero element).  Each element becomes the round-to-nearest-even
// e4m3fn byte of x * 2^k, subnormals included; columns d..127 are zero; NaN and +-Inf become the NaN byte 0x7F with the
// element's sign.  The bytes are those of torch's (x.float() * 2.0**k).to(torch.float8_e4m3fn): the conversion below is
// c10's fp8e4m3fn_from_fp32_value step for step, and x * 2^k is formed by one exact ldexp (torch's product by the power of two
// rounds once too, and the same way).
#include "evdr_common.h"
#include "quant8_device.h"

namespace {

constexpr int kQThreads = 256;

__device__ __forceinline__ uint32_t load_bits(const void* x, int dtype, int64_t i) {
    if (dtype == EVDR_BF16) return (uint32_t)reinterpret_cast<const uint16_t*>(x)[i] << 16;
    return reinterpret_cast<const uint32_t*>(x)[i];
}

// one workgroup per group: absmax pass, then one output word (4 columns) per thread and step
__global__ void __launch_bounds__(kQThreads) quantize_fp8_kernel(const void* x, int dtype, int64_t rpg, int d, uint8_t* x8,
                                                                  int32_t* shift) {
    __shared__ uint32_t red[kQThreads / 64];
    const int64_t grp = blockIdx.x;
    const int64_t r0 = grp * rpg;
    const int64_t n = rpg * d;
    uint32_t m = 0u;
    for (int64_t i = threadIdx.x; i < n; i += kQThreads) {
        const uint32_t b = load_bits(x, dtype, r0 * d + i) & 0x7FFFFFFFu;
        if (b < 0x7F800000u) m = max(m, b);              // finite elements only: NaN / Inf never move amax
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    const int k = fp8_shift(m);
    const int64_t words = rpg * (EVDR_D / 4);
    for (int64_t w = threadIdx.x; w < words; w += kQThreads) {
        const int64_t row = w >> 5;
        const int col = (int)(w & 31) * 4;
        uint32_t word = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (col + e < d) word |= e4m3_byte(load_bits(x, dtype, (r0 + row) * d + col + e), k) << (8 * e);
        *reinterpret_cast<uint32_t*>(x8 + (r0 + row) * EVDR_D + col) = word;
    }
    if (threadIdx.x == 0) shift[grp] = k;
}

}  // namespace

hipError_t evdr_launch_quantize_fp8(const void* x, int dtype, int64_t groups, int64_t rows_per_group, int64_t d, uint8_t* x8,
                                    int32_t* shift, hipStream_t stream) {
    if (groups == 0) return hipSuccess;
    hipLaunchKernelGGL(quantize_fp8_kernel, dim3((unsigned)groups), dim3(kQThreads), 0, stream, x, dtype, rows_per_group, (int)d,
                       x8, shift);
    return hipGetLastError();
}
