// The two pairwise ranking losses of criterion.py (pairwise_distillation_loss: RankNet, lambda_loss: LambdaLoss pairs), each with its
// gradient in ONE launch and O(B * N) memory.  The torch form materialises several (B, N, N) fp32 tensors.
//
// Geometry (both kernels): a workgroup of four waves owns PL_TILE = 64 consecutive i of one row (lane = i) and the whole j range of that
// row, cut into four contiguous quarters, one per wave.  The j loop is wave-uniform, so a row's j values arrive as scalar loads (one
// value for all 64 lanes, no LDS staging, no barrier inside the loop).  Each lane keeps its gradient partial (fp32) and its loss partial
// (fp64: the loss is a sum of up to N * N terms of one sign; fp32 accumulation alone would cost ~N/4 * 2^-24 relative) in ascending j.
// The four waves' partials meet in LDS and are added in wave order; the workgroup's loss partial goes to the workspace and the workgroup
// that draws the last ticket adds all partials in index order.  No floating-point atomics anywhere: the same bits every launch, and a
// row's gradient depends on that row alone.
//
// Range: every transcendental is taken of -|x| (e = exp(-|x|) in [0, 1], 1 / (1 + e), log1p(e)), so margins of +-1e4 (the scorer's fill
// value for masked pages), pairs of two fill values (margin 0, target 0.5) and rows wider than fp32's exp range are ordinary inputs.
#include "evdr_common.h"

namespace {

constexpr int PL_TILE = EVDR_PAIR_TILE;   // i per workgroup = lanes of a wave
static_assert(PL_TILE == 64, "one i per lane of a wave");
constexpr int PL_WAVES = 4;          // j quarters per workgroup
constexpr int PL_THREADS = PL_TILE * PL_WAVES;
constexpr float PL_LOG2E = 1.44269504088896340736f;
constexpr float PL_LN2 = 0.69314718055994530942f;

// e = exp(-|x|): 0 < e <= 1, flushes to 0 below fp32's range (then sigmoid and softplus below are exact limits)
__device__ __forceinline__ float pl_exp_neg_abs(float x) { return __builtin_amdgcn_exp2f(-PL_LOG2E * __builtin_fabsf(x)); }

// log(1 + e) for 0 <= e <= 1.  1 + e rounds away up to 2^-24 of e, which is all of e when e is small: below 2^-6 the alternating
// series through e^4 (truncation < e^4 / 5 < 2^-26 relative) takes over.
__device__ __forceinline__ float pl_log1p_unit(float e) {
    const float big = PL_LN2 * __builtin_amdgcn_logf(1.f + e);
    const float small = e * (1.f + e * (-0.5f + e * (0.33333334f + e * -0.25f)));
    return e < 0.015625f ? small : big;
}

// sum over the wave's 64 lanes, fixed butterfly order (every lane gets the sum)
__device__ __forceinline__ double pl_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Common tail: the four waves' partials in wave order, gradient store, workgroup loss partial, last-ticket total.
// part: (gridDim.x * gridDim.y) doubles; ticket: zero before the first launch, left zero by every launch.
__device__ __forceinline__ void pl_finish(float g, double l, bool live, float gscale, double lscale, float* __restrict__ grad_row, int i,
                                          double* __restrict__ part, unsigned int* __restrict__ ticket, float* __restrict__ loss) {
    __shared__ float gred[PL_WAVES][PL_TILE];
    __shared__ double lred[PL_WAVES];
    __shared__ int is_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    l = pl_wave_sum(live ? l : 0.0);
    gred[wave][lane] = g;
    if (lane == 0) lred[wave] = l;
    __syncthreads();
    if (wave == 0 && live && grad_row != nullptr) grad_row[i] = gscale * (((gred[0][lane] + gred[1][lane]) + gred[2][lane]) + gred[3][lane]);
    const unsigned int nwg = gridDim.x * gridDim.y;
    if (tid == 0) {
        part[blockIdx.y * gridDim.x + blockIdx.x] = ((lred[0] + lred[1]) + lred[2]) + lred[3];
        __threadfence();
        is_last = (atomicAdd(ticket, 1u) == nwg - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    const volatile double* p = part;                  // written by other CUs: read past this CU's vector L1
    double v = 0.0;
    for (unsigned int k = tid; k < nwg; k += PL_THREADS) v += p[k];
    v = pl_wave_sum(v);
    __syncthreads();                                  // lred is read above by tid 0 only, which is past it here
    if (lane == 0) lred[wave] = v;
    __syncthreads();
    if (tid == 0) {
        loss[0] = (float)((((lred[0] + lred[1]) + lred[2]) + lred[3]) * lscale);
        *ticket = 0u;                                 // ready for the next call
    }
}

// j range of this wave: quarter `wave` of [0, n), the quarters being ceil(n / 4) long (the last ones may be short or empty)
__device__ __forceinline__ void pl_j_range(int n, int& j0, int& j1) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = (n + PL_WAVES - 1) / PL_WAVES;
    j0 = wave * q < n ? wave * q : n;
    j1 = j0 + q < n ? j0 + q : n;
}

// RankNet: term(i, j) = softplus(m) - y * m, d term / d m = sigmoid(m) - y, with m = s_i - s_j, y = sigmoid(t_i - t_j).
// With q = min(y, 1 - y) = e_d / (1 + e_d) (relatively accurate where y is near 0 or 1) and m' = m where y < 1/2, -m where y >= 1/2:
// term = softplus(m') - q * m'  (softplus(m) - m = softplus(-m)), which never forms (1 - y) * m from a rounded y.
__global__ void __launch_bounds__(PL_THREADS) pairwise_distill_kernel(const float* __restrict__ ss, const float* __restrict__ st, int n,
                                                                      float gscale, double lscale, float* __restrict__ grad,
                                                                      double* __restrict__ part, unsigned int* __restrict__ ticket,
                                                                      float* __restrict__ loss) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * PL_TILE + lane;
    const bool live = i < n;
    const int ic = live ? i : n - 1;                  // idle lanes of the last tile compute a real element and drop it
    const float* __restrict__ s = ss + (int64_t)blockIdx.y * n;
    const float* __restrict__ t = st + (int64_t)blockIdx.y * n;
    const float si = s[ic], ti = t[ic];
    int j0, j1;
    pl_j_range(n, j0, j1);
    float g = 0.f;
    double l = 0.0;
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const float m = si - s[j];
        const float d = ti - t[j];
        const float em = pl_exp_neg_abs(m), ed = pl_exp_neg_abs(d);
        const float rm = __builtin_amdgcn_rcpf(1.f + em), rd = __builtin_amdgcn_rcpf(1.f + ed);
        const float pm = em * rm, q = ed * rd;        // the smaller of sigmoid(+-m), sigmoid(+-d)
        const bool up = d >= 0.f;                     // y >= 1/2
        const float mp = up ? -m : m;
        const float term = (fmaxf(mp, 0.f) + pl_log1p_unit(em)) - q * mp;
        const float sig = m >= 0.f ? 1.f - pm : pm;
        const float y = up ? 1.f - q : q;
        g += sig - y;
        l += (double)term;
    }
    pl_finish(g, l, live, gscale, lscale, grad != nullptr ? grad + (int64_t)blockIdx.y * n : nullptr, i, part, ticket, loss);
}

// LambdaLoss pairs in the teacher's order: term(i < j) = w_ij * softplus(-alpha (s_i - s_j)), w_ij = 10 |gain_i - gain_j| |disc_i - disc_j|.
// Element i collects -alpha w sigmoid(-alpha (s_i - s_j)) from every j > i and +alpha w sigmoid(alpha (s_i - s_j)) from every j < i: with
// z = -+alpha (s_i - s_j) (j > i / j < i) both are -+alpha w sigmoid(z); the loss counts j > i only.  w_ii = 0.
__global__ void __launch_bounds__(PL_THREADS) lambda_pairs_kernel(const float* __restrict__ ss, const float* __restrict__ gain,
                                                                  const float* __restrict__ disc, int n, float alpha, float gscale,
                                                                  double lscale, float* __restrict__ grad, double* __restrict__ part,
                                                                  unsigned int* __restrict__ ticket, float* __restrict__ loss) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * PL_TILE + lane;
    const bool live = i < n;
    const int ic = live ? i : n - 1;
    const float* __restrict__ s = ss + (int64_t)blockIdx.y * n;
    const float* __restrict__ gn = gain + (int64_t)blockIdx.y * n;
    const float si = s[ic], gi = gn[ic], di = disc[ic];
    int j0, j1;
    pl_j_range(n, j0, j1);
    float g = 0.f;
    double l = 0.0;
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const float w = (__builtin_fabsf(gi - gn[j]) * __builtin_fabsf(di - disc[j])) * 10.f;
        const bool later = j > ic;
        const float x = alpha * (si - s[j]);
        const float z = later ? -x : x;
        const float e = pl_exp_neg_abs(z);
        const float r = __builtin_amdgcn_rcpf(1.f + e);
        const float sig = z >= 0.f ? r : e * r;
        const float sp = fmaxf(z, 0.f) + pl_log1p_unit(e);
        const float c = w * sig;
        g += later ? -c : c;
        l += later ? (double)(w * sp) : 0.0;
    }
    pl_finish(g, l, live, gscale * alpha, lscale, grad != nullptr ? grad + (int64_t)blockIdx.y * n : nullptr, i, part, ticket, loss);
}

}  // namespace

hipError_t evdr_launch_pairwise_distill(const float* ss, const float* st, int64_t b, int64_t n, float* loss, float* grad, double* part,
                                        unsigned int* ticket, hipStream_t stream) {
    const double pairs = (double)b * (double)n * (double)n;
    dim3 grid((unsigned)((n + PL_TILE - 1) / PL_TILE), (unsigned)b);
    hipLaunchKernelGGL(pairwise_distill_kernel, grid, dim3(PL_THREADS), 0, stream, ss, st, (int)n, (float)(2.0 / pairs), 1.0 / pairs, grad,
                       part, ticket, loss);
    return hipGetLastError();
}

hipError_t evdr_launch_lambda_pairs(const float* ss, const float* gain, const float* disc, int64_t b, int64_t n, float alpha, float eps,
                                    float* loss, float* grad, double* part, unsigned int* ticket, hipStream_t stream) {
    const double denom = (double)n * (double)(n - 1) / 2.0 + (double)eps;
    dim3 grid((unsigned)((n + PL_TILE - 1) / PL_TILE), (unsigned)b);
    hipLaunchKernelGGL(lambda_pairs_kernel, grid, dim3(PL_THREADS), 0, stream, ss, gain, disc, (int)n, alpha, (float)(1.0 / denom),
                       1.0 / denom, grad, part, ticket, loss);
    return hipGetLastError();
}
