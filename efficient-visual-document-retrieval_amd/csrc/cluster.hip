// On-device token clustering: every page's valid patches grouped into at most ls groups by spherical k-means, emitted as the per-page
// CSR grouping the pooling kernels take (the rule: include/evdr.h "token clustering").
//
// One 256-thread workgroup owns a page from the start labels to the final lists (a capped grid walks its pages), so all iterations
// run inside ONE launch with workgroup barriers between the phases:
//   csr     labels -> members / offsets, written straight into the caller's output rows (the last build is the result).  The thread
//           of group j counts the labels below j (its offset), then walks the labels again and places its patches: ascending order
//           by construction, no atomics, no scan across threads.  The label reads are wave-uniform, four labels per load.
//   update  the centroid of a group = csrc/pool.hip's pooled token of its list: a team of 16 threads, 8 columns each, members added in
//           list order from +0.0f, correctly rounded divide, x / (||x|| + 1e-12) with the octet / pair-tree sum of squares.  A live
//           group without a member keeps its centroid.
//   assign  walks the members list, i.e. the valid patches only.  Four lanes share a patch, a quarter of the row (4 octets) each, and
//           a lane holds its quarter of FOUR patches in registers: a centroid value read once serves four patches, which keeps the
//           centroid reads (LDS for ls <= EVDR_CLUSTER_LDS_GROUPS, else the workgroup's slice of the workspace) at a quarter of what
//           the multiplies could consume.  16 independent chains of separately rounded multiply and add per lane; the pair tree's
//           first two levels inside the lane, the last two by DPP inside the quad (a + b and b + a are the same bits); the compare
//           is made on the ORDER of the bit patterns (the build assumes no NaNs: a float compare is not to be trusted with one).
// Labels (4 B per patch) and, for ls > EVDR_CLUSTER_LDS_GROUPS, the centroids live in the workgroup's slice of the workspace, whose
// size depends on the grid cap and never on the number of pages.
#include "ingest_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTeam = EVDR_D / 8;                                     // threads per centroid in the update
constexpr int kQP = 4;                                                // patches per lane in the assign

// separately rounded fp32 operations: no contraction of a multiply and an add into an FMA, whatever -ffp-contract says
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// a signed key that orders non-NaN floats as `<` does, -0.0f and +0.0f being equal
__device__ __forceinline__ int32_t order_key(uint32_t b) {
    if (b == 0x80000000u) b = 0u;
    const int32_t k = (int32_t)b;
    return k ^ ((k >> 31) & 0x7FFFFFFF);
}

// v of lane ^ 1 / lane ^ 2 (quad_perm [1,0,3,2] / [2,3,0,1]); every lane of the wave is active where these are used
__device__ __forceinline__ float quad_xor1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ float quad_xor2(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
}

// labels -> lists.  lab is read-only here and disjoint from mem / offs, which is what lets the label loads run ahead of the stores
__device__ __forceinline__ void build_lists(const int32_t* __restrict__ lab, int32_t* __restrict__ mem, int32_t* __restrict__ offs,
                                            int lp_src, int ls, int g, int nv, int tid) {
    const int lp4 = lp_src & ~3;                                      // the label row is 16-byte aligned
    for (int j = tid; j < g; j += kThreads) {
        int lt = 0;
        for (int p = 0; p < lp4; p += 4) {
            const int4 l = *reinterpret_cast<const int4*>(lab + p);
            lt += ((unsigned)l.x < (unsigned)j ? 1 : 0) + ((unsigned)l.y < (unsigned)j ? 1 : 0) + ((unsigned)l.z < (unsigned)j ? 1 : 0) +
                  ((unsigned)l.w < (unsigned)j ? 1 : 0);
        }
        for (int p = lp4; p < lp_src; ++p) lt += (unsigned)lab[p] < (unsigned)j ? 1 : 0;
        offs[j] = lt;
        int pos = lt;
        auto place = [&](int l, int p) {
            if (l == j && pos < lp_src) mem[pos++] = p;               // pos < nv by construction; the test keeps a store inside the row
        };
        for (int p = 0; p < lp4; p += 4) {
            const int4 l = *reinterpret_cast<const int4*>(lab + p);
            place(l.x, p);
            place(l.y, p + 1);
            place(l.z, p + 2);
            place(l.w, p + 3);
        }
        for (int p = lp4; p < lp_src; ++p) place(lab[p], p);
    }
    for (int j = g + tid; j <= ls; j += kThreads) offs[j] = nv;       // groups >= g stay empty behind the last live one
    for (int p = nv + tid; p < lp_src; p += kThreads) mem[p] = -1;    // holes behind offsets[ls]
}

template <int SRC, bool VEC, bool LDS_CENT>
__global__ void __launch_bounds__(kThreads) cluster_pages_kernel(const EvdrClusterParams q) {
    constexpr int EB = SRC == EVDR_F32 ? 4 : 2;                      // bytes per source element
    extern __shared__ __attribute__((aligned(16))) char smem[];       // [ls x 128 fp32 centroids (LDS_CENT)] [4 wave sums]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lp_src = q.lp_src, d_src = q.d_src, ls = q.ls;
    char* slice = reinterpret_cast<char*>(q.workspace) + (int64_t)blockIdx.x * q.slice_bytes;
    int32_t* lab = reinterpret_cast<int32_t*>(slice);
    float* cent = LDS_CENT ? reinterpret_cast<float*>(smem) : reinterpret_cast<float*>(slice + q.cent_off);
    int* wsum = reinterpret_cast<int*>(smem + (LDS_CENT ? (size_t)ls * EVDR_D * 4 : 0));

    for (int64_t page = blockIdx.x; page < q.b; page += gridDim.x) {
        const char* src = reinterpret_cast<const char*>(q.src) + page * q.src_stride * EB;
        const uint8_t* mrow = q.pmask ? q.pmask + page * lp_src : nullptr;
        int32_t* mem = q.members + page * lp_src;
        int32_t* offs = q.offsets + page * (ls + 1);
        auto valid = [&](int p) { return mrow == nullptr || mrow[p] != 0; };

        // ---- nv, the number of valid patches
        int nv = 0;
        for (int p = tid; p < lp_src; p += kThreads) nv += valid(p) ? 1 : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) nv += __shfl_xor(nv, o);
        __syncthreads();                                              // the previous page's readers of wsum and lab are done
        if (lane == 0) wsum[wv] = nv;
        __syncthreads();
        nv = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        const int g = min(ls, nv);                                    // live groups

        // ---- start: valid patch number i gets label floor(i * g / nv); masked patches -1
        int before = 0;                                               // valid patches in front of this chunk
        for (int c = 0; c < lp_src; c += kThreads) {
            const int p = c + tid;
            const bool v = p < lp_src && valid(p);
            const uint64_t bal = __ballot(v);
            __syncthreads();
            if (lane == 0) wsum[wv] = __builtin_popcountll(bal);
            __syncthreads();
            int i = before + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
            for (int w = 0; w < wv; ++w) i += wsum[w];
            if (p < lp_src) lab[p] = v ? i * g / max(nv, 1) : -1;     // i * g < 65535 * 4096
            before += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        }
        __syncthreads();

        for (int it = 0;; ++it) {
            // ---- csr: offsets[j] = labels in [0, j); group j's patches ascending behind it; slots behind offsets[ls] = nv are holes
            build_lists(lab, mem, offs, lp_src, ls, g, nv, tid);
            __syncthreads();
            if (it == q.iters) break;

            // ---- update: the pooled token (normalize = 1) of every live group's list, as corpus_pool_ingest_kernel forms it
            for (int base = 0; base < g * kTeam; base += kThreads) {
                const int u = base + tid, row = u / kTeam, col = (u % kTeam) * 8;
                float acc[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
                int cnt = 0;
                if (row < g) {
                    const int beg = offs[row], end = offs[row + 1];
                    for (int j = beg; j < end; j += 4) {
                        uint32_t w[4][8];
                        bool ok[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int idx = j + k < end ? mem[j + k] : -1;
                            ok[k] = (unsigned)idx < (unsigned)lp_src;
                            if (ok[k]) {
                                load_oct<SRC, VEC>(src + (int64_t)idx * d_src * EB, col, d_src, w[k]);
                            } else {
#pragma unroll
                                for (int e = 0; e < 8; ++e) w[k][e] = 0u;
                            }
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k) {                 // list order
                            if (ok[k]) {
#pragma unroll
                                for (int e = 0; e < 8; ++e) acc[e] = add_rn(acc[e], __builtin_bit_cast(float, w[k][e]));
                                ++cnt;
                            }
                        }
                    }
                }
                if (cnt > 0) {
                    const float c = (float)cnt;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = acc[e] / c;  // correctly rounded (the compiler's default for HIP)
                }
                float t = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; ++e) t = add_rn(t, mul_rn(acc[e], acc[e]));
#pragma unroll
                for (int o = 1; o < kTeam; o <<= 1) t = add_rn(t, __shfl_xor(t, o));    // adjacent pairs, then pairs of those
                const float den = add_rn(__builtin_sqrtf(t), 1e-12f);
                if (cnt > 0) {                                        // an emptied group keeps the centroid it had
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = col + e < d_src ? acc[e] / den : 0.0f;
                    float4* o = reinterpret_cast<float4*>(cent + row * EVDR_D + col);
                    o[0] = make_float4(v[0], v[1], v[2], v[3]);
                    o[1] = make_float4(v[4], v[5], v[6], v[7]);
                }
            }
            __syncthreads();

            // ---- assign: the lowest live group with the largest non-NaN score; none above -inf -> group 0.  Lane = (slot, quarter):
            // a wave takes 64 list positions at a time, slot s the positions t0 + s + 16 * i
            const int qr = lane & 3, slot = lane >> 2;
            for (int t0 = wv * 64; t0 < nv; t0 += kThreads) {         // wave-uniform
                int pidx[kQP];
                float x[kQP][32];
                // the width as a per-lane value the compiler cannot see through: the column tests of the rows are then vector
                // compares made here, not wave-uniform masks held in scalar registers across the loops
                int dv = d_src;
                asm volatile("" : "+v"(dv));
#pragma unroll
                for (int i = 0; i < kQP; ++i) {
                    const int t = t0 + 16 * i + slot;
                    const int idx = t < nv ? mem[t] : -1;
                    pidx[i] = (unsigned)idx < (unsigned)lp_src ? idx : -1;
                    const char* r = src + (int64_t)max(pidx[i], 0) * d_src * EB;
#pragma unroll
                    for (int o = 0; o < 4; ++o) {
                        uint32_t w[8];
                        load_oct<SRC, VEC>(r, 32 * qr + 8 * o, dv, w);
#pragma unroll
                        for (int e = 0; e < 8; ++e) x[i][8 * o + e] = __builtin_bit_cast(float, w[e]);
                    }
                }
                int32_t best[kQP];
                int label[kQP];
#pragma unroll
                for (int i = 0; i < kQP; ++i) {
                    best[i] = order_key(0xFF800000u);
                    label[i] = 0;
                }
                for (int j = 0; j < g; ++j) {
                    const float4* c4 = reinterpret_cast<const float4*>(cent + j * EVDR_D + 32 * qr);
                    float c[32];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float4 v = c4[k];
                        c[4 * k] = v.x; c[4 * k + 1] = v.y; c[4 * k + 2] = v.z; c[4 * k + 3] = v.w;
                    }
#pragma unroll
                    for (int i = 0; i < kQP; ++i) {
                        float s[4];
#pragma unroll
                        for (int o = 0; o < 4; ++o) {                 // the lane's octets 4 * qr + o, each summed ascending from +0.0f
                            float a = 0.0f;
#pragma unroll
                            for (int e = 0; e < 8; ++e) a = add_rn(a, mul_rn(x[i][8 * o + e], c[8 * o + e]));
                            s[o] = a;
                        }
                        float v = add_rn(add_rn(s[0], s[1]), add_rn(s[2], s[3]));       // tree levels 1 and 2: the quarter's sum
                        v = add_rn(v, quad_xor1(v));                                  // level 3: quarters 0 + 1, 2 + 3
                        v = add_rn(v, quad_xor2(v));                                  // level 4
                        const uint32_t sb = __builtin_bit_cast(uint32_t, v);
                        const int32_t key = order_key(sb);
                        if ((sb & 0x7FFFFFFFu) <= 0x7F800000u && key > best[i]) {
                            best[i] = key;
                            label[i] = j;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < kQP; ++i)
                    if (qr == 0 && pidx[i] >= 0) lab[pidx[i]] = label[i];
            }
            __syncthreads();
        }

        if (q.labels != nullptr)
            for (int p = tid; p < lp_src; p += kThreads) q.labels[page * lp_src + p] = lab[p];
    }
}

template <int SRC, bool VEC, bool LDS_CENT>
hipError_t launch(const EvdrClusterParams& p, unsigned grid, hipStream_t stream) {
    auto kern = cluster_pages_kernel<SRC, VEC, LDS_CENT>;
    const int lds = (LDS_CENT ? p.ls * EVDR_D * 4 : 0) + 16;
    static std::atomic<uint64_t> attr_devs{0};
    if (hipError_t e = evdr_ensure_dyn_lds((const void*)kern, (LDS_CENT ? EVDR_CLUSTER_LDS_GROUPS * EVDR_D * 4 : 0) + 16, attr_devs); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, stream, p);
    return hipGetLastError();
}

template <int SRC>
hipError_t launch_src(const EvdrClusterParams& p, bool vec, unsigned grid, hipStream_t stream) {
    const bool lds = p.ls <= EVDR_CLUSTER_LDS_GROUPS;
    if (vec) return lds ? launch<SRC, true, true>(p, grid, stream) : launch<SRC, true, false>(p, grid, stream);
    return lds ? launch<SRC, false, true>(p, grid, stream) : launch<SRC, false, false>(p, grid, stream);
}

}  // namespace

// arguments are the caller's to check (evdr_cluster_pages does): dtype valid, b >= 1, the workspace holds EVDR_CLUSTER_GRID slices
hipError_t evdr_launch_cluster_pages(const EvdrClusterParams& p, hipStream_t stream) {
    const int64_t eb = p.src_dtype == EVDR_F32 ? 4 : 2;
    const bool vec = p.d_src % 8 == 0 && reinterpret_cast<uintptr_t>(p.src) % 16 == 0 && (p.src_stride * eb) % 16 == 0;
    const unsigned grid = (unsigned)(p.b < EVDR_CLUSTER_GRID ? p.b : EVDR_CLUSTER_GRID);
    if (p.src_dtype == EVDR_F32) return launch_src<EVDR_F32>(p, vec, grid, stream);
    if (p.src_dtype == EVDR_BF16) return launch_src<EVDR_BF16>(p, vec, grid, stream);
    return launch_src<EVDR_F16>(p, vec, grid, stream);
}
