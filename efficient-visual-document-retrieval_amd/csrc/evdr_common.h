// Shared declarations for the gfx950 kernels and the C-ABI dispatch (include/evdr.h).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/evdr.h"

#define EVDR_VERSION_NUM 303   /* 0.3.3: evdr_maxsim_fwd_prepared_subset + evdr_qcache_* (0.3.2: evdr_adamw_step, AdamW hyper-parameters as doubles; 0.3.1: evdr_maxsim_bwd_adamw_planes; 0.3.0: debug hooks instead of environment switches) */

#define EVDR_D 128              /* embedding width the kernels are specialised for */
#define EVDR_TILE_PATCHES 32    /* patches per LDS tile (two 16-row MFMA halves) */

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// fp32 -> fp16 hi/lo planes: the tensor is scaled by 2^k so that its absmax lands in [2^14, 2^15) (top of the fp16 range:
// the lo plane of every element that matters stays a NORMAL fp16 number).  k from the absmax's exponent field; tensors
// whose absmax is 0, denormal, inf or NaN are left unscaled.
__host__ __device__ static inline int evdr_h2_shift(uint32_t amax_bits) {
    const int e = (int)((amax_bits >> 23) & 0xFFu);
    return (e == 0 || e == 255) ? 0 : 141 - e;
}

// ---- forward --------------------------------------------------------------------------------
struct EvdrFwdParams {
    const uint16_t* Q;          // bf16 planes; query q, token n at Q + q*q_stride + n*128
    int64_t q_stride;           // elements between queries
    int64_t q_plane_stride;     // elements between Q planes
    const uint16_t* P;          // bf16 planes; page-major (np, lp, 128) per plane
    int64_t p_stride;           // elements between pages
    int64_t p_plane_stride;     // elements between P planes
    const uint32_t* q_amax;     // fp16 hi/lo planes (nplanes = 2): absmax bits of the fp32 tensor they were split from
    const uint32_t* p_amax;     //   (evdr_h2_shift gives the power-of-two the planes were scaled by); null = unscaled
    const uint8_t* qmask;       // (nq, lq) or null
    const int32_t* qlist;       // later token slices: compacted indices of the queries with a valid token in the slice, or null
    const int32_t* qcount;      //   ... and their number (device memory)
    const uint32_t* tilemask;   // (np, ntiles)
    const uint32_t* pageflags;  // (np)
    float* out;                 // (nq, out_stride)
    int64_t out_stride;
    uint16_t* argmax;           // (nq, np, lq) or null
    int nq, lq, np, lp, ntiles; // lq = tokens scored by THIS launch (<= 32), starting at token tok0
    int tok0, lq_total;         // lq_total = row length of qmask / argmax (queries longer than 32 tokens
    int accumulate;             //   are scored in 32-token slices, later slices add into out)
    int pages_per_block, n_qgroups, n_chunks;
    int64_t per_token;          // > 0: Q holds this many SINGLE-token queries packed 32 to a "query"; out / argmax get one
                                //      row per token (out (per_token, np), argmax (per_token, np)) instead of the token sum
    int inblock_refill;         // staged kernel: issue the ring refill inside the MFMA block (else right after the barrier)
    int ncorpus;                // page-subset instances only: pages of the corpus the list indexes (fills the padding in front of dbg)
    unsigned long long* dbg;    // diagnostic builds only: per-wave cycle sums (null in production)
    const int32_t* gather;      // rerank instances only (evdr_launch_maxsim_gather16[_bf16]): (nq, np) corpus page of each list position
    const int32_t* gcount;      //   ... and (nq) list lengths; np is then the list capacity and out column = list position
                                // page-subset instances (evdr_launch_maxsim_pages16): gather = ONE (np) list for the whole batch, gcount unused
};

// Pages per workgroup.  Workgroups are equal-sized and one fits per CU, so a launch runs in ceil(workgroups / 256) rounds
// of `ppb` pages each plus a fixed cost per workgroup (query load + ring fill, worth about 16 tiles of MFMA work).
// Pick the ppb in [lo, 64] that minimises rounds x (ppb + fixed): this avoids e.g. 1539 workgroups = 6 full rounds + a
// seventh for 3 workgroups.  lo: a workgroup should stream >= ~64 tiles, otherwise the fixed cost dominates -- unless
// that would leave CUs without any workgroup.  Many rounds (>= 64) need no tuning: take 64 pages.
static inline int evdr_pages_per_block(int64_t np, int64_t n_qgroups, int64_t ntiles, int64_t slots = 256) {
    const int64_t total = np * n_qgroups;
    int64_t lo = (64 + ntiles - 1) / ntiles;
    const int64_t fill = (total + slots - 1) / slots;    // pages per workgroup that still gives every workgroup slot one workgroup
    if (lo > fill) lo = fill;
    if (lo < 1) lo = 1;
    int64_t hi = total / (6 * slots);                    // ~6 rounds
    if (hi > 64) hi = 64;
    if (hi < lo) hi = lo;
    if (hi > np) hi = np;
    if (lo > hi) lo = hi;
    if (total / (slots * hi) >= 64) return (int)hi;      // tail round <= 1.5 % whatever the choice
    int64_t best = hi;
    double best_cost = 1e30;
    for (int64_t ppb = np < 64 ? np : 64; ppb >= lo; --ppb) {
        const int64_t wgs = ((np + ppb - 1) / ppb) * n_qgroups;
        const int64_t rounds = (wgs + slots - 1) / slots;
        const double cost = (double)rounds * ((double)ppb + 16.0 / (double)ntiles);
        if (cost < best_cost) { best_cost = cost; best = ppb; }   // ties: the larger ppb (fewer workgroups)
    }
    return (int)best;
}

// The dynamic-LDS limit of a kernel is a per-(function, device) attribute: remember the devices it was raised on, so that
// one process driving several GPUs (torch.cuda.set_device between calls) gets it on each of them.
// Safe from several host threads: the bit set is atomic, and two threads that both find the bit clear both raise the limit
// to the same value (idempotent) before either launches.
static inline hipError_t evdr_ensure_dyn_lds(const void* kern, int bytes, std::atomic<uint64_t>& devs_done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (devs_done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) devs_done.fetch_or(bit, std::memory_order_release);
    return e;
}

// debug hooks (maxsim_fwd.hip): forced kernel variant, pages-per-workgroup override, name of the last dispatched instance
int evdr_fwd_variant_exchange(int v);
int evdr_pages_per_block_exchange(int v);
int evdr_pages_per_block_override();
void evdr_note_fwd_kernel(const char* name);
const char* evdr_last_fwd_kernel_name();

// launches (defined in the .hip files; all enqueue on `stream` and return the launch status)
hipError_t evdr_launch_maxsim_fwd(const EvdrFwdParams& p, int nplanes, bool want_argmax, hipStream_t stream);
hipError_t evdr_launch_maxsim_fwd16(const EvdrFwdParams& p, int qw, int waves, int nplanes, bool want_argmax, int geom,
                                    hipStream_t stream);
hipError_t evdr_launch_maxsim_coarse16(const EvdrFwdParams& p, hipStream_t stream);
hipError_t evdr_launch_maxsim_gather16(const EvdrFwdParams& p, hipStream_t stream);
hipError_t evdr_launch_maxsim_gather16_bf16(const EvdrFwdParams& p, hipStream_t stream);
hipError_t evdr_launch_maxsim_pages16(const EvdrFwdParams& p, int nplanes, hipStream_t stream);
hipError_t evdr_launch_cand_compact(const int32_t* cand, int64_t nq, int r, int32_t idx_base, int64_t np, int32_t* glist, int32_t* gpos,
                                    int32_t* gcount, float* out, int64_t out_stride, int32_t* cand_clean, hipStream_t stream);
hipError_t evdr_launch_cand_scatter(const float* tmp, const int32_t* gpos, const int32_t* gcount, int64_t nq, int r, float* out,
                                    int64_t out_stride, hipStream_t stream);
hipError_t evdr_launch_select_topr(const float* scores, int64_t nq, int64_t n, int64_t row_stride, int32_t idx_base, int r,
                                   int32_t* out, hipStream_t stream);
hipError_t evdr_launch_maxsim_align(const uint16_t* Q, const uint16_t* P, const uint8_t* qmask, const uint32_t* tilemask,
                                    const uint32_t* pageflags, const int32_t* cand, int r, int32_t idx_base, float* sim, int32_t* patch,
                                    float* heat, int64_t nq, int lq, int64_t np, int lp, int nplanes, int64_t p_stride,
                                    int64_t p_plane_stride, const uint32_t* q_amax, const uint32_t* p_amax, hipStream_t stream);
hipError_t evdr_launch_pack_pmask(const uint8_t* pmask, int64_t np, int64_t lp, uint32_t* tilemask,
                                  uint32_t* pageflags, hipStream_t stream);
hipError_t evdr_launch_build_qlist(const uint8_t* qmask, int64_t nq, int64_t lq, int64_t tok0, int32_t* qlist, int32_t* qcount,
                                   hipStream_t stream);
hipError_t evdr_launch_split_f32(const float* x, int64_t rows, uint16_t* planes, uint32_t* amax_bits, hipStream_t stream);
hipError_t evdr_launch_split_f32_segments(const float* x, int64_t rows, int64_t seg_rows, uint16_t* planes, uint32_t* amax_bits,
                                          hipStream_t stream);
hipError_t evdr_launch_split_f32_pages(const float* x, int64_t rows, uint16_t* planes, uint32_t* amax_bits, const uint8_t* rowmask,
                                       int64_t rows_per_page, uint32_t* pageflags, hipStream_t stream);
hipError_t evdr_launch_flag_nonfinite(const void* P, int kind, const uint8_t* pmask, int64_t np, int64_t lp, int64_t p_stride,
                                      uint32_t* pageflags, hipStream_t stream);
hipError_t evdr_launch_maxsim_bwd(const float* g, const float* Q, const uint8_t* qmask, const uint8_t* pmask,
                                  const uint16_t* argmax, float* dP, int64_t nq, int64_t lq, int64_t np,
                                  int64_t lp, hipStream_t stream);
hipError_t evdr_launch_maxsim_bwd_adamw(const float* g, const float* Q, const uint8_t* qmask, const uint8_t* pmask,
                                        const uint16_t* argmax, float* x, float* exp_avg, float* exp_avg_sq, int64_t nq,
                                        int64_t lq, int64_t np, int64_t lp, double lr, double beta1, double beta2, double eps,
                                        double weight_decay, double bc1, double bc2_sqrt, float eps_norm, const void* state,
                                        void* next_planes, uint32_t* next_amax, uint32_t* pageflags, hipStream_t stream);
hipError_t evdr_launch_adamw_advance(void* state, double beta1, double beta2, hipStream_t stream);
hipError_t evdr_launch_adamw(const float* g, float* x, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                             double beta2, double eps, double weight_decay, double bc1, double bc2_sqrt, hipStream_t stream);
hipError_t evdr_launch_maxsim_bwd_q(const float* g, const float* P, const uint8_t* qmask, const uint32_t* pageflags,
                                    const uint16_t* argmax, float* dQ, float* partials, int64_t nq, int64_t lq, int64_t np,
                                    int64_t lp, hipStream_t stream);
int evdr_bwd_q_segments(int64_t pairs, int64_t np);
hipError_t evdr_launch_l2norm_fwd(const float* x, const uint8_t* rowmask, int64_t rows, float eps, float* y, float* norm,
                                  uint16_t* planes, uint32_t* amax_bits, uint32_t* pageflags, int64_t rows_per_page,
                                  hipStream_t stream);
hipError_t evdr_launch_l2norm_bwd(const float* gy, const float* x, const uint8_t* rowmask, const float* norm, int64_t rows,
                                  float eps, float* dx, hipStream_t stream);
hipError_t evdr_launch_topk(const float* scores, const int32_t* idx_map, int64_t nq, int64_t n,
                            int64_t row_stride, int32_t idx_base, int k, float* top_scores, int32_t* top_idx,
                            void* workspace, hipStream_t stream);
int evdr_topk_segments(int64_t nq, int64_t n);
hipError_t evdr_launch_qcache_lookup_plan(const EvdrQCache& c, const void* Q, const uint8_t* qmask, const uint32_t* q_amax, int64_t nq,
                                          uint64_t* hashes, int32_t* hit, int32_t* qsel, int32_t* qsel_count, uint32_t* ticket,
                                          hipStream_t stream);
hipError_t evdr_launch_qcache_exchange(const EvdrQCache& c, const void* Q, const uint8_t* qmask, int64_t nq, const int32_t* hit,
                                       float* out, int64_t out_stride, hipStream_t stream);
hipError_t evdr_launch_infonce(const float* ss, const float* st, int64_t b, int64_t n, float temperature,
                               float* loss, float* dscore, float* row_loss, hipStream_t stream);
hipError_t evdr_launch_infonce_ws(const float* ss, const float* st, int64_t b, int64_t n, float temperature, float* loss,
                                  float* dscore, float* workspace, hipStream_t stream);
// csrc/pairloss.hip: i per workgroup (the launch grid is (ceil(n / EVDR_PAIR_TILE), b)) and the shape limits of the two kernels
#define EVDR_PAIR_TILE 64
#define EVDR_PAIR_MAX_B 65535
#define EVDR_PAIR_MAX_N 1048576
hipError_t evdr_launch_pairwise_distill(const float* ss, const float* st, int64_t b, int64_t n, float* loss, float* grad, double* part,
                                        unsigned int* ticket, hipStream_t stream);
hipError_t evdr_launch_lambda_pairs(const float* ss, const float* gain, const float* disc, int64_t b, int64_t n, float alpha, float eps,
                                    float* loss, float* grad, double* part, unsigned int* ticket, hipStream_t stream);

// ---- fp8 (e4m3fn) corpora (csrc/quant8.hip, csrc/maxsim_fwd8.hip) ----------------------------------------------------------
// The forward takes the geometry of EvdrFwdParams (block_work / evdr_set_geometry) with Q / P holding e4m3 BYTES (strides in
// bytes), plus the power-of-two shifts the quantiser chose per query and per page.
struct EvdrFwd8Params {
    EvdrFwdParams g;
    const int32_t* q_shift;     // (nq): query q holds x * 2^q_shift[q]
    const int32_t* p_shift;     // (np): page p holds x * 2^p_shift[p]
};
hipError_t evdr_launch_maxsim_fwd8(const EvdrFwd8Params& p, hipStream_t stream);
hipError_t evdr_launch_maxsim_fwd8_pages(const EvdrFwd8Params& p, hipStream_t stream);     // p.g.gather / np / ncorpus as the page-subset instances
hipError_t evdr_launch_quantize_fp8(const void* x, int dtype, int64_t groups, int64_t rows_per_group, int64_t d, uint8_t* x8,
                                    int32_t* shift, hipStream_t stream);

// ---- growable corpus: fused page ingest (csrc/ingest.hip) ---------------------------------------------------------------------
// The arguments of evdr_corpus_ingest, as checked there; one workgroup per source page.
struct EvdrIngestParams {
    const void* src;            // (b, lp_src, d_src) of src_dtype, dense rows, src_stride ELEMENTS between pages
    int src_dtype;              // EVDR_F32 / EVDR_BF16 / EVDR_F16
    const uint8_t* pmask;       // (b, lp_src) bytes or null = every source patch valid
    int64_t b, src_stride;
    int lp_src, d_src;
    void* planes;               // the corpus: planes of `kind` for `capacity` pages of lp patches
    int kind;                   // EVDR_CORPUS_BF16 / _F16_HILO / _FP8
    int lp;
    int64_t capacity, p_stride, p_plane_stride;
    uint32_t* tilemask;         // (capacity, ceil(lp / 32))
    uint32_t* pageflags;        // (capacity)
    int32_t* shift;             // (capacity): fp8 kind
    const uint32_t* p_amax;     // the corpus's absmax word: fp16 hi/lo kind
    int64_t first_page;         // destination = first_page + source page ...
    const int32_t* dst_pages;   //   ... or, when given, dst_pages[source page]; outside [0, capacity) = hole, page skipped
    uint32_t* status;           // or null; bit 0: a finite element lies above the corpus's binade (fp16 hi/lo kind)
};
hipError_t evdr_launch_corpus_ingest(const EvdrIngestParams& p, hipStream_t stream);

// ---- pooled corpora: fused group-mean pooling while ingesting (csrc/pool.hip) -------------------------------------
// The arguments of evdr_corpus_pool_ingest / evdr_pool_pages, as checked there; one workgroup per source page.  `g` is the ingest
// call's source and destination with g.lp_src = patches of a SOURCE page and g.lp = patches of a destination page (>= ls; pooled
// tokens [ls, lp) are masked zeros).  g.kind = EVDR_POOL_PLAIN writes fp32 rows and mask bytes instead of planes and words.
#define EVDR_POOL_PLAIN 0
struct EvdrPoolParams {
    EvdrIngestParams g;
    const int32_t* members;     // source patch indices, group by group; outside [0, g.lp_src) = hole, skipped
    const int32_t* offsets;     // ls + 1 entries: group t owns members[offsets[t] : offsets[t + 1]]
    int64_t members_stride;     // elements between the pages' lists; 0 = one grouping shared by all pages
    int64_t offsets_stride;
    int m;                      // members per list
    int ls;                     // pooled tokens per page
    int normalize;              // 1: x / (||x|| + 1e-12) per pooled token, sum of squares in the pinned order
    float* out;                 // EVDR_POOL_PLAIN: (b, ls, d_out) fp32 ...
    uint8_t* out_mask;          //   ... and (b, ls) mask bytes
    int d_out;                  // d_src or 128
};
hipError_t evdr_launch_corpus_pool(const EvdrPoolParams& p, hipStream_t stream);

// ---- token clustering: spherical k-means per page, emitted as the per-page CSR grouping of the pooling calls (csrc/cluster.hip;
// DESIGN.md §4.11) ---------------------------------------------------------------------------------------------------------------------
// The arguments of evdr_cluster_pages, as checked there.  One workgroup per page on a grid of at most EVDR_CLUSTER_GRID workgroups;
// workgroup w owns workspace bytes [w * slice_bytes, (w + 1) * slice_bytes): lp_src label words, and from cent_off on the ls x 128
// fp32 centroids when they do not fit the LDS (ls > EVDR_CLUSTER_LDS_GROUPS).
#define EVDR_CLUSTER_GRID 512
#define EVDR_CLUSTER_LDS_GROUPS 312
struct EvdrClusterParams {
    const void* src;            // (b, lp_src, d_src) pages of src_dtype, dense rows, src_stride elements between pages
    int src_dtype;
    const uint8_t* pmask;       // (b, lp_src) or null
    int64_t b, src_stride;
    int lp_src, d_src;
    int ls, iters;
    int32_t* members;           // (b, lp_src)
    int32_t* offsets;           // (b, ls + 1)
    int32_t* labels;            // (b, lp_src) or null
    void* workspace;
    int64_t slice_bytes, cent_off;
};
inline int64_t evdr_cluster_label_bytes(int64_t lp_src) { return (lp_src * 4 + 255) / 256 * 256; }
inline int64_t evdr_cluster_slice_bytes(int64_t lp_src, int64_t ls) {
    return evdr_cluster_label_bytes(lp_src) + (ls > EVDR_CLUSTER_LDS_GROUPS ? ls * EVDR_D * 4 : 0);
}
hipError_t evdr_launch_cluster_pages(const EvdrClusterParams& p, hipStream_t stream);

// ---- document-level search: segmented arg-max, list collapse (csrc/docs.hip) ------------------------------------------
// The arguments of evdr_doc_max / evdr_collapse_topk, as checked there; evdr_launch_doc_finish is evdr_doc_topk's last step: top_doc
// holds evdr_topk's columns on entry.
hipError_t evdr_launch_doc_max(const float* scores, const int32_t* members, const int32_t* offsets, const int32_t* idx_map, int64_t nq,
                               int64_t n, int64_t row_stride, int64_t nm, int64_t n_docs, int32_t idx_base, float* doc_scores,
                               int64_t doc_stride, int32_t* doc_best, hipStream_t stream);
hipError_t evdr_launch_collapse_topk(const float* scores, const int32_t* page, const int32_t* doc, const int32_t* doc_of_page, int64_t np,
                                     int32_t idx_base, int64_t nq, int r, int64_t row_stride, int k, float* top_scores,
                                     int32_t* top_doc, int32_t* top_page, hipStream_t stream);
hipError_t evdr_launch_doc_finish(const float* top_scores, int32_t* top_doc, int32_t* top_page, const int32_t* doc_best, int64_t nq,
                                  int64_t n_docs, int k, hipStream_t stream);
