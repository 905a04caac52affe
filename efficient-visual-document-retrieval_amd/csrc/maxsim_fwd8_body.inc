// Body of the fp8 forward kernel (maxsim_fwd8.hip: maxsim_fwd8_kernel and maxsim_fwd8_pages_kernel include it as their function body).
// It expects the kernel argument `p8` and, as template parameters or constants of the including kernel, QW, ST, NSTAGE and PAGES.
// Kept as included text rather than an inlined function so that a kernel compiles to the instruction stream it has with the body
// written in place (as maxsim_fwd16s_body.inc).
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
    // PAGES: the batch's list, positions [pg0, pg0 + npages), read as SCALAR loads (constant address space: lgkmcnt, like the page
    // flags -- a vector load inside the ring loop would make the compiler wait on vmcnt, i.e. on the ring's pieces in flight).  An
    // entry outside [0, p.ncorpus) is a hole: it never forms an address (its stages re-read page 0, which exists: the entry refuses
    // a list over an empty corpus), nothing of it is folded, and its column is -inf.
    constexpr uint32_t HOLE_FLAGS = 0x80000000u;          // no page's flag word (bits 0..3 only)
    [[maybe_unused]] ciptr_t glist = nullptr;
    if constexpr (PAGES) glist = (ciptr_t)(uintptr_t)(p.gather + pg0);

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
        int cpage = pg0 + pgi;
        if constexpr (PAGES) {
            const int e = glist[pgi];
            cpage = (uint32_t)e < (uint32_t)p.ncorpus ? e : 0;
        }
        const uint8_t* pbase = P8 + (int64_t)cpage * p.p_stride;
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
    // corpus page / flag word of the workgroup's page i (PAGES: of list position pg0 + i; a hole: page 0 / HOLE_FLAGS)
    auto page_at = [&](int i) -> int {
        if constexpr (PAGES) { const int e = glist[i]; return (uint32_t)e < (uint32_t)p.ncorpus ? e : 0; }
        else return pg0 + i;
    };
    auto flags_at = [&](int i) -> uint32_t {
        if constexpr (PAGES) return (uint32_t)glist[i] < (uint32_t)p.ncorpus ? pageflags_c[page_at(i)] : HOLE_FLAGS;
        else return pageflags_c[pg0 + i];
    };
    uint32_t pflags = flags_at(0);
    int kp = pshift_c[page_at(0)];
    for (int s = 0; s < nstages; ++s) {
        // stage s has landed once only the younger stages' pieces remain (waits + barrier as one statement: ring_barrier)
        if (NSTAGE >= 4 && s + 2 < nstages) ring_barrier<2 * G>();
        else if (s + 1 < nstages) ring_barrier<G>();
        else ring_barrier<0>();
        if (s + NSTAGE - 1 < nstages) issue_stage(s + NSTAGE - 1, slot == 0 ? NSTAGE - 1 : slot - 1);
        const int page = page_at(pgi);
        if (active) {
            const char* sb = smem + slot * SLOT_BYTES;
            const int t0 = sip * ST;
            // (a hole folds no tile: its slot holds page 0's bytes, fetched to keep the ring's piece count)
            const int tcount = (PAGES && pflags == HOLE_FLAGS) ? 0 : (sip == spp - 1) ? T - t0 : ST;
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
                    if (PAGES && pflags == HOLE_FLAGS) cs = neg_inf();          // also for a NaN query, in every slice (-inf + -inf)
                    if (lane == 0 && qreal[j] >= 0) {
                        float* o = p.out + (int64_t)qreal[j] * p.out_stride + (PAGES ? pg0 + pgi : page);     // PAGES: the list position
                        if (p.accumulate) atomicAdd(o, cs);
                        else *o = cs;
                    }
                }
            }
        }
        if (++sip == spp) {
            sip = 0;
            if (++pgi < npages) {
                pflags = flags_at(pgi);
                kp = pshift_c[page_at(pgi)];
            }
        }
        slot = (slot == NSTAGE - 1) ? 0 : slot + 1;
    }
