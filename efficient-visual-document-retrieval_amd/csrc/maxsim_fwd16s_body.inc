// Body of the staged forward kernel (maxsim_fwd16.hip: maxsim_fwd16s_kernel and maxsim_fwd16s_pages_kernel include it as their function
// body).  It expects the kernel argument `p` and, as template parameters or constants of the including kernel, QW, NPL, ARGMAX, ST,
// NSTAGE, DIAG, BAL, WAVES, NT, NCB, HI, GATHER and PAGES.  Kept as included text rather than an inlined function so that a kernel
// compiles to the instruction stream it has with the body written in place.
    static_assert(!HI || (NPL == 1 && NCB == 1 && !ARGMAX), "coarse pass: the hi plane alone, one product per k-step");
    static_assert(!GATHER || (QW == 1 && !ARGMAX), "rerank: one query per workgroup");
    static_assert(!PAGES || (!GATHER && !ARGMAX && !HI && NCB == 1), "page subset: scores only, bf16 or fp16 hi/lo planes of width 128");
    constexpr bool SCALED = (NPL == 2) || HI;            // fp16 planes of x * 2^k: scaled units, -1e4 joins at the page end
    using frag = typename FragOf<SCALED ? 2 : 1>::type;
    constexpr int NPLN = NPL * NCB;                       // planes of a tile in memory, in LDS and in the query fragments
    static_assert(NCB == 1 || (NCB == 2 && NPL == 2 && QW == 1), "256-wide embeddings: fp16 hi/lo planes, one query per wave");
    static_assert(WAVES == 8 || (WAVES == 4 && !BAL), "8 waves (one workgroup per CU) or 4 (two independent workgroups per CU)");
    constexpr int TILE_B = NPLN * TILE_BYTES;             // planes of one tile are adjacent 8-KiB images
    constexpr int SLOT_TILES = ST + 1;                    // a ring slot holds one tile more than a stage's ST ...
    constexpr int STAGE_BYTES = SLOT_TILES * TILE_B;
    constexpr int G = ST * NPLN * 8 / WAVES;              // LDS-DMA pieces per wave per stage (8 pieces per tile and plane)
    // plane products (A = page plane, B = query plane), smaller magnitude first
    // per column block cb: lo_cb x hi_cb, hi_cb x lo_cb, hi_cb x hi_cb (hi = value plane 0, lo = value plane 1; plane = value * NCB + cb)
    constexpr int NPROD = ((NPL == 1) ? 1 : 3) * NCB;
    constexpr int PA[6] = {(NPL - 1) * NCB, 0, 0, (NPL - 1) * NCB + 1, 1, 1};
    constexpr int PB[6] = {0, (NPL - 1) * NCB, 0, 1, (NPL - 1) * NCB + 1, 1};
    static_assert(NPL == 1 || NPL == 2, "one bf16 plane or fp16 hi/lo planes");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15;
    const int g = lane >> 4;

    const BlockWork bw = block_work(p);
    if (!bw.valid) return;
    const int qg = bw.qg, pg0 = bw.pg0;
    int npages = bw.npages;
    // a launch over a device-side query list (later token slices, evdr_maxsim_fwd_prepared_subset): a workgroup whose queries all lie
    // beyond the list has nothing to score and nothing to fetch (workgroup-uniform: before any barrier)
    if (p.qlist != nullptr && qg * WAVES * QW >= __builtin_amdgcn_readfirstlane(*p.qcount)) return;
    // rerank: list positions [pg0, pg0 + npages) of query qg, cut to its candidate count (a fallback query has none).  Count and list
    // are read as SCALAR loads (constant address space: lgkmcnt, like the page flags): a vector load inside the page loop would make
    // the compiler wait on vmcnt, i.e. on the ring's LDS-DMA pieces in flight (scratch/audit_ring_isa.py)
    typedef const __attribute__((address_space(4))) int32_t* clist_t;
    clist_t glist = nullptr;
    if constexpr (GATHER) {
        npages = min(npages, ((clist_t)(uintptr_t)p.gcount)[qg] - pg0);
        if (npages <= 0) return;
        glist = (clist_t)(uintptr_t)(p.gather + (int64_t)qg * p.np + pg0);
    }
    if constexpr (PAGES) glist = (clist_t)(uintptr_t)(p.gather + pg0);       // the batch's list, positions [pg0, pg0 + npages)
    // corpus page of the workgroup's page i (its output column is pg0 + i)
    auto cpage = [&](int i) -> int {
        if constexpr (PAGES) { const int e = glist[i]; return (uint32_t)e < (uint32_t)p.ncorpus ? e : 0; }
        else if constexpr (GATHER) return glist[i];
        else return pg0 + i;
    };
    // ... so that a page of k*ST + 1 tiles (1030 patches = 4*8 + 1) is k stages, the last one carrying the tail tile,
    // instead of k + 1 stages with a whole barrier / refill round for one 6-patch tile
    const bool ext = (p.ntiles % ST == 1) && (p.ntiles > ST);
    const int spp = ext ? p.ntiles / ST : (p.ntiles + ST - 1) / ST;      // stages per page
    unsigned long long d_t0 = 0, d_pro = 0, d_bar = 0, d_ref = 0, d_fast = 0, d_gen = 0, d_fin = 0, d_a = 0, d_ctl = 0, d_c0 = 0;
    if constexpr (DIAG) d_t0 = stamp();

    const int q0 = (qg * WAVES + wave) * QW;
    int qreal[QW];                                        // wave-uniform: the queries of this wave, -1 = none
    resolve_queries<QW>(p, q0, qreal);
    if constexpr (GATHER) qreal[0] = (wave == 0 && qg < p.nq) ? qg : -1;
    bool active = qreal[0] >= 0;
    frag bq[QW][NPLN][2][4];
    float qwt[QW][2];
    // Query fragments come in THROUGH LDS (below, once the first stage is on its way): a fragment load straight from global
    // memory touches 16 rows x 64 B per instruction -- half of every 128-B line -- and the four k-steps of a row are four
    // instructions, each fetching its line from L2 again: 2 x the query bytes per workgroup, all 256 workgroups at once on
    // the same 0.5 MB, and the load ISSUE of the prologue took 15.5 k cycles (stamped: 10 % of a 150 k-cycle student
    // forward, 8 us of every launch).  Here: the mask bytes only.
    int qrows[QW];                                        // wave-uniform: rows of query j that exist in Q (0 = no query)
    bool qok[QW][2];
    uint32_t qmk[QW][2];
    // no mask: the same (unconditional) byte loads read query data and are ignored
    const uint8_t* qmp = p.qmask != nullptr ? p.qmask : reinterpret_cast<const uint8_t*>(p.Q);
#pragma unroll
    for (int j = 0; j < QW; ++j) {
        const int q = qreal[j];
        // per_token: "query" q is the pack of single-token queries 32 q .. 32 q + 31, the last pack may be short
        int nr = 0;
        if (q >= 0) nr = p.per_token ? (int)min((int64_t)p.lq, p.per_token - (int64_t)q * 32) : p.lq;
        qrows[j] = nr;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool ok = 16 * t + c < nr;
            qok[j][t] = ok;
            qmk[j][t] = qmp[ok ? (int64_t)q * p.lq_total + p.tok0 + 16 * t + c : (int64_t)0];
        }
    }
    auto set_qwt = [&]() {
#pragma unroll
        for (int j = 0; j < QW; ++j)
#pragma unroll
            for (int t = 0; t < 2; ++t) qwt[j][t] = (qok[j][t] && (p.qmask == nullptr || qmk[j][t] != 0u)) ? 1.f : 0.f;
    };
    uint32_t qbad[QW];                                    // wave-uniform: tokens of query j with a NaN / Inf element
    // fp16 planes carry x * 2^k: scores come back to real units with one exact power-of-two factor
    float inv = 1.f;
    if constexpr (SCALED) {
        const int kq = p.q_amax ? evdr_h2_shift(*p.q_amax) : 0;
        const int kp = p.p_amax ? evdr_h2_shift(*p.p_amax) : 0;
        inv = __builtin_ldexpf(1.f, -(kq + kp));
    }
    if (p.accumulate && p.argmax == nullptr) {          // later 32-token slice: see maxsim_fwd16_kernel
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        set_qwt();
        float any = 0.f;
#pragma unroll
        for (int j = 0; j < QW; ++j) any += qwt[j][0] + qwt[j][1];
        active = active && (__ballot(any != 0.f) != 0ull);
        // workgroup-wide OR through the first word of the (not yet used) ring: the fp16 instances own all 160 KiB of LDS as
        // dynamic memory, a static flag (__syncthreads_or) would push them over the limit
        volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(smem);
        if (threadIdx.x == 0) *flag = 0u;
        __syncthreads();
        if (active && lane == 0) *flag = 1u;
        __syncthreads();
        const bool wg_active = *flag != 0u;
        __syncthreads();
        if (!wg_active) return;
    }

    const uint32_t smem_base = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
    // A stage = up to ST (+1) consecutive tiles of ONE page (rows beyond the page are clamped: masked anyway).
    // Per-lane byte offset of this lane's 16 B inside a 1-KiB piece: LDS row (4 piece + lane/16) of the tile receives source
    // chunk (lane%16) ^ (row & 15) of patch row (row0 + lane/16):
    // The DMA's lane offset is zero-extended, so rows past the page end (masked anyway) are clamped by clamping the
    // scalar base row and giving each lane a non-negative row delta.
    // = ((c ^ g) << 4 | g << 8) ^ ((piece & 3) << 6) with c = lane % 16, g = lane / 16: ONE live VGPR and one v_xor per piece
    const uint32_t voff0 = (uint32_t)((((lane & 15) ^ (lane >> 4)) << 4) | ((lane >> 4) << 8));
    // piece i (of G) of this wave for stage k of page pgi.  [tlo, thi]: the tiles of the page that hold a valid patch
    // (pages whose valid patches form one range, page flag bit 2): with a 2-slot ring every wait is vmcnt(0), so tiles
    // outside it -- and tiles beyond the page -- are not fetched at all
    auto stage_base = [&](int pgi, int k) -> const uint16_t* {          // first row of stage k of page pgi, plane 0
        return p.P + (int64_t)cpage(pgi) * p.p_stride + (int64_t)(k * ST * EVDR_TILE_PATCHES) * EVDR_D;
    };
    auto issue_piece = [&](const uint16_t* sbp, int t0, int tlo, int thi, int slot, int i, auto full_tag) {
        constexpr bool KNOWN_FULL = decltype(full_tag)::value;       // caller guarantees the stage has all ST tiles
        const int pc = wave * G + i;
        const int tis = pc / (8 * NPLN);
        const int rem = pc - tis * (8 * NPLN);
        const int pl = rem >> 3, piece = rem & 7;
        if (!KNOWN_FULL && (t0 + tis >= p.ntiles || t0 + tis < tlo || t0 + tis > thi)) return;
        const int rrel = tis * EVDR_TILE_PATCHES + piece * 4;                        // piece's first row inside the stage (uniform)
        const int row0 = t0 * EVDR_TILE_PATCHES + rrel;
        int rb = rrel;
        if (!KNOWN_FULL) rb = min(row0, p.lp - 1) - t0 * EVDR_TILE_PATCHES;          // clamp rows beyond the page (masked anyway)
        const uint16_t* sb = sbp + (int64_t)pl * p.p_plane_stride + (int64_t)rb * EVDR_D;
        uint32_t voff = voff0 ^ ((uint32_t)(piece & 3) << 6);
        if (!KNOWN_FULL && row0 + 3 >= p.lp)                                         // uniform: only a page's tail tile
            voff = (voff & 0xFFu) + (uint32_t)(min(row0 + (lane >> 4), p.lp - 1) - min(row0, p.lp - 1)) * 256u;
        const uint32_t dst = __builtin_amdgcn_readfirstlane(smem_base + slot * STAGE_BYTES + tis * TILE_B + pl * TILE_BYTES + piece * 1024);
        if constexpr (NT) lds_dma_16B_sbase_nt(sb, voff, dst); else lds_dma_16B_sbase(sb, voff, dst);
    };
    // the extra (ST-th) tile of an extended last stage: piece `wave` of each plane of that tile, always clamped
    auto issue_extra = [&](int pgi, int k, int thi, int slot) {
        if (!(ext && k == spp - 1) || thi < k * ST + ST) return;
#pragma unroll
        for (int pc = 0; pc < 8 / WAVES; ++pc) {
            const int piece = wave + pc * WAVES;
            const int row0 = (k * ST + ST) * EVDR_TILE_PATCHES + piece * 4;
            const int rbase = min(row0, p.lp - 1);
            const uint32_t voff = ((voff0 ^ ((uint32_t)(piece & 3) << 6)) & 0xFFu) + (uint32_t)(min(row0 + (lane >> 4), p.lp - 1) - rbase) * 256u;
#pragma unroll
            for (int pl = 0; pl < NPLN; ++pl) {
                const uint16_t* sb = p.P + (int64_t)pl * p.p_plane_stride + (int64_t)cpage(pgi) * p.p_stride + (int64_t)rbase * EVDR_D;
                lds_dma_16B_sbase(sb, voff,
                                  __builtin_amdgcn_readfirstlane(smem_base + slot * STAGE_BYTES + ST * TILE_B + pl * TILE_BYTES + piece * 1024));
            }
        }
    };
    auto issue_stage = [&](int pgi, int k, int tlo, int thi, int slot) {
        const uint16_t* sbp = stage_base(pgi, k);
#pragma unroll
        for (int i = 0; i < G; ++i) issue_piece(sbp, k * ST, tlo, thi, slot, i, std::false_type{});
        issue_extra(pgi, k, thi, slot);
    };
    // in-block refill: NPL pieces per tile of the straight-line block, one scalar base pointer per stage and one live VGPR
    // (every instance: the QW = 2 argmax instance on fp16 planes, once excluded for its spills, has none left and gains 2 %)

    typedef const __attribute__((address_space(4))) uint32_t* cptr_t;
    cptr_t tilemask_c = (cptr_t)(uintptr_t)p.tilemask;
    cptr_t pageflags_c = (cptr_t)(uintptr_t)p.pageflags;
    // flag word of the workgroup's page i.  A hole gets HOLE_FLAGS: a range page [va, vb) = [1, 0) with masked patches -- no valid patch,
    // so one stage, nothing fetched and an exact 0 -- which no real page carries (pack_pmask writes ranges with va <= vb): the page
    // epilogue recognises the word and stores -inf
    constexpr uint32_t HOLE_FLAGS = 6u | (1u << 4);
    // -inf of a hole's column, from a scalar register made opaque at the use: as a plain constant it is hoisted out of the page loop
    // into a VGPR that stays live across the MFMA blocks, which the instances at 256 registers pay for with spills
    auto hole_value = [&]() -> float {
        uint32_t b = 0xFF800000u;
        asm volatile("" : "+s"(b));
        return __builtin_bit_cast(float, b);
    };
    auto cflags = [&](int i) -> uint32_t {
        if constexpr (PAGES) {
            const uint32_t f = pageflags_c[cpage(i)];
            return (uint32_t)glist[i] < (uint32_t)p.ncorpus ? f : HOLE_FLAGS;
        } else {
            return pageflags_c[cpage(i)];
        }
    };

    float run[QW][2];
    int ridx[QW][2];
    const int gx = g ^ c;
    const char* a_lane = smem + c * (EVDR_D * 2);
    auto load_half = [&](frag (&a)[NPLN][4], const char* sbase, int tis, int u) {
        const char* tb = sbase + tis * TILE_B + u * (16 * EVDR_D * 2);
#pragma unroll
        for (int pl = 0; pl < NPLN; ++pl)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) a[pl][s4] = *reinterpret_cast<const frag*>(tb + pl * TILE_BYTES + (((4 * s4) ^ gx) << 4));
    };
    auto chain = [&](const frag (&a)[NPLN][4], int j, int t) {
        f32x4v acc = {0, 0, 0, 0};
#pragma unroll
        for (int pr = 0; pr < NPROD; ++pr)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) acc = mfma16(a[PA[pr]][s4], bq[j][PB[pr]][t][s4], acc);
        return acc;
    };
    // fold one chain's accumulator (patches pb .. pb + 3 of this lane, all valid) into the running max / argmax
    auto fold = [&](const f32x4v& acc, int j, int t, int pb) {
        if constexpr (!ARGMAX) {
            float m = run[j][t];
            m = __builtin_fmaxf(__builtin_fmaxf(m, acc[0]), acc[1]);
            m = __builtin_fmaxf(__builtin_fmaxf(m, acc[2]), acc[3]);
            run[j][t] = m;
        } else {
            float best = run[j][t];
            int bi = ridx[j][t];
#pragma unroll
            for (int i = 0; i < 4; ++i) {                                  // increasing patch order: the first max wins
                const bool take = acc[i] > best;
                best = take ? acc[i] : best;
                bi = take ? pb + i : bi;
            }
            run[j][t] = best;
            ridx[j][t] = bi;
        }
    };
    // pbase: first patch index of the 16-patch half (uniform); the lane's accumulator i is patch pbase + 4g + i
    auto chains_full = [&](const frag (&a)[NPLN][4], int pbase) {          // all 16 patches of the half valid
        const int pb = pbase + 4 * g;
        if constexpr (NPL == 1 && (QW <= 2 || QW >= 8)) {
            // one or two queries per wave: the 2 QW chains of a half-tile are issued INTERLEAVED (k-step outermost), so that
            // consecutive MFMAs never depend on each other; with 8 chains (QW = 4) the other wave of the SIMD fills those
            // slots and keeping one accumulator live at a time matters more (+4..5 % at 5-16 queries per launch).
            // QW = 8 (one wave per SIMD, experiment): nothing else fills a dependent chain's gaps, and the VGPR half has the
            // room for 16 live accumulators
            f32x4v acc[QW][2];
#pragma unroll
            for (int j = 0; j < QW; ++j) acc[j][0] = acc[j][1] = f32x4v{0, 0, 0, 0};
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int j = 0; j < QW; ++j)
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[j][t] = mfma16(a[0][s4], bq[j][0][t][s4], acc[j][t]);
#pragma unroll
            for (int j = 0; j < QW; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) fold(acc[j][t], j, t, pb);
        } else {
#pragma unroll
            for (int j = 0; j < QW; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) fold(chain(a, j, t), j, t, pb);
        }
    };
    auto chains_masked = [&](const frag (&a)[NPLN][4], uint32_t bits, int pbase) {
        const int pb = pbase + 4 * g;
        uint32_t mybits = bits >> (4 * g);
        asm volatile("" : "+v"(mybits));
#pragma unroll
        for (int j = 0; j < QW; ++j)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f32x4v acc = chain(a, j, t);
                if constexpr (!ARGMAX) {
                    float m = run[j][t];
#pragma unroll
                    for (int i = 0; i < 4; ++i) m = __builtin_fmaxf(m, ((mybits >> i) & 1u) ? acc[i] : neg_inf());
                    run[j][t] = m;
                } else {
                    float best = run[j][t];
                    int bi = ridx[j][t];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const bool take = ((mybits >> i) & 1u) && (acc[i] > best);
                        best = take ? acc[i] : best;
                        bi = take ? pb + i : bi;
                    }
                    run[j][t] = best;
                    ridx[j][t] = bi;
                }
            }
    };

    static_assert(NSTAGE == 2, "the stage cursors below keep exactly one stage in flight");
    // ---- stage sequence.  A page whose valid patches form ONE range [va, vb) (page flag bit 2: all valid, a ragged
    // prefix, an image between masked text tokens -- what utils/preprocess_data.py:101 produces) is walked only over the
    // stages that hold a valid patch, and only the tiles inside the range are fetched: a 700-patch page of a 1030-patch
    // corpus costs 3 stages and 22 tiles, not 4 and 33.  Pages with holes walk all their stages and read mask words.
    // Two cursors run over the same sequence one stage apart: `nx*` = the stage being fetched, `c*` = the one computed.
    auto page_span = [&](uint32_t pf, int& klo, int& khi, int& tlo, int& thi) {
        klo = 0; khi = spp; tlo = 0; thi = p.ntiles - 1;
        if (pf & 4u) {
            const int va = (int)((pf >> 4) & 0xFFFu), vb = (int)(pf >> 16);
            if (vb > va) {
                tlo = va >> 5;
                thi = (vb - 1) >> 5;
                klo = min(tlo / ST, spp - 1);
                khi = min(thi / ST, spp - 1) + 1;
            } else {                                    // no valid patch at all: one stage, nothing fetched
                khi = 1; tlo = 1; thi = 0;
            }
        }
    };
    // fetch cursor: page, stage, flag word of its page, and the base pointer of the stage (advanced by one stage stride
    // inside a page, recomputed at a page change: no 64-bit multiply per stage)
    int npgi = 0, nk;
    uint32_t npf = cflags(0);
    // flag word of the page AFTER the fetch cursor's, loaded a whole page before it is needed: the first stage of the next
    // page is chosen from it, and a scalar-load latency in front of every page's first refill would sit on the critical
    // path of HBM-bound launches
    uint32_t apf = npages > 1 ? cflags(1) : 0u;
    {
        int khi0, tlo0, thi0;
        page_span(npf, nk, khi0, tlo0, thi0);
        issue_stage(0, nk, tlo0, thi0, 0);
    }
    const uint16_t* fbase = stage_base(0, nk);
    // ---- query fragments through LDS.  The first stage is on its way into slot 0; slot 1 is free until the refill that
    // follows the first stage barrier.  One round per (query, plane): the wave's 32 token rows (8 KiB, the shape of a page
    // tile) arrive in its own 8-KiB window of slot 1 as eight 1-KiB LDS-DMA pieces -- whole 128-B lines, each line fetched
    // from L2 once -- with the page tiles' XOR swizzle, and leave it as MFMA fragments through the same ds_read_b128
    // addressing as a page tile's.  Each wave reads back only what it fetched itself: vmcnt, no barrier.  Rows that do not
    // exist (short queries, a short last token pack, no query at all) are clamped to an existing row and zeroed afterwards.
    {
        static_assert(WAVES * TILE_BYTES <= STAGE_BYTES, "the waves' query windows fit into ring slot 1");
        const uint32_t qwin = STAGE_BYTES + wave * TILE_BYTES;
#pragma unroll
        for (int j = 0; j < QW; ++j) {
            const int nr = max(qrows[j], 1);
            const uint16_t* qb = p.Q + (int64_t)max(qreal[j], 0) * p.q_stride + (int64_t)p.tok0 * EVDR_D;
#pragma unroll
            for (int pl = 0; pl < NPLN; ++pl) {
                if (j + pl > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the window's previous tenant has been read
#pragma unroll
                for (int piece = 0; piece < 8; ++piece) {
                    const int row0 = piece * 4;
                    const int rb = min(row0, nr - 1);
                    uint32_t voff = voff0 ^ ((uint32_t)(piece & 3) << 6);
                    if (row0 + 3 >= nr) voff = (voff & 0xFFu) + (uint32_t)(min(row0 + (lane >> 4), nr - 1) - rb) * 256u;
                    lds_dma_16B_sbase(qb + (int64_t)pl * p.q_plane_stride + (int64_t)rb * EVDR_D, voff,
                                      __builtin_amdgcn_readfirstlane(smem_base + qwin + piece * 1024));
                }
                wait_vmcnt<0>();
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4)
                        bq[j][pl][t][s4] = *reinterpret_cast<const frag*>(a_lane + qwin + t * (16 * EVDR_D * 2) + (((4 * s4) ^ gx) << 4));
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    set_qwt();
#pragma unroll
    for (int j = 0; j < QW; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (!qok[j][t]) {
#pragma unroll
                for (int pl = 0; pl < NPLN; ++pl)
#pragma unroll
                    for (int s = 0; s < 4; ++s) bq[j][pl][t][s] = frag{0, 0, 0, 0, 0, 0, 0, 0};
            }
#pragma unroll
    for (int j = 0; j < QW; ++j) {                        // the hi planes (one per column block): NaN and Inf survive the split there
        uint32_t c0 = 0u, c1 = 0u;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int s = 0; s < 4; ++s) { c0 |= frag_exp_carry(bq[j][cb][0][s]); c1 |= frag_exp_carry(bq[j][cb][1][s]); }
        qbad[j] = token_bad_bits((c0 & 0x80008000u) != 0u, (c1 & 0x80008000u) != 0u);
    }
    if constexpr (QW >= 8) {
        // one wave per SIMD, 512 registers: the 256 registers of query fragments are pinned to the AGPR half here -- an "a"-class
        // value stays there, and v_mfma reads its B operand from AGPRs directly -- which leaves the whole VGPR half to the page
        // fragments, accumulators and running maxima (left to itself the allocator put accumulators and page fragments into
        // AGPRs and paid 5 444 v_accvgpr_read for 4 736 MFMAs)
#pragma unroll
        for (int j = 0; j < QW; ++j)
#pragma unroll
            for (int pl = 0; pl < NPLN; ++pl)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4) asm volatile("" : "+a"(bq[j][pl][t][s4]));
    }
    if constexpr (DIAG) d_pro = stamp() - d_t0;
    const bool spread_ok = p.inblock_refill != 0;
    int slot = 0;
    bool page_open = true;                              // the compute cursor is at the first stage of its page
    // ---- page-end stores, deferred by one hand-over.  A finished page's score / arg-max words are kept in registers and stored
    // right BEHIND the next stage hand-over instead of in front of it: global stores count on vmcnt like the LDS-DMA pieces, so a
    // store issued at the page end made the next hand-over's vmcnt(0) wait for its write acknowledgement (~1 us from L2) with every
    // wave of the workgroup parked -- 4 us of a 76-us student forward (scratch/fwd_store_ab.py: the launch without any store).
    // Behind the hand-over the acknowledgement has a whole stage of matrix work to arrive in.  Same values, same addresses.
    // Only the fp16-plane instances (the training step's forwards: a 206-patch page is two stages, every second hand-over follows a
    // page end): their straight-line blocks leave the registers for it.  The bf16 instances sit at 256 VGPRs with the per-page values
    // live across the block (deferring there spills: 1-3 VGPRs in the QW = 2 / 4 instances), and a 1030-patch bf16 page amortises the
    // acknowledgement over four 512-MFMA stages (launch without stores: -0.3 %); they store at the page end as before.
    constexpr bool DEFER = (NPL == 2);
    int pend_page = -1;                                  // wave-uniform: the page whose stores are pending (-1: none)
    float pend_cs[QW];
    int pend_bi[QW][2];
    auto store_page = [&](int spage, const float (&scs)[QW], const int (&sbi)[QW][2]) {
#pragma unroll
        for (int j = 0; j < QW; ++j) {
            if constexpr (ARGMAX) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    // (opaque per page: otherwise the 64-bit per-lane output offsets of all (query, token) slots are hoisted out of
                    // the page loop -- 16 VGPRs that end up spilled, with their reloads landing inside the MFMA blocks)
                    int tok = 16 * t + c;
                    asm volatile("" : "+v"(tok));
                    if (g == 0 && tok < p.lq && qreal[j] >= 0)
                        p.argmax[((int64_t)qreal[j] * p.np + spage) * p.lq_total + p.tok0 + tok] = (uint16_t)sbi[j][t];
                }
            }
            if (lane == 0 && qreal[j] >= 0) {
                float* o = p.out + (int64_t)qreal[j] * p.out_stride + spage;
                if (p.accumulate) atomicAdd(o, scs[j]);
                else *o = scs[j];
            }
        }
    };
    auto flush_pending = [&]() {
        if constexpr (!DEFER) return;
        if (pend_page < 0) return;
        store_page(pend_page, pend_cs, pend_bi);
        pend_page = -1;
    };
    // per-page values of the compute cursor, decoded once when the page is opened
    uint32_t pflags = 0u;
    int va = 0, vb = 0, first_masked = 0, khi = 0;
    while (npgi < npages) {
        if constexpr (DIAG) d_c0 = stamp();
        // the compute cursor takes over the stage that was fetched last; the fetch cursor moves on
        const int pgi = npgi, k = nk;
        const int page = cpage(pgi);                    // corpus page: masks and flags
        const int ocol = pg0 + pgi;                     // output column (= page, except over a list: the list position)
        const uint16_t* cbase = fbase;                  // this stage's rows (a refill that stays in the page starts from it)
        if (page_open) {
            pflags = npf;
            // range pages: [va, vb); pages with holes: va = vb = -1 (mask words decide)
            va = (pflags & 4u) ? (int)((pflags >> 4) & 0xFFFu) : -1;
            vb = (pflags & 4u) ? (int)(pflags >> 16) : -1;
            // index torch.max reports for an all-masked page / where the -1e4 fill first appears
            first_masked = (pflags & 4u) ? (va > 0 ? 0 : vb) : (int)(pflags >> 16);
            int klo, tlo, thi;
            page_span(pflags, klo, khi, tlo, thi);
#pragma unroll
            for (int j = 0; j < QW; ++j) {
                // NPL = 1: a masked patch inside [0, lp) puts -1e4 into the max right away; NPL = 2 works in scaled units and
                // lets the -1e4 join at the page end
                run[j][0] = run[j][1] = (!SCALED && (pflags & 2u)) ? -1e4f : neg_inf();
                ridx[j][0] = ridx[j][1] = (!SCALED) ? first_masked : 0;
            }
        }
        const bool page_close = (k + 1 == khi);
        bool load_apf = false;
        if (!page_close) {
            ++nk;
            fbase = cbase + (int64_t)ST * EVDR_TILE_PATCHES * EVDR_D;
        } else {
            ++npgi;
            if (npgi < npages) {
                npf = apf;
                load_apf = npgi + 1 < npages;           // (issued behind the hand-over below: its lgkmcnt(0) would expose the latency)
                int khi2, tlo, thi;
                page_span(npf, nk, khi2, tlo, thi);
                fbase = stage_base(npgi, nk);
            }
        }
        const bool refill = npgi < npages;
        {
            // ---- everything this stage's control flow and the refill need is worked out BEFORE the wait for the stage's
            // data: flag / mask-word loads, spans and addresses overlap with the wait, and between the barrier and the first
            // LDS-DMA instruction of the refill only the DMA issue itself is left (in HBM-bound launches that gap is dead time
            // of the corpus stream: 511 instructions with seven scalar-load waits before, a few dozen now)
            const int nslot = slot ^ 1;
            const int t0 = k * ST;
            // a stage runs as the straight-line block when all its ST tiles are fully valid: from the valid range for
            // range pages, from the mask words (one scalar load each) for pages with holes.
            // bf16 kernels: the FIRST tile of the stage may be partial (the masked text tokens in front of the image patches
            // put the partial tile at the head of a page's first stage): its two half-tile steps then take the per-patch
            // select inside the same straight-line block (`headmask` = that tile's mask word, all ones otherwise)
            uint32_t headmask = 0xFFFFFFFFu;
            bool fast;
            if (va >= 0) {
                const int h0 = va - t0 * EVDR_TILE_PATCHES;            // valid patches start here, relative to the stage
                fast = active && vb >= (t0 + ST) * EVDR_TILE_PATCHES && h0 < (NPL == 1 ? EVDR_TILE_PATCHES : 1);
                if (h0 > 0 && h0 < EVDR_TILE_PATCHES) headmask = ~((1u << h0) - 1u);
            } else {
                fast = false;
                if (active && t0 + ST <= p.ntiles) {
                    uint32_t all = 0xFFFFFFFFu;
#pragma unroll
                    for (int i = 1; i < ST; ++i) all &= tilemask_c[(int64_t)page * p.ntiles + t0 + i];
                    headmask = tilemask_c[(int64_t)page * p.ntiles + t0];
                    fast = (all == 0xFFFFFFFFu) && (NPL == 1 || headmask == 0xFFFFFFFFu);
                }
            }
            // In-block refill: when this stage runs the straight-line block AND the next stage is a full one (all ST tiles
            // exist and lie inside the page rows), its LDS-DMA pieces are issued NPL per tile INSIDE the block, where their
            // scalar/address work hides under MFMAs; otherwise the refill is issued right after the barrier.
            // (In-block, the whole next stage is fetched, also tiles outside the page's valid range.)
            const bool next_rows = (nk + 1) * ST * EVDR_TILE_PATCHES <= p.lp;     // every row of the next stage exists
            const bool next_full = refill && next_rows;
#if defined(EVDR_RING_FAULT) && EVDR_RING_FAULT >= 3
            const bool spread = false;                                     // (control build: the whole refill goes out in front of the hand-over, below)
#else
            const bool spread = fast && next_full && spread_ok;
#endif
            // one base pointer for the whole next stage (two SGPRs), the tile window of its page, and which of this wave's G
            // pieces lie inside it
            const uint16_t* nbase = fbase;
            const int nt0 = nk * ST;
            int ntlo = 0, nthi = -1;
            uint32_t want = 0u;
            if (refill && !spread) {
                int klo, khi;
                page_span(npf, klo, khi, ntlo, nthi);
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    const int t = nt0 + (wave * G + i) / (8 * NPLN);
                    want |= (t >= ntlo && t <= nthi && t < p.ntiles) ? (1u << i) : 0u;
                }
            }
            if constexpr (DIAG) { d_a = stamp(); d_ctl += d_a - d_c0; }
            // stage hand-over (ring_barrier, maxsim_device.h): this wave's pieces of the stage have landed and every ds_read it
            // has issued is retired BEFORE it arrives; nothing can be scheduled into or across the statement
#if defined(EVDR_RING_FAULT) && EVDR_RING_FAULT >= 3
            // WAR control of the sentinel instrument for THIS (staged, two-slot) ring -- never a shipped build (build.py ring_fault=3,
            // scratch/sentinel_control.py): the refill of slot `nslot` is issued IN FRONT of the hand-over that retires the
            // ds_reads of the stage the slower waves of the workgroup may still be computing from that very slot.  This wave's own
            // reads of the slot are retired first (lgkmcnt(0)), so what is left is exactly the cross-wave write-after-read edge the
            // hand-over exists for.  (RAW stays intact: the hand-over's vmcnt(0) below also covers the pieces issued here.)
            // EVDR_RING_FAULT == 4: the same, with the race window held OPEN -- one wave of the workgroup sleeps ~14 us in front of
            // its reads of the stage's last tile (fault_hold in the fast block), so that the other waves' early refill of that slot is
            // certain to overtake it: what the instrument shows when the race really happens, as opposed to build 3, which only
            // removes the edge and leaves the timing to the hardware.
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (refill) {
                if (next_rows) {
#pragma unroll
                    for (int i = 0; i < G; ++i)
                        if ((want >> i) & 1u) issue_piece(nbase, nt0, 0, 0, nslot, i, std::true_type{});
                    issue_extra(npgi, nk, nthi, nslot);
                } else {
                    issue_stage(npgi, nk, ntlo, nthi, nslot);
                }
            }
#endif
            // page subset: the list entry of that page is fetched in FRONT of the hand-over (whose lgkmcnt(0) retires it under the wait
            // for the stage), so that behind it the flag word is ONE scalar load, as in the contiguous launch, not two dependent ones
            int aent = 0;
            if constexpr (PAGES) {
                if (load_apf) aent = glist[npgi + 1];
            }
            ring_barrier<0>();
            // the flag word of the page after the fetch cursor's: a scalar load with a whole stage to land in (the next hand-over
            // retires it; the value is first used when the fetch cursor opens that page)
            if constexpr (PAGES) {
                if (load_apf) {
                    const bool in = (uint32_t)aent < (uint32_t)p.ncorpus;
                    const uint32_t f = pageflags_c[in ? aent : 0];
                    apf = in ? f : HOLE_FLAGS;
                }
            } else {
                if (load_apf) apf = cflags(npgi + 1);
            }
            if constexpr (DIAG) { const unsigned long long t = stamp(); d_bar += t - d_a; d_a = t; }
#if defined(EVDR_RING_FAULT) && EVDR_RING_FAULT >= 3
            if (false) {
#else
            if (refill && !spread) {
#endif
                if (next_rows) {                                        // no row of the stage needs clamping: constant offsets
                    if (want == (1u << G) - 1u) {
#pragma unroll
                        for (int i = 0; i < G; ++i) issue_piece(nbase, nt0, 0, 0, nslot, i, std::true_type{});
                    } else {
#pragma unroll
                        for (int i = 0; i < G; ++i)
                            if ((want >> i) & 1u) issue_piece(nbase, nt0, 0, 0, nslot, i, std::true_type{});
                    }
                    issue_extra(npgi, nk, nthi, nslot);
                } else {
                    issue_stage(npgi, nk, ntlo, nthi, nslot);
                }
            }
            flush_pending();                                             // the previous page's stores: behind the hand-over and the refill
            if constexpr (DIAG) { const unsigned long long t = stamp(); d_ref += t - d_a; d_a = t; }
            const char* sbase = a_lane + slot * STAGE_BYTES;
            const int nt = (k == spp - 1) ? p.ntiles - t0 : ST;          // tiles in this stage (ST + 1 in an extended last stage)
            // ---- generic path: one tile, per 16-patch half, masks from the valid range or the mask words
            auto generic_tile = [&](int tis) {
                const int tip = t0 + tis;
                uint32_t tm;
                if (va >= 0) {
                    const int lo = max(va - tip * EVDR_TILE_PATCHES, 0), hi = min(vb - tip * EVDR_TILE_PATCHES, 32);
                    tm = hi > lo ? ((hi >= 32 ? 0xFFFFFFFFu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u)) : 0u;
                } else {
                    tm = tilemask_c[(int64_t)page * p.ntiles + tip];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t bits = (tm >> (16 * u)) & 0xFFFFu;
                    if (bits == 0u) continue;
                    frag a[NPLN][4];
                    load_half(a, sbase, tis, u);
                    const int pbase = tip * EVDR_TILE_PATCHES + 16 * u;
                    if (bits == 0xFFFFu) chains_full(a, pbase); else chains_masked(a, bits, pbase);
                }
            };
            if (active) {
                if (fast) {
                    // ---- fast stage: ST all-valid tiles of one page, one basic block (two instances: with / without refill)
                    auto fast_block = [&](auto spread_tag, auto young_tag, auto head_tag) {
                        constexpr bool SP = decltype(spread_tag)::value;
                        constexpr bool YOUNG = decltype(young_tag)::value;   // second-dispatched half of the workgroup
                        constexpr bool HEAD = decltype(head_tag)::value;     // the stage's first tile is partial (mask `headmask`)
                        // self-balancing priority: 3,2,1,0 over the quarters of the block.  The two waves of a SIMD run this
                        // same block; the one the arbiter favours reaches the lower-priority quarters first and yields, so
                        // both arrive at the stage barrier together instead of one idling while the other finishes alone.
                        // Priority falls with progress (half-tile step h of 2 ST): second-dispatched half of the workgroup
                        // 3,3,2,2,1,1,0,0 (per tile, ST = 8); first half, which wins equal-priority arbitration by age, an
                        // eighth of the block earlier: 3,2,2,1,1,0,0,0
                        auto prio_at = [](int h) {
                            const int off = YOUNG ? 0 : (ST >= 4 ? ST / 4 : 1);
                            const int q = 4 * (h + off) / (2 * ST);
                            return 3 - (q > 3 ? 3 : q);
                        };
                        // in-block refill: which of this wave's G pieces of the NEXT stage go out during tile `ti` of this one.
                        // EVDR_REFILL_FRONT = 0: G / ST per tile, evenly over the block; = 1 (A/B build): twice as many per tile over the
                        // FIRST half of the block, so that the last piece has half a block -- not one tile -- to land before the hand-over
                        auto refill_lo = [&](int ti) {
#if defined(EVDR_REFILL_FRONT) && EVDR_REFILL_FRONT == 1
                            const int v = 2 * ti * (G / ST);
#else
                            const int v = ti * (G / ST);
#endif
                            return v < G ? v : G;
                        };
                        auto refill_hi = [&](int ti) { return refill_lo(ti + 1); };
                        // control build 4 only (see the hand-over below): ONE wave sleeps in front of its reads of the stage's last tile
                        auto fault_hold = [&](bool here) {
#if defined(EVDR_RING_FAULT) && EVDR_RING_FAULT == 4
                            if (here && wave == WAVES - 3) {
#pragma unroll 1
                                for (int z = 0; z < 4; ++z) __builtin_amdgcn_s_sleep(127);
                            }
#else
                            (void)here;
#endif
                        };
                        auto set_prio = [&](int h) {
                            if constexpr (BAL) {
                                const int pr = prio_at(h);
                                if (h == 0 || pr != prio_at(h - 1)) {
                                    if (pr == 3) __builtin_amdgcn_s_setprio(3);
                                    else if (pr == 2) __builtin_amdgcn_s_setprio(2);
                                    else if (pr == 1) __builtin_amdgcn_s_setprio(1);
                                    else __builtin_amdgcn_s_setprio(0);
                                }
                            }
                        };
                        if constexpr (NPL == 1) {
                            // Fragment prefetch distance in half-tiles.  A half-tile is 2 QW chains of 4 MFMAs: 512 cycles of
                            // matrix work at QW = 4, but only 128 at QW = 1 -- less than an LDS read takes to come back, so
                            // with the one-half-ahead ping-pong of the QW = 4 instance a wave of the 1-16-query launches
                            // stalled on every fragment (measured with the LDS-DMA removed: 30-40 cycles per MFMA).  The small
                            // instances have the registers for a deeper ring of fragments: 4 halves ahead at QW = 1 and 2 (not with the argmax).
                            constexpr int DEPTH = (QW <= 2 && !ARGMAX) ? 4 : 2;
                            frag a[DEPTH][NPLN][4];
#pragma unroll
                            for (int h = 0; h < DEPTH; ++h) load_half(a[h], sbase, h >> 1, h & 1);
#pragma unroll
                            for (int h = 0; h < 2 * ST; ++h) {
                                const int pbase = (t0 + (h >> 1)) * EVDR_TILE_PATCHES + 16 * (h & 1);
                                set_prio(h);
                                if (HEAD && h == 0) chains_masked(a[h % DEPTH], headmask & 0xFFFFu, pbase);
                                else if (HEAD && h == 1) chains_masked(a[h % DEPTH], headmask >> 16, pbase);
                                else chains_full(a[h % DEPTH], pbase);
                                fault_hold(h == 2 * ST - 2 - DEPTH);
                                if (h + DEPTH < 2 * ST) load_half(a[h % DEPTH], sbase, (h + DEPTH) >> 1, (h + DEPTH) & 1);
                                if constexpr (SP) {
                                    if ((h & 1) == 0) {
#pragma unroll
                                        for (int i = refill_lo(h >> 1); i < refill_hi(h >> 1); ++i) issue_piece(nbase, nt0, 0, 0, nslot, i, std::true_type{});
                                    }
                                }
                            }
                        } else {
                            // fp16 hi/lo planes: per 16-patch half, phase 1 = page-lo x query-hi on all 2 QW chains, phase 2 =
                            // page-hi x query-lo, then page-hi x query-hi.  Only ONE plane's fragments of the current half and
                            // the prefetched plane of the next are live (32 VGPRs instead of 64 for both planes of both halves),
                            // which is what lets QW = 2 (128 VGPRs of query fragments) fit; accumulation order per chain is
                            // the same as chain()'s.
                            auto load_plane = [&](frag (&a)[4], int h, int pl) {
                                const char* tb = sbase + (h >> 1) * TILE_B + (h & 1) * (16 * EVDR_D * 2) + pl * TILE_BYTES;
                                // with the argmax the register file is full: the swizzle term is made opaque per call, so that the four
                                // LDS address variants are rebuilt (4 VALU) instead of being hoisted out of the page loop and spilled
                                int gx = g ^ c;
                                if constexpr (ARGMAX || ST == 3) asm volatile("" : "+v"(gx));
#pragma unroll
                                for (int s4 = 0; s4 < 4; ++s4) a[s4] = *reinterpret_cast<const frag*>(tb + (((4 * s4) ^ gx) << 4));
                            };
                            // (NCB column blocks: the same three phases per block, into the same accumulators; page planes hi_cb = cb,
                            // lo_cb = NCB + cb, and likewise for the query fragments)
                            frag al[4], ah[4];
                            load_plane(al, 0, NCB);
                            load_plane(ah, 0, 0);
#pragma unroll
                            for (int h = 0; h < 2 * ST; ++h) {
                                set_prio(h);
                                f32x4v acc[QW][2];
#pragma unroll
                                for (int j = 0; j < QW; ++j) acc[j][0] = acc[j][1] = f32x4v{0, 0, 0, 0};
#pragma unroll
                                for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
                                    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                                        for (int j = 0; j < QW; ++j)
#pragma unroll
                                            for (int t = 0; t < 2; ++t) acc[j][t] = mfma16(al[s4], bq[j][cb][t][s4], acc[j][t]);
                                    asm volatile("" ::: "memory");
                                    if (cb == 0) fault_hold(h == 2 * ST - 3);
                                    if (cb + 1 < NCB) load_plane(al, h, NCB + cb + 1);
                                    else if (h + 1 < 2 * ST) load_plane(al, h + 1, NCB);
                                    if constexpr (SP) {
                                        if (cb == 0 && (h & 1) == 0) {
#pragma unroll
                                            for (int i = refill_lo(h >> 1); i < refill_hi(h >> 1); ++i) issue_piece(nbase, nt0, 0, 0, nslot, i, std::true_type{});
                                        }
                                    }
#pragma unroll
                                    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                                        for (int j = 0; j < QW; ++j)
#pragma unroll
                                            for (int t = 0; t < 2; ++t) acc[j][t] = mfma16(ah[s4], bq[j][NCB + cb][t][s4], acc[j][t]);
#pragma unroll
                                    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                                        for (int j = 0; j < QW; ++j)
#pragma unroll
                                            for (int t = 0; t < 2; ++t) acc[j][t] = mfma16(ah[s4], bq[j][cb][t][s4], acc[j][t]);
                                    // the next half's hi-plane fragments go into the registers the last product just released: the
                                    // LDS reads must not be hoisted above it (the scheduler did, and paid with spills INSIDE the block,
                                    // whose scratch reloads wait on vmcnt -- i.e. on the LDS-DMA refill in flight)
                                    asm volatile("" ::: "memory");
                                    if (cb + 1 < NCB) load_plane(ah, h, cb + 1);
                                    else if (h + 1 < 2 * ST) load_plane(ah, h + 1, 0);
                                }
                                const int pb = (t0 + (h >> 1)) * EVDR_TILE_PATCHES + 16 * (h & 1) + 4 * g;
#pragma unroll
                                for (int j = 0; j < QW; ++j)
#pragma unroll
                                    for (int t = 0; t < 2; ++t) fold(acc[j][t], j, t, pb);
                            // argmax on fp16 planes: the scheduler may not pull the next half-step's work above this half-step's
                            // (VALU-heavy) fold -- it did, ran out of registers and spilled inside the block (23 -> 9 spilled VGPRs, -3.5 % time)
                            if constexpr (NPL == 2 && ARGMAX) __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    };
                    // one straight-line instance per (refill placement, workgroup half): no run-time branch inside the block
                    auto by_half = [&](auto sp, auto hd) {
                        if (BAL && wave >= WAVES / 2) fast_block(sp, std::true_type{}, hd); else fast_block(sp, std::false_type{}, hd);
                    };
                    if constexpr (NPL == 1) {
                        if (headmask != 0xFFFFFFFFu) {
                            if (spread) by_half(std::true_type{}, std::true_type{}); else by_half(std::false_type{}, std::true_type{});
                        } else {
                            if (spread) by_half(std::true_type{}, std::false_type{}); else by_half(std::false_type{}, std::false_type{});
                        }
                    } else {
                        if (spread) by_half(std::true_type{}, std::false_type{}); else by_half(std::false_type{}, std::false_type{});
                    }
                    if (spread) issue_extra(npgi, nk, p.ntiles, nslot);      // the next stage's tail-tile pieces, after the block
                    if constexpr (DIAG) { const unsigned long long t = stamp(); d_fast += t - d_a; d_a = t; }
                    if (nt > ST) generic_tile(ST);                       // tail tile riding in this (last) stage
                    if constexpr (DIAG) { const unsigned long long t = stamp(); d_gen += t - d_a; d_a = t; }
                } else {
                    // ---- partially valid stage (the boundary stage of a ragged page, a stage with a few masked patches --
                    // e.g. the text-prefix tokens in front of the image patches, utils/preprocess_data.py:101): runs of FULL
                    // tiles go through a rolled per-tile loop with the fast block's fragment prefetch and no mask logic in
                    // between (one tile = 32 x QW MFMAs per loop-back); only partial tiles take the per-half generic path, and
                    // empty tiles cost nothing.  Which tiles are full: from the valid range, or from the mask words.
                    uint32_t fullbits = 0u;
                    if (va >= 0) {                                    // tiles [ceil(va/32), floor(vb/32)) of the page are full
                        int f0 = ((va + 31) >> 5) - t0, f1 = (vb >> 5) - t0;
                        f0 = f0 < 0 ? 0 : f0;
                        f1 = f1 > nt ? nt : f1;
                        if (f1 > f0) fullbits = ((1u << f1) - 1u) & ~((1u << f0) - 1u);
                    } else {
                        for (int tis = 0; tis < nt; ++tis)
                            fullbits |= (tilemask_c[(int64_t)page * p.ntiles + t0 + tis] == 0xFFFFFFFFu ? 1u : 0u) << tis;
                    }
                    auto full_run = [&](int tis0, int len) {
                        if constexpr (NPL == 1) {
                            frag alo[NPLN][4], ahi[NPLN][4];
                            load_half(alo, sbase, tis0, 0);
                            load_half(ahi, sbase, tis0, 1);
#pragma unroll 1
                            for (int i = 0; i < len; ++i) {
                                const int tis = tis0 + i;
                                const int nx = (i + 1 < len) ? tis + 1 : tis;        // the last prefetch re-reads its own tile
                                const int pbase = (t0 + tis) * EVDR_TILE_PATCHES;
                                chains_full(alo, pbase);
                                load_half(alo, sbase, nx, 0);
                                chains_full(ahi, pbase + 16);
                                load_half(ahi, sbase, nx, 1);
                            }
                        } else {
                            auto load_plane = [&](frag (&a)[4], int h, int pl) {
                                const char* tb = sbase + (h >> 1) * TILE_B + (h & 1) * (16 * EVDR_D * 2) + pl * TILE_BYTES;
                                // with the argmax the register file is full: the swizzle term is made opaque per call, so that the four
                                // LDS address variants are rebuilt (4 VALU) instead of being hoisted out of the page loop and spilled
                                int gx = g ^ c;
                                if constexpr (ARGMAX || ST == 3) asm volatile("" : "+v"(gx));
#pragma unroll
                                for (int s4 = 0; s4 < 4; ++s4) a[s4] = *reinterpret_cast<const frag*>(tb + (((4 * s4) ^ gx) << 4));
                            };
                            frag al[4], ah[4];
                            load_plane(al, 2 * tis0, NCB);
                            load_plane(ah, 2 * tis0, 0);
#pragma unroll 1
                            for (int i = 0; i < len; ++i) {
#pragma unroll
                                for (int u = 0; u < 2; ++u) {
                                    const int h = 2 * (tis0 + i) + u;
                                    const int hn = (u == 0 || i + 1 < len) ? h + 1 : h;
                                    f32x4v acc[QW][2];
#pragma unroll
                                    for (int j = 0; j < QW; ++j) acc[j][0] = acc[j][1] = f32x4v{0, 0, 0, 0};
#pragma unroll
                                    for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
                                        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                                            for (int j = 0; j < QW; ++j)
#pragma unroll
                                                for (int t = 0; t < 2; ++t) acc[j][t] = mfma16(al[s4], bq[j][cb][t][s4], acc[j][t]);
                                        if (cb + 1 < NCB) load_plane(al, h, NCB + cb + 1); else load_plane(al, hn, NCB);
#pragma unroll
                                        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                                            for (int j = 0; j < QW; ++j)
#pragma unroll
                                                for (int t = 0; t < 2; ++t) acc[j][t] = mfma16(ah[s4], bq[j][NCB + cb][t][s4], acc[j][t]);
#pragma unroll
                                        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                                            for (int j = 0; j < QW; ++j)
#pragma unroll
                                                for (int t = 0; t < 2; ++t) acc[j][t] = mfma16(ah[s4], bq[j][cb][t][s4], acc[j][t]);
                                        if (cb + 1 < NCB) load_plane(ah, h, cb + 1); else load_plane(ah, hn, 0);
                                    }
                                    const int pb = (t0 + (h >> 1)) * EVDR_TILE_PATCHES + 16 * (h & 1) + 4 * g;
#pragma unroll
                                    for (int j = 0; j < QW; ++j)
#pragma unroll
                                        for (int t = 0; t < 2; ++t) fold(acc[j][t], j, t, pb);
                                // argmax on fp16 planes: the scheduler may not pull the next half-step's work above this half-step's
                                // (VALU-heavy) fold -- it did, ran out of registers and spilled inside the block (23 -> 9 spilled VGPRs, -3.5 % time)
                                if constexpr (NPL == 2 && ARGMAX) __builtin_amdgcn_sched_barrier(0);
                                }
                            }
                        }
                    };
                    for (int tis = 0; tis < nt;) {
                        const uint32_t rest = fullbits >> tis;
                        if (rest & 1u) {
                            int len = __builtin_ctz(~rest);                           // length of the run of full tiles
                            len = len > nt - tis ? nt - tis : len;
                            full_run(tis, len);
                            tis += len;
                        } else {
                            generic_tile(tis);
                            ++tis;
                        }
                    }
                }
            }
            if constexpr (DIAG) { if (!fast) { const unsigned long long t = stamp(); d_gen += t - d_a; d_a = t; } }
            slot ^= 1;
        }
        page_open = page_close;
        if (!page_close) continue;
        if constexpr (DIAG) d_a = stamp();
        // ---- page finished: fold lane groups, weight, reduce over tokens, store
        if (active) {
            const float has = (pflags & 1u) ? 1.f : 0.f;
#pragma unroll
            for (int j = 0; j < QW; ++j) {
                float cs = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float v = run[j][t];
                    int bi = ridx[j][t];
                    if constexpr (ARGMAX) xgroup_argmax(v, bi); else v = xgroup_max(v);
                    if constexpr (SCALED) {
                        v *= inv;
                        if (pflags & 2u) {                                 // the masked patches' -1e4 joins the max here
                            const int fm = first_masked;
                            const bool take = (-1e4f > v) || (-1e4f == v && fm < bi);
                            v = take ? -1e4f : v;
                            bi = take ? fm : bi;
                        }
                    }
                    // (opaque per page: otherwise the 64-bit per-lane output offsets of all (query, token) slots are hoisted out of
                    // the page loop -- 16 VGPRs that end up spilled, with their reloads landing inside the MFMA blocks)
                    int tok = 16 * t + c;
                    asm volatile("" : "+v"(tok));
                    if (p.per_token) {
                        // packed single-token queries: one score (and argmax) per token, no sum over the pack
                        const int64_t qrow = (int64_t)qreal[j] * 32 + tok;
                        if (g == 0 && qreal[j] >= 0 && qrow < p.per_token) {
                            float o = v * has * qwt[j][t];
                            if ((pflags & 1u) && ((pflags & 8u) || ((qbad[j] >> tok) & 1u))) o = opaque_nan();
                            if constexpr (PAGES) o = (pflags == HOLE_FLAGS) ? hole_value() : o;
                            p.out[qrow * p.out_stride + ocol] = o;
                            if constexpr (ARGMAX) p.argmax[qrow * p.np + ocol] = (uint16_t)bi;
                        }
                        continue;
                    }
                    if constexpr (ARGMAX) {
                        if constexpr (DEFER) {
                            pend_bi[j][t] = bi;                            // stored by flush_pending(), behind the next hand-over
                        } else {
                            if (g == 0 && tok < p.lq && qreal[j] >= 0)
                                p.argmax[((int64_t)qreal[j] * p.np + ocol) * p.lq_total + p.tok0 + tok] = (uint16_t)bi;
                        }
                    }
                    cs += v * has * qwt[j][t];
                }
                if (p.per_token) continue;
                cs = row16_sum(cs);
                if ((pflags & 1u) && ((pflags & 8u) || qbad[j] != 0u)) cs = opaque_nan();
                if constexpr (PAGES) cs = (pflags == HOLE_FLAGS) ? hole_value() : cs;             // a hole's column: -inf in every slice (-inf + -inf)
                if constexpr (DEFER) {
                    pend_cs[j] = cs;
                } else {
                    if (lane == 0 && qreal[j] >= 0) {
                        float* o = p.out + (int64_t)qreal[j] * p.out_stride + ocol;
                        if (p.accumulate) atomicAdd(o, cs);
                        else *o = cs;
                    }
                }
            }
            if constexpr (DEFER) {
                if (!p.per_token) pend_page = ocol;
            }
        }
        if constexpr (DIAG) d_fin += stamp() - d_a;
    }
    flush_pending();                                    // the workgroup's last page
    if constexpr (DIAG) {
        if (p.dbg != nullptr && lane == 0 && blockIdx.x < 4096) {
            unsigned long long* o = p.dbg + ((size_t)blockIdx.x * 8 + wave) * 8;
            o[0] = stamp() - d_t0; o[1] = d_pro; o[2] = d_bar; o[3] = d_ref; o[4] = d_fast; o[5] = d_gen; o[6] = d_fin;
            o[7] = d_ctl;
        }
    }
