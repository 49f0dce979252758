// k_gexp_v7.inc -- K1s with TWO HALF-SIZE ACCUMULATOR SETS (VERDICT r4 #1b), included by k_gemm.hip behind k_gexp_v6.inc, whose
// register map, MFMA / fragment-read / epilogue-group helpers and operand image it shares.
//   replaces  image_features @ text_features.T  (concept_vit/utils.py:594)  fused with  softmax(a * clip_feats, dim=1)'s
//   numerator (concept_vit/similarity.py:54), stress chain only (bf16, no parity claim).
//
// v6 runs the epilogue of tile i inside the first two k-steps of tile i + 1: a boundary phase of ~7 900 cycles that is bound by
// the ONE wave's instruction issue while the matrix pipe is 39 % busy, followed by 14 plain k-steps in which the wave's issue is
// half empty (profiles/r05_gexp_v6.txt (h), (i), (k)).  v7 spreads the epilogue evenly instead:
//   * a workgroup tile is 256 concepts x 128 images, a wave's 128 x 64: 32 accumulator blocks, and the 8 x 8 block grid of v6's
//     register map holds TWO of them -- image columns 0..3 (tiles of even parity) and 4..7 (odd parity);
//   * while the 16 k-steps of tile i + 1 accumulate into one set (32 MFMAs each), k-step u carries step u of tile i's epilogue on
//     the other set -- one 8-concept group of one image column: 8 v_exp_f32, 4 v_cvt_pk_bf16_f32, its 16-byte piece into the
//     transposition buffer, the read-back of one 4-row slice of the previous column, the store of the slice read one step
//     earlier, one row-sum MFMA -- each in its own MFMA gap.  The last column's slices leave in steps 0..4 of the tile after;
//   * per k-step a wave issues 6 DMA pieces (A 16 + B 8 pieces of 1 KB per workgroup) and 12 fragment reads.
// One E store per k-step rides in the vmcnt window of every sync point (in order, stores count): they sit in front of the
// step's DMA pieces, so a sync point waits for the stores that are three steps old.
//
// Registers: as v6 (v0..v59 compiler | v60..v63 constant block | accumulator blocks (mi, nj) | fragment sets | selectors);
// the row sums of even / odd tiles collect in a204..a207 / a208..a211.
#ifndef MCD_K_GEXP_V7_INC
#define MCD_K_GEXP_V7_INC

constexpr int G7_SLOT = 24576;       // one k-step of the ring: A pieces 0..15 | B pieces 0..7
constexpr int G7_RING = 4 * G7_SLOT;
constexpr int G7_LDS = G7_RING + 4 * G6_LT;

// block (MI, NJ) += A fragment MI x B fragment JB of set SET; FIRST: C = the constant block
template <int MI, int NJ, int JB, int SET, bool FIRST>
__device__ __forceinline__ void g7_mfma() {
    constexpr int d = g6_acc_reg(MI, NJ), fa = G6_FRAG0 + 64 * SET + 4 * MI, fb = G6_FRAG0 + 64 * SET + 32 + 4 * JB;
    if constexpr (NJ < 6) {
        constexpr int c = FIRST ? G6_VCB0 : d;
        asm volatile("v_mfma_f32_16x16x32_bf16 v[%c0:%c1], a[%c2:%c3], a[%c4:%c5], v[%c6:%c7]"
                     ::"i"(d), "i"(d + 3), "i"(fa), "i"(fa + 3), "i"(fb), "i"(fb + 3), "i"(c), "i"(c + 3));
    } else {
        constexpr int c = FIRST ? G6_CB0 : d;
        asm volatile("v_mfma_f32_16x16x32_bf16 a[%c0:%c1], a[%c2:%c3], a[%c4:%c5], a[%c6:%c7]"
                     ::"i"(d), "i"(d + 3), "i"(fa), "i"(fa + 3), "i"(fb), "i"(fb + 3), "i"(c), "i"(c + 3));
    }
}
template <int R>
__device__ __forceinline__ void g7_exp() { asm volatile("v_exp_f32 v%c0, v%c0" ::"i"(R)); }
template <int D, int A, int B>
__device__ __forceinline__ void g7_cvt() { asm volatile("v_cvt_pk_bf16_f32 v%c0, v%c1, v%c2" ::"i"(D), "i"(A), "i"(B)); }
// row-sum MFMA of the piece in block (2 P, NJ)'s registers into row-sum block RS (FIRST: C = 0)
template <int P, int NJ, int RS, bool FIRST>
__device__ __forceinline__ void g7_epi_sum() {
    constexpr int b0 = g6_acc_reg(2 * P, NJ), sel = G6_SEL0 + 4 * NJ, rs = G6_RS0 + 4 * RS;
    if constexpr (FIRST)
        asm volatile("v_mfma_f32_16x16x32_bf16 a[%c0:%c1], a[%c2:%c3], v[%c4:%c5], 0" ::"i"(rs), "i"(rs + 3), "i"(sel), "i"(sel + 3), "i"(b0), "i"(b0 + 3));
    else
        asm volatile("v_mfma_f32_16x16x32_bf16 a[%c0:%c1], a[%c2:%c3], v[%c4:%c5], a[%c0:%c1]" ::"i"(rs), "i"(rs + 3), "i"(sel), "i"(sel + 3), "i"(b0), "i"(b0 + 3));
}
template <int NJ, int RS>
__device__ __forceinline__ void g7_rowsum(const u32x4& v) {
    constexpr int sel = G6_SEL0 + 4 * NJ, rs = G6_RS0 + 4 * RS;
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 a[%c1:%c2], a[%c3:%c4], %0, a[%c1:%c2]" ::"v"(v), "i"(rs), "i"(rs + 3), "i"(sel), "i"(sel + 3));
}
template <int N>
__device__ __forceinline__ void g7_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ABLATE: 0 product, 1 no E stores, 4 K loop only (no epilogue work at all), 8 s_memtime stamps at every tile top (+1: without the stores)
template <int ABLATE, int STAUX = 2>
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_num_vgpr(G6_NVGPR))) void gemm_nt_bf16_exp_v7_kernel(
    const unsigned short* __restrict__ A /* concepts, fragment-major, paired, pre-scaled by a log2(e) */,
    const unsigned short* __restrict__ B /* images, fragment-major */, int64_t Kp, int64_t Mc, int64_t Ni,
    unsigned short* __restrict__ E, int64_t ldE, float* __restrict__ part, int64_t ldpart, float s1 /* a * log2(e) */,
    int tiles_m /* of 256 concepts */, int tiles_n /* of 128 images */) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    g6_claim_registers();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileWalkR W(tiles_m, tiles_n);
    const int nt = (int)(Kp >> 5), nt4 = nt >> 2;          // host: nt % 4 == 0, nt >= 16
    if (W.count() == 0) return;
    const int wr = wave >> 1, wc = wave & 1;
    g6_for<8>([&](auto n_c) __attribute__((always_inline)) { g6_set_sel<decltype(n_c)::value>((unsigned)lane); });
    g6_setc(-s1);
    constexpr bool NOEPI = (ABLATE & 4) != 0;
    constexpr int NS = (ABLATE & 5) ? 0 : 1;           // E stores per epilogue step

    // ---- DMA side: this wave's pieces of a k-step: A row blocks 4 i + wave (i = 0..3), B row blocks 4 i + wave (i = 0, 1)
    const int nrbA = (int)(((Mc + 31) >> 5) << 1), nrbB = (int)((Ni + 15) >> 4);
    __amdgpu_buffer_rsrc_t ra_ = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, (int)((int64_t)nrbA * 16 * Kp * 2), 0x00020000);
    __amdgpu_buffer_rsrc_t rb_ = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, (int)((int64_t)nrbB * 16 * Kp * 2), 0x00020000);
    const unsigned vlane = (unsigned)(lane * 16);
    const int wave1024 = wave * 1024;
    int oa0, oa1, oa2, oa3, ob0, ob1;
#define G7_BLK(nrb_, b_) ((((b_) < (nrb_)) ? (b_) : (nrb_) - 1) * nt * 1024)
#define G7_SET_TILE(tm_, tn_)                                                        \
    do {                                                                             \
        const int ba_ = (tm_) * 16 + wave, bb_ = (tn_) * 8 + wave;                   \
        oa0 = G7_BLK(nrbA, ba_); oa1 = G7_BLK(nrbA, ba_ + 4); oa2 = G7_BLK(nrbA, ba_ + 8); oa3 = G7_BLK(nrbA, ba_ + 12); \
        ob0 = G7_BLK(nrbB, bb_); ob1 = G7_BLK(nrbB, bb_ + 4);                        \
    } while (0)
#define G7_DMA(U_, i_, kt1024_)                                                                                              \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                                                \
        (i_) < 4 ? ra_ : rb_,                                                                                                \
        (__attribute__((address_space(3))) void*)(smem + (U_) * G7_SLOT + ((i_) < 4 ? 0 : 16384) + 4096 * ((i_) & 3) + wb_), \
        16, vlane, ((i_) == 0 ? oa0 : (i_) == 1 ? oa1 : (i_) == 2 ? oa2 : (i_) == 3 ? oa3 : (i_) == 4 ? ob0 : ob1) + (kt1024_), 0, 0)

    // ---- compute side: fragment i of this wave's A / B part of the k-step in slot U
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned a_lo = lds0 + (unsigned)(lane * 16 + wr * 8192), b_lo = lds0 + (unsigned)(lane * 16 + 16384 + wc * 4096);
    unsigned a_hi = a_lo + 2u * G7_SLOT, b_hi = b_lo + 2u * G7_SLOT;
    asm volatile("" : "+v"(a_hi), "+v"(b_hi));
#define G7_RDA(SET_, U_, i_) g6_read<SET_, false, i_, ((U_) & 1) * G7_SLOT + (i_) * 1024>((U_) < 2 ? a_lo : a_hi)
#define G7_RDB(SET_, U_, j_) g6_read<SET_, true, j_, ((U_) & 1) * G7_SLOT + (j_) * 1024>((U_) < 2 ? b_lo : b_hi)

    int ci = -1, tm, tn;
    W.next(ci, tm, tn);
    G7_SET_TILE(tm, tn);
    {
        const int wb_ = wave1024;
        g6_for<4>([&](auto u_c) __attribute__((always_inline)) {
            constexpr int u = decltype(u_c)::value;
            G7_DMA(u, 0, u * 1024); G7_DMA(u, 1, u * 1024); G7_DMA(u, 2, u * 1024); G7_DMA(u, 3, u * 1024);
            G7_DMA(u, 4, u * 1024); G7_DMA(u, 5, u * 1024);
        });
    }
    asm volatile("s_waitcnt vmcnt(18) lgkmcnt(0)" ::: "memory");   // k-step 0 landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    g6_for<8>([&](auto i_c) __attribute__((always_inline)) { G7_RDA(0, 0, decltype(i_c)::value); });
    g6_for<4>([&](auto j_c) __attribute__((always_inline)) { G7_RDB(0, 0, decltype(j_c)::value); });
    // the walk after the first tile without a division per tile (as v6)
    const int wq_ = W.nslot / W.nrow_x, wd_ = W.nslot - wq_ * W.nrow_x;
    int seq_ = W.slot, wr_idx = (tm - W.xcd) >> 3;
    int ntm = tm, ntn = tn;
    bool has_next;
#define G7_WALK_NEXT()                                                                  \
    do {                                                                                \
        seq_ += W.nslot;                                                                \
        has_next = seq_ < W.n_seq;                                                      \
        int r_ = wr_idx + wd_, c_ = ntn + wq_;                                          \
        if (r_ >= W.nrow_x) { r_ -= W.nrow_x; ++c_; }                                   \
        wr_idx = r_;                                                                    \
        ntn = c_;                                                                       \
        ntm = W.xcd + 8 * r_;                                                           \
    } while (0)
    G7_WALK_NEXT();

    unsigned long long* const stamps = reinterpret_cast<unsigned long long*>(part) + wave * 256;
    int tile_no = 0;

    // ---- what the epilogue needs of a tile (its E window, row-sum row, edge): kept for the tile whose exponentials ride the
    // current K loop ("prev") and for the one before ("pp": its last column's slices and its row sums leave in steps 0..4)
    // lane-dependent constants of the epilogue (live across the K loop: the loop itself needs few vector registers)
    const unsigned rrow = (unsigned)lane >> 4, rchunk = (unsigned)lane & 15u, efr = rchunk, efq = rrow;
    unsigned lane_base2 = (rrow * (unsigned)ldE + rchunk * 8u) * 2u;           // byte offset of this lane's 16 bytes within a 4-row slice
    const unsigned tb0 = lds0 + (unsigned)(G7_RING + wave * G6_LT) + efr * 256;
    unsigned wa0 = tb0 + ((efq ^ efr) << 4), wa1 = tb0 + (((4u + efq) ^ efr) << 4), wa2 = tb0 + (((8u + efq) ^ efr) << 4),
             wa3 = tb0 + (((12u + efq) ^ efr) << 4);
    const unsigned tbr = lds0 + (unsigned)(G7_RING + wave * G6_LT);
    unsigned ra0 = tbr + rrow * 256 + ((rchunk ^ rrow) << 4), ra1 = tbr + (4u + rrow) * 256 + ((rchunk ^ (4u + rrow)) << 4),
             ra2 = tbr + (8u + rrow) * 256 + ((rchunk ^ (8u + rrow)) << 4), ra3 = tbr + (12u + rrow) * 256 + ((rchunk ^ (12u + rrow)) << 4);
    asm volatile("" : "+v"(wa0), "+v"(wa1), "+v"(wa2), "+v"(wa3), "+v"(ra0), "+v"(ra1), "+v"(ra2), "+v"(ra3), "+v"(lane_base2));
    const unsigned lane4 = (unsigned)lane * 4u;
    struct Desc {
        unsigned short* e_base;     // this wave's first element of the tile in E
        float* p_base;              // this wave's first row sum of the tile
        int e_room, p_room;         // bytes of the E / row-sum windows (0: nothing is stored)
        int c_room, p_crem;         // concepts of this wave inside the row pitch / real (clamped to +-4096)
    };
    auto make_desc = [&](int tm_, int tn_) __attribute__((always_inline)) {
        Desc d;
        const int c0_ = tm_ * 256 + wr * 128, i0_ = tn_ * 128 + wc * 64;
        const int left_ = (int)Ni - i0_;
        const int rows_ = left_ < 64 ? (left_ > 0 ? left_ : 0) : 64;
        d.e_base = E + ((int64_t)i0_ * ldE + c0_);
        d.p_base = part + ((int64_t)(tm_ * 2 + wr) * ldpart + i0_);
        d.e_room = __builtin_amdgcn_readfirstlane(rows_ > 0 ? rows_ * (int)ldE * 2 - c0_ * 2 : 0);
        d.p_room = __builtin_amdgcn_readfirstlane(rows_ * 4);
        const int croom_ = (int)ldE - c0_, crem_ = (int)Mc - c0_;
        d.c_room = croom_ < 4096 ? (croom_ > -4096 ? croom_ : -4096) : 4096;
        d.p_crem = crem_ < 4096 ? (crem_ > -4096 ? crem_ : -4096) : 4096;
        return d;
    };
    Desc d_prev{E, part, 0, 0, 4096, 4096}, d_pp{E, part, 0, 0, 4096, 4096};
    u32x4 wq = {0u, 0u, 0u, 0u};                      // the slice read in the previous step, not yet stored

#define G7_LDS_U32X4(a_) (*(__attribute__((address_space(3))) u32x4*)(uintptr_t)(a_))
#define G7_READ_SLICE(col_, p_) G7_LDS_U32X4(((p_) == 0 ? ra0 : (p_) == 1 ? ra1 : (p_) == 2 ? ra2 : ra3) + ((col_) & 1) * 4096)
#define G7_STORE_SLICE(w_, rs_, off2_, col_, p_)                                                                             \
    do {                                                                                                                     \
        if constexpr (ABLATE & 1) {                                                                                          \
            asm volatile("" ::"v"(w_));                                                                                      \
        } else {                                                                                                             \
            __builtin_amdgcn_raw_buffer_store_b128(w_, rs_, (off2_) + (unsigned)((((col_) * 16 + 4 * (p_)) * (int)ldE) * 2), 0, STAUX); \
        }                                                                                                                    \
    } while (0)

    // ---- one k-step.  U: its number within the tile's first four ring rounds (MODE 0) or within a later round (MODE 1: no epilogue
    // work); T: the parity of the tile being accumulated (its blocks: image columns 4 T .. 4 T + 3); the epilogue step (MODE 0)
    // works on the other set: group p = U & 3 of local column U >> 2 of tile "prev".
    // Gap k (behind MFMA k of 32): 0 the store of the slice read one step earlier (+ row sums of "pp" in step 1); odd k <= 11 the
    // fragment reads of k-step U + 1, two per gap; odd 13..23 the DMA pieces of k-step U + 4 (behind the store: the vmcnt windows
    // rely on it); even 2..16 the exponentials; 18, 20 the packs; 22 mask; 24 piece -> buffer; 26 slice read; 28 row-sum MFMA.
    auto kstep = [&](auto u_c, auto t_c, auto m_c, int kt1024, bool prev_e, bool first_plain, const __amdgpu_buffer_rsrc_t rs_prev,
                     const __amdgpu_buffer_rsrc_t rs_pp, const __amdgpu_buffer_rsrc_t rs_part, unsigned off2_prev, unsigned off2_pp,
                     bool edge_prev, int p_crem_prev) __attribute__((always_inline)) {
        constexpr int U = decltype(u_c)::value, T = decltype(t_c)::value, MODE = decltype(m_c)::value;
        constexpr int SL = U & 3, SET = U & 1, SN = (U + 1) & 3, NSET = SET ^ 1;
        constexpr bool EPI = MODE == 0 && !NOEPI;
        constexpr bool FIRST = MODE == 0 && U == 0;
        constexpr int EP = T ^ 1, p = U & 3, itl = (U >> 2) & 3, IT = 4 * EP + itl;
        int wb_ = wave1024;
        asm volatile("" : "+s"(wb_));
        // sync point: own pieces of k-step U + 1 landed; younger than them: the 12 pieces of the next two k-steps and the stores of the
        // last two steps (one per epilogue step, two in step 1)
        if constexpr (MODE == 0 && !NOEPI) {
            if constexpr (U == 0) { if (prev_e) g7_wait_vm<12 + 2 * NS>(); else g7_wait_vm<12>(); }
            else if constexpr (U == 1) { if (prev_e) g7_wait_vm<12 + 2 * NS>(); else g7_wait_vm<12 + NS>(); }
            else if constexpr (U == 2 || U == 3) g7_wait_vm<12 + 2 * NS + 1>();
            else g7_wait_vm<12 + 2 * NS>();
        } else if constexpr (MODE == 1 && !NOEPI) {
            if constexpr (U == 0) { if (first_plain) g7_wait_vm<12 + 2 * NS>(); else g7_wait_vm<12>(); }
            else if constexpr (U == 1) { if (first_plain) g7_wait_vm<12 + NS>(); else g7_wait_vm<12>(); }
            else g7_wait_vm<12>();
        } else {
            g7_wait_vm<12>();
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        [[maybe_unused]] float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f, e4 = 0.f, e5 = 0.f, e6 = 0.f, e7 = 0.f;
        [[maybe_unused]] u32x4 v = {0u, 0u, 0u, 0u};
        g6_for<32>([&](auto k_c) __attribute__((always_inline)) {
            constexpr int k = decltype(k_c)::value;
            g7_mfma<(k >> 2), 4 * T + (k & 3), (k & 3), SET, FIRST>();
            __builtin_amdgcn_sched_barrier(0);
            // fragment reads of the next k-step into the other register set, two per gap
            if constexpr ((k & 1) && k <= 11) {
                constexpr int r = (k - 1) >> 1;
                if constexpr (r < 4) { G7_RDA(NSET, SN, r); G7_RDB(NSET, SN, r); }
                else { G7_RDA(NSET, SN, (2 * r - 4)); G7_RDA(NSET, SN, (2 * r - 3)); }
            }
            // DMA pieces of k-step U + 4 into this slot (behind the step's stores)
            if constexpr ((k & 1) && k >= 13 && k <= 23) G7_DMA(SL, ((k - 13) >> 1), kt1024);
            if constexpr (EPI) {
                constexpr int b0 = g6_acc_reg(2 * p, IT), b1 = g6_acc_reg(2 * p + 1, IT);
                if constexpr (k == 0) {
                    // the slice read one step earlier: steps 0..4 finish tile "pp" (column 2 slice 3, column 3), 5..15 serve "prev".
                    // (First in the step: the compiler, which does not see the fragment reads, waits lgkmcnt(0) for the slice here,
                    // and right behind the sync point nothing is in flight.)
                    if constexpr (U == 0) G7_STORE_SLICE(wq, rs_pp, off2_pp, 2, 3);
                    else if constexpr (U <= 4) G7_STORE_SLICE(wq, rs_pp, off2_pp, 3, U - 1);
                    else G7_STORE_SLICE(wq, rs_prev, off2_prev, ((U - 1) >> 2) - 1, (U - 1) & 3);
                    if constexpr (U == 1 && !(ABLATE & 8)) {
                        // row sums of tile "pp" (same parity as this tile): lane (fq, fr): image 16 fq + fr of the wave's 64
                        const float rsum = g6_acc<G6_RS0 + 4 * T + 2 * T>();
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rsum), rs_part, lane4, 0, 0);
                    }
                }
                if constexpr (IT < 6) {
                    if constexpr (k == 2) g7_exp<b0>();
                    if constexpr (k == 4) g7_exp<b0 + 1>();
                    if constexpr (k == 6) g7_exp<b0 + 2>();
                    if constexpr (k == 8) g7_exp<b0 + 3>();
                    if constexpr (k == 10) g7_exp<b1>();
                    if constexpr (k == 12) g7_exp<b1 + 1>();
                    if constexpr (k == 14) g7_exp<b1 + 2>();
                    if constexpr (k == 16) g7_exp<b1 + 3>();
                    if constexpr (k == 18) { g7_cvt<b0, b0, b0 + 1>(); g7_cvt<b0 + 1, b0 + 2, b0 + 3>(); }
                    if constexpr (k == 20) { g7_cvt<b0 + 2, b1, b1 + 1>(); g7_cvt<b0 + 3, b1 + 2, b1 + 3>(); }
                } else {
                    if constexpr (k == 2) e0 = __builtin_amdgcn_exp2f(g6_acc<b0>());
                    if constexpr (k == 4) e1 = __builtin_amdgcn_exp2f(g6_acc<b0 + 1>());
                    if constexpr (k == 6) e2 = __builtin_amdgcn_exp2f(g6_acc<b0 + 2>());
                    if constexpr (k == 8) e3 = __builtin_amdgcn_exp2f(g6_acc<b0 + 3>());
                    if constexpr (k == 10) e4 = __builtin_amdgcn_exp2f(g6_acc<b1>());
                    if constexpr (k == 12) e5 = __builtin_amdgcn_exp2f(g6_acc<b1 + 1>());
                    if constexpr (k == 14) e6 = __builtin_amdgcn_exp2f(g6_acc<b1 + 2>());
                    if constexpr (k == 16) e7 = __builtin_amdgcn_exp2f(g6_acc<b1 + 3>());
                    if constexpr (k == 18) { v.x = pack_bf16(e0, e1); v.y = pack_bf16(e2, e3); }
                    if constexpr (k == 20) { v.z = pack_bf16(e4, e5); v.w = pack_bf16(e6, e7); }
                }
                if constexpr (k == 22) {
                    if (edge_prev) {      // concepts past the last one: cleared in the packed piece
                        const int n = p_crem_prev - 8 * (int)efq - 32 * p;
                        const unsigned m0 = n >= 2 ? 0xffffffffu : n == 1 ? 0xffffu : 0u, m1 = n >= 4 ? 0xffffffffu : n == 3 ? 0xffffu : 0u;
                        const unsigned m2 = n >= 6 ? 0xffffffffu : n == 5 ? 0xffffu : 0u, m3 = n >= 8 ? 0xffffffffu : n == 7 ? 0xffffu : 0u;
                        if constexpr (IT < 6) g6_epi_mask<p, IT>(m0, m1, m2, m3); else v &= u32x4{m0, m1, m2, m3};
                    }
                }
                if constexpr (k == 24) {
                    if constexpr (IT < 6) g6_epi_put<p, IT, (itl & 1) * 4096>(p == 0 ? wa0 : p == 1 ? wa1 : p == 2 ? wa2 : wa3);
                    else G7_LDS_U32X4((p == 0 ? wa0 : p == 1 ? wa1 : p == 2 ? wa2 : wa3) + (itl & 1) * 4096) = v;
                }
                if constexpr (k == 26) wq = G7_READ_SLICE(itl == 0 ? 3 : itl - 1, p);
                if constexpr (k == 28) { if constexpr (IT < 6) g7_epi_sum<p, IT, EP, U == 0>(); else g7_rowsum<IT, EP>(v); }
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    };

    // ---- an epilogue step on its own (behind a workgroup's last tile): EP = the parity of the tile whose sums are in the accumulators
    auto drain_step = [&](auto u_c, auto ep_c, const __amdgpu_buffer_rsrc_t rs_prev, const __amdgpu_buffer_rsrc_t rs_pp,
                          const __amdgpu_buffer_rsrc_t rs_part, unsigned off2_prev, unsigned off2_pp, int p_crem_prev)
                          __attribute__((always_inline)) {
        constexpr int U = decltype(u_c)::value, EP = decltype(ep_c)::value;
        constexpr int p = U & 3, itl = U >> 2, IT = 4 * EP + itl;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        [[maybe_unused]] u32x4 v = {0u, 0u, 0u, 0u};
        if constexpr (IT < 6) {
            g6_epi_exp<p, IT>();
        } else {
            constexpr int r0 = g6_acc_reg(2 * p, IT), r1 = g6_acc_reg(2 * p + 1, IT);
            const float e0 = __builtin_amdgcn_exp2f(g6_acc<r0 + 0>()), e1 = __builtin_amdgcn_exp2f(g6_acc<r0 + 1>());
            const float e2 = __builtin_amdgcn_exp2f(g6_acc<r0 + 2>()), e3 = __builtin_amdgcn_exp2f(g6_acc<r0 + 3>());
            const float e4 = __builtin_amdgcn_exp2f(g6_acc<r1 + 0>()), e5 = __builtin_amdgcn_exp2f(g6_acc<r1 + 1>());
            const float e6 = __builtin_amdgcn_exp2f(g6_acc<r1 + 2>()), e7 = __builtin_amdgcn_exp2f(g6_acc<r1 + 3>());
            v = u32x4{pack_bf16(e0, e1), pack_bf16(e2, e3), pack_bf16(e4, e5), pack_bf16(e6, e7)};
        }
        {   // (the masked form serves any tile)
            const int n = p_crem_prev - 8 * (int)efq - 32 * p;
            const unsigned m0 = n >= 2 ? 0xffffffffu : n == 1 ? 0xffffu : 0u, m1 = n >= 4 ? 0xffffffffu : n == 3 ? 0xffffu : 0u;
            const unsigned m2 = n >= 6 ? 0xffffffffu : n == 5 ? 0xffffu : 0u, m3 = n >= 8 ? 0xffffffffu : n == 7 ? 0xffffu : 0u;
            if constexpr (IT < 6) g6_epi_mask<p, IT>(m0, m1, m2, m3); else v &= u32x4{m0, m1, m2, m3};
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (U == 0) G7_STORE_SLICE(wq, rs_pp, off2_pp, 2, 3);
        else if constexpr (U <= 4) G7_STORE_SLICE(wq, rs_pp, off2_pp, 3, U - 1);
        else G7_STORE_SLICE(wq, rs_prev, off2_prev, ((U - 1) >> 2) - 1, (U - 1) & 3);
        if constexpr (U == 1 && !(ABLATE & 8)) {
            const float rsum = g6_acc<G6_RS0 + 4 * (EP ^ 1) + 2 * (EP ^ 1)>();
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rsum), rs_part, lane4, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (IT < 6) g6_epi_put<p, IT, (itl & 1) * 4096>(p == 0 ? wa0 : p == 1 ? wa1 : p == 2 ? wa2 : wa3);
        else G7_LDS_U32X4((p == 0 ? wa0 : p == 1 ? wa1 : p == 2 ? wa2 : wa3) + (itl & 1) * 4096) = v;
        __builtin_amdgcn_sched_barrier(0);
        wq = G7_READ_SLICE(itl == 0 ? 3 : itl - 1, p);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (IT < 6) g7_epi_sum<p, IT, EP, U == 0>(); else g7_rowsum<IT, EP>(v);
        __builtin_amdgcn_sched_barrier(0);
    };

    using g7_m0 = std::integral_constant<int, 0>;
    using g7_m1 = std::integral_constant<int, 1>;
#define G7_OFF2(d_) ((((int)rchunk * 8 + 8 <= (d_).c_room) ? lane_base2 : 0x80000000u))
#define G7_EDGE(d_) ((d_).p_crem < 128)
#define G7_RS_E(d_) __builtin_amdgcn_make_buffer_rsrc((void*)(d_).e_base, 0, (d_).e_room, 0x00020000)
#define G7_RS_P(d_) __builtin_amdgcn_make_buffer_rsrc((void*)(d_).p_base, 0, (d_).p_room, 0x00020000)
    // ---- one tile of parity T: four ring rounds with the previous tile's epilogue, then the plain rounds (K > 512)
    auto tile = [&](auto t_c) __attribute__((always_inline)) {
        constexpr int T = decltype(t_c)::value;
        using tt = std::integral_constant<int, T>;
        const __amdgpu_buffer_rsrc_t rs_prev = G7_RS_E(d_prev), rs_pp = G7_RS_E(d_pp), rs_part = G7_RS_P(d_pp);
        const unsigned off2_prev = G7_OFF2(d_prev), off2_pp = G7_OFF2(d_pp);
        const bool edge_prev = G7_EDGE(d_prev);
        const int p_crem_prev = d_prev.p_crem;
        const bool prev_e = tile_no > 0 && nt4 == 4;
        if constexpr ((ABLATE & 8) != 0) {
            if (blockIdx.x == 0 && lane == 0 && tile_no < 64) stamps[tile_no] = __builtin_amdgcn_s_memtime();
        }
        g6_for<4>([&](auto r_c) __attribute__((always_inline)) {
            constexpr int r = decltype(r_c)::value;
            if (r == nt4 - 1 && has_next) G7_SET_TILE(ntm, ntn);
            const int kb = (r == nt4 - 1) ? 0 : (r + 1) * 4096;
            g6_for<4>([&](auto q_c) __attribute__((always_inline)) {
                constexpr int U = 4 * r + decltype(q_c)::value;
                kstep(std::integral_constant<int, U>{}, tt{}, g7_m0{}, kb + (U & 3) * 1024, prev_e, false, rs_prev, rs_pp, rs_part,
                      off2_prev, off2_pp, edge_prev, p_crem_prev);
            });
        });
        for (int r = 4; r < nt4; ++r) {
            if (r == nt4 - 1 && has_next) G7_SET_TILE(ntm, ntn);
            const int kb = (r == nt4 - 1) ? 0 : (r + 1) * 4096;
            g6_for<4>([&](auto q_c) __attribute__((always_inline)) {
                constexpr int U = decltype(q_c)::value;
                kstep(std::integral_constant<int, U>{}, tt{}, g7_m1{}, kb + U * 1024, false, r == 4, rs_prev, rs_pp, rs_part, off2_prev,
                      off2_pp, edge_prev, p_crem_prev);
            });
        }
    };

    for (;;) {
        if (tile_no & 1) tile(std::integral_constant<int, 1>{}); else tile(std::integral_constant<int, 0>{});
        d_pp = d_prev;
        d_prev = make_desc(tm, tn);
        ++tile_no;
        if (!has_next) break;
        tm = ntm;
        tn = ntn;
        G7_WALK_NEXT();
    }
    // ---- behind the last tile: its epilogue on its own, then the last column's slices and the last two tiles' row sums
    if constexpr (!NOEPI) {
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");          // the last MFMAs' results
        {
            const __amdgpu_buffer_rsrc_t rs_prev = G7_RS_E(d_prev), rs_pp = G7_RS_E(d_pp), rs_part = G7_RS_P(d_pp);
            const unsigned off2_prev = G7_OFF2(d_prev), off2_pp = G7_OFF2(d_pp);
            const int p_crem_prev = d_prev.p_crem;
            if ((tile_no - 1) & 1) {
                g6_for<16>([&](auto u_c) __attribute__((always_inline)) {
                    drain_step(u_c, std::integral_constant<int, 1>{}, rs_prev, rs_pp, rs_part, off2_prev, off2_pp, p_crem_prev);
                });
            } else {
                g6_for<16>([&](auto u_c) __attribute__((always_inline)) {
                    drain_step(u_c, std::integral_constant<int, 0>{}, rs_prev, rs_pp, rs_part, off2_prev, off2_pp, p_crem_prev);
                });
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            G7_STORE_SLICE(wq, rs_prev, off2_prev, 2, 3);
            const u32x4 w0 = G7_READ_SLICE(3, 0), w1 = G7_READ_SLICE(3, 1), w2 = G7_READ_SLICE(3, 2), w3 = G7_READ_SLICE(3, 3);
            G7_STORE_SLICE(w0, rs_prev, off2_prev, 3, 0);
            G7_STORE_SLICE(w1, rs_prev, off2_prev, 3, 1);
            G7_STORE_SLICE(w2, rs_prev, off2_prev, 3, 2);
            G7_STORE_SLICE(w3, rs_prev, off2_prev, 3, 3);
            asm volatile("s_nop 7" ::: "memory");                    // the last row-sum MFMA is a handful of instructions old
            const __amdgpu_buffer_rsrc_t rs_last = G7_RS_P(d_prev);
            const float r_even = g6_acc<G6_RS0>(), r_odd = g6_acc<G6_RS0 + 4 + 2>();
            if constexpr (!(ABLATE & 8)) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(((tile_no - 1) & 1) ? r_odd : r_even), rs_last, lane4, 0, 0);
        }
    }
    // the refills past the last k-step are still in flight: they must land before this workgroup's LDS is handed to the next one
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef G7_RS_P
#undef G7_RS_E
#undef G7_EDGE
#undef G7_OFF2
#undef G7_STORE_SLICE
#undef G7_READ_SLICE
#undef G7_LDS_U32X4
#undef G7_WALK_NEXT
#undef G7_RDA
#undef G7_RDB
#undef G7_DMA
#undef G7_SET_TILE
#undef G7_BLK
}

#endif
