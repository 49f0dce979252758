// k_gexp_v6.inc -- K1s, round 5: included by k_gemm.hip inside its anonymous namespace, which provides the tile walk (TileWalkR),
// pack_bf16, the vector types and the fragment-major operand image (frag_major_off).
//   replaces  image_features @ text_features.T  (concept_vit/utils.py:594)  fused with  softmax(a * clip_feats, dim=1)'s
//   numerator (concept_vit/similarity.py:54), stress chain only (bf16, no parity claim).
//
// What v4 left on the table (profiles/r04_gexp_v4.txt (e), (f)): a tile costs 21 000 cycles of K loop + 7 600-8 400 cycles of
// epilogue with the matrix pipe idle, and of the epilogue's ~4 300 vector issue cycles 1 250 were v_accvgpr_read (a VALU
// instruction cannot read an AGPR) and 640 the row-sum adds.  v6 changes WHERE THINGS LIVE in the 512-entry register file:
//   * the MFMA's C / D may be arch VGPRs and its A / B may be AGPRs (gfx90a+), so 48 of the 64 accumulator blocks live in
//     v64..v255, where v_exp_f32 / v_cvt_pk_bf16_f32 work on them IN PLACE, and the fragments live in a64..a191, filled by
//     ds_read_b128 straight into AGPRs.  The compiler is held to v0..v59 (amdgpu_num_vgpr) and never sees any of this: every
//     MFMA, fragment read and epilogue group is an asm statement on registers addressed by name.  (16 blocks -- image blocks 6
//     and 7 -- stay in a0..a63 and still pay their v_accvgpr_read: 64 of v4's 256.)
//   * the row sums are MFMAs: the packed 16-byte piece of a lane (8 consecutive concepts of one image) IS a B fragment of
//     v_mfma_f32_16x16x32_bf16 (k = 8 fq + j <-> concept 32 p + 8 fq + j, column = image fr), so ones[16 x 32] x piece, accumulated
//     over the 4 pieces of an image block, leaves the sum over the wave's 128 concepts in every row of a 16 x 16 block: 32 MFMAs
//     (3 % of the tile's 1 024) replace 128 v_pk_add_f32 + 16 cross-lane shuffles, and the sum is the sum of the bf16 values that
//     are stored (S = E * rinv then sums to 1 over what K4s reads).
//   * the epilogue of tile i runs INSIDE the first two k-steps of tile i + 1.  A k-step's MFMAs
//     are dealt by image block (column-major): behind the epilogue of column nj come the 16 MFMAs of column nj -- k-steps 0 and
//     1, whose fragments are both register sets -- so the vector work of one column rides the matrix work of the previous one
//     (a v_mfma_f32_16x16x32_bf16 holds the vector issue for 8 of its 16 cycles: MI355X_MICROARCH.md, cycle constants).
//   * the DMA pieces of the K loop are asm statements, not the builtin: ONE M0 write per four pieces, one MFMA ahead of the first
//     (G6_DMA_ASM below) -- every instruction beside an MFMA is an issue slot of the one wave that feeds the matrix pipe AND the
//     DMA path, and the K loop of a 256 x 256 tile waits for that path (profiles/r05_gexp_v6.txt (k), (o)).
//
// (Rounds 4-5 carried this kernel's timing ablations, other placements and walks of a k-step, other cache policies of the E stores,
// the epilogue behind its own tile or inside ONE k-step, and a two-accumulator-set form, scripts/archive/k_gexp_v7.inc, as template parameters and a
// second kernel.  All measured, none faster: profiles/r05_gexp_v6.txt, r04_gexp_place.txt, r05_mfma_order.txt, r05_store_exp.txt.
// They were retired; scripts/README.md's archive row names the commit that builds them.)
//
// Registers (per lane):  v0..v59 compiler | v60..v63 constant block | v[64 + 4 (6 mi + nj)] block (mi, nj < 6) | a[4 (2 mi + nj - 6)] block (mi, nj >= 6)
//   a[64 + 64 s + 4 i] A fragment i of set s | a[96 + 64 s + 4 j] B fragment j of set s | a196..a199 constant block (C of a tile's first MFMAs on
//   the AGPR blocks) | a204..a207 the row-sum block | a[212 + 4 nj] selector fragment of image block nj.
#ifndef MCD_K_GEXP_V6_INC
#define MCD_K_GEXP_V6_INC

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef int i32x4v __attribute__((ext_vector_type(4)));

constexpr int G6_SLOT = 32768;       // one k-step of the ring: A pieces 0..15 | B pieces 0..15
constexpr int G6_RING = 4 * G6_SLOT;
constexpr int G6_LT = 8192;          // per-wave transposition buffers: 2 x (16 images x 256 B)
constexpr int G6_LDS = G6_RING + 4 * G6_LT;
constexpr int G6_IMM = 1;           // 1: a k-step's K-tile offset rides the DMA instruction's immediate field (0: in the scalar offset)

template <int I> using g6_ic = std::integral_constant<int, I>;
template <typename F, int... Is>
__device__ __forceinline__ void g6_for_impl(F&& f, std::integer_sequence<int, Is...>) { (f(g6_ic<Is>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void g6_for(F&& f) { g6_for_impl(f, std::make_integer_sequence<int, N>{}); }

template <int REG>
__device__ __forceinline__ float g6_acc() {
    float x;
    asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(x) : "i"(REG));
    return x;
}

// Where a k-step's 24 memory instructions sit in its stream of 64 MFMAs (k = 8 mi + nj, row-major over the wave tile's 8 x 8 block
// grid, block (mi, nj) = A fragment mi x B fragment nj): the code of the operation issued behind MFMA k -- 0 none, 1 + i DMA piece i,
// 9 + i A fragment i, 17 + i B fragment i of the next k-step.  The 16 fragment reads in rows 0-3 (behind MFMAs 1, 3, 5, 7), the 8
// pieces in rows 4-7 (behind MFMAs 1 and 5): the last read is 32 MFMAs old at the sync point's lgkmcnt(0) (profiles/r04_gexp_place.txt;
// the other placements and the other walks of the grid that were measured: profiles/r05_mfma_order.txt, r05_gexp_v6.txt (g)).
constexpr int g6_op_after(int k) {
    const int row = k >> 3, c = k & 7;
    if (row < 4) return c == 1 ? 9 + 2 * row : c == 3 ? 17 + 2 * row : c == 5 ? 10 + 2 * row : c == 7 ? 18 + 2 * row : 0;
    return c == 1 ? 1 + 2 * (row - 4) : c == 5 ? 2 + 2 * (row - 4) : 0;
}
constexpr int g6_acc_reg(int mi, int nj) { return nj < 6 ? 64 + 4 * (6 * mi + nj) : 4 * (2 * mi + nj - 6); }
constexpr int G6_FRAG0 = 64, G6_CB0 = 196, G6_RS0 = 204, G6_SEL0 = 212;
constexpr int G6_NVGPR = 60, G6_VCB0 = 60;     // the compiler's registers end at v59; v60..v63: the constant block of the VGPR-resident accumulators

// block (MI, NJ) += A fragment MI x B fragment NJ of set SET; FIRST: C = the constant block (-a log2(e)) instead of the block itself
template <int MI, int NJ, int SET, bool FIRST>
__device__ __forceinline__ void g6_mfma() {
    constexpr int d = g6_acc_reg(MI, NJ), fa = G6_FRAG0 + 64 * SET + 4 * MI, fb = G6_FRAG0 + 64 * SET + 32 + 4 * NJ;
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
// The constant blocks, written ONCE per launch: v60..v63 for the VGPR-resident blocks (C and D of an MFMA are both VGPRs or both
// AGPRs), a196..a199 for the blocks of image columns 6 and 7.  Every accumulator starts from -a log2(e) (the scale is folded into
// the concept operand, so an accumulator IS the exp2 argument); concepts past the last one are masked in the packed pieces
// (g6_epi_mask), on the tiles that have any.
__device__ __forceinline__ void g6_setc(float c) {
    asm volatile("v_accvgpr_write_b32 a%c1, %0\n\tv_accvgpr_write_b32 a%c2, %0\n\tv_accvgpr_write_b32 a%c3, %0\n\tv_accvgpr_write_b32 a%c4, %0\n\t"
                 "v_mov_b32 v%c5, %0\n\tv_mov_b32 v%c6, %0\n\tv_mov_b32 v%c7, %0\n\tv_mov_b32 v%c8, %0\n\ts_nop 3"
                 ::"v"(c), "i"(G6_CB0), "i"(G6_CB0 + 1), "i"(G6_CB0 + 2), "i"(G6_CB0 + 3), "i"(G6_VCB0), "i"(G6_VCB0 + 1), "i"(G6_VCB0 + 2), "i"(G6_VCB0 + 3));
}
// fragment I (A or B) of set SET <- LDS at addr + OFF (the compiler does not count this read: the k-step's sync point waits lgkmcnt(0))
template <int SET, bool ISB, int I, int OFF>
__device__ __forceinline__ void g6_read(unsigned addr) {
    constexpr int r = G6_FRAG0 + 64 * SET + (ISB ? 32 : 0) + 4 * I;
    asm volatile("ds_read_b128 a[%c1:%c2], %0 offset:%c3" ::"v"(addr), "i"(r), "i"(r + 3), "i"(OFF) : "memory");
}
// Epilogue group (P, NJ), NJ < 6, in three statements (the caller puts the previous slice's store between the first two, so that
// no wait for the LDS sits right behind an LDS instruction):
//   1. the 8 accumulators of blocks (2 P, NJ), (2 P + 1, NJ) -> exp2 -> 4 packed dwords IN the first block's registers (a
//      v_exp_f32 result is not read by the instruction behind it: gfx940 trans forwarding hazard, 1 state);
//   2. the 16-byte piece into the transposition buffer;
//   3. the row-sum MFMA on the piece (C = 0 for the column's first); at least two instructions lie between the piece's last
//      write and this read.
template <int P, int NJ>
__device__ __forceinline__ void g6_epi_exp() {
    constexpr int b0 = g6_acc_reg(2 * P, NJ), b1 = g6_acc_reg(2 * P + 1, NJ);
    asm volatile(
        "v_exp_f32 v%c0, v%c0\n\tv_exp_f32 v%c1, v%c1\n\tv_exp_f32 v%c2, v%c2\n\tv_exp_f32 v%c3, v%c3\n\t"
        "v_exp_f32 v%c4, v%c4\n\tv_exp_f32 v%c5, v%c5\n\tv_exp_f32 v%c6, v%c6\n\tv_exp_f32 v%c7, v%c7\n\t"
        "v_cvt_pk_bf16_f32 v%c0, v%c0, v%c1\n\tv_cvt_pk_bf16_f32 v%c1, v%c2, v%c3\n\t"
        "v_cvt_pk_bf16_f32 v%c2, v%c4, v%c5\n\tv_cvt_pk_bf16_f32 v%c3, v%c6, v%c7"
        ::"i"(b0), "i"(b0 + 1), "i"(b0 + 2), "i"(b0 + 3), "i"(b1), "i"(b1 + 1), "i"(b1 + 2), "i"(b1 + 3));
}
// the same with MFMAs of the NEXT tile's first two k-steps between the exponentials (the overlapped boundary phase): blocks
// (MI0, NJ0), (MI0 + 1, NJ0) of k-step 0 (register set 0, C = the constant block) and, when NJ1 >= 0, blocks (MI0, NJ1),
// (MI0 + 1, NJ1) of k-step 1 (set 1, C = the block) -- columns whose epilogue is done, NJ1 one behind NJ0.  All VGPR-resident.
template <int P, int NJ, int MI0, int NJ0, int NJ1>
__device__ __forceinline__ void g6_epi_exp_mm() {
    static_assert(NJ0 < 6 && NJ1 < 6, "VGPR-resident blocks only");
    constexpr int b0 = g6_acc_reg(2 * P, NJ), b1 = g6_acc_reg(2 * P + 1, NJ);
    constexpr int d0 = g6_acc_reg(MI0, NJ0), d1 = g6_acc_reg(MI0 + 1, NJ0), fa0 = G6_FRAG0 + 4 * MI0, fa1 = fa0 + 4, fb = G6_FRAG0 + 32 + 4 * NJ0;
    if constexpr (NJ1 < 0) {
        asm volatile(
            "v_exp_f32 v%c0, v%c0\n\tv_exp_f32 v%c1, v%c1\n\tv_exp_f32 v%c2, v%c2\n\tv_exp_f32 v%c3, v%c3\n\t"
            "v_mfma_f32_16x16x32_bf16 v[%c8:%c9], a[%c10:%c11], a[%c14:%c15], v[%c16:%c17]\n\t"
            "v_exp_f32 v%c4, v%c4\n\tv_exp_f32 v%c5, v%c5\n\tv_exp_f32 v%c6, v%c6\n\tv_exp_f32 v%c7, v%c7\n\t"
            "v_mfma_f32_16x16x32_bf16 v[%c18:%c19], a[%c12:%c13], a[%c14:%c15], v[%c16:%c17]\n\t"
            "v_cvt_pk_bf16_f32 v%c0, v%c0, v%c1\n\tv_cvt_pk_bf16_f32 v%c1, v%c2, v%c3\n\t"
            "v_cvt_pk_bf16_f32 v%c2, v%c4, v%c5\n\tv_cvt_pk_bf16_f32 v%c3, v%c6, v%c7"
            ::"i"(b0), "i"(b0 + 1), "i"(b0 + 2), "i"(b0 + 3), "i"(b1), "i"(b1 + 1), "i"(b1 + 2), "i"(b1 + 3),
            "i"(d0), "i"(d0 + 3), "i"(fa0), "i"(fa0 + 3), "i"(fa1), "i"(fa1 + 3), "i"(fb), "i"(fb + 3), "i"(G6_VCB0), "i"(G6_VCB0 + 3),
            "i"(d1), "i"(d1 + 3));
    } else {
        constexpr int NJ1c = NJ1 < 0 ? 0 : NJ1;
        constexpr int e0 = g6_acc_reg(MI0, NJ1c), e1 = g6_acc_reg(MI0 + 1, NJ1c), ga0 = fa0 + 64, ga1 = ga0 + 4, gb = G6_FRAG0 + 64 + 32 + 4 * NJ1c;
        asm volatile(
            "v_exp_f32 v%c0, v%c0\n\tv_exp_f32 v%c1, v%c1\n\t"
            "v_mfma_f32_16x16x32_bf16 v[%c8:%c9], a[%c10:%c11], a[%c14:%c15], v[%c16:%c17]\n\t"
            "v_exp_f32 v%c2, v%c2\n\tv_exp_f32 v%c3, v%c3\n\t"
            "v_mfma_f32_16x16x32_bf16 v[%c18:%c19], a[%c12:%c13], a[%c14:%c15], v[%c16:%c17]\n\t"
            "v_exp_f32 v%c4, v%c4\n\tv_exp_f32 v%c5, v%c5\n\t"
            "v_mfma_f32_16x16x32_bf16 v[%c20:%c21], a[%c24:%c25], a[%c28:%c29], v[%c20:%c21]\n\t"
            "v_exp_f32 v%c6, v%c6\n\tv_exp_f32 v%c7, v%c7\n\t"
            "v_mfma_f32_16x16x32_bf16 v[%c22:%c23], a[%c26:%c27], a[%c28:%c29], v[%c22:%c23]\n\t"
            "v_cvt_pk_bf16_f32 v%c0, v%c0, v%c1\n\tv_cvt_pk_bf16_f32 v%c1, v%c2, v%c3\n\t"
            "v_cvt_pk_bf16_f32 v%c2, v%c4, v%c5\n\tv_cvt_pk_bf16_f32 v%c3, v%c6, v%c7"
            ::"i"(b0), "i"(b0 + 1), "i"(b0 + 2), "i"(b0 + 3), "i"(b1), "i"(b1 + 1), "i"(b1 + 2), "i"(b1 + 3),
            "i"(d0), "i"(d0 + 3), "i"(fa0), "i"(fa0 + 3), "i"(fa1), "i"(fa1 + 3), "i"(fb), "i"(fb + 3), "i"(G6_VCB0), "i"(G6_VCB0 + 3),
            "i"(d1), "i"(d1 + 3), "i"(e0), "i"(e0 + 3), "i"(e1), "i"(e1 + 3), "i"(ga0), "i"(ga0 + 3), "i"(ga1), "i"(ga1 + 3), "i"(gb), "i"(gb + 3));
    }
}
// one MFMA of the next tile's first k-step on its own (beside the compiler-made groups of image columns 6, 7 and in the tail)
template <int MI0, int NJ0>
__device__ __forceinline__ void g6_mfma_k0() { g6_mfma<MI0, NJ0, 0, true>(); }
template <int MI0, int NJ0>
__device__ __forceinline__ void g6_mfma_k1() { g6_mfma<MI0, NJ0, 1, false>(); }
// concepts past the last one: dword j of the piece keeps 2, 1 or 0 of its bf16 values (m0..m3 from the lane's count of real
// concepts in this piece)
template <int P, int NJ>
__device__ __forceinline__ void g6_epi_mask(unsigned m0, unsigned m1, unsigned m2, unsigned m3) {
    constexpr int b0 = g6_acc_reg(2 * P, NJ);
    asm volatile("v_and_b32 v%c4, v%c4, %0\n\tv_and_b32 v%c5, v%c5, %1\n\tv_and_b32 v%c6, v%c6, %2\n\tv_and_b32 v%c7, v%c7, %3"
                 ::"v"(m0), "v"(m1), "v"(m2), "v"(m3), "i"(b0), "i"(b0 + 1), "i"(b0 + 2), "i"(b0 + 3));
}
template <int P, int NJ, int OFF>
__device__ __forceinline__ void g6_epi_put(unsigned lds_addr) {
    constexpr int b0 = g6_acc_reg(2 * P, NJ);
    asm volatile("ds_write_b128 %0, v[%c1:%c2] offset:%c3" ::"v"(lds_addr), "i"(b0), "i"(b0 + 3), "i"(OFF) : "memory");
}
// Row sums as MFMAs: D[i][image] += SEL_nj[i][k] x piece[k][image], SEL_nj = 1 on the rows {4 (nj % 4) + 2 (nj / 4), + 1}, 0 elsewhere.
// After the tile's 32 of them ONE 16 x 16 block holds every image block's sums: lane (fq, fr), register 0 (= 1): the sum of image
// 16 fq + fr, register 2 (= 3): of image 16 (fq + 4) + fr -- over this wave's 128 concepts (of the bf16 values that are stored).
template <int P, int NJ>
__device__ __forceinline__ void g6_epi_sum() {
    constexpr int b0 = g6_acc_reg(2 * P, NJ), sel = G6_SEL0 + 4 * NJ;
    if constexpr (P == 0 && NJ == 0)
        asm volatile("v_mfma_f32_16x16x32_bf16 a[%c0:%c1], a[%c2:%c3], v[%c4:%c5], 0" ::"i"(G6_RS0), "i"(G6_RS0 + 3), "i"(sel), "i"(sel + 3), "i"(b0), "i"(b0 + 3));
    else
        asm volatile("v_mfma_f32_16x16x32_bf16 a[%c0:%c1], a[%c2:%c3], v[%c4:%c5], a[%c0:%c1]" ::"i"(G6_RS0), "i"(G6_RS0 + 3), "i"(sel), "i"(sel + 3), "i"(b0), "i"(b0 + 3));
}
// the same for a packed piece in compiler registers (the groups of image columns 6 and 7: read from the accumulator file)
template <int NJ>
__device__ __forceinline__ void g6_rowsum(const u32x4& v) {
    constexpr int sel = G6_SEL0 + 4 * NJ;
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 a[%c1:%c2], a[%c3:%c4], %0, a[%c1:%c2]" ::"v"(v), "i"(G6_RS0), "i"(G6_RS0 + 3), "i"(sel), "i"(sel + 3));
}
// selector fragment of image block NJ: lane l holds row l & 15 (all k alike): bf16 1.0 pairs or zeros
template <int NJ>
__device__ __forceinline__ void g6_set_sel(unsigned lane) {
    constexpr int sel = G6_SEL0 + 4 * NJ, r0 = 4 * (NJ % 4) + 2 * (NJ / 4);
    const unsigned row = lane & 15u;
    const unsigned x = (row == (unsigned)r0 || row == (unsigned)(r0 + 1)) ? 0x3f803f80u : 0u;
    asm volatile("v_accvgpr_write_b32 a%c1, %0\n\tv_accvgpr_write_b32 a%c2, %0\n\tv_accvgpr_write_b32 a%c3, %0\n\tv_accvgpr_write_b32 a%c4, %0"
                 ::"v"(x), "i"(sel), "i"(sel + 1), "i"(sel + 2), "i"(sel + 3));
}

// v60 .. v255 and a0 .. a255 belong to the asm statements of the K1s kernels (this also makes the kernel descriptor allocate them)
__device__ __forceinline__ void g6_claim_registers() {
    asm volatile("" ::: "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255");
    asm volatile("" ::: "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255");
}

__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_num_vgpr(G6_NVGPR))) void gemm_nt_bf16_exp_v6_kernel(
    const unsigned short* __restrict__ A /* concepts, fragment-major, paired, pre-scaled by a log2(e) */,
    const unsigned short* __restrict__ B /* images, fragment-major */, int64_t Kp, int64_t Mc, int64_t Ni,
    unsigned short* __restrict__ E, int64_t ldE, float* __restrict__ part, int64_t ldpart, float s1 /* a * log2(e) */,
    int tiles_m, int tiles_n, int stagger /* cycles of one tile period, 0 = off */) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    g6_claim_registers();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileWalkR W(tiles_m, tiles_n);
    const int nt = (int)(Kp >> 5), nt4 = nt >> 2;          // host: nt % 4 == 0
    if (W.count() == 0) return;
    // late start of the workgroups with the shorter tile walk (as v4: spreads the store bursts)
    if (stagger > 0) {
        const int cmax = (W.n_seq + W.nslot - 1) / W.nslot;
        const int nlong = W.n_seq - (cmax - 1) * W.nslot;
        if (W.count() < cmax && W.nslot > nlong) {
            const int wait = (int)((int64_t)stagger * (W.slot - nlong + 1) / (W.nslot - nlong + 1));
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
            while ((long long)(__builtin_amdgcn_s_memtime() - t0) < wait) __builtin_amdgcn_s_sleep(8);
        }
    }
    const int wr = wave >> 1, wc = wave & 1;
    // the selector fragments of the row-sum MFMAs and the accumulators' starting value
    g6_for<8>([&](auto n_c) __attribute__((always_inline)) { g6_set_sel<decltype(n_c)::value>((unsigned)lane); });
    g6_setc(-s1);

    // ---- DMA side: this wave's pieces of a k-step are A pieces 4 wave + i and B pieces 4 wave + i, i = 0..3
    const int nrbA = (int)(((Mc + 31) >> 5) << 1), nrbB = (int)((Ni + 15) >> 4);
    __amdgpu_buffer_rsrc_t ra_ = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, (int)((int64_t)nrbA * 16 * Kp * 2), 0x00020000);
    __amdgpu_buffer_rsrc_t rb_ = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, (int)((int64_t)nrbB * 16 * Kp * 2), 0x00020000);
    const unsigned vlane = (unsigned)(lane * 16);
    const int wave4096 = wave * 4096;             // this wave's four pieces of an operand's 16 are neighbours in the slot (4 KB)
    int oa0, oa1, oa2, oa3, ob0, ob1, ob2, ob3;            // byte offsets of the DMA tile's row blocks (K-tile 0)
    // the same two descriptors as scalar quads, for the DMA instructions written as asm statements (G6_DMA_ASM below)
    // (based 3 KB in front of the operand: a piece's scalar offset carries + 3 072 - 1 024 x (its place among the wave's four), which
    // the instruction's offset field adds back -- that field moves the LDS address too, and so one M0 write serves four pieces)
    const uintptr_t A3 = (uintptr_t)A - 3072, B3 = (uintptr_t)B - 3072;
    const i32x4v ra4 = {(int)A3, (int)((A3 >> 32) & 0xffffu), (int)((int64_t)nrbA * 16 * Kp * 2 + 3072), 0x00020000};
    const i32x4v rb4 = {(int)B3, (int)((B3 >> 32) & 0xffffu), (int)((int64_t)nrbB * 16 * Kp * 2 + 3072), 0x00020000};
    unsigned vlane1 = vlane + 1024u, vlane2 = vlane + 2048u, vlane3 = vlane + 3072u;     // + the k-step's K-tile within its ring round
    asm volatile("" : "+v"(vlane1), "+v"(vlane2), "+v"(vlane3));
#define G6_BLK(nrb_, b_) ((((b_) < (nrb_)) ? (b_) : (nrb_) - 1) * nt * 1024)
#define G6_SET_TILE(tm_, tn_)                                                        \
    do {                                                                             \
        const int ba_ = (tm_) * 16 + 4 * wave, bb_ = (tn_) * 16 + 4 * wave;         \
        oa0 = G6_BLK(nrbA, ba_); oa1 = G6_BLK(nrbA, ba_ + 1); oa2 = G6_BLK(nrbA, ba_ + 2); oa3 = G6_BLK(nrbA, ba_ + 3); \
        ob0 = G6_BLK(nrbB, bb_); ob1 = G6_BLK(nrbB, bb_ + 1); ob2 = G6_BLK(nrbB, bb_ + 2); ob3 = G6_BLK(nrbB, bb_ + 3); \
    } while (0)
// (kt1024_ = the ring round's first K-tile + U_ K-tiles, in bytes: the U_ * 1 024 go into the instruction's 12-bit offset field --
// which the hardware adds to the LDS address as well, hence the same amount off the LDS pointer -- so that the scalar offset is
// the same for the four k-steps of a round: one s_add per piece and ROUND instead of one per piece and k-step in the MFMA stream)
#define G6_DMA(U_, i_, kt1024_)                                                                                              \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                                                \
        (i_) < 4 ? ra_ : rb_,                                                                                                \
        (__attribute__((address_space(3))) void*)(smem + (U_) * G6_SLOT + ((i_) < 4 ? 0 : 16384) + 1024 * ((i_) & 3) + wb_ - G6_IMM * (U_) * 1024), \
        16, vlane,                                                                                                           \
        ((i_) == 0 ? oa0 : (i_) == 1 ? oa1 : (i_) == 2 ? oa2 : (i_) == 3 ? oa3 : (i_) == 4 ? ob0 : (i_) == 5 ? ob1 : (i_) == 6 ? ob2 : ob3) + ((kt1024_) - G6_IMM * (U_) * 1024), \
        G6_IMM * (U_) * 1024, 0)

    // The plain k-steps issue their pieces as asm statements: ONE M0 write (LDS destination of the wave's four neighbouring pieces
    // of an operand) one MFMA ahead of the first of the four loads; a load's place among the four is its instruction offset (added
    // to the global AND the LDS address), the k-step's K-tile is in the lane offset.  Through the builtin every piece had its own M0
    // write right in front of it, a wait state behind that (an s_nop, or the s_add of its scalar offset): 16 scalar issue slots
    // per k-step in the MFMA stream, now 2.
#define G6_DMA_M0(U_, g_) asm volatile("s_add_i32 m0, %0, %1" ::"s"(wbl_), "i"((U_) * G6_SLOT + (g_) * 16384) : "memory")
#define G6_DMA_ASM(U_, i_, kt1024_)                                                                                          \
    do {                                                                                                                     \
        const int so_ = ((i_) == 0 ? oa0 : (i_) == 1 ? oa1 : (i_) == 2 ? oa2 : (i_) == 3 ? oa3 : (i_) == 4 ? ob0 : (i_) == 5 ? ob1 : (i_) == 6 ? ob2 : ob3) + ((kt1024_) - (U_) * 1024) + (3072 - ((i_) & 3) * 1024); \
        const unsigned vo_ = (U_) == 0 ? vlane : (U_) == 1 ? vlane1 : (U_) == 2 ? vlane2 : vlane3;                           \
        if constexpr ((i_) < 4) asm volatile("buffer_load_dwordx4 %0, %1, %2 offen offset:%c3 lds" ::"v"(vo_), "s"(ra4), "s"(so_), "i"(((i_) & 3) * 1024) : "memory"); \
        else asm volatile("buffer_load_dwordx4 %0, %1, %2 offen offset:%c3 lds" ::"v"(vo_), "s"(rb4), "s"(so_), "i"(((i_) & 3) * 1024) : "memory"); \
    } while (0)
    // ---- compute side: fragment i of this wave's A / B half of the k-step in slot U: piece (wr | wc) * 8 + i at
    // (slot base) + (A: 0 | B: 16 384) + (wr | wc) * 8 192 + i * 1 024 + 16 * lane; the 16-bit offset field holds slot parity + i
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned a_lo = lds0 + (unsigned)(lane * 16 + wr * 8192), b_lo = lds0 + (unsigned)(lane * 16 + 16384 + wc * 8192);
    unsigned a_hi = a_lo + 2u * G6_SLOT, b_hi = b_lo + 2u * G6_SLOT;
    asm volatile("" : "+v"(a_hi), "+v"(b_hi));
#define G6_RDA(SET_, U_, i_) g6_read<SET_, false, i_, ((U_) & 1) * G6_SLOT + (i_) * 1024>((U_) < 2 ? a_lo : a_hi)
#define G6_RDB(SET_, U_, i_) g6_read<SET_, true, i_, ((U_) & 1) * G6_SLOT + (i_) * 1024>((U_) < 2 ? b_lo : b_hi)

    int ci = -1, tm, tn;
    W.next(ci, tm, tn);
    G6_SET_TILE(tm, tn);
#define G6_STAGE_ALL(U_, kt1024_)                                                                            \
    do {                                                                                                     \
        G6_DMA(U_, 0, kt1024_); G6_DMA(U_, 1, kt1024_); G6_DMA(U_, 2, kt1024_); G6_DMA(U_, 3, kt1024_);     \
        G6_DMA(U_, 4, kt1024_); G6_DMA(U_, 5, kt1024_); G6_DMA(U_, 6, kt1024_); G6_DMA(U_, 7, kt1024_);     \
    } while (0)
    {
        const int wb_ = wave4096;
        G6_STAGE_ALL(0, 0);
        G6_STAGE_ALL(1, 1024);
        G6_STAGE_ALL(2, 2048);
        G6_STAGE_ALL(3, 3072);
    }
    asm volatile("s_waitcnt vmcnt(24) lgkmcnt(0)" ::: "memory");   // k-step 0 landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    g6_for<8>([&](auto i_c) __attribute__((always_inline)) {
        constexpr int i = decltype(i_c)::value;
        G6_RDA(0, 0, i);
        G6_RDB(0, 0, i);
    });
    // the walk after the first tile, WITHOUT a division per tile (TileWalkR::next divides by the XCD's row count: ~40 scalar
    // instructions between two tiles, with the matrix pipe idle): seq advances by nslot = q nrow_x + d, so the row index within the
    // XCD's rows advances by d (mod nrow_x) and the image tile by q (+ 1 on a wrap)
    const int wq_ = W.nslot / W.nrow_x, wd_ = W.nslot - wq_ * W.nrow_x;
    int seq_ = W.slot, wr_idx = (tm - W.xcd) >> 3;         // this tile's sequence number and its row index within the XCD's rows
    int ntm = tm, ntn = tn;
    bool has_next;
#define G6_WALK_NEXT()                                                                  \
    do {                                                                                \
        seq_ += W.nslot;                                                                \
        has_next = seq_ < W.n_seq;                                                      \
        int r_ = wr_idx + wd_, c_ = ntn + wq_;                                          \
        if (r_ >= W.nrow_x) { r_ -= W.nrow_x; ++c_; }                                   \
        wr_idx = r_;                                                                    \
        ntn = c_;                                                                       \
        ntm = W.xcd + 8 * r_;                                                           \
    } while (0)
    G6_WALK_NEXT();

    constexpr int G6_NST = 32;                         // E stores a wave issues per epilogue
    bool pending = false;                              // the previous tile's sums wait in the accumulators: its epilogue, stores included, rides this tile's first k-steps

    // ---- the sync point in front of the k-step in slot U: own pieces of k-step g+1 landed (the 16 pieces of g+2 and g+3 stay in
    // flight -- and, in a tile's first three k-steps, the 32 stores of the previous tile's epilogue, which are YOUNGER than
    // those pieces: vmcnt is in order.  The stores ride k-steps 0 and 1: nothing extra in front of
    // k-step 0, the same 32 in front of k-steps 1 and 2, and 29 in front of k-step 3, which waits for k-step 4's pieces: they
    // are issued one per step in steps 0-7 of the phase, the last one behind the stores of steps 5, 6 and 7)
#define G6_SYNC(U_, R0_)                                                                                                    \
    do {                                                                                                                     \
        if ((R0_) && (U_) >= 1 && pending)                                                                                   \
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(16 + ((U_) == 3 ? G6_NST - 3 : G6_NST)) : "memory");                    \
        else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");                                                               \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  /* own reads of k-step g done: slot U can be refilled */         \
        __builtin_amdgcn_sched_barrier(0);                                                                                   \
        __builtin_amdgcn_s_barrier();                                                                                        \
        asm volatile("" ::: "memory");                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                                   \
    } while (0)
    // the memory operation behind MFMA position k of the k-step in slot U (g6_op_after: 1 + i DMA piece i of k-step g + 4 into
    // slot U, 9 + i / 17 + i fragment A i / B i of k-step g + 1 into the other register set)
#define G6_OP(U_, op_, kt1024_)                                                                                              \
    do {                                                                                                                     \
        constexpr int nxt_ = ((U_) & 1) ^ 1, SN_ = ((U_) + 1) & 3;                                                           \
        if constexpr ((op_) != 0) {                                                                                          \
            __builtin_amdgcn_sched_barrier(0);                                                                               \
            if constexpr ((op_) <= 8) G6_DMA_ASM(U_, (op_) - 1, kt1024_);                                                    \
            else if constexpr ((op_) <= 16) G6_RDA(nxt_, SN_, (op_) - 9);                                                    \
            else G6_RDB(nxt_, SN_, (op_) - 17);                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                                               \
        }                                                                                                                    \
    } while (0)
    // ---- one k-step: 64 MFMAs row-major, the 24 memory operations where g6_op_after puts them
#define G6_KSTEP(U_, FIRST_, R0_, kt1024_)                                                                                   \
    do {                                                                                                                     \
        int wb_ = wave4096;                                                                                                  \
        asm volatile("" : "+s"(wb_));                                                                                        \
        const int wbl_ = (int)lds0 + wb_;                                                                                    \
        G6_SYNC(U_, R0_);                                                                                                    \
        g6_for<64>([&](auto k_c) __attribute__((always_inline)) {                                                            \
            constexpr int k_ = decltype(k_c)::value, op_ = g6_op_after(k_), opn_ = k_ < 63 ? g6_op_after(k_ + 1) : 0;        \
            g6_mfma<(k_ >> 3), (k_ & 7), (U_) & 1, (FIRST_)>();                                                              \
            if constexpr (opn_ == 1 || opn_ == 5) {                                                                          \
                static_assert(op_ == 0, "the gap in front of a group's first piece is empty");                               \
                __builtin_amdgcn_sched_barrier(0);                                                                           \
                G6_DMA_M0(U_, (opn_ - 1) >> 2);                                                                              \
                __builtin_amdgcn_sched_barrier(0);                                                                           \
            }                                                                                                                \
            G6_OP(U_, op_, kt1024_);                                                                                         \
        });                                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                                   \
    } while (0)
    // the tile whose sums are in the accumulators (its epilogue runs at the top of the NEXT tile's K loop)
    int ptm = 0, ptn = 0;
    // ---- the epilogue of tile (ptm, ptn).
    // Block (2p + h, nj), register r: concept = row0 + wr*128 + 32 p + 8 fq + 4 h + r, image = col0 + wc*128 + 16 nj + fr.
    // Step s = 4 it + p (it = image block = column of the 8 x 8 block grid, p = pair of concept blocks), s = 0..31:
    //   A  vector work of group (p, it): exp2 + pack (+ mask)          B  store of the 4-row slice read in step s - 1
    //   C  the group's 16-byte piece into transposition buffer it & 1  D  read slice p of column it - 1 from the other buffer
    //   E  row-sum MFMA of the piece
    // Every wait for the LDS (B's, for the slice) sits a whole group behind the LDS instructions it waits for (C, D of the
    // previous step): with store and read right behind the piece's write, as in v4, each group exposed an LDS round trip.
    // RIDE (the overlapped boundary phase; false behind the walk's last tile): this IS the next tile's k-steps in slots 0 and 1.  Behind its sync point come the k-step's 8
    // DMA pieces (k-step 4 into slot 0; in front of every store: the vmcnt counts of the next sync points rely on it), the 16
    // fragment reads of k-step 1 (two per step, steps 0-7) and, in the steps of column it + 1, the 8 MFMAs of column it, which
    // overwrite blocks whose pieces have left.
    // EDGE: the tile has concepts past the last one (or past the row pitch): their bf16 values are cleared in the piece.
#define G6_STORE_SLICE(w_, col_, p_) /* nontemporal (aux 2): profiles/r05_gexp_v6.txt, r05_store_exp.txt */ \
    __builtin_amdgcn_raw_buffer_store_b128(w_, rs_e, lane_off2 + (unsigned)((((col_) * 16 + 4 * (p_)) * (int)ldE) * 2), 0, 2)
#define G6_LDS_U32X4(a_) (*(__attribute__((address_space(3))) u32x4*)(uintptr_t)(a_))
#define G6_READ_SLICE(col_, p_) G6_LDS_U32X4(((p_) == 0 ? ra0 : (p_) == 1 ? ra1 : (p_) == 2 ? ra2 : ra3) + ((col_) & 1) * 4096)
    // lane-dependent constants of the epilogue, computed once per launch (round 5, late: they are live across the K loop, which
    // itself needs few vector registers; recomputed per tile they were ~35 vector instructions in front of every boundary phase)
    const unsigned rrow = (unsigned)lane >> 4, rchunk = (unsigned)lane & 15u, efr = rchunk, efq = rrow;
    unsigned lane_base2 = (rrow * (unsigned)(int)ldE + rchunk * 8u) * 2u;      // this lane's 16 bytes within a 4-row slice
    // transposition buffer: the 16-byte piece (image fr, chunk 4 p + fq) at fr * 256 + ((chunk ^ fr) << 4); one address per p
    const unsigned tb0 = lds0 + (unsigned)(G6_RING + wave * G6_LT) + efr * 256;
    unsigned wa0 = tb0 + ((efq ^ efr) << 4), wa1 = tb0 + (((4u + efq) ^ efr) << 4), wa2 = tb0 + (((8u + efq) ^ efr) << 4),
             wa3 = tb0 + (((12u + efq) ^ efr) << 4);
    // the read-back side: slice p = image rows 4 p + rrow of the block, 16-byte chunk rchunk of each (one address per p)
    const unsigned tbr = lds0 + (unsigned)(G6_RING + wave * G6_LT);
    unsigned ra0 = tbr + rrow * 256 + ((rchunk ^ rrow) << 4), ra1 = tbr + (4u + rrow) * 256 + ((rchunk ^ (4u + rrow)) << 4),
             ra2 = tbr + (8u + rrow) * 256 + ((rchunk ^ (8u + rrow)) << 4), ra3 = tbr + (12u + rrow) * 256 + ((rchunk ^ (12u + rrow)) << 4);
    asm volatile("" : "+v"(wa0), "+v"(wa1), "+v"(wa2), "+v"(wa3), "+v"(ra0), "+v"(ra1), "+v"(ra2), "+v"(ra3), "+v"(lane_base2));
    const unsigned lane4 = (unsigned)lane * 4u;
    auto epilogue = [&](auto ride_c, auto edge_c, [[maybe_unused]] int kt1024) __attribute__((always_inline)) {
        constexpr bool RIDE = decltype(ride_c)::value;      // the next tile's first two k-steps ride this epilogue
        constexpr bool EDGE = decltype(edge_c)::value;
        [[maybe_unused]] int wb_ = wave4096;
        asm volatile("" : "+s"(wb_));
        [[maybe_unused]] const int wbl_ = (int)lds0 + wb_;
        // 32-bit arithmetic wherever the host's limits allow it (N, C, ldE < 2^31, ldE * 257 < 2^31): 64-bit compares are vector
        // instructions, and this setup runs with the matrix pipe idle.  (Hoisted under the MFMAs of the tile's k-step 3 -- pinned
        // there by an asm statement, or the compiler sinks it to the loop latch -- its ~50 scalar instructions, issued in one
        // piece, stalled the MFMA stream for as long as they had cost here: profiles/r05_gexp_v6.txt (i).)
        const int c0_ = ptm * 256 + wr * 128, i0_ = ptn * 256 + wc * 128;      // first concept / image of this wave's 128 x 128
        const int rows_ = (int)Ni - i0_ < 128 ? ((int)Ni - i0_ > 0 ? (int)Ni - i0_ : 0) : 128;   // image rows left from there
        const int64_t e_first = (int64_t)((uint64_t)(uint32_t)i0_ * (uint32_t)(int)ldE) + c0_;
        // E stores go through a buffer descriptor based at this wave's first element of the tile and ending with the last real image's
        // row -- offsets r * ldE * 2 + c * 2, r < rows_, c < ldE - c0_ (the hardware drops what lies past it); a lane whose 8 concepts
        // lie outside the row pitch gets an offset past any range
        // (readfirstlane on the window's size: where the compiler takes the clamps as vector selects the descriptor would not be
        // provably uniform, and every store would be wrapped in a waterfall loop -- cdna_hip_programming.md T20)
        const int e_room_ = rows_ * (int)ldE * 2 - c0_ * 2;                     // (rows_ = 0: negative)
        const int e_room = __builtin_amdgcn_readfirstlane(e_room_ > 0 ? e_room_ : 0);
        const __amdgpu_buffer_rsrc_t rs_e = __builtin_amdgcn_make_buffer_rsrc((void*)(E + e_first), 0, e_room, 0x00020000);
        const int croom_ = (int)ldE - c0_, crem_ = (int)Mc - c0_;              // concepts of this wave inside the pitch / real
        const int c_room = croom_ < 4096 ? (croom_ > -4096 ? croom_ : -4096) : 4096;
        [[maybe_unused]] const int p_crem = crem_ < 4096 ? (crem_ > -4096 ? crem_ : -4096) : 4096;
        const unsigned lane_off2 = ((int)rchunk * 8 + 8 <= c_room) ? lane_base2 : 0x80000000u;
        // real concepts of this lane's piece p: eclim - 32 p (this lane's first concept of the piece is wave-relative 32 p + 8 fq)
        [[maybe_unused]] int eclim = 0;
        if constexpr (EDGE) eclim = p_crem - 8 * (int)efq;
        if constexpr (RIDE) {
            G6_SYNC(0, true);
        } else {
            asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs' results
        }
        u32x4 wq = {0u, 0u, 0u, 0u};                  // the slice read in the previous step, not yet stored
        g6_for<32>([&](auto s_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value, IT = S >> 2, p = S & 3;
            [[maybe_unused]] u32x4 v;
            [[maybe_unused]] unsigned m0 = 0, m1 = 0, m2 = 0, m3 = 0;
            // (k-step 1's fragments, read in steps 0-7 by statements the compiler does not count, are used from here on)
            if constexpr (RIDE && S == 8) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // k-step 1's sync point, inside the phase: every wave has its fragments of k-step 1 (slot 1 may be refilled) and its
            // pieces of k-step 2 have landed -- in flight behind them: k-step 3's 8 pieces, k-step 4's 8 (steps 0-7), 7 stores (steps 5-11)
            if constexpr (RIDE && S == 12) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(16 + 7) : "memory");
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (EDGE) {
                const int n = eclim - 32 * p;
                m0 = n >= 2 ? 0xffffffffu : n == 1 ? 0xffffu : 0u;
                m1 = n >= 4 ? 0xffffffffu : n == 3 ? 0xffffu : 0u;
                m2 = n >= 6 ? 0xffffffffu : n == 5 ? 0xffffu : 0u;
                m3 = n >= 8 ? 0xffffffffu : n == 7 ? 0xffffu : 0u;
            }
            if constexpr (IT < 6) {
                if constexpr (RIDE && IT >= 1) g6_epi_exp_mm<p, IT, 2 * p, IT - 1, IT >= 2 ? IT - 2 : -1>(); else g6_epi_exp<p, IT>();
                if constexpr (EDGE) g6_epi_mask<p, IT>(m0, m1, m2, m3);
            } else {
                constexpr int r0 = g6_acc_reg(2 * p, IT), r1 = g6_acc_reg(2 * p + 1, IT);
                const float e0 = __builtin_amdgcn_exp2f(g6_acc<r0 + 0>()), e1 = __builtin_amdgcn_exp2f(g6_acc<r0 + 1>());
                const float e2 = __builtin_amdgcn_exp2f(g6_acc<r0 + 2>()), e3 = __builtin_amdgcn_exp2f(g6_acc<r0 + 3>());
                if constexpr (RIDE) { __builtin_amdgcn_sched_barrier(0); g6_mfma_k0<2 * p, IT - 1>(); g6_mfma_k1<2 * p, IT - 2>(); __builtin_amdgcn_sched_barrier(0); }
                const float e4 = __builtin_amdgcn_exp2f(g6_acc<r1 + 0>()), e5 = __builtin_amdgcn_exp2f(g6_acc<r1 + 1>());
                const float e6 = __builtin_amdgcn_exp2f(g6_acc<r1 + 2>()), e7 = __builtin_amdgcn_exp2f(g6_acc<r1 + 3>());
                if constexpr (RIDE) { __builtin_amdgcn_sched_barrier(0); g6_mfma_k0<2 * p + 1, IT - 1>(); g6_mfma_k1<2 * p + 1, IT - 2>(); __builtin_amdgcn_sched_barrier(0); }
                v = u32x4{pack_bf16(e0, e1), pack_bf16(e2, e3), pack_bf16(e4, e5), pack_bf16(e6, e7)};
                if constexpr (EDGE) v &= u32x4{m0, m1, m2, m3};
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (S >= 5) G6_STORE_SLICE(wq, ((S - 1) >> 2) - 1, (S - 1) & 3);
            __builtin_amdgcn_sched_barrier(0);
            // the LDS destination (M0) of the four DMA pieces whose first goes out further down in this step
            if constexpr (RIDE && (S == 0 || S == 4)) G6_DMA_M0(0, S >> 2);
            if constexpr (RIDE && (S == 12 || S == 20)) G6_DMA_M0(1, (S - 12) >> 3);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (IT < 6) {
                g6_epi_put<p, IT, (IT & 1) * 4096>(p == 0 ? wa0 : p == 1 ? wa1 : p == 2 ? wa2 : wa3);
            } else {
                G6_LDS_U32X4((p == 0 ? wa0 : p == 1 ? wa1 : p == 2 ? wa2 : wa3) + (IT & 1) * 4096) = v;
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (IT >= 1) wq = G6_READ_SLICE(IT - 1, p);
            if constexpr (RIDE && S < 8) {              // fragments of k-step 1 (slot 1) into register set 1; piece S of k-step 4 -> slot 0
                __builtin_amdgcn_sched_barrier(0);
                G6_RDA(1, 1, S);
                G6_RDB(1, 1, S);
                G6_DMA_ASM(0, S, kt1024);
            }
            if constexpr (RIDE && S >= 12) {
                // behind k-step 1's sync point (step 12): the pieces of k-step 5 -> slot 1, one every other step; the B fragments of
                // k-step 2 into the register-set-0 slots whose column has had its k-step-0 MFMAs (column j: steps 4 j + 4 .. 4 j + 7)
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (S % 2 == 0 && S <= 26) G6_DMA_ASM(1, (S - 12) / 2, kt1024 + 1024);
                if constexpr (S == 12) G6_RDB(0, 2, 0);
                if constexpr (S == 13) G6_RDB(0, 2, 1);
                if constexpr (S == 16) G6_RDB(0, 2, 2);
                if constexpr (S == 20) G6_RDB(0, 2, 3);
                if constexpr (S == 24) G6_RDB(0, 2, 4);
                if constexpr (S == 28) G6_RDB(0, 2, 5);
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (IT < 6) g6_epi_sum<p, IT>(); else g6_rowsum<IT>(v);
            __builtin_amdgcn_sched_barrier(0);
        });
        // the tail: the last slice of column 6, then column 7's four slices (read together: one exposed LDS round trip, under
        // column 7's k-step-0 MFMAs when the next tile rides)
        G6_STORE_SLICE(wq, 6, 3);
        const u32x4 w0 = G6_READ_SLICE(7, 0), w1 = G6_READ_SLICE(7, 1), w2 = G6_READ_SLICE(7, 2), w3 = G6_READ_SLICE(7, 3);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RIDE) {
            g6_for<8>([&](auto m_c) __attribute__((always_inline)) { g6_mfma_k0<decltype(m_c)::value, 7>(); });
        } else {
            asm volatile("s_nop 7" ::: "memory");     // the last row-sum MFMA is a handful of instructions old
        }
        __builtin_amdgcn_sched_barrier(0);
        G6_STORE_SLICE(w0, 7, 0);
        G6_STORE_SLICE(w1, 7, 1);
        G6_STORE_SLICE(w2, 7, 2);
        G6_STORE_SLICE(w3, 7, 3);
        // partial row sums of this wave's 128 concepts: lane (fq, fr) holds image 16 fq + fr in register 0 of the row-sum block
        // and image 16 (fq + 4) + fr in register 2; images past the last one fall outside the descriptor
        {
            const __amdgpu_buffer_rsrc_t rs_p = __builtin_amdgcn_make_buffer_rsrc((void*)(part + ((int64_t)(ptm * 2 + wr) * ldpart + i0_)), 0, __builtin_amdgcn_readfirstlane(rows_ * 4), 0x00020000);
            const float r0 = g6_acc<G6_RS0>(), r2 = g6_acc<G6_RS0 + 2>();
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r0), rs_p, lane4, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r2), rs_p, lane4 + 256u, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RIDE) {
            // columns 6 and 7 of k-step 1 and, under them, the rest of k-step 2's fragments: its A side (every k-step-0 MFMA has
            // been issued: register set 0 is free) and B 6, B 7
            g6_for<16>([&](auto j_c) __attribute__((always_inline)) {
                constexpr int j = decltype(j_c)::value;
                g6_mfma_k1<j & 7, 6 + (j >> 3)>();
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (j < 8) G6_RDA(0, 2, j);
                if constexpr (j == 8) G6_RDB(0, 2, 6);
                if constexpr (j == 9) G6_RDB(0, 2, 7);
                __builtin_amdgcn_sched_barrier(0);
            });
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    using g6_true = std::integral_constant<bool, true>;
    using g6_false = std::integral_constant<bool, false>;
    // a tile needs the mask when this wave's 128 concepts reach past the last concept
#define G6_EDGE() (ptm * 256 + wr * 128 + 128 > (int)Mc)

    for (;;) {
        int t4 = 0;
#define G6_KB(t4_) ((t4_) == nt4 - 1 ? 0 : ((t4_) + 1) * 4096)
#define G6_TAIL_SWITCH()                                 \
    do {                                                 \
        if (t4 == nt4 - 1 && has_next) G6_SET_TILE(ntm, ntn); \
    } while (0)
        // ---- first ring round.  In the tile's last round the DMA side crosses into the next tile (past the last tile it
        // re-stages this one: nobody reads it, and the issue / wait sequence stays free of conditions)
        {
            G6_TAIL_SWITCH();
            const int kb = G6_KB(t4);
            if (pending) {                     // k-steps 0 and 1 ride the previous tile's epilogue
                if (G6_EDGE()) epilogue(g6_true{}, g6_true{}, kb); else epilogue(g6_true{}, g6_false{}, kb);
            } else {
                G6_KSTEP(0, true, true, kb);
            }
            if (!pending) G6_KSTEP(1, false, true, kb + 1024);     // (a test of its own: inside the else above, hipcc lays the K loop out differently)
            G6_KSTEP(2, false, true, kb + 2048);
            G6_KSTEP(3, false, true, kb + 3072);
        }
        for (t4 = 1; t4 < nt4; ++t4) {
            G6_TAIL_SWITCH();
            const int kb = G6_KB(t4);
            G6_KSTEP(0, false, false, kb);
            G6_KSTEP(1, false, false, kb + 1024);
            G6_KSTEP(2, false, false, kb + 2048);
            G6_KSTEP(3, false, false, kb + 3072);
        }
        ptm = tm;
        ptn = tn;
        pending = true;
        if (!has_next) break;
        tm = ntm;
        tn = ntn;
        G6_WALK_NEXT();
    }
    epilogue(g6_false{}, g6_true{}, 0);   // the last tile's, with nothing riding it (the masked form serves any tile)
    // the refills past the last k-step are still in flight: they must land before this workgroup's LDS is handed to the next one
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef G6_WALK_NEXT
#undef G6_KB
#undef G6_TAIL_SWITCH
#undef G6_EDGE
#undef G6_READ_SLICE
#undef G6_STORE_SLICE
#undef G6_KSTEP
#undef G6_OP
#undef G6_SYNC
#undef G6_STAGE_ALL
#undef G6_RDA
#undef G6_RDB
#undef G6_DMA
#undef G6_DMA_ASM
#undef G6_DMA_M0
#undef G6_SET_TILE
#undef G6_BLK
}

#endif
