// k_gemm.hip -- K1: P = I_hat @ T_hat^T, the one dense contraction of the path (MFMA).
//   replaces  clip_feats = image_features @ text_features.T   concept_vit/utils.py:594
//
// Both operands are K-contiguous ("NT" GEMM: I is [N,D], T is [C,D]), which is exactly the
// fragment order the MFMA A and B operands want.
//
// mode MCD_GEMM_F32 (parity mode): v_mfma_f32_32x32x2_f32 -- exact fp32, bit-for-bit a k-ordered
//   fmaf chain (64 FLOP/clk/SIMD, 157 TFLOP/s peak).  128x128 output tile per 256-thread workgroup,
//   4 waves as 2x2, each wave 64x64 = 2x2 MFMA tiles (64 accumulator registers), BK = 32, operands
//   staged through a double-buffered LDS image with 33-float rows so the per-lane fragment reads
//   (row = lane&31, k = kk + lane>>5) hit 32 distinct banks; the next K-tile is prefetched into registers
//   under the MFMAs.
#include "mcd_common.h"
#include <string.h>
#include <stdlib.h>
#include <type_traits>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int BM = 128, BN = 128, BK = 32, LDK = BK + 1;

// Tile of this workgroup.  Workgroups go to the XCDs round-robin (id % 8), so the column tiles of one row-tile are
// given to ONE XCD (consecutive ids of that XCD): its L2 fetches the A rows once instead of once per column tile
// (measured at 10 000 x 763 x 512 with the plain 2-D grid: 130 MB fetched for 22 MB of operands).
__device__ __forceinline__ bool xcd_tile(int64_t M, int64_t Nc, int& tile_r, int& tile_c) {
    const int ncol = (int)((Nc + BN - 1) / BN), nrow = (int)((M + BM - 1) / BM);
    const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
    tile_r = (seq / ncol) * 8 + xcd;
    tile_c = seq % ncol;
    return tile_r < nrow;
}

// global -> registers: thread t fetches 4 quads of the 128 x 32 tile: f = t + 256*it -> row f/8, k-quad (f%8)*4
template <bool ALIGNED>
__device__ __forceinline__ void fetch_tile(const float* __restrict__ G, int64_t ldg, int64_t rows, int64_t row0,
                                           int64_t Kd /* elements at or past it read as 0 */, int64_t k0,
                                           float4 (&v)[4]) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int f = threadIdx.x + 256 * it;
        const int r = f >> 3, kq = (f & 7) * 4;
        const int64_t gr = row0 + r, gk = k0 + kq;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gr < rows) {
            const float* src = G + gr * ldg + gk;
            if (ALIGNED && gk + 3 < Kd) {
                t = *reinterpret_cast<const float4*>(src);
            } else {
                if (gk + 0 < Kd) t.x = src[0];
                if (gk + 1 < Kd) t.y = src[1];
                if (gk + 2 < Kd) t.z = src[2];
                if (gk + 3 < Kd) t.w = src[3];
            }
        }
        v[it] = t;
    }
}

// registers -> LDS tile (33-float rows)
__device__ __forceinline__ void store_tile(const float4 (&v)[4], float* __restrict__ L) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int f = threadIdx.x + 256 * it;
        float* d = L + (f >> 3) * LDK + (f & 7) * 4;
        d[0] = v[it].x; d[1] = v[it].y; d[2] = v[it].z; d[3] = v[it].w;
    }
}

// Software pipeline: the loads of K-tile t+1 are issued before the 64 MFMAs of tile t and land in registers
// while the matrix pipe works; they are written to the OTHER LDS buffer after the MFMAs, one barrier per tile.
//
// K-blocks.  The reference's P comes from torch's CPU matmul = MKL sgemm, which on the torch 2.10 build that made the
// golden vectors cuts K into blocks, runs one fma chain per block from 0 and adds the block results in order (rule in
// gemm_kblocks() below; DESIGN.md section 5 states how it was established).  KBLOCKS = true follows it: K-tiles never
// cross a block end (the staging zero-fills past it, and fma(0, 0, acc) = acc), and after a block's last tile the
// accumulators are folded into `tot` and cleared.  P is then bit-identical to the reference's for the embedding
// widths it has (512; also 768 and 1024).  64 more registers (208): still the 2 workgroups per CU the LDS allows.
template <bool ALIGNED, bool KBLOCKS>
__global__ __launch_bounds__(256, 2) void gemm_nt_f32_kernel(const float* __restrict__ A, int64_t lda,
                                                           const float* __restrict__ B, int64_t ldb, int64_t M,
                                                           int64_t Nc, int64_t Kd, float* __restrict__ Cc,
                                                           int64_t ldc, int64_t kb_first, int64_t kb_step) {
    __shared__ float As[2][BM * LDK];
    __shared__ float Bs[2][BN * LDK];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    int tile_r, tile_c;
    if (!xcd_tile(M, Nc, tile_r, tile_c)) return;
    const int64_t row0 = (int64_t)tile_r * BM, col0 = (int64_t)tile_c * BN;
    const int fr = lane & 31, fk = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    f32x16 tot[KBLOCKS ? 2 : 1][KBLOCKS ? 2 : 1];
    if (KBLOCKS) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[mi * KBLOCKS][ni * KBLOCKS][r] = 0.f;
    }
    // K-tiles walk the blocks one after the other: a tile never crosses a block end (fetch_tile() zero-fills past
    // `k_end`, and fma(0, 0, acc) = acc exactly), so a block's chain ends with its last tile, where it is folded.
    int64_t k0 = 0;                                        // start of the tile being computed
    int64_t k_end = KBLOCKS ? kb_first : Kd;               // end of its block
    float4 ra[4], rb[4];
    fetch_tile<ALIGNED>(A, lda, M, row0, k_end, 0, ra);
    fetch_tile<ALIGNED>(B, ldb, Nc, col0, k_end, 0, rb);
    store_tile(ra, As[0]);
    store_tile(rb, Bs[0]);
    __syncthreads();
    for (int cur = 0; k0 < Kd; cur ^= 1) {
        // the tile after this one: next in the block, or the first of the next block
        const bool block_ends = k0 + BK >= k_end;
        const int64_t n0 = block_ends ? k_end : k0 + BK;
        int64_t n_end = k_end;
        if (KBLOCKS && block_ends) n_end = kb_step > 0 ? (k_end + kb_step < Kd ? k_end + kb_step : Kd) : Kd;
        const bool more = n0 < Kd;
        if (more) {
            fetch_tile<ALIGNED>(A, lda, M, row0, n_end, n0, ra);
            fetch_tile<ALIGNED>(B, ldb, Nc, col0, n_end, n0, rb);
        }
        const float* as = As[cur];
        const float* bs = Bs[cur];
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float a[2], b[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[mi] = as[(wr * 64 + mi * 32 + fr) * LDK + kk + fk];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) b[ni] = bs[(wc * 64 + ni * 32 + fr) * LDK + kk + fk];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
        if (KBLOCKS && block_ends) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tot[mi * KBLOCKS][ni * KBLOCKS][r] += acc[mi][ni][r];
                        acc[mi][ni][r] = 0.f;
                    }
        }
        if (more) {
            store_tile(ra, As[cur ^ 1]);
            store_tile(rb, Bs[cur ^ 1]);
        }
        __syncthreads();
        k0 = n0;
        k_end = n_end;
    }

    // C/D layout of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t gr = row0 + wr * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
                const int64_t gc = col0 + wc * 64 + ni * 32 + fr;
                const float v = KBLOCKS ? tot[mi * KBLOCKS][ni * KBLOCKS][r] : acc[mi][ni][r];
                if (gr < M && gc < Nc) Cc[gr * ldc + gc] = v;
            }
}

// DMA form of the fp32 kernel above for the aligned case (rows 16-byte aligned, every K-tile whole and inside one K-block, the
// operands below 2 GB): the K-tiles go from global memory straight into LDS (`buffer_load_dwordx4 ... lds`, two 32 KB stages), no
// staging registers, no LDS stores, no bounds tests.  A lane's 16 bytes are four consecutive k of one row; the stage holds them
// quad-major ([k-quad][row], 16-byte units), so a wave's instruction fills 1 KB of LDS linearly and the 32x32x2 fragment read is
// ds_read_b32 at ((q * 128 + row) * 4 + e) words -- rows r and r + 16 share a bank (two passes per read; the reads are 1/60 of the
// MFMA time).  One barrier per K-tile hands over the tile that has landed and frees the stage the next one is issued into.
// Same MFMA instruction over the same k order as the kernel above: the same bits.  10 000 x 763 x 512: 0.0812-0.0816 against
// 0.0845-0.0848 ms; 3.95 against 4.14 us per K-tile in the steady state (profiles/r04_k1_ksweep.txt).  (K-tiles of 16, three
// workgroups per CU instead of two: the same time -- with one or two tiles per CU the launch is as long as a CU's two tiles.)
// Round 5: the NEXT K-tile's eight DMA instructions do not sit back to back behind the barrier -- an LDS-DMA
// instruction with no MFMA in flight costs its wave ~150 issue cycles, ~1 200 idle cycles of the matrix pipe per K-tile for a workgroup
// that has its CU to itself -- but one behind every fourth MFMA of the tile's first half, with the fragments double-buffered one k-quad
// ahead: 85.3 -> 81.4 us in cold-clock traces, 74.9 -> 70.9 us (0.70 of the fp32 MFMA peak) once the clock has ramped
// (profiles/r05_k1_notes.txt, r05_k1_spread.txt; tests/test_k1s_isa_cpu.py pins the placement).
// (What else rounds 4-5 measured on this kernel and retired -- all DMA instructions behind the barrier, the hand-over moved in front
// of the tile's last quad, wave priorities by progress, a 256 x 128 tile with one 512-thread workgroup per CU and two K-tiles in
// flight: none faster, profiles/r05_k1_notes.txt, r05_k1_spread.txt, r05_k1_wide.txt; the code: scripts/README.md, archive row.)
// BST: the output through a buffer descriptor (the epilogue below); host: max(M, BM) * ldc * 4 < 2^31, else the plain stores.
template <bool KBLOCKS, bool BST>
__global__ __launch_bounds__(256, 2) void gemm_nt_f32_dma_kernel(const float* __restrict__ A, int64_t lda,
                                                               const float* __restrict__ B, int64_t ldb, int64_t M,
                                                               int64_t Nc, int64_t Kd, float* __restrict__ Cc,
                                                               int64_t ldc, int64_t kb_first, int64_t kb_step) {
    constexpr int NI = BK / 8;                                                // DMA instructions per operand, wave and K-tile: 4
    __shared__ __attribute__((aligned(16))) float s_t[2][2 * BM * BK];      // [stage][A: 8 quads x 128 rows x 4 | B: likewise]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wr = wave >> 1, wc = wave & 1;
    int tile_r, tile_c;
    if (!xcd_tile(M, Nc, tile_r, tile_c)) return;
    const int64_t row0 = (int64_t)tile_r * BM, col0 = (int64_t)tile_c * BN;
    const int fr = lane & 31, fk = lane >> 5;

    // DMA side: instruction j (0..3) of this wave moves the 16-byte units p = j * 256 + wave * 64 + lane, unit p = quad (p >> 7)
    // of row (p & 127); rows past the operand's last clamp to it (their products are never stored)
    const __amdgpu_buffer_rsrc_t ra_ = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, (int)(M * lda * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_ = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, (int)(Nc * ldb * 4), 0x00020000);
    unsigned va[NI], vb[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int pu = j * 256 + (int)threadIdx.x;
        const int q = pu >> 7, r = pu & 127;
        const int64_t ga = row0 + r < M ? row0 + r : M - 1, gb = col0 + r < Nc ? col0 + r : Nc - 1;
        va[j] = (unsigned)((ga * lda + 4 * q) * 4);
        vb[j] = (unsigned)((gb * ldb + 4 * q) * 4);
    }
    char* sb = reinterpret_cast<char*>(&s_t[0][0]);
    // all 2 NI instructions of a K-tile (the prologue's)
#define MCD_K1_DMA(stage_, k0_)                                                                                              \
    do {                                                                                                                     \
        char* d_ = sb + (stage_) * (2 * BM * BK * 4) + wave * 1024;                                                          \
        const int so_ = (int)(k0_) * 4;                                                                                      \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (__attribute__((address_space(3))) void*)(d_), 16, va[0], so_, 0, 0);          \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (__attribute__((address_space(3))) void*)(d_ + 4096), 16, va[1], so_, 0, 0);   \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (__attribute__((address_space(3))) void*)(d_ + 8192), 16, va[2], so_, 0, 0);   \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (__attribute__((address_space(3))) void*)(d_ + 12288), 16, va[3], so_, 0, 0);  \
        char* e_ = d_ + BM * BK * 4;                                                                                         \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (__attribute__((address_space(3))) void*)(e_), 16, vb[0], so_, 0, 0);          \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (__attribute__((address_space(3))) void*)(e_ + 4096), 16, vb[1], so_, 0, 0);   \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (__attribute__((address_space(3))) void*)(e_ + 8192), 16, vb[2], so_, 0, 0);   \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (__attribute__((address_space(3))) void*)(e_ + 12288), 16, vb[3], so_, 0, 0);  \
    } while (0)
    // ONE of the wave's 2 NI instructions of a K-tile: j < NI operand A's unit block j, else operand B's j - NI
#define MCD_K1_DMA1(stage_, k0_, j_)                                                                                         \
    do {                                                                                                                     \
        char* d_ = sb + (stage_) * (2 * BM * BK * 4) + wave * 1024 + ((j_) < NI ? 0 : BM * BK * 4) + ((j_) % NI) * 4096;     \
        if ((j_) < NI) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra_, (__attribute__((address_space(3))) void*)(d_), 16, va[(j_) % NI], (int)(k0_) * 4, 0, 0); \
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rb_, (__attribute__((address_space(3))) void*)(d_), 16, vb[(j_) % NI], (int)(k0_) * 4, 0, 0); \
    } while (0)

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    f32x16 tot[KBLOCKS ? 2 : 1][KBLOCKS ? 2 : 1];
    if (KBLOCKS) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[mi * KBLOCKS][ni * KBLOCKS][r] = 0.f;
    }
    // fragment reads: row (w? * 64 + m * 32 + fr), quad kk >> 2, element (kk & 3) + fk -- kk is even, so the quad is a compile-time
    // constant and the lane's own part of the address does not change over the K-tile
    const int a_lane = ((wr * 64 + fr) * 4 + fk) * 4, b_lane = (BM * BK + (wc * 64 + fr) * 4 + fk) * 4;   // bytes
    int64_t k_end = KBLOCKS ? kb_first : Kd;
    MCD_K1_DMA(0, 0);
    int cur = 0;
    float fa[2][2][2], fb[2][2][2];         // fragment registers, [buffer][mi | ni][k pair within the quad]
    static_assert((BK / 4) % 2 == 0, "the fragment buffers' parity carries over from a K-tile's last quad to the next one's first");
    for (int64_t k0 = 0; k0 < Kd; k0 += BK, cur ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's pieces of the tile have landed ...
        __syncthreads();                                     // ... everyone's have, and everyone is done with the other stage
        const char* st_ = sb + cur * (2 * BM * BK * 4);
        // The next K-tile's 2 NI DMA instructions go out BETWEEN this tile's MFMAs, two per quad of k (8 MFMAs) in the tile's first
        // half -- an LDS-DMA instruction that is not under MFMAs costs its wave ~150 cycles of issue (MI355X_MICROARCH.md, cycle
        // constants), and eight of them behind the barrier were ~1 200 of the ~1 570 cycles a K-tile took beyond its 4 096 cycles
        // of MFMAs when its workgroup had the CU to itself (profiles/r05_k1_notes.txt: 2.75 us per K-tile alone, 4.8 per pair).
        // The fragments of quad q + 1 are read at the top of quad q (double-buffered registers); sched_barriers hold the
        // written order.  Same MFMAs over the same k in the same order per accumulator: the same bits.
        const bool more = k0 + BK < Kd;
        auto frag = [&](const char* stg, int qd, int bf) __attribute__((always_inline)) {
            const char* base = stg + qd * (BM * 16);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    fa[bf][m][h] = *reinterpret_cast<const float*>(base + a_lane + h * 8 + m * 32 * 16);
                    fb[bf][m][h] = *reinterpret_cast<const float*>(base + b_lane + h * 8 + m * 32 * 16);
                }
        };
        frag(st_, 0, 0);
#pragma unroll
        for (int qd = 0; qd < BK / 4; ++qd) {
            const int c = qd & 1;
            if (qd + 1 < BK / 4) frag(st_, qd + 1, c ^ 1);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][0][0], fb[c][0][0], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][0][0], fb[c][1][0], acc[0][1], 0, 0, 0);
            if (qd < NI) {
                __builtin_amdgcn_sched_barrier(0);
                if (more) MCD_K1_DMA1(cur ^ 1, k0 + BK, 2 * qd);
                __builtin_amdgcn_sched_barrier(0);
            }
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][1][0], fb[c][1][0], acc[1][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][1][0], fb[c][0][0], acc[1][0], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][0][1], fb[c][0][1], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][0][1], fb[c][1][1], acc[0][1], 0, 0, 0);
            if (qd < NI) {
                __builtin_amdgcn_sched_barrier(0);
                if (more) MCD_K1_DMA1(cur ^ 1, k0 + BK, 2 * qd + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][1][1], fb[c][1][1], acc[1][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][1][1], fb[c][0][1], acc[1][0], 0, 0, 0);
        }
        if (KBLOCKS && k0 + BK >= k_end) {                   // the block's chain ends with this tile: fold it
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tot[mi * KBLOCKS][ni * KBLOCKS][r] += acc[mi][ni][r];
                        acc[mi][ni][r] = 0.f;
                    }
            k_end = kb_step > 0 ? (k_end + kb_step < Kd ? k_end + kb_step : Kd) : Kd;
        }
    }
#undef MCD_K1_DMA
#undef MCD_K1_DMA1
    // C/D layout of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    if constexpr (BST) {
        // The 64 values of a lane leave through ONE buffer descriptor based at the tile's first element and ending with the
        // matrix's last row: a row past it is dropped by the hardware's range check, a column past the last one by an offset
        // past any range -- one v_add + one store per value.  (The plain form below spends ~14 instructions per value on 64-bit
        // address products, compares and a branch: ~900 instructions, the 2.4 us per workgroup of profiles/r05_k1_notes.txt.)
        const int room = __builtin_amdgcn_readfirstlane((int)((((M - row0) * ldc) - col0) * 4));      // host: max(M, BM) * ldc * 4 < 2^31 (every row of the tile, real or not, gets an offset) -- test_embed_gemm_wide_pitch_keeps_the_gap
        const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc((void*)(Cc + (row0 * ldc + col0)), 0, room, 0x00020000);
        const int ldc4 = (int)ldc * 4;
        const unsigned vbase = (unsigned)((wr * 64 + 4 * fk) * ldc4 + (wc * 64 + fr) * 4);
        unsigned vcol[2];
        vcol[0] = col0 + wc * 64 + fr < Nc ? vbase : 0x80000000u;
        vcol[1] = col0 + wc * 64 + 32 + fr < Nc ? vbase + 128u : 0x80000000u;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int roff = (mi * 32 + (r & 3) + 8 * (r >> 2)) * ldc4;      // uniform
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const float v = KBLOCKS ? tot[mi * KBLOCKS][ni * KBLOCKS][r] : acc[mi][ni][r];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs_c, vcol[ni] + (unsigned)roff, 0, 0);
                }
            }
    } else {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t gr = row0 + wr * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
                    const int64_t gc = col0 + wc * 64 + ni * 32 + fr;
                    const float v = KBLOCKS ? tot[mi * KBLOCKS][ni * KBLOCKS][r] : acc[mi][ni][r];
                    if (gr < M && gc < Nc) Cc[gr * ldc + gc] = v;
                }
    }
}

// MKL's K cut as observed (see the kernel comment): first boundary and the distance between the following ones
// (0: none follow).  Returns false when there is a single block.
inline bool gemm_kblocks(int64_t K, int64_t& first, int64_t& step) {
    if (K <= 384) return false;
    if (K <= 768) {
        first = ((K + 1) / 2 + 3) / 4 * 4;
        step = 0;
    } else {
        first = 384;
        step = 384;
    }
    return true;
}

// ---- bf16 MFMA modes ---------------------------------------------------------------------------------
// MCD_GEMM_BF16X3: every fp32 operand is split on the fly (while it is staged into LDS) into hi = bf16(x) and
// lo = bf16(x - hi); the product is accumulated in fp32 as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16
// (the lo*lo term, ~2^-18 relative, is dropped): |dP| <= ~1.2e-5 * sum|a_k b_k| (1e-6 observed on 512-d unit
// vectors, against 2.4e-7 for the exact fp32 mode) at the
// bf16 MFMA rate (16x the fp32 MFMA rate per instruction, 3 instructions per product).
// MCD_GEMM_BF16: hi*hi only (|dP| ~ 4e-3): for the stress configuration, no parity claim.
// Same 128x128 tile / 2x2 waves / register-prefetch pipeline as the fp32 kernel.  LDS rows are 32 bf16 + 8 pad
// (80 B): the 16-byte fragment reads of a 16-lane group then fall on 16 distinct 4-bank groups (conflict-free).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
constexpr int LDB = BK + 8;  // bf16 elements per LDS row

__device__ __forceinline__ unsigned short f32_to_bf16_rne(float x) {  // finite inputs (normalised embeddings)
    const unsigned u = __float_as_uint(x);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

template <bool SPLIT>
__device__ __forceinline__ void store_tile_bf16(const float4 (&v)[4], unsigned short* __restrict__ Lhi,
                                                unsigned short* __restrict__ Llo) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int f = threadIdx.x + 256 * it;
        const int o = (f >> 3) * LDB + (f & 7) * 4;
        const float x[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
        unsigned short h[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[j] = f32_to_bf16_rne(x[j]);
            l[j] = SPLIT ? f32_to_bf16_rne(x[j] - bf16_to_f32(h[j])) : 0;
        }
        *reinterpret_cast<uint2*>(Lhi + o) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
        if (SPLIT)
            *reinterpret_cast<uint2*>(Llo + o) = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
    }
}

template <bool ALIGNED, bool SPLIT>
__global__ __launch_bounds__(256) void gemm_nt_bf16_kernel(const float* __restrict__ A, int64_t lda,
                                                            const float* __restrict__ B, int64_t ldb, int64_t M,
                                                            int64_t Nc, int64_t Kd, float* __restrict__ Cc,
                                                            int64_t ldc) {
    constexpr int NARR = SPLIT ? 2 : 1;
    __shared__ __attribute__((aligned(16))) unsigned short As[2][NARR][BM * LDB];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[2][NARR][BN * LDB];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    int tile_r, tile_c;
    if (!xcd_tile(M, Nc, tile_r, tile_c)) return;
    const int64_t row0 = (int64_t)tile_r * BM, col0 = (int64_t)tile_c * BN;
    const int fr = lane & 31, fh = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    float4 ra[4], rb[4];
    fetch_tile<ALIGNED>(A, lda, M, row0, Kd, 0, ra);
    fetch_tile<ALIGNED>(B, ldb, Nc, col0, Kd, 0, rb);
    store_tile_bf16<SPLIT>(ra, As[0][0], As[0][NARR - 1]);
    store_tile_bf16<SPLIT>(rb, Bs[0][0], Bs[0][NARR - 1]);
    __syncthreads();
    const int64_t nt = (Kd + BK - 1) / BK;
    for (int64_t t = 0; t < nt; ++t) {
        const int cur = (int)(t & 1);
        if (t + 1 < nt) {
            fetch_tile<ALIGNED>(A, lda, M, row0, Kd, (t + 1) * BK, ra);
            fetch_tile<ALIGNED>(B, ldb, Nc, col0, Kd, (t + 1) * BK, rb);
        }
#pragma unroll
        for (int ks = 0; ks < BK; ks += 16) {
            bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ao = (wr * 64 + i * 32 + fr) * LDB + ks + 8 * fh;
                const int bo = (wc * 64 + i * 32 + fr) * LDB + ks + 8 * fh;
                ah[i] = *reinterpret_cast<const bf16x8*>(&As[cur][0][ao]);
                bh[i] = *reinterpret_cast<const bf16x8*>(&Bs[cur][0][bo]);
                if (SPLIT) {
                    al[i] = *reinterpret_cast<const bf16x8*>(&As[cur][NARR - 1][ao]);
                    bl[i] = *reinterpret_cast<const bf16x8*>(&Bs[cur][NARR - 1][bo]);
                }
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    if (SPLIT) {  // small terms first
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh[ni], acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl[ni], acc[mi][ni], 0, 0, 0);
                    }
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh[ni], acc[mi][ni], 0, 0, 0);
                }
        }
        if (t + 1 < nt) {
            store_tile_bf16<SPLIT>(ra, As[cur ^ 1][0], As[cur ^ 1][NARR - 1]);
            store_tile_bf16<SPLIT>(rb, Bs[cur ^ 1][0], Bs[cur ^ 1][NARR - 1]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t gr = row0 + wr * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                const int64_t gc = col0 + wc * 64 + ni * 32 + fr;
                if (gr < M && gc < Nc) Cc[gr * ldc + gc] = acc[mi][ni][r];
            }
}

// ---- large bf16 GEMM (stress shape: tens of thousands of images x thousands of concepts) -------------------
// Operands are converted ONCE to bf16 (hi, and lo for the split mode) by split_bf16_kernel: rows of Kp = D rounded
// up to 64 elements, zero padded, so the GEMM stages raw bytes.  This kernel is the split mode's (MCD_GEMM_BF16X3; the
// single-pass mode runs the persistent kernel further down): 256 x 256 output tile per 512-thread workgroup,
// 8 waves as 2 (M) x 4 (N), each wave 128 x 64 = 4 x 2 tiles of v_mfma_f32_32x32x16_bf16 (128 accumulator
// registers).  K-tiles of 32 elements go global -> LDS by global_load_lds_dwordx4 (no VGPR round trip, 16 B per
// lane, the wave's 1 KB lands contiguously) into two LDS stages of 64 KB (four arrays: A hi, A lo, B hi, B lo), the
// DMAs of the next K-tile in flight under the MFMAs of this one.  The wait for stage t is an s_waitcnt vmcnt
// followed by a raw s_barrier.
// LDS image of a tile: row r (64 bytes) holds its four 16-byte chunks permuted, chunk c at position
//   c ^ ((r / 4) % 4)
// (the permutation is applied to the per-lane GLOBAL address, the LDS side of the DMA is lane-linear); the 16 lanes
// that one ds_read_b128 services together then cover the 16 distinct 16-byte slots of the 256-byte bank row:
// conflict-free fragment reads (SQ_LDS_BANK_CONFLICT = 0 measured).
// Tile order: workgroup id -> XCD (id % 8) -> bands of 2 row-tiles dealt round-robin to the XCDs; inside a band the
// column tiles advance with the 2 row-tiles innermost, so an XCD's L2 keeps its band's A rows (2 x 256 KB at D=512)
// for the whole band and every B tile it fetches serves 2 row-tiles at once.  The output goes out with
// nontemporal stores: 256 KB per tile that nobody on this XCD reads again must not evict the operands.
constexpr int GB_M = 256, GB_N = 256, GB_K = 32, GB_THREADS = 512, GB_RS = 2;
constexpr int GB_RB = 2 * GB_K;             // bytes per LDS tile row
constexpr int GB_T_BYTES = 256 * GB_RB;     // one 256-row K-tile of one array: 16 KB

// element offset of element k of row r in the fragment-major image of the K1s kernel (k_gexp_v6.inc; nkt = K-tiles of 32
// per row): 1-KB pieces [row block of 16][K-tile], inside a piece the 16-byte chunk j = row (j & 15), k-chunk (j >> 4) -- the lane
// order of a v_mfma_f32_16x16x32_bf16 fragment.  paired (the concept side): the rows of two adjacent blocks are interleaved,
// block 2p + h, row i <-> row 32 p + 8 (i / 4) + 4 h + i % 4 of the operand.
__device__ __forceinline__ int64_t frag_major_off(int64_t r, int64_t k, int64_t nkt, bool paired) {
    int64_t rb;
    int i;
    if (paired) {
        const int w = (int)(r & 31);
        rb = ((r >> 5) << 1) + ((w >> 2) & 1);
        i = ((w >> 3) << 2) + (w & 3);
    } else {
        rb = r >> 4;
        i = (int)(r & 15);
    }
    return ((rb * nkt + (k >> 5)) << 9) + ((int64_t)((((int)(k >> 3) & 3) << 4) + i) << 3) + (k & 7);
}

// bf16 operand layouts the conversion kernels write: pitch > 0 row-major rows of `pitch` elements; -2 fragment-major;
// -3 fragment-major, paired rows
__device__ __forceinline__ int64_t operand_off(int64_t r, int64_t k, int64_t Kp, int64_t pitch) {
    return pitch > 0 ? r * pitch + k : frag_major_off(r, k, Kp >> 5, pitch == -3);
}
// rows the layout stages as whole blocks (the rows that pad the last block are written as zeros)
__device__ __forceinline__ int64_t operand_rows(int64_t rows, int64_t pitch) {
    return pitch >= 0 ? rows : pitch == -3 ? (rows + 31) / 32 * 32 : (rows + 15) / 16 * 16;
}

// pitch > 0: row-major rows of `pitch` elements; pitch == 0: pitch = Kp; pitch < 0: see operand_off()
__global__ __launch_bounds__(256) void split_bf16_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows,
                                                          int64_t cols, int64_t Kp, unsigned short* __restrict__ hi,
                                                          unsigned short* __restrict__ lo, int64_t pitch = 0,
                                                          float scale = 1.0f) {
    if (pitch == 0) pitch = Kp;
    const int64_t nq = Kp / 4;  // quads per output row
    const int64_t rows_w = operand_rows(rows, pitch);   // blocked layouts: the last row block is written whole (zeros)
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rows_w * nq; q += (int64_t)gridDim.x * 256) {
        const int64_t r = q / nq, k = (q - r * nq) * 4;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (r < rows && k + j < cols) ? x[r * ldx + k + j] * scale : 0.f;
        unsigned short h[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[j] = f32_to_bf16_rne(v[j]);
            l[j] = f32_to_bf16_rne(v[j] - bf16_to_f32(h[j]));
        }
        const int64_t o = operand_off(r, k, Kp, pitch);
        *reinterpret_cast<uint2*>(hi + o) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
        if (lo) *reinterpret_cast<uint2*>(lo + o) = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
    }
}

__device__ __forceinline__ int gb_pos(int r, int c) { return c ^ ((r >> 2) & 3); }

// DMA of one 256-row K-tile: rows row0.. (clamped to the last valid row), K offset k0 (elements), into LDS at lds.
// One wave instruction moves 1 KB = 16 rows x 64 B; 16 instructions per tile, 2 per wave.
__device__ __forceinline__ void stage_tile(const unsigned short* __restrict__ G, int64_t Kp, int64_t rows, int64_t row0,
                                           int k0, char* lds, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = wave + 8 * i;                   // which 1 KB piece of the tile
        const int r = q * 16 + (lane >> 2);           // tile row of this lane
        const int c = gb_pos(r, lane & 3);            // the chunk this lane's LDS slot must hold
        int64_t gr = row0 + r;
        if (gr >= rows) gr = rows - 1;
        const unsigned short* src = G + gr * Kp + k0 + c * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(lds + q * 1024), 16, 0, 0);
    }
}

__global__ __launch_bounds__(GB_THREADS) void gemm_nt_bf16_big_kernel(
    const unsigned short* __restrict__ Ahi, const unsigned short* __restrict__ Alo,
    const unsigned short* __restrict__ Bhi, const unsigned short* __restrict__ Blo, int64_t Kp, int64_t M, int64_t Nc,
    float* __restrict__ Cc, int64_t ldc, int tiles_m, int tiles_n) {
    constexpr int STAGE = 4 * GB_T_BYTES;          // the four arrays of one K-tile: 64 KB
    constexpr int NSTAGE = 2;                      // 128 KB of LDS
    constexpr int PD = NSTAGE - 1;                 // K-tiles in flight ahead of the one being consumed
    extern __shared__ __attribute__((aligned(1024))) char smem[];  // [NSTAGE][A hi, A lo, B hi, B lo]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile of this workgroup (see the header comment)
    const int xcd = blockIdx.x & 7;
    const int seq = blockIdx.x >> 3;
    const int per_band = GB_RS * tiles_n;
    const int band = (seq / per_band) * 8 + xcd;
    const int j = seq % per_band;
    const int tm = band * GB_RS + j % GB_RS, tn = j / GB_RS;
    if (tm >= tiles_m) return;  // padding of the band grid (whole workgroup)
    const int64_t row0 = (int64_t)tm * GB_M, col0 = (int64_t)tn * GB_N;
    const int wr = wave >> 2, wc = wave & 3;
    const int fr = lane & 31, fh = lane >> 5;

    f32x16 acc[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    auto stage = [&](int t) {
        char* base = smem + (t % NSTAGE) * STAGE;
        stage_tile(Ahi, Kp, M, row0, t * GB_K, base, wave, lane);
        stage_tile(Alo, Kp, M, row0, t * GB_K, base + GB_T_BYTES, wave, lane);
        stage_tile(Bhi, Kp, Nc, col0, t * GB_K, base + 2 * GB_T_BYTES, wave, lane);
        stage_tile(Blo, Kp, Nc, col0, t * GB_K, base + 3 * GB_T_BYTES, wave, lane);
    };
    const int nt = (int)(Kp / GB_K);   // >= 2 (Kp is a multiple of 64)
#pragma unroll
    for (int s0 = 0; s0 < PD; ++s0)
        if (s0 < nt) stage(s0);
    for (int t = 0; t < nt; ++t) {
        // Stage t must have landed: the wait covers this wave's DMAs, the barrier the other waves'; the barrier also
        // says every wave is done with stage t-1, whose buffer the refill below overwrites.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + PD < nt) stage(t + PD);
        const char* base = smem + (t % NSTAGE) * STAGE;
        const char* a_hi = base;
        const char* a_lo = base + GB_T_BYTES;
        const char* b_hi = base + 2 * GB_T_BYTES;
        const char* b_lo = b_hi + GB_T_BYTES;
#pragma unroll
        for (int ks = 0; ks < GB_K / 16; ++ks) {
            bf16x8 ah[4], al[4], bh[2], bl[2];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int r = wr * 128 + mi * 32 + fr;
                const int o = r * GB_RB + gb_pos(r, 2 * ks + fh) * 16;
                ah[mi] = *reinterpret_cast<const bf16x8*>(a_hi + o);
                al[mi] = *reinterpret_cast<const bf16x8*>(a_lo + o);
            }
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int r = wc * 64 + ni * 32 + fr;
                const int o = r * GB_RB + gb_pos(r, 2 * ks + fh) * 16;
                bh[ni] = *reinterpret_cast<const bf16x8*>(b_hi + o);
                bl[ni] = *reinterpret_cast<const bf16x8*>(b_lo + o);
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    // small terms first
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh[ni], acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl[ni], acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh[ni], acc[mi][ni], 0, 0, 0);
                }
        }
    }
    // C/D layout of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    const bool interior = row0 + GB_M <= M && col0 + GB_N <= Nc;  // workgroup-uniform: no per-store bounds test
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t gr = row0 + wr * 128 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                const int64_t gc = col0 + wc * 64 + ni * 32 + fr;
                if (interior || (gr < M && gc < Nc)) __builtin_nontemporal_store(acc[mi][ni][r], Cc + gr * ldc + gc);
            }
}

// ---- persistent form of the large single-pass bf16 GEMM ----------------------------------------------------
// Measured on the 256 x 256 kernel above at 50 000 x 10 000 x 512: main loop alone 0.47 ms, output stores alone
// 0.39 ms, together 0.82 ms -- with one workgroup per CU nothing overlaps a tile's epilogue (and the next tile's
// first DMA round trip).  Here ONE workgroup per CU walks its XCD's tile sequence, and the roles are split:
//   waves 0-7   compute, 2 (M) x 4 (N), each 96 x 64 = 3 x 2 MFMA tiles of a 192 x 256 output tile: per K-tile one
//               barrier, fragment reads, 12 MFMAs; after the last K-tile of an output tile they issue its stores
//               and go straight on -- they never issue a load, so they never wait on vmcnt and the stores drain
//               under the next tile's MFMAs;
//   waves 8-11  DMA loaders: each issues a quarter of every 28 KB stage (7 global_load_lds_dwordx4), keeps up to four
//               stages (112 KB per CU) in flight ACROSS tile boundaries, and arrives at the barrier of stage g only
//               after a counted s_waitcnt vmcnt says its share of stage g has landed.
// Barrier g therefore means: stage g is in LDS (loaders waited) and stage g-1 has been consumed (the compute waves
// passed their MFMAs), so the loaders refill buffer (g-1) % 5 with stage g+4 right after it.  Every wave executes
// exactly one barrier per stage of the workgroup's whole sequence; a workgroup without tiles executes none.
// 12 waves are 3 per SIMD: 168 registers per wave, which is why the tile is 192 and not 256 rows (96 accumulator
// registers; the 128 of a 256-row tile spill into the K loop, and a scratch reload is a vmcnt wait).
// Ablation at 50 000 x 10 000 x 512 (whole call, 0.06 ms of it the bf16 conversion): MFMAs + barriers + fragment
// reads alone 0.39 ms; + DMA 0.53; + stores 0.54; everything 0.70 ms.  Loads and stores ADD: the kernel sits on the
// CU <-> L2 interface (about 40 GB/s per CU for 28 KB staged + 12 KB stored per K-tile), not on the matrix pipe.
constexpr int GP_LW = 4;   // loader waves
constexpr int GP_M = 192, GP_N = 256, GP_WAVES = 8 + GP_LW, GP_THREADS = 64 * GP_WAVES, GP_NSTAGE = 5, GP_PD = GP_NSTAGE - 1;
constexpr int GP_A_BYTES = GP_M * GB_RB, GP_B_BYTES = GP_N * GB_RB, GP_STAGE = GP_A_BYTES + GP_B_BYTES;  // 12 + 16 KB
constexpr int GP_AP = GP_A_BYTES / 1024 / GP_LW, GP_BP = GP_B_BYTES / 1024 / GP_LW;   // 1 KB pieces per loader: 6 + 8
constexpr int GP_IPL = GP_AP + GP_BP;                                                // DMA operations per loader per stage

// Tile order of the persistent kernel: XCD x (workgroup id % 8) owns the column tiles tn = x, x+8, ... for the
// whole launch -- its share of B (tiles_n/8 x 256 KB at D = 512: 1.3 MB for 10 000 concepts) stays in that XCD's
// 4 MB L2, and each A row-tile is fetched from the Infinity Cache once per XCD and then serves all of the XCD's
// column tiles (the row index advances slowest).  Measured before this order (row bands dealt to the XCDs): 27 % of
// the staging requests missed L2 and the ring's 112 KB in flight could not cover their latency.
struct TileWalk {   // the tiles of one persistent workgroup, in order
    int xcd, slot, nslot, ncol_x, n_seq;
    __device__ __forceinline__ TileWalk(int tiles_m, int tiles_n) {
        xcd = blockIdx.x & 7;
        slot = blockIdx.x >> 3;
        nslot = gridDim.x >> 3;
        ncol_x = (tiles_n - xcd + 7) / 8;
        n_seq = tiles_m * ncol_x;
    }
    // advance i to this workgroup's next tile; false when the sequence is exhausted
    __device__ __forceinline__ bool next(int& i, int& tm, int& tn) const {
        ++i;
        const int seq = slot + i * nslot;
        if (seq >= n_seq) return false;
        tm = seq / ncol_x;
        tn = xcd + 8 * (seq - tm * ncol_x);
        return true;
    }
    __device__ __forceinline__ int count() const { return slot < n_seq ? (n_seq - slot + nslot - 1) / nslot : 0; }
};

__global__ __launch_bounds__(GP_THREADS) void gemm_nt_bf16_persist_kernel(
    const unsigned short* __restrict__ A, const unsigned short* __restrict__ B, int64_t Kp, int64_t M, int64_t Nc,
    float* __restrict__ Cc, int64_t ldc, int tiles_m, int tiles_n) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];  // [5 stages][A tile 12 KB, B tile 16 KB]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileWalk W(tiles_m, tiles_n);
    const int nt = (int)(Kp / GB_K);
    const int G = W.count() * nt;   // stages of this workgroup's whole sequence
    if (G == 0) return;

    if (wave >= 8) {
        // ---------------- loader ----------------
        const int lw = wave - 8;
        int li = -1, ltm = 0, ltn = 0, lt = nt;        // next stage to issue: tile li, K-tile lt (nt = "fetch a tile")
        const unsigned short* pa[GP_AP];
        const unsigned short* pb[GP_BP];
        int issued = 0;
        auto issue_one = [&]() {
            if (lt == nt) {                             // first stage of the next tile: per-lane row pointers
                W.next(li, ltm, ltn);
                lt = 0;
#pragma unroll
                for (int k = 0; k < GP_BP; ++k) {
                    const int q = GP_LW * k + lw;       // 1 KB piece (16 rows) of the tile
                    const int r = q * 16 + (lane >> 2);
                    const int c = gb_pos(r, lane & 3);
                    int64_t ga = (int64_t)ltm * GP_M + r, gb = (int64_t)ltn * GP_N + r;
                    if (ga >= M) ga = M - 1;
                    if (gb >= Nc) gb = Nc - 1;
                    if (k < GP_AP) pa[k] = A + ga * Kp + c * 8;
                    pb[k] = B + gb * Kp + c * 8;
                }
            }
            char* base = smem + (issued % GP_NSTAGE) * GP_STAGE;
            const int k0 = lt * GB_K;
#pragma unroll
            for (int k = 0; k < GP_AP; ++k)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa[k] + k0),
                                                 (__attribute__((address_space(3))) void*)(base + (GP_LW * k + lw) * 1024), 16, 0,
                                                 0);
#pragma unroll
            for (int k = 0; k < GP_BP; ++k)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pb[k] + k0),
                                                 (__attribute__((address_space(3))) void*)(base + GP_A_BYTES + (GP_LW * k + lw) * 1024),
                                                 16, 0, 0);
            ++lt;
            ++issued;
        };
        for (int p = 0; p < GP_PD && issued < G; ++p) issue_one();
        for (int g = 0; g < G; ++g) {
            const int later = issued - (g + 1);         // stages issued after stage g: 14 operations each
            if (later >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * GP_IPL) : "memory");
            else if (later == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * GP_IPL) : "memory");
            else if (later == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GP_IPL) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (issued < G) issue_one();
        }
        return;
    }

    // ---------------- compute ----------------
    const int wr = wave >> 2, wc = wave & 3;
    const int fr = lane & 31, fh = lane >> 5;
    // Fragment addresses inside a stage.  Rows 32 apart share the chunk permutation ((r/4)%4 is unchanged), so the
    // 3 (2) row blocks of A (B) are immediate offsets of ONE per-lane address, and the second 16-element K step is
    // the first with chunk bit 1 flipped (address ^ 32): four address registers in all.
    const int ra = wr * 96 + fr, rb = wc * 64 + fr;
    const unsigned a_off0 = (unsigned)(ra * GB_RB + gb_pos(ra, fh) * 16), a_off1 = a_off0 ^ 32u;
    const unsigned b_off0 = (unsigned)(GP_A_BYTES + rb * GB_RB + gb_pos(rb, fh) * 16), b_off1 = b_off0 ^ 32u;
    // this lane's position inside an output tile, as a 32-bit element offset (256 * ldc < 2^31, host-checked)
    const unsigned c_lane = (unsigned)((wr * 96 + 4 * fh) * (int)ldc + wc * 64 + fr);
    int ci = -1, tm, tn, g = 0;
    while (W.next(ci, tm, tn)) {
        f32x16 acc[3][2];
#pragma unroll
        for (int mi = 0; mi < 3; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
        for (int t = 0; t < nt; ++t, ++g) {
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const char* st = smem + (g % GP_NSTAGE) * GP_STAGE;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const char* pa_ = st + (ks ? a_off1 : a_off0);
                const char* pb_ = st + (ks ? b_off1 : b_off0);
                bf16x8 ah[3], bh[2];
#pragma unroll
                for (int mi = 0; mi < 3; ++mi) ah[mi] = *reinterpret_cast<const bf16x8*>(pa_ + mi * 32 * GB_RB);
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) bh[ni] = *reinterpret_cast<const bf16x8*>(pb_ + ni * 32 * GB_RB);
#pragma unroll
                for (int mi = 0; mi < 3; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh[ni], acc[mi][ni], 0, 0, 0);
            }
        }
        // epilogue: C/D layout of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
        // Address = uniform tile base + uniform (row block, register) offset + the lane's 32-bit offset.
        const int64_t row0 = (int64_t)tm * GP_M, col0 = (int64_t)tn * GP_N;
        float* tile = Cc + row0 * ldc + col0;
        const bool interior = row0 + GP_M <= M && col0 + GP_N <= Nc;
        if (interior) {
#pragma unroll
            for (int mi = 0; mi < 3; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float* dst = tile + (int64_t)(mi * 32 + (r & 3) + 8 * (r >> 2)) * ldc + ni * 32 + c_lane;
                        __builtin_nontemporal_store(acc[mi][ni][r], dst);
                    }
        } else {
#pragma unroll
            for (int mi = 0; mi < 3; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t gr = row0 + wr * 96 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                        const int64_t gc = col0 + wc * 64 + ni * 32 + fr;
                        if (gr < M && gc < Nc) Cc[gr * ldc + gc] = acc[mi][ni][r];
                    }
        }
    }
}

// ---- K1s: the stress chain's GEMM -- exp epilogue, bf16 output, row sums (no parity claim) ------------------------
// What the stress configuration (BASELINE configs[4]: 10 000 concepts, bf16 MFMA similarity) needs of K1 + K2 is
//     S[n, c] = softmax_c(a P[n, c]),   P = I_hat T_hat^T.
// Writing fp32 P (1 GB at 25 000 x 10 000) and re-reading it in K2 is what kept the round-1 kernel at 30 % of the bf16
// MFMA peak: the output stream alone cost as much as the matrix work.  Since |P| <= 1 on normalised embeddings,
// exp(a (P - 1)) cannot overflow and needs no row maximum, so the softmax numerator is an ELEMENTWISE function of
// the accumulator: this kernel writes E = bf16(exp(a (P - 1))) straight from the MFMA accumulators (half the bytes of
// fp32 P, and K2 disappears) plus per-tile partial row sums; K4s multiplies by 1 / rowsum when it gathers a row.
//
// The operand roles are SWAPPED against the plain GEMMs above: the MFMA's M side (accumulator registers) runs over CONCEPTS and
// its N side (lanes) over IMAGES, so a lane holds consecutive concepts of ONE image: packing to bf16 needs no lane exchange and
// a row sum is a sum over registers.  The kernel itself: k_gexp_v6.inc (one wave per SIMD, fragment-major operands, epilogue of
// tile i inside the first two k-steps of tile i + 1).
// Tile walk: XCD x owns the concept tiles x, x+8, ... (its share of T_hat, 7 x 192 KB at 10 000 concepts, stays in
// that L2); the image tiles stream past and each is fetched once per XCD.
struct TileWalkR {
    int xcd, slot, nslot, nrow_x, n_seq;
    __device__ __forceinline__ TileWalkR(int tiles_m, int tiles_n) {
        xcd = blockIdx.x & 7;
        slot = blockIdx.x >> 3;
        nslot = gridDim.x >> 3;
        nrow_x = (tiles_m - xcd + 7) / 8;
        n_seq = tiles_n * nrow_x;
    }
    __device__ __forceinline__ bool next(int& i, int& tm, int& tn) const {
        ++i;
        const int seq = slot + i * nslot;
        if (seq >= n_seq) return false;
        tn = seq / nrow_x;
        tm = xcd + 8 * (seq - tn * nrow_x);
        return true;
    }
    __device__ __forceinline__ int count() const { return slot < n_seq ? (n_seq - slot + nslot - 1) / nslot : 0; }
};

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {   // v_cvt_pk_bf16_f32 (RNE, NaN stays NaN)
    const bf16x2 h = __builtin_convertvector(f32x2{lo, hi}, bf16x2);
    unsigned u;
    __builtin_memcpy(&u, &h, 4);
    return u;
}

// (Rounds 2-4 kept three generations of this kernel side by side -- the 12-wave loader / compute kernel on row-major operands,
// round 3's one-wave-per-SIMD kernel on piece-major operands, round 4's v4 on fragment-major operands -- as shape fallbacks
// for one another.  Round 5 guarantees the one remaining kernel's preconditions inside the library instead -- K is padded to a
// multiple of 128 in the operand image, an E pitch that is not a multiple of 16 elements is rejected -- and the older kernels
// left the build: scripts/archive/k_gexp_v4.inc, git history for the others; their measurements: profiles/HISTORY.md.)

// Row L2-normalisation fused with the bf16 conversion (K1a + split_bf16_kernel in one pass over the raw embeddings):
// one wave per row, the row in registers (cols <= 64 * 4 * NQ), y = bf16(x / ||x||), zero padding up to Kp.  The stress
// chain makes no bit-exactness claim, so the sum of squares is a plain wave reduction, not ATen's 8-chain order.
// Both operands in ONE launch (workgroups [0, blocks_a) take the concepts, the rest the images): one dispatch less in front of the GEMM.
template <int NQ>
__global__ __launch_bounds__(256) void normalize_to_bf16_kernel(const float* __restrict__ xa, int64_t lda, int64_t rows_a,
                                                                 unsigned short* __restrict__ ya, float scale_a, unsigned blocks_a,
                                                                 const float* __restrict__ xb, int64_t ldb, int64_t rows_b,
                                                                 unsigned short* __restrict__ yb, float scale_b,
                                                                 int64_t cols, int64_t Kp, int64_t pitch) {
    const bool first = blockIdx.x < blocks_a;              // workgroup-uniform
    const float* __restrict__ x = first ? xa : xb;
    const int64_t ldx = first ? lda : ldb, rows = first ? rows_a : rows_b;
    unsigned short* __restrict__ y = first ? ya : yb;
    const float scale = first ? scale_a : scale_b;
    if (pitch == -2 && first) pitch = -3;       // fragment-major: the first operand (concepts) has its rows paired
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // uniform: the row's descriptor stays in scalar registers
    const int64_t r = (int64_t)(blockIdx.x - (first ? 0u : blocks_a)) * 4 + wave;
    if (r >= rows) {
        // blocked layouts: the rows that pad the last row block are zeros (the 4-wave kernels stage whole blocks)
        if (pitch < 0 && r < operand_rows(rows, pitch)) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int64_t k = (int64_t)(q * 64 + lane) * 4;
                if (k < Kp) *reinterpret_cast<uint2*>(y + operand_off(r, k, Kp, pitch)) = make_uint2(0u, 0u);
            }
        }
        return;
    }
    // The row as NQ 16-byte buffer loads per lane, issued together (behind a per-quad bounds branch hipcc waited for each load
    // before issuing the next); elements at or past `cols` come back as 0, which is what the padded operand holds there.  A row
    // needs dword alignment only.
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(x + r * ldx), 0, (int)cols * 4, 0x00020000);
    float v[NQ][4];
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, q * 1024, 0);
        v[q][0] = __uint_as_float(t[0]); v[q][1] = __uint_as_float(t[1]); v[q][2] = __uint_as_float(t[2]); v[q][3] = __uint_as_float(t[3]);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) ss = __builtin_fmaf(v[q][j], v[q][j], ss);
    ss = mcd_wave_sum(ss);
    const float inv = scale / sqrtf(ss);       // scale: 1, or a log2(e) on the concept side of the folded 4-wave kernel
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int64_t k = (int64_t)(q * 64 + lane) * 4;
        if (k < Kp)
            *reinterpret_cast<uint2*>(y + operand_off(r, k, Kp, pitch)) =
                make_uint2(pack_bf16(v[q][0] * inv, v[q][1] * inv), pack_bf16(v[q][2] * inv, v[q][3] * inv));
    }
}

#include "k_gexp_v6.inc"

// rinv[n] = 1 / sum_t part[t][n]: the partial row sums of the 2 * tiles_m (concept tile, wave row) pairs.  64 images
// per workgroup x 4 interleaved slices of t, folded in a fixed order.
__global__ __launch_bounds__(256) void rowsum_finish_kernel(const float* __restrict__ part, int64_t ldpart, int n_part,
                                                             int64_t Ni, float* __restrict__ rinv) {
    __shared__ float s_p[4][64];
    const int li = threadIdx.x & 63, tg = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * 64 + li;
    float s = 0.f;
    if (n < Ni) {
        float s4[4] = {0.f, 0.f, 0.f, 0.f};       // four loads in flight per thread
        int t = tg;
        for (; t + 12 < n_part; t += 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s4[j] += part[(int64_t)(t + 4 * j) * ldpart + n];
        }
        for (; t < n_part; t += 4) s4[0] += part[(int64_t)t * ldpart + n];
        s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    }
    s_p[tg][li] = s;
    __syncthreads();
    if (tg == 0 && n < Ni) rinv[n] = 1.0f / ((s_p[0][li] + s_p[1][li]) + (s_p[2][li] + s_p[3][li]));
}

// columns [c0, ldE) of every row of E cleared with 16-byte stores (c0 and ldE multiples of 16 concepts, E 16-byte aligned): the
// padding past the last 256-concept tile, which the GEMM kernel never visits
__global__ __launch_bounds__(256) void gexp_zero_pad_kernel(unsigned short* __restrict__ E, int64_t ldE, int64_t Ni, int64_t c0) {
    const int64_t per_row = (ldE - c0) / 8, total = Ni * per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / per_row, q = i - r * per_row;
        *reinterpret_cast<uint4*>(E + r * ldE + c0 + 8 * q) = make_uint4(0u, 0u, 0u, 0u);
    }
}

}  // namespace

// This file reads no development knob: the variants rounds 4-5 measured against these kernels were retired (DESIGN.md section 8;
// scripts/README.md, archive row, names the commit that builds them).  The one environment variable it looks at is a retired knob
// that mcd_embed_gemm_exp refuses instead of silently measuring something else.
static int64_t gemm_kp(int64_t D) { return (D + 63) / 64 * 64; }
// the 256 x 256-tile kernel pays once the tiles outnumber the 256 CUs several times over
static bool gemm_use_big(int64_t N, int64_t C) { return mcd_cdiv(N, GB_M) * mcd_cdiv(C, GB_N) >= 512; }

// CUs of the current device (the persistent kernels launch one workgroup per CU)
static int gemm_cu_count() {
    static std::atomic<int> n_cu_dev[MCD_MAX_DEVICES];      // 0: not asked yet; threads that race store the same count
    const int dev = mcd_cur_device();
    int n_cu = n_cu_dev[dev].load(std::memory_order_acquire);
    if (n_cu == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
        if (n_cu < 8) n_cu = 256;
        n_cu_dev[dev].store(n_cu, std::memory_order_release);
    }
    return n_cu;
}

extern "C" size_t mcd_embed_gemm_workspace(int64_t N, int64_t C, int64_t D, int mode) {
    if (mode == MCD_GEMM_F32 || !gemm_use_big(N, C)) return 0;
    const size_t arrays = (mode == MCD_GEMM_BF16X3) ? 2 : 1;
    return arrays * (size_t)(N + C) * (size_t)gemm_kp(D) * sizeof(unsigned short);
}

extern "C" int mcd_embed_gemm(const float* I, int64_t ldi, const float* T, int64_t ldt, int64_t N, int64_t C,
                              int64_t D, int mode, float* P, int64_t ldp, void* ws, size_t ws_bytes,
                              mcd_stream_t stream) {
    MCD_REQUIRE(I && T && P, MCD_E_ARG, "mcd_embed_gemm: NULL pointer");
    MCD_REQUIRE(N >= 0 && C > 0 && D > 0 && ldi >= D && ldt >= D && ldp >= C, MCD_E_ARG,
                "mcd_embed_gemm: bad shape N=%lld C=%lld D=%lld", (long long)N, (long long)C, (long long)D);
    MCD_REQUIRE(mode == MCD_GEMM_F32 || mode == MCD_GEMM_BF16X3 || mode == MCD_GEMM_BF16, MCD_E_ARG,
                "mcd_embed_gemm: unknown mode %d", mode);
    if (N == 0) return MCD_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t need = mcd_embed_gemm_workspace(N, C, D, mode);
    if (need > 0 && ws && ws_bytes >= need && ((uintptr_t)ws) % 16 == 0 && N < (1LL << 31) && C < (1LL << 31)) {
        // ---- large bf16 path: convert once, then a DMA-staged kernel (split: 256 x 256 tiles; single pass: persistent) ----
        const bool split = mode == MCD_GEMM_BF16X3;
        const int64_t Kp = gemm_kp(D);
        unsigned short* a_hi = (unsigned short*)ws;
        unsigned short* a_lo = split ? a_hi + N * Kp : nullptr;
        unsigned short* b_hi = a_hi + (split ? 2 : 1) * N * Kp;
        unsigned short* b_lo = split ? b_hi + C * Kp : nullptr;
        const unsigned ga = (unsigned)((N * (Kp / 4) + 255) / 256 < 8192 ? (N * (Kp / 4) + 255) / 256 : 8192);
        const unsigned gb = (unsigned)((C * (Kp / 4) + 255) / 256 < 8192 ? (C * (Kp / 4) + 255) / 256 : 8192);
        hipLaunchKernelGGL(split_bf16_kernel, dim3(ga), dim3(256), 0, st, I, ldi, N, D, Kp, a_hi, a_lo);
        hipLaunchKernelGGL(split_bf16_kernel, dim3(gb), dim3(256), 0, st, T, ldt, C, D, Kp, b_hi, b_lo);
        MCD_LAUNCH_CHECK("split_bf16_kernel");
        if (split) {
            const int tiles_m = (int)mcd_cdiv(N, GB_M), tiles_n = (int)mcd_cdiv(C, GB_N);
            const int64_t nbands = mcd_cdiv(tiles_m, GB_RS);
            const int64_t grid64 = mcd_cdiv(nbands, 8) * 8 * GB_RS * tiles_n;
            MCD_REQUIRE(grid64 < (1LL << 31), MCD_E_UNSUPPORTED, "mcd_embed_gemm: too many tiles for one launch");
            const size_t shmem = 8u * (size_t)GB_T_BYTES;   // 2 stages x 4 arrays: 128 KB
            MCD_RESERVE_LDS_ONCE(gemm_nt_bf16_big_kernel, shmem, "mcd_embed_gemm: cannot reserve 128 KB of LDS");
            hipLaunchKernelGGL(gemm_nt_bf16_big_kernel, dim3((unsigned)grid64), dim3(GB_THREADS), shmem, st, a_hi, a_lo, b_hi,
                               b_lo, Kp, N, C, P, ldp, tiles_m, tiles_n);
        } else {
            MCD_RESERVE_LDS_ONCE(gemm_nt_bf16_persist_kernel, GP_NSTAGE * GP_STAGE, "mcd_embed_gemm: cannot reserve 128 KB of LDS");
            const int ptiles_m = (int)mcd_cdiv(N, GP_M), ptiles_n = (int)mcd_cdiv(C, GP_N);
            MCD_REQUIRE((int64_t)GP_M * ldp < (1LL << 31), MCD_E_UNSUPPORTED, "mcd_embed_gemm: ldp too large");
            const unsigned pgrid = (unsigned)((gemm_cu_count() / 8) * 8);   // one workgroup per CU, a multiple of the 8 XCDs
            hipLaunchKernelGGL(gemm_nt_bf16_persist_kernel, dim3(pgrid), dim3(GP_THREADS), GP_NSTAGE * GP_STAGE, st, a_hi, b_hi, Kp,
                               N, C, P, ldp, ptiles_m, ptiles_n);
        }
        MCD_LAUNCH_CHECK("gemm_nt_bf16_big_kernel");
        return MCD_OK;
    }
    const int64_t g64 = mcd_cdiv(mcd_cdiv(N, BM), 8) * 8 * mcd_cdiv(C, BN);   // see xcd_tile()
    MCD_REQUIRE(g64 < (1LL << 31), MCD_E_UNSUPPORTED, "mcd_embed_gemm: too many tiles for one launch");
    const dim3 grid((unsigned)g64);
    const bool aligned = (ldi % 4 == 0) && (ldt % 4 == 0) && (((uintptr_t)I) % 16 == 0) && (((uintptr_t)T) % 16 == 0);
#define MCD_GEMM_LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(256), 0, st, I, ldi, T, ldt, N, C, D, P, ldp)
    if (mode == MCD_GEMM_F32) {
        int64_t kb_first = D, kb_step = 0;
        const bool kblocks = gemm_kblocks(D, kb_first, kb_step);
        // the DMA form: every K-tile whole and inside one K-block, 16-byte aligned rows, 31-bit byte offsets
        const bool dma = aligned && D % BK == 0 && kb_first % BK == 0 && kb_step % BK == 0 && N * ldi < (1LL << 29) &&
                         C * ldt < (1LL << 29);
        // its output through a buffer descriptor: 31-bit byte offsets from the tile's first element
        // (the kernel forms 32-bit offsets for all BM rows of a tile: with N < BM the tile's extent bounds them, or rows past N wrap
        // back inside the descriptor -- pinned by tests/test_gpu_abi_contracts.py::test_embed_gemm_wide_pitch_keeps_the_gap)
        const bool bst = (N > BM ? N : BM) * ldp * 4 < (1LL << 31);
#define MCD_GEMM_LAUNCH_F32(...) \
    hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(256), 0, st, I, ldi, T, ldt, N, C, D, P, ldp, kb_first, kb_step)
#define MCD_GEMM_F32_FORM(KB)                                                 \
    do {                                                                      \
        if (dma && bst) MCD_GEMM_LAUNCH_F32(gemm_nt_f32_dma_kernel<KB, true>); \
        else if (dma) MCD_GEMM_LAUNCH_F32(gemm_nt_f32_dma_kernel<KB, false>);  \
        else if (aligned) MCD_GEMM_LAUNCH_F32(gemm_nt_f32_kernel<true, KB>);   \
        else MCD_GEMM_LAUNCH_F32(gemm_nt_f32_kernel<false, KB>);               \
    } while (0)
        if (kblocks) MCD_GEMM_F32_FORM(true); else MCD_GEMM_F32_FORM(false);
#undef MCD_GEMM_F32_FORM
#undef MCD_GEMM_LAUNCH_F32
    } else if (mode == MCD_GEMM_BF16X3) {
        if (aligned) MCD_GEMM_LAUNCH(gemm_nt_bf16_kernel<true, true>); else MCD_GEMM_LAUNCH(gemm_nt_bf16_kernel<false, true>);
    } else {
        if (aligned) MCD_GEMM_LAUNCH(gemm_nt_bf16_kernel<true, false>); else MCD_GEMM_LAUNCH(gemm_nt_bf16_kernel<false, false>);
    }
#undef MCD_GEMM_LAUNCH
    MCD_LAUNCH_CHECK("gemm_nt kernel");
    return MCD_OK;
}


// ---- K1s host side ---------------------------------------------------------------------------------------------
static int64_t gexp_ldpart(int64_t N) { return (N + 63) / 64 * 64; }
// the kernel walks K in ring rounds of four 32-deep k-steps: the operand image is zero-padded to a multiple of 128
static int64_t gexp_kp(int64_t D) { return (D + 127) / 128 * 128; }

// bytes of the two bf16 operand copies (fragment-major: the row counts rounded up to whole 16-row blocks, the concept blocks
// in pairs), rounded to 256 bytes
static size_t gexp_ops_bytes(int64_t N, int64_t C, int64_t Kp) {
    const size_t pm = (size_t)(mcd_cdiv(N, 16) + 2 * mcd_cdiv(C, 32)) * 16 * (size_t)Kp * sizeof(unsigned short);
    return (pm + 255) / 256 * 256;
}

// ---- measurement hook: HIP events around the GEMM kernel of mcd_embed_gemm_exp (include/mcd_hip.h) ----------------------
static int g_gexp_time = 0;
static hipEvent_t g_gexp_ev[MCD_MAX_DEVICES][2];
static int g_gexp_ev_state[MCD_MAX_DEVICES];     // 0 no events yet, 1 created, 2 a pair has been recorded
static int g_gexp_reps_recorded[MCD_MAX_DEVICES]; // launches ISSUED between the recorded pair

extern "C" int mcd_embed_gemm_exp_time_kernel(int reps) {
    MCD_REQUIRE(reps >= 0 && reps <= 64, MCD_E_ARG, "mcd_embed_gemm_exp_time_kernel: reps = %d outside [0, 64]", reps);
    g_gexp_time = reps;
    return MCD_OK;
}

extern "C" float mcd_embed_gemm_exp_kernel_ms(void) {
    const int dev = mcd_cur_device();
    if (g_gexp_ev_state[dev] != 2) return -1.0f;
    float ms = -1.0f;
    if (hipEventSynchronize(g_gexp_ev[dev][1]) != hipSuccess) return -1.0f;
    if (hipEventElapsedTime(&ms, g_gexp_ev[dev][0], g_gexp_ev[dev][1]) != hipSuccess) return -1.0f;
    return ms / (float)(g_gexp_reps_recorded[dev] > 0 ? g_gexp_reps_recorded[dev] : 1);
}

// which = 0 in front of the kernel, 1 behind it; launches = how many times the kernel was launched in between (the
// quotient must use what was issued, not what was asked for)
static void gexp_time_mark(int dev, int which, hipStream_t st, int launches) {
    if (!g_gexp_time) return;
    if (g_gexp_ev_state[dev] == 0) {
        if (hipEventCreate(&g_gexp_ev[dev][0]) != hipSuccess || hipEventCreate(&g_gexp_ev[dev][1]) != hipSuccess) return;
        g_gexp_ev_state[dev] = 1;
    }
    if (hipEventRecord(g_gexp_ev[dev][which], st) == hipSuccess && which == 1) {
        g_gexp_ev_state[dev] = 2;
        g_gexp_reps_recorded[dev] = launches;
    }
}

extern "C" size_t mcd_embed_gemm_exp_workspace(int64_t N, int64_t C, int64_t D) {
    if (N <= 0 || C <= 0 || D <= 0) return 0;
    const size_t parts = (size_t)(2 * mcd_cdiv(C, 256)) * (size_t)gexp_ldpart(N) * sizeof(float);   // one row per (concept tile, wave row)
    return gexp_ops_bytes(N, C, gexp_kp(D)) + parts;
}

extern "C" int mcd_embed_gemm_exp(const float* I, int64_t ldi, const float* T, int64_t ldt, int64_t N, int64_t C,
                                  int64_t D, float a, int flags, uint16_t* E, int64_t ldE, float* rinv, void* ws,
                                  size_t ws_bytes, mcd_stream_t stream) {
    MCD_REQUIRE(I && T && E && rinv, MCD_E_ARG, "mcd_embed_gemm_exp: NULL pointer");
    MCD_REQUIRE(N >= 0 && C > 0 && D > 0 && ldi >= D && ldt >= D && ldE >= C, MCD_E_ARG,
                "mcd_embed_gemm_exp: bad shape N=%lld C=%lld D=%lld", (long long)N, (long long)C, (long long)D);
    MCD_REQUIRE(((uintptr_t)E) % 16 == 0, MCD_E_ARG, "mcd_embed_gemm_exp: E must be 16-byte aligned");
    // the kernel stores whole 16-byte pieces of 8 concepts at 16-concept steps of a row: rows must start on 32-byte boundaries
    // (the Python binding allocates a pitch that is a multiple of 128, which K4s wants anyway)
    MCD_REQUIRE(ldE % 16 == 0, MCD_E_UNSUPPORTED,
                "mcd_embed_gemm_exp: the leading dimension of E (%lld) must be a multiple of 16 elements", (long long)ldE);
    MCD_REQUIRE(a > 0.f && a <= 64.f, MCD_E_ARG, "mcd_embed_gemm_exp: a = %g outside (0, 64] (exp(-2a) must stay normal)", (double)a);
    MCD_REQUIRE(N < (1LL << 31) && C < (1LL << 31) && ldE * 257 < (1LL << 31), MCD_E_UNSUPPORTED, "mcd_embed_gemm_exp: too large");
    const int64_t Kp = gexp_kp(D);
    MCD_REQUIRE((N + C + 64) * Kp * 2 < (1LL << 31), MCD_E_UNSUPPORTED,
                "mcd_embed_gemm_exp: a bf16 operand of 2 GB or more (32-bit buffer offsets)");
    if (N == 0) return MCD_OK;
    const size_t need = mcd_embed_gemm_exp_workspace(N, C, D);
    MCD_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws) % 16 == 0, MCD_E_WORKSPACE,
                "mcd_embed_gemm_exp: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    unsigned short* a_bf = (unsigned short*)ws;                          // concepts: fragment-major, block rows paired
    unsigned short* b_bf = a_bf + mcd_cdiv(C, 32) * 32 * Kp;             // images: fragment-major
    // a log2(e) is folded into the concept operand; every accumulator starts at -a log2(e): an accumulator IS the exp2 argument
    const float s1 = a * 1.44269504088896340736f;
    float* part = (float*)((char*)ws + gexp_ops_bytes(N, C, Kp));
    const int64_t ldpart = gexp_ldpart(N);
    if ((flags & MCD_GEMM_EXP_NORMALIZE) && Kp <= 64 * 4 * 8) {
        // raw embeddings: normalise and convert in one pass (D <= 2048)
#define MCD_N2B(NQ)                                                                                                     \
    do {                                                                                                                \
        const unsigned blocks_a_ = (unsigned)(mcd_cdiv(C, 32) * 8), blocks_b_ = (unsigned)(mcd_cdiv(N, 16) * 4);        \
        hipLaunchKernelGGL(normalize_to_bf16_kernel<NQ>, dim3(blocks_a_ + blocks_b_), dim3(256), 0, st, T, ldt, C, a_bf, s1, \
                           blocks_a_, I, ldi, N, b_bf, 1.0f, D, Kp, (int64_t)-2);                                       \
    } while (0)
        if (Kp <= 512) MCD_N2B(2);
        else if (Kp <= 1024) MCD_N2B(4);
        else MCD_N2B(8);
#undef MCD_N2B
        MCD_LAUNCH_CHECK("normalize_to_bf16_kernel");
    } else {
        MCD_REQUIRE(!(flags & MCD_GEMM_EXP_NORMALIZE), MCD_E_UNSUPPORTED, "mcd_embed_gemm_exp: fused normalisation needs D <= 2048");
        const unsigned ga = (unsigned)((C * (Kp / 4) + 255) / 256 < 8192 ? (C * (Kp / 4) + 255) / 256 : 8192);
        const unsigned gb = (unsigned)((N * (Kp / 4) + 255) / 256 < 8192 ? (N * (Kp / 4) + 255) / 256 : 8192);
        hipLaunchKernelGGL(split_bf16_kernel, dim3(ga), dim3(256), 0, st, T, ldt, C, D, Kp, a_bf, (unsigned short*)nullptr, (int64_t)-3, s1);
        hipLaunchKernelGGL(split_bf16_kernel, dim3(gb), dim3(256), 0, st, I, ldi, N, D, Kp, b_bf, (unsigned short*)nullptr, (int64_t)-2, 1.0f);
        MCD_LAUNCH_CHECK("split_bf16_kernel");
    }
    const int dev = mcd_cur_device();
    const unsigned pgrid = (unsigned)((gemm_cu_count() / 8) * 8);       // one persistent workgroup per CU, a multiple of the 8 XCDs
    // A set ablation knob is refused instead of silently ignored.  Read on EVERY call, not cached: a caller may set
    // it after earlier calls in the same process (tests/test_gpu_kernels.py::test_product_library_refuses_the_ablation_knob).
    const char* ablate_env = getenv("MCD_GEMM_EXP_ABLATE");
    MCD_REQUIRE(!(ablate_env && atoi(ablate_env) != 0), MCD_E_UNSUPPORTED,
                "mcd_embed_gemm_exp: MCD_GEMM_EXP_ABLATE is set, but the ablation kernels were retired: neither the product library "
                "nor libmcd_hip_dev.so carries them (their measurements: profiles/r05_gexp_v6.txt; the commit that builds them: "
                "scripts/README.md, archive row)");
    // late start of the workgroups with the shorter tile walk (k_gexp_v6.inc), in cycles of one tile period: ~1 200 per k-step
    // + ~7 000 of boundary phase
    const int stagger = (int)(Kp / 32) * 1200 + 7000;
    MCD_RESERVE_LDS_ONCE(gemm_nt_bf16_exp_v6_kernel, G6_LDS, "mcd_embed_gemm_exp: cannot reserve the LDS ring");
    int launches = 0;
    gexp_time_mark(dev, 0, st, 0);
    for (int rep_ = 0; rep_ < (g_gexp_time > 1 ? g_gexp_time : 1); ++rep_) {   // (timing: the same launch, back to back)
        hipLaunchKernelGGL(gemm_nt_bf16_exp_v6_kernel, dim3(pgrid), dim3(256), G6_LDS, st, a_bf, b_bf, Kp, C, N, E, ldE, part,
                           ldpart, s1, (int)mcd_cdiv(C, 256), (int)mcd_cdiv(N, 256), stagger);
        ++launches;
    }
    gexp_time_mark(dev, 1, st, launches);
    MCD_LAUNCH_CHECK("gemm_nt_bf16_exp_v6_kernel");
    hipLaunchKernelGGL(rowsum_finish_kernel, dim3((unsigned)mcd_cdiv(N, 64)), dim3(256), 0, st, part, ldpart,
                       2 * (int)mcd_cdiv(C, 256), N, rinv);
    MCD_LAUNCH_CHECK("rowsum_finish_kernel");
    // "columns C..ldE-1 written as 0": the kernel clears up to the end of its last 256-concept tile; a wider pitch's remainder is
    // cleared here (never at the binding's pitches) -- pinned by tests/test_gpu_abi_contracts.py::test_embed_gemm_exp_pitches
    const int64_t c_span = mcd_cdiv(C, 256) * 256;
    if (ldE > c_span) {
        const int64_t pieces = N * ((ldE - c_span) / 8);
        hipLaunchKernelGGL(gexp_zero_pad_kernel, dim3((unsigned)(mcd_cdiv(pieces, 256) < 4096 ? mcd_cdiv(pieces, 256) : 4096)), dim3(256), 0,
                           st, E, ldE, N, c_span);
        MCD_LAUNCH_CHECK("gexp_zero_pad_kernel");
    }
    return MCD_OK;
}
