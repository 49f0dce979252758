// k_image.hip -- K22 and K23: the probe sets' image transforms on the device (K23: per-image min-max, below K22).
// K22: probe-image preprocessing, packed RGB uint8 [n, H, W, 3] -> fp32 [n, 3, OH, OW] in one launch.
//   replaces Resize -> CenterCrop -> ToTensor -> Normalize on PIL images:
//     get_resnet_imagenet_preprocess   concept_vit/data_utils.py:95-100
//     CLIP's _transform                concept_vit/clip/clip.py:79-86
//     the EMBED sets' Resize + ToTensor  concept_vit/data_utils.py:176-179
//     imagenet_subsets' ToTensor + Normalize  concept_vit/data_utils.py:111
// The arithmetic is PIL's 8-bit two-pass resampler (Resample.c, PRECISION_BITS = 22) in int32, then one table look-up
// per byte for ToTensor / Normalize: no floating-point operation runs on the device.
//
// A workgroup owns a TH x 32 tile of the CROPPED output of one image.  The table rows of its 32 columns and TH rows and
// the look-up table are copied into LDS first (every tap would otherwise be a global load of its coefficient), then:
//   1. the source rows its vertical taps need are resampled horizontally, for the tile's 32 columns only, into LDS as
//      bytes, one plane per channel ([row][channel][32 columns]);
//   2. the vertical pass reads those bytes (lanes on consecutive bytes of one plane);
//   3. each 32-lane half wave stores 128 consecutive bytes of one channel plane of dst.
// Rows and columns outside the crop window are never computed.  An image is addressed from a 64-bit base with 32-bit
// offsets inside it.
#include "mcd_common.h"

namespace {

constexpr int kTileW = 32;                 // output columns of a tile
constexpr int kMaxTileH = 16;              // output rows of a tile, halved until the LDS stage fits
constexpr int kStageBytes = 32 * 1024;     // LDS stage: rows x 3 x kTileW bytes (+ at most 25 KB of table rows + 3 KB)
constexpr int kMaxTaps = 128;              // coefficients per table row (bicubic up to ratio 31, bilinear up to 63)
constexpr int kPrecisionBits = 22;

// {first, count} of a table row, brought inside [0, size) and [0, k]: a table that names pixels outside the image gives
// a wrong picture, never an access outside the buffers
__device__ __forceinline__ void tap_window(const int32_t* row, int k, int size, int& first, int& count) {
    first = row[0];
    count = row[1];
    count = count < 0 ? 0 : (count > k ? k : count);
    count = count > size ? size : count;
    first = first < 0 ? 0 : first;
    first = first + count > size ? size - count : first;
}

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrecisionBits;      // arithmetic shift
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void image_preprocess_kernel(
        const uint8_t* __restrict__ src, int H, int W, const int32_t* __restrict__ xtab, int kx,
        const int32_t* __restrict__ ytab, int ky, int top, int left, int OH, int OW, int TH, int tiles_x, int tiles,
        int stage_rows, const float* __restrict__ lut, float* __restrict__ dst, int64_t dst_img) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];      // [stage_rows][3][kTileW], then the table rows
    __shared__ float slut[3 * 256];
    const int tid = threadIdx.x;
    const int64_t img = (int64_t)blockIdx.x / tiles;
    const int tile = (int)((int64_t)blockIdx.x - img * tiles);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * TH;
    const int tw = OW - x0 < kTileW ? OW - x0 : kTileW, th = OH - y0 < TH ? OH - y0 : TH;
    for (int i = tid; i < 3 * 256; i += 256) slut[i] = lut[i];
    // this tile's rows of the two tables, at an odd row stride (lanes of a wave read 32 different rows of xt)
    const int sx = (2 + kx) | 1, sy = (2 + ky) | 1;
    int32_t* xt = reinterpret_cast<int32_t*>(stage + (stage_rows * 3 * kTileW + 15) / 16 * 16);
    int32_t* yt = xt + (xtab ? kTileW * sx : 0);
    if (xtab)
        for (int i = tid; i < tw * (2 + kx); i += 256)
            xt[(i / (2 + kx)) * sx + i % (2 + kx)] = xtab[(int64_t)(left + x0) * (2 + kx) + i];
    if (ytab)
        for (int i = tid; i < th * (2 + ky); i += 256)
            yt[(i / (2 + ky)) * sy + i % (2 + ky)] = ytab[(int64_t)(top + y0) * (2 + ky) + i];
    __syncthreads();

    // the source rows this tile's vertical taps read: [row0, row0 + rows)
    int row0, row1;
    if (ytab) {
        row0 = H;
        row1 = 0;
        for (int yy = 0; yy < th; ++yy) {
            int first, count;
            tap_window(yt + yy * sy, ky, H, first, count);
            row0 = first < row0 ? first : row0;
            row1 = first + count > row1 ? first + count : row1;
        }
        row1 = row1 < row0 ? row0 : row1;
    } else {
        row0 = top + y0;
        row1 = row0 + th;
    }
    const int rows = row1 - row0 < stage_rows ? row1 - row0 : stage_rows;
    const uint8_t* __restrict__ s = src + img * ((int64_t)H * W * 3);

    // 1. horizontal pass into LDS
    for (int idx = tid; idx < rows * 3 * kTileW; idx += 256) {
        const int xx = idx % kTileW, c = (idx / kTileW) % 3, r = idx / (3 * kTileW);
        if (xx >= tw) continue;
        const uint8_t* __restrict__ p = s + ((row0 + r) * W) * 3 + c;
        const int o = left + x0 + xx;
        int v;
        if (xtab) {
            const int32_t* t = xt + xx * sx;
            int first, count;
            tap_window(t, kx, W, first, count);
            int acc = 1 << (kPrecisionBits - 1);
            p += first * 3;
            for (int j = 0; j < count; ++j) acc += (int)p[j * 3] * t[2 + j];
            v = clip8(acc);
        } else {
            v = p[o * 3];
        }
        stage[idx] = (uint8_t)v;
    }
    __syncthreads();

    // 2. vertical pass from LDS, 3. the look-up and the store
    float* __restrict__ d = dst + img * dst_img;
    for (int idx = tid; idx < th * 3 * kTileW; idx += 256) {
        const int xx = idx % kTileW, c = (idx / kTileW) % 3, yy = idx / (3 * kTileW);
        if (xx >= tw) continue;
        int v;
        if (ytab) {
            const int32_t* t = yt + yy * sy;
            int first, count;
            tap_window(t, ky, H, first, count);
            first -= row0;                                   // >= 0: row0 is the minimum over the tile
            count = first + count > rows ? rows - first : count;
            int acc = 1 << (kPrecisionBits - 1);
            const uint8_t* q = stage + (first * 3 + c) * kTileW + xx;
            for (int j = 0; j < count; ++j) acc += (int)q[j * 3 * kTileW] * t[2 + j];
            v = clip8(acc);
        } else {
            v = yy < rows ? stage[(yy * 3 + c) * kTileW + xx] : 0;
        }
        d[((int64_t)c * OH + (y0 + yy)) * OW + (x0 + xx)] = slut[c * 256 + v];
    }
}

inline bool overlaps(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace

extern "C" int mcd_image_preprocess(const uint8_t* src, int64_t n, int64_t H, int64_t W, const int32_t* xtab, int64_t kx,
                                    int64_t RW, const int32_t* ytab, int64_t ky, int64_t RH, int64_t top, int64_t left,
                                    int64_t OH, int64_t OW, const float* lut, float* dst, int64_t dst_img,
                                    mcd_stream_t stream) {
    MCD_REQUIRE(src && lut && dst, MCD_E_ARG, "mcd_image_preprocess: NULL pointer");
    MCD_REQUIRE(n >= 0 && H >= 1 && W >= 1 && RH >= 1 && RW >= 1 && OH >= 1 && OW >= 1 && top >= 0 && left >= 0, MCD_E_ARG,
                "mcd_image_preprocess: bad shape n=%lld H=%lld W=%lld RH=%lld RW=%lld OH=%lld OW=%lld top=%lld left=%lld",
                (long long)n, (long long)H, (long long)W, (long long)RH, (long long)RW, (long long)OH, (long long)OW,
                (long long)top, (long long)left);
    MCD_REQUIRE(top + OH <= RH && left + OW <= RW, MCD_E_ARG,
                "mcd_image_preprocess: the crop window leaves the %lld x %lld resized image", (long long)RH, (long long)RW);
    MCD_REQUIRE((xtab || RW == W) && (ytab || RH == H), MCD_E_ARG,
                "mcd_image_preprocess: a NULL table means that axis keeps its size");
    MCD_REQUIRE((!xtab || kx >= 1) && (!ytab || ky >= 1), MCD_E_ARG, "mcd_image_preprocess: a table needs k >= 1");
    MCD_REQUIRE((uintptr_t)dst % 4 == 0 && (uintptr_t)lut % 4 == 0 && (uintptr_t)xtab % 4 == 0 && (uintptr_t)ytab % 4 == 0,
                MCD_E_ARG, "mcd_image_preprocess: lut, dst and the tables must be 4-byte aligned");
    const int64_t lim = (int64_t)1 << 31;
    MCD_REQUIRE((!xtab || kx <= kMaxTaps) && (!ytab || ky <= kMaxTaps), MCD_E_UNSUPPORTED,
                "mcd_image_preprocess: %lld x %lld taps per output pixel, the kernel takes %d per axis", (long long)kx,
                (long long)ky, kMaxTaps);
    if (!xtab) kx = 0;
    if (!ytab) ky = 0;
    MCD_REQUIRE(n < lim && RH < lim / (2 + kMaxTaps) && RW < lim / (2 + kMaxTaps) && H <= (lim - 1) / 3 / W &&
                    OH <= (lim - 1) / 12 / OW,
                MCD_E_UNSUPPORTED, "mcd_image_preprocess: one image (H*W*3 or 3*OH*OW*4 bytes) reaches 2^31");
    MCD_REQUIRE(dst_img >= 3 * OH * OW && dst_img < ((int64_t)1 << 40), MCD_E_ARG,
                "mcd_image_preprocess: dst_img %lld is not in [3*OH*OW, 2^40)", (long long)dst_img);
    if (n == 0) return MCD_OK;
    const int64_t out_bytes = ((n - 1) * dst_img + 3 * OH * OW) * 4;
    MCD_REQUIRE(!overlaps(src, n * H * W * 3, dst, out_bytes) && !overlaps(lut, 3 * 256 * 4, dst, out_bytes) &&
                    !(xtab && overlaps(xtab, RW * (2 + kx) * 4, dst, out_bytes)) &&
                    !(ytab && overlaps(ytab, RH * (2 + ky) * 4, dst, out_bytes)),
                MCD_E_ARG, "mcd_image_preprocess: src, lut or a table overlaps dst");

    // The tile height: the largest of 16, 8, .. 1 whose source rows fit the stage.  The rows first .. first + count of TH
    // consecutive outputs span at most (TH - 1) H / RH + 1 + ky source rows (first = int(center - support + 0.5) with
    // center = (o + 0.5) H / RH); one more row of slack for the table's double arithmetic.
    const int cap = kStageBytes / (3 * kTileW);
    int TH = kMaxTileH;
    int64_t need;
    for (;; TH /= 2) {
        need = ytab ? ((int64_t)(TH - 1) * H) / RH + (TH > 1 ? 2 : 0) + ky : TH;
        if (need <= cap || TH == 1) break;
    }
    if (need > cap) need = cap;      // TH == 1 and ky <= kMaxTaps: never taken
    const int64_t tiles_x = mcd_cdiv(OW, kTileW), tiles = tiles_x * mcd_cdiv(OH, TH);
    MCD_REQUIRE(n * tiles < lim, MCD_E_UNSUPPORTED, "mcd_image_preprocess: %lld tiles in one call", (long long)(n * tiles));
    const size_t lds = (size_t)((need * 3 * kTileW + 15) / 16 * 16) +
                       4 * (size_t)((xtab ? kTileW * ((2 + kx) | 1) : 0) + (ytab ? TH * ((2 + ky) | 1) : 0));
    hipLaunchKernelGGL(image_preprocess_kernel, dim3((unsigned)(n * tiles)), dim3(256), lds, (hipStream_t)stream, src,
                       (int)H, (int)W, xtab, (int)kx, ytab, (int)ky, (int)top, (int)left, (int)OH, (int)OW, TH, (int)tiles_x,
                       (int)tiles, (int)need, lut, dst, dst_img);
    MCD_LAUNCH_CHECK("image_preprocess_kernel");
    return MCD_OK;
}

// ---- K23: per-image min-max normalisation of the mammogram probe sets ---------------------------------------------------
//   replaces img.astype('float32'); img -= img.min(); img /= img.max(); (img - mean) / std
//                                            data/dataset/image_classification_zs.py:81-84  (vindr, vindr_alt)
//            the permute to [B, 3, H, W]     concept_vit/utils.py:176
//            np.array(Image.open(path), dtype=np.float32) repeated to three channels + ToTensor
//                                            data/dataset/CSAW_dataset.py:49-55             (csaw, csaw_all_splits)
// Two launches, no atomics, no memset:
//   (a) minmax_partial_kernel, grid (chunks, n): a workgroup reduces one contiguous chunk of an image's bytes to an int32
//       (min, max) pair.  16-byte loads on the aligned body, bytes on the chunk's head and tail; nothing outside the image
//       is read.
//   (b) minmax_apply_kernel, grid (tiles, n): every workgroup folds its image's <= 256 pairs, thread v computes the table
//       entry of byte v with the reference's four fp32 operations (each rounded once: the file is compiled with
//       -fno-fast-math -ffp-contract=off, and the divisions stay divisions), then the tile is streamed: packed bytes in,
//       one LDS look-up per byte, fp32 planes out.  Wide path: a lane reads 4 consecutive pixels (one dword, three for
//       RGB) and stores one float4 per plane, so a wave's store instruction covers 1 KB of one plane without a gap.
// min and max are integers, so their fold is order-independent: an image's bits depend neither on the batch nor on its
// place in it.
namespace {

constexpr int kMinMaxChunk = MCD_IMAGE_MINMAX_CHUNK;   // bytes of one partial reduction (doubled while an image has more than 256)
constexpr int kMinMaxMaxChunks = 256;
constexpr int kApplyTile = 8192;                       // pixels of one apply workgroup: 8 steps of 256 lanes x 4 pixels

typedef unsigned short mcd_u16x2 __attribute__((ext_vector_type(2)));

// chunk bytes for an image of `bytes` bytes: kMinMaxChunk, doubled until at most 256 chunks cover the image
inline int64_t minmax_chunk_bytes(int64_t bytes) {
    int64_t c = kMinMaxChunk;
    while (mcd_cdiv(bytes, c) > kMinMaxMaxChunks) c *= 2;
    return c;
}

__device__ __forceinline__ void fold_byte(int v, int& mn, int& mx) {
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
}

// min / max over the four bytes of w, two bytes at a time as packed 16-bit lanes
__device__ __forceinline__ void fold_dword(uint32_t w, mcd_u16x2& mn, mcd_u16x2& mx) {
    const uint32_t e = w & 0x00ff00ffu, o = (w >> 8) & 0x00ff00ffu;
    const mcd_u16x2 ev = __builtin_bit_cast(mcd_u16x2, e), ov = __builtin_bit_cast(mcd_u16x2, o);
    mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(ev, ov));
    mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(ev, ov));
}

// (min, max) over the workgroup's 256 threads; the result is valid in every thread
__device__ __forceinline__ void block_minmax(int& mn, int& mx, int* smem /* [8] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        smem[wave] = mn;
        smem[4 + wave] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        mn = smem[w] < mn ? smem[w] : mn;
        mx = smem[4 + w] > mx ? smem[4 + w] : mx;
    }
}

__global__ __launch_bounds__(256) void minmax_partial_kernel(const uint8_t* __restrict__ src, int64_t img_bytes, int chunk,
                                                             int chunks, int32_t* __restrict__ ws) {
    __shared__ int smem[8];
    const int tid = threadIdx.x;
    const uint8_t* __restrict__ s = src + (int64_t)blockIdx.y * img_bytes;
    const int64_t c0 = (int64_t)blockIdx.x * chunk;
    const int len = (int)(img_bytes - c0 < chunk ? img_bytes - c0 : chunk);       // >= 1: chunks = cdiv(img_bytes, chunk)
    const uint8_t* __restrict__ p = s + c0;
    // head: the bytes in front of the first 16-byte boundary; body: whole 16-byte pieces; tail: what is left
    int head = (int)((16 - ((uintptr_t)p & 15)) & 15);
    head = head > len ? len : head;
    const int body = (len - head) / 16;
    int mn = 255, mx = 0;
    if (tid < head) fold_byte(p[tid], mn, mx);
    const uint4* __restrict__ q = reinterpret_cast<const uint4*>(p + head);
    mcd_u16x2 vmn = {255, 255}, vmx = {0, 0};
    for (int i = tid; i < body; i += 256) {
        const uint4 w = q[i];
        fold_dword(w.x, vmn, vmx);
        fold_dword(w.y, vmn, vmx);
        fold_dword(w.z, vmn, vmx);
        fold_dword(w.w, vmn, vmx);
    }
    const int bmn = vmn.x < vmn.y ? vmn.x : vmn.y, bmx = vmx.x > vmx.y ? vmx.x : vmx.y;     // {255, 0} without a body
    mn = bmn < mn ? bmn : mn;
    mx = bmx > mx ? bmx : mx;
    const int t0 = head + body * 16;
    if (t0 + tid < len) fold_byte(p[t0 + tid], mn, mx);                             // the tail is under 16 bytes
    block_minmax(mn, mx, smem);
    if (tid == 0) {
        int32_t* __restrict__ o = ws + 2 * ((int64_t)blockIdx.y * chunks + blockIdx.x);
        o[0] = mn;
        o[1] = mx;
    }
}

// CH: 1 (grey [n, H, W]) or 3 (packed RGB [n, H, W, 3]).  WIDE: HW % 16 == 0 and src, dst, dst_img aligned for dword loads
// of 4 pixels and float4 stores.  chunks == 0: MCD_IMG_RAW, the table is f32(v) and ws is not read.
template <int CH, bool WIDE>
__global__ __launch_bounds__(256) void minmax_apply_kernel(const uint8_t* __restrict__ src, int HW, const int32_t* __restrict__ ws,
                                                           int chunks, float mean, float std, float* __restrict__ dst,
                                                           int64_t dst_img) {
    __shared__ float slut[256];
    __shared__ int smem[8];
    const int tid = threadIdx.x;
    const int64_t img = blockIdx.y;
    if (chunks > 0) {
        int mn = 255, mx = 0;
        if (tid < chunks) {
            const int32_t* __restrict__ w = ws + 2 * (img * chunks + tid);
            mn = w[0];
            mx = w[1];
        }
        block_minmax(mn, mx, smem);
        float t = (float)tid - (float)mn;      // img -= img.min()
        t = t / (float)(mx - mn);              // img /= img.max()    (0 / 0 = NaN for a constant image)
        t = t - mean;
        t = t / std;
        slut[tid] = t;
    } else {
        slut[tid] = (float)tid;
    }
    __syncthreads();

    const uint8_t* __restrict__ s = src + img * ((int64_t)HW * CH);
    float* __restrict__ d = dst + img * dst_img;
    const int p0 = blockIdx.x * kApplyTile;
    if (WIDE) {
        constexpr int kSteps = kApplyTile / 1024;
        uint32_t w[kSteps][CH];
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            const int p = p0 + k * 1024 + tid * 4;
            if (p < HW) {                      // HW % 4 == 0: the four pixels are inside together
                const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(s + (int64_t)p * CH);
#pragma unroll
                for (int c = 0; c < CH; ++c) w[k][c] = q[c];
            }
        }
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            const int p = p0 + k * 1024 + tid * 4;
            if (p < HW) {
                if (CH == 1) {
                    const uint32_t v = w[k][0];
                    const float4 o = make_float4(slut[v & 255], slut[(v >> 8) & 255], slut[(v >> 16) & 255], slut[v >> 24]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(d + (int64_t)c * HW + p) = o;
                } else {
                    // 12 bytes r0 g0 b0 r1 g1 b1 r2 g2 b2 r3 g3 b3 in three dwords
                    float f[12];
#pragma unroll
                    for (int j = 0; j < 12; ++j) f[j] = slut[(w[k][(j / 4) % CH] >> (8 * (j % 4))) & 255];
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        *reinterpret_cast<float4*>(d + (int64_t)c * HW + p) = make_float4(f[c], f[3 + c], f[6 + c], f[9 + c]);
                }
            }
        }
    } else {
        const int p1 = HW - p0 < kApplyTile ? HW : p0 + kApplyTile;
        for (int p = p0 + tid; p < p1; p += 256) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[(int64_t)c * HW + p] = slut[s[(int64_t)p * CH + (CH == 1 ? 0 : c)]];
        }
    }
}

}  // namespace

extern "C" size_t mcd_image_minmax_workspace(int64_t n, int64_t H, int64_t W, int64_t channels) {
    if (n < 1 || H < 1 || W < 1 || (channels != 1 && channels != 3)) return 0;
    if (H > (((int64_t)1 << 31) - 1) / channels / W) return 0;
    const int64_t bytes = H * W * channels;
    return (size_t)(n * mcd_cdiv(bytes, minmax_chunk_bytes(bytes)) * 2 * (int64_t)sizeof(int32_t));
}

extern "C" int mcd_image_minmax_normalize(const uint8_t* src, int64_t n, int64_t H, int64_t W, int64_t channels, int mode,
                                          float mean, float std, float* dst, int64_t dst_img, void* ws, size_t ws_bytes,
                                          mcd_stream_t stream) {
    MCD_REQUIRE(src && dst, MCD_E_ARG, "mcd_image_minmax_normalize: NULL pointer");
    MCD_REQUIRE(channels == 1 || channels == 3, MCD_E_ARG, "mcd_image_minmax_normalize: channels %lld is not 1 or 3",
                (long long)channels);
    MCD_REQUIRE(mode == MCD_IMG_MINMAX || mode == MCD_IMG_RAW, MCD_E_ARG, "mcd_image_minmax_normalize: unknown mode %d", mode);
    MCD_REQUIRE(n >= 0 && H >= 1 && W >= 1, MCD_E_ARG, "mcd_image_minmax_normalize: bad shape n=%lld H=%lld W=%lld",
                (long long)n, (long long)H, (long long)W);
    MCD_REQUIRE((uintptr_t)dst % 4 == 0 && (uintptr_t)ws % 8 == 0, MCD_E_ARG,
                "mcd_image_minmax_normalize: dst must be 4-byte and ws 8-byte aligned");
    const bool minmax = mode == MCD_IMG_MINMAX;
    MCD_REQUIRE(!minmax || ws, MCD_E_ARG, "mcd_image_minmax_normalize: MCD_IMG_MINMAX needs a workspace");
    const int64_t lim = (int64_t)1 << 31;
    MCD_REQUIRE(n <= 65535, MCD_E_UNSUPPORTED, "mcd_image_minmax_normalize: n %lld > 65535 images in one call", (long long)n);
    MCD_REQUIRE(H <= (lim - 1) / channels / W && H <= (lim - 1) / 12 / W, MCD_E_UNSUPPORTED,
                "mcd_image_minmax_normalize: one image (H*W*channels or 3*H*W*4 bytes) reaches 2^31");
    const int64_t HW = H * W, img_bytes = HW * channels;
    MCD_REQUIRE(dst_img >= 3 * HW && dst_img < ((int64_t)1 << 40), MCD_E_ARG,
                "mcd_image_minmax_normalize: dst_img %lld is not in [3*H*W, 2^40)", (long long)dst_img);
    if (n == 0) return MCD_OK;
    const int64_t out_bytes = ((n - 1) * dst_img + 3 * HW) * 4;
    const int64_t chunk = minmax_chunk_bytes(img_bytes), chunks = mcd_cdiv(img_bytes, chunk);
    const int64_t need = n * chunks * 2 * (int64_t)sizeof(int32_t);
    MCD_REQUIRE(!overlaps(src, n * img_bytes, dst, out_bytes), MCD_E_ARG, "mcd_image_minmax_normalize: src overlaps dst");
    if (minmax) {
        MCD_REQUIRE(ws_bytes >= (size_t)need, MCD_E_WORKSPACE,
                    "mcd_image_minmax_normalize: workspace %zu < %lld bytes", ws_bytes, (long long)need);
        MCD_REQUIRE(!overlaps(ws, need, dst, out_bytes), MCD_E_ARG, "mcd_image_minmax_normalize: ws overlaps dst");
    }

    hipStream_t st = (hipStream_t)stream;
    int32_t* pairs = static_cast<int32_t*>(ws);
    if (minmax) {
        hipLaunchKernelGGL(minmax_partial_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(256), 0, st, src, img_bytes,
                           (int)chunk, (int)chunks, pairs);
        MCD_LAUNCH_CHECK("minmax_partial_kernel");
    }
    const bool wide = HW % 16 == 0 && dst_img % 4 == 0 && (uintptr_t)dst % 16 == 0 && (uintptr_t)src % 4 == 0;
    const dim3 grid((unsigned)mcd_cdiv(HW, kApplyTile), (unsigned)n);
    const int fold = minmax ? (int)chunks : 0;
#define MCD_APPLY(CH, WIDE)                                                                                              \
    hipLaunchKernelGGL((minmax_apply_kernel<CH, WIDE>), grid, dim3(256), 0, st, src, (int)HW, pairs, fold, mean, std, dst, \
                       dst_img)
    if (channels == 1) {
        if (wide) MCD_APPLY(1, true); else MCD_APPLY(1, false);
    } else {
        if (wide) MCD_APPLY(3, true); else MCD_APPLY(3, false);
    }
#undef MCD_APPLY
    MCD_LAUNCH_CHECK("minmax_apply_kernel");
    return MCD_OK;
}
