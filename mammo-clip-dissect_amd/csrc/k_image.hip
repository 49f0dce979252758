// k_image.hip -- K22: probe-image preprocessing, packed RGB uint8 [n, H, W, 3] -> fp32 [n, 3, OH, OW] in one launch.
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
