// k_clip.hip -- K25: QuickGELU of the OpenAI-CLIP towers (include/mcd_clip.h), one launch behind every c_fc.
//   replaces concept_vit/clip/model.py:162-164  x * torch.sigmoid(1.702 * x)  -- mul, sigmoid, mul: three passes
// A streaming kernel: 4 bytes read and 4 written per element, a dozen VALU instructions between them.  Each thread moves
// QG_U float4s, a workgroup's loads QG_THREADS * 16 bytes apart (whole cache lines per wave instruction), all QG_U loads
// in flight before the first use.  The n % 4 tail is done by the first lanes of workgroup 0, element by element.
// (K9A, the other entry of that header, shares K9's workgroup body and lives in k_attn.hip.)
#include "mcd_common.h"
#include "../../include/mcd_clip.h"

namespace {

constexpr int QG_THREADS = 256;
constexpr int QG_U = 4;            // float4s per thread

// x * (1 / (1 + e^(-1.702 x))), e^t = 2^(t log2 e) on v_exp_f32.  t = +-inf (|x| near the top of the range) is fine:
// 2^inf = inf -> 1 / inf = 0 -> x * 0 = -0 (x is negative there), 2^-inf = 0 -> x * 1.
__device__ __forceinline__ float quick_gelu(float x) {
    const float t = -(1.702f * x);
    const float e = __builtin_amdgcn_exp2f(t * 1.44269504088896340736f);
    return x * (1.0f / (1.0f + e));
}

__global__ __launch_bounds__(QG_THREADS) void quick_gelu_kernel(const float* x, int64_t n4, int tail, float* out) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* o4 = reinterpret_cast<float4*>(out);
    const int64_t i0 = (int64_t)blockIdx.x * (QG_THREADS * QG_U) + threadIdx.x;
    float4 v[QG_U];
#pragma unroll
    for (int u = 0; u < QG_U; ++u) {
        const int64_t i = i0 + u * QG_THREADS;
        if (i < n4) v[u] = x4[i];
    }
#pragma unroll
    for (int u = 0; u < QG_U; ++u) {
        const int64_t i = i0 + u * QG_THREADS;
        if (i < n4) o4[i] = make_float4(quick_gelu(v[u].x), quick_gelu(v[u].y), quick_gelu(v[u].z), quick_gelu(v[u].w));
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
        const int64_t i = 4 * n4 + threadIdx.x;
        out[i] = quick_gelu(x[i]);
    }
}

}  // namespace

extern "C" int mcd_quick_gelu(const float* x, int64_t n, float* out, mcd_stream_t stream) {
    MCD_REQUIRE(n >= 0, MCD_E_ARG, "mcd_quick_gelu: n=%lld", (long long)n);
    if (n == 0) return MCD_OK;
    MCD_REQUIRE(x && out, MCD_E_ARG, "mcd_quick_gelu: NULL pointer");
    MCD_REQUIRE(((uintptr_t)x) % 16 == 0 && ((uintptr_t)out) % 16 == 0, MCD_E_ARG,
                "mcd_quick_gelu: x and out must be 16-byte aligned");
    const int64_t n4 = n / 4;
    const int64_t blocks = std::max<int64_t>(1, mcd_cdiv(n4, QG_THREADS * QG_U));
    MCD_REQUIRE(blocks <= INT32_MAX, MCD_E_UNSUPPORTED, "mcd_quick_gelu: n=%lld is too large a grid", (long long)n);
    hipLaunchKernelGGL(quick_gelu_kernel, dim3((unsigned)blocks), dim3(QG_THREADS), 0, (hipStream_t)stream, x, n4, (int)(n % 4),
                       out);
    MCD_LAUNCH_CHECK("quick_gelu_kernel");
    return MCD_OK;
}
