// mcd_blaslt.cpp -- libmcd_blaslt.so: the encoder's "linear + bias + residual" as ONE hipBLASLt call.
//   out[M,N] = res[M,N] + h[M,K] . W[N,K]^T + bias[N]          (fp32, fp32 MFMA, row-major operands)
// replaces, inside the ViT blocks of the image tower (the forwards that concept_vit/utils.py:117-148 drives),
//   x = x + proj(attention)        and        x = x + fc2(gelu(fc1(...)))
// i.e. nn.Linear (a hipBLASLt GEMM with the bias epilogue) followed by ATen's elementwise add, which re-reads and
// re-writes the whole residual stream (454 MB per add at 250 images: 69 us, twice per block = 2.4 % of the headline
// step).  hipBLASLt's own epilogue takes the bias AND beta * C in the same kernel: the residual is read once inside
// the GEMM (hidden under the MFMAs) and the sum is written once.
// mcd_linear_residual_relu is the same call with the library's ReLU epilogue on the whole sum: a ResNet Bottleneck's
// conv3 + folded bn3 + skip add + relu on channels-last rows.
// A plain library GEMM (no hand-written kernel here); kept in its own shared object so that libmcd_hip.so carries no
// dependency on hipBLASLt -- the Python side loads this one lazily and keeps PyTorch's two-kernel path if it is absent.
//
// Algorithm choice: the first call for a shape asks the heuristic for up to 32 candidates, times each (3 runs, into a
// scratch D) on the caller's stream and keeps the fastest for the life of the process -- the same thing PyTorch's
// TunableOp does for the other GEMMs of the tower.  (So the first call per shape synchronises; not capturable.)
// A timed pick can differ from process to process, and different algorithms sum in different orders, so the SAME image
// could encode to different bits on different ranks.  Two ways to make the choice reproducible:
//   * MCD_BLASLT_PICK=heuristic -- take the first usable heuristic candidate, time nothing;
//   * mcd_linear_residual_get_picks / _set_pick -- read the picks one process made (index into the heuristic list, which
//     is a deterministic function of the problem and the library) and force them in the others: the multi-rank host code
//     broadcasts rank 0's picks after its warm-up pass (pipeline.sync_encoder_gemm_picks).
// All per-process state is keyed by the HIP device (handle, plans).
#include <hip/hip_runtime.h>
#include <hipblaslt/hipblaslt.h>

#include <map>
#include <mutex>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <tuple>
#include <vector>

#include "../../include/mcd_blaslt.h"
#include "../../include/mcd_hip.h"   // the MCD_E_* status codes

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

struct Plan {
    hipblasLtMatmulDesc_t desc = nullptr;
    hipblasLtMatrixLayout_t a = nullptr, b = nullptr, c = nullptr, d = nullptr;
    hipblasLtMatmulAlgo_t algo;
    size_t ws = 0;
    float ms = 0.f;
    int tried = 0;
    int pick = 0;        // index of the kept algorithm in the heuristic's candidate list
};

constexpr int kMaxDev = 64;
using Key = std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int, int, int>;   // ..., device
using ShapeKey = std::tuple<int64_t, int64_t, int64_t, int>;                                            // M, N, K, has_res
// The has_res field of both keys (and of the get_picks / set_pick records): bit 0 = a residual operand, bit 1 = the ReLU
// epilogue of mcd_linear_residual_relu.  The two entries never share a plan or a pick.
std::mutex g_mu;
hipblasLtHandle_t g_handles[kMaxDev] = {};
std::map<Key, Plan> g_plans;
std::map<ShapeKey, int> g_forced;

int cur_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDev) d = 0;
    return d;
}

void destroy_plan(Plan& p) {
    if (p.a) hipblasLtMatrixLayoutDestroy(p.a);
    if (p.b) hipblasLtMatrixLayoutDestroy(p.b);
    if (p.c) hipblasLtMatrixLayoutDestroy(p.c);
    if (p.d) hipblasLtMatrixLayoutDestroy(p.d);
    if (p.desc) hipblasLtMatmulDescDestroy(p.desc);
}

#define LT(call)                                                                                          \
    do {                                                                                                  \
        hipblasStatus_t s__ = (call);                                                                     \
        if (s__ != HIPBLAS_STATUS_SUCCESS) return fail(MCD_E_LAUNCH, "mcd_linear_residual: %s -> %d", #call, (int)s__); \
    } while (0)

}  // namespace

extern "C" const char* mcd_blaslt_last_error(void) { return g_err; }

extern "C" size_t mcd_linear_residual_workspace(void) { return (size_t)32 << 20; }

// Time (ms) of the algorithm chosen for the last-planned shape with these sizes, and how many candidates were timed
// (0 / 0 when the shape has not been seen): lets the tests and the bench report what was picked.
extern "C" int mcd_linear_residual_plan_info(int64_t M, int64_t N, int64_t K, float* ms, int* tried) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_plans)
        if (std::get<0>(kv.first) == M && std::get<1>(kv.first) == N && std::get<2>(kv.first) == K) {
            if (ms) *ms = kv.second.ms;
            if (tried) *tried = kv.second.tried;
            return MCD_OK;
        }
    if (ms) *ms = 0.f;
    if (tried) *tried = 0;
    return MCD_OK;
}

// The picks this process holds: up to `cap` records of 5 int64 (M, N, K, has_res, pick) into `out`; returns how many
// there are (which may exceed cap).
extern "C" int mcd_linear_residual_get_picks(int64_t* out, int cap) {
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    for (auto& kv : g_plans) {
        if (out && n < cap) {
            out[5 * n + 0] = std::get<0>(kv.first);
            out[5 * n + 1] = std::get<1>(kv.first);
            out[5 * n + 2] = std::get<2>(kv.first);
            out[5 * n + 3] = std::get<7>(kv.first);
            out[5 * n + 4] = kv.second.pick;
        }
        ++n;
    }
    return n;
}

// Force the algorithm for a shape (pick = index into the heuristic list; < 0 removes the forcing).  A plan this process
// already made for the shape is dropped and rebuilt with the forced pick on the next call.
extern "C" int mcd_linear_residual_set_pick(int64_t M, int64_t N, int64_t K, int has_res, int pick) {
    std::lock_guard<std::mutex> lk(g_mu);
    const int flags = has_res & 3;
    const ShapeKey sk{M, N, K, flags};
    if (pick < 0) g_forced.erase(sk);
    else g_forced[sk] = pick;
    for (auto it = g_plans.begin(); it != g_plans.end();) {
        if (std::get<0>(it->first) == M && std::get<1>(it->first) == N && std::get<2>(it->first) == K &&
            std::get<7>(it->first) == flags) {
            destroy_plan(it->second);
            it = g_plans.erase(it);
        } else {
            ++it;
        }
    }
    return MCD_OK;
}

namespace {

int linear_residual(const float* h, int64_t ldh, const float* W, int64_t ldw, const float* bias, const float* res,
                    int64_t ldr, float* out, int64_t ldo, int64_t M, int64_t N, int64_t K, void* ws, size_t ws_bytes,
                    mcd_blaslt_stream_t stream, bool relu) {
    if (!h || !W || !out) return fail(MCD_E_ARG, "mcd_linear_residual: NULL pointer");
    if (M < 0 || N <= 0 || K <= 0 || ldh < K || ldw < K || ldo < N || (res && ldr < N))
        return fail(MCD_E_ARG, "mcd_linear_residual: bad shape M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    if (M == 0) return MCD_OK;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_mu);
    const int dev = cur_device();
    if (!g_handles[dev]) LT(hipblasLtCreate(&g_handles[dev]));
    hipblasLtHandle_t g_handle = g_handles[dev];
    const int flags = (res ? 1 : 0) | (relu ? 2 : 0);
    const Key key{M, N, K, ldh, ldw, res ? ldr : 0, ldo, flags, bias ? 1 : 0, dev};
    auto it = g_plans.find(key);
    const float one = 1.f, zero = 0.f;
    const float* beta = res ? &one : &zero;
    const void* cptr = res ? (const void*)res : (const void*)out;
    if (it == g_plans.end()) {
        Plan p;
        // column-major view: D^T[N, M] = op(A) . op(B) with A = W ([K, N] col-major, transposed), B = h ([K, M])
        LT(hipblasLtMatmulDescCreate(&p.desc, HIPBLAS_COMPUTE_32F, HIP_R_32F));
        const int32_t ta = HIPBLAS_OP_T, tb = HIPBLAS_OP_N;
        LT(hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_TRANSA, &ta, sizeof(ta)));
        LT(hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_TRANSB, &tb, sizeof(tb)));
        if (bias || relu) {
            const uint32_t ep = bias ? (relu ? HIPBLASLT_EPILOGUE_RELU_BIAS : HIPBLASLT_EPILOGUE_BIAS) : HIPBLASLT_EPILOGUE_RELU;
            LT(hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &ep, sizeof(ep)));
            if (bias) LT(hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias, sizeof(bias)));
        }
        LT(hipblasLtMatrixLayoutCreate(&p.a, HIP_R_32F, (uint64_t)K, (uint64_t)N, ldw));
        LT(hipblasLtMatrixLayoutCreate(&p.b, HIP_R_32F, (uint64_t)K, (uint64_t)M, ldh));
        LT(hipblasLtMatrixLayoutCreate(&p.c, HIP_R_32F, (uint64_t)N, (uint64_t)M, res ? ldr : ldo));
        LT(hipblasLtMatrixLayoutCreate(&p.d, HIP_R_32F, (uint64_t)N, (uint64_t)M, ldo));
        hipblasLtMatmulPreference_t pref;
        LT(hipblasLtMatmulPreferenceCreate(&pref));
        const uint64_t max_ws = ws ? ws_bytes : 0;
        LT(hipblasLtMatmulPreferenceSetAttribute(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &max_ws, sizeof(max_ws)));
        int want = 32;   // MCD_BLASLT_CANDIDATES: how many heuristic candidates to time (experiments)
        if (const char* e = getenv("MCD_BLASLT_CANDIDATES")) {
            want = atoi(e);
            if (want < 1) want = 1;
            if (want > 512) want = 512;
        }
        std::vector<hipblasLtMatmulHeuristicResult_t> cand(want);
        int n = 0;
        LT(hipblasLtMatmulAlgoGetHeuristic(g_handle, p.desc, p.a, p.b, p.c, p.d, pref, (int)cand.size(), cand.data(), &n));
        hipblasLtMatmulPreferenceDestroy(pref);
        if (n <= 0) return fail(MCD_E_UNSUPPORTED, "mcd_linear_residual: hipBLASLt offers no algorithm for %lld x %lld x %lld",
                                (long long)M, (long long)N, (long long)K);
        // a forced pick (mcd_linear_residual_set_pick) or MCD_BLASLT_PICK=heuristic: nothing is timed
        // A pick is recorded per (M, N, K, has_res), the heuristic's list also depends on the leading dimensions: the same
        // shape called on packed rows and on rows strided out of a larger tensor may get two lists.  An index forced for
        // one that is past the other's list, or names a candidate it cannot run, falls back to the first usable one.
        int forced = -1;
        {
            auto usable = [&](int i) { return cand[i].state == HIPBLAS_STATUS_SUCCESS && cand[i].workspaceSize <= max_ws; };
            int first = 0;
            for (int i = 0; i < n; ++i)
                if (usable(i)) { first = i; break; }
            auto f = g_forced.find(ShapeKey{M, N, K, flags});
            if (f != g_forced.end()) forced = (f->second < n && usable(f->second)) ? f->second : first;
            else if (const char* e = getenv("MCD_BLASLT_PICK")) {
                if (e[0] == 'h') forced = first;
            }
        }
        // time the candidates into a scratch D (the caller's out must be written exactly once)
        float* scratch = nullptr;
        if (forced < 0 && n > 1 && hipMalloc((void**)&scratch, (size_t)M * ldo * sizeof(float)) != hipSuccess) {
            scratch = nullptr;
            (void)hipGetLastError();
        }
        int best = forced >= 0 ? forced : 0;
        float best_ms = 0.f;
        if (scratch) {
            hipEvent_t e0, e1;
            hipEventCreate(&e0);
            hipEventCreate(&e1);
            best = -1;
            for (int i = 0; i < n; ++i) {
                if (cand[i].state != HIPBLAS_STATUS_SUCCESS || cand[i].workspaceSize > max_ws) continue;
                bool ok = true;
                float ms = 0.f;
                for (int rep = 0; rep < 4 && ok; ++rep) {   // rep 0 warms up
                    if (rep == 1) hipEventRecord(e0, st);
                    ok = hipblasLtMatmul(g_handle, p.desc, &one, W, p.a, h, p.b, beta, cptr, p.c, scratch, p.d, &cand[i].algo, ws,
                                         cand[i].workspaceSize, st) == HIPBLAS_STATUS_SUCCESS;
                }
                hipEventRecord(e1, st);
                if (hipEventSynchronize(e1) != hipSuccess) ok = false;
                if (ok) hipEventElapsedTime(&ms, e0, e1);
                ++p.tried;
                if (ok && (best < 0 || ms < best_ms)) {
                    best = i;
                    best_ms = ms;
                }
            }
            hipEventDestroy(e0);
            hipEventDestroy(e1);
            hipFree(scratch);
            if (best < 0) return fail(MCD_E_LAUNCH, "mcd_linear_residual: every hipBLASLt candidate failed");
        }
        p.algo = cand[best].algo;
        p.ws = cand[best].workspaceSize;
        p.ms = best_ms / 3.f;
        p.pick = best;
        it = g_plans.emplace(key, p).first;
    }
    Plan& p = it->second;
    if (bias) LT(hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias, sizeof(bias)));
    if (p.ws > (ws ? ws_bytes : 0)) return fail(MCD_E_ARG, "mcd_linear_residual: workspace of %zu bytes needed", p.ws);
    LT(hipblasLtMatmul(g_handle, p.desc, &one, W, p.a, h, p.b, beta, cptr, p.c, out, p.d, &p.algo, ws, p.ws, st));
    return MCD_OK;
}

}  // namespace

extern "C" int mcd_linear_residual(const float* h, int64_t ldh, const float* W, int64_t ldw, const float* bias,
                                   const float* res, int64_t ldr, float* out, int64_t ldo, int64_t M, int64_t N, int64_t K,
                                   void* ws, size_t ws_bytes, mcd_blaslt_stream_t stream) {
    return linear_residual(h, ldh, W, ldw, bias, res, ldr, out, ldo, M, N, K, ws, ws_bytes, stream, false);
}

// out = relu(res + h . W^T + bias): the same call with hipBLASLt's ReLU epilogue (RELU_BIAS, or RELU without a bias),
// which the library applies to the whole sum alpha*A.B + beta*C + bias.
extern "C" int mcd_linear_residual_relu(const float* h, int64_t ldh, const float* W, int64_t ldw, const float* bias,
                                        const float* res, int64_t ldr, float* out, int64_t ldo, int64_t M, int64_t N,
                                        int64_t K, void* ws, size_t ws_bytes, mcd_blaslt_stream_t stream) {
    return linear_residual(h, ldh, W, ldw, bias, res, ldr, out, ldo, M, N, K, ws, ws_bytes, stream, true);
}
