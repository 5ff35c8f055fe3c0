// ce_loss.hip -- softmax cross-entropy over B x C x N scores as one operator with its own gradient: per-cloud NLL sums, the log-sum-exp
// kept for the gradient, the predicted class, correct / bad-target counts and the confusion table from ONE read of the scores
// (sonet_ce_loss_f32), and the gradient with respect to the scores from one more launch (sonet_ce_grad_f32).  N = 1 is the classifier's
// B x C.
//
// Replaces models/losses.py:30-43 (CrossEntropyLossSeg: log_softmax on a 4-D view + NLLLoss), models/classifier.py:95,105
// (nn.CrossEntropyLoss on the classifier's scores) and the per-batch host step of modelnet/train.py:81-87 (torch.max, the correct mask
// and its .cpu()).
//
// Forward: one thread per point, CE_THREADS points per workgroup, blockIdx.y = cloud; the loop over the C scores of a point reads
// score[b][c][n], consecutive lanes consecutive addresses.  Everything after the load is float64.  A workgroup leaves one (NLL sum,
// correct, bad) partial in the workspace -- lanes by an xor tree, waves in wave order -- and the finalize launch adds a cloud's partials
// in ascending order: no floating-point atomics, no counter to zero.  The only atomics are the integer ones of the caller's confusion table.
// With N == 1 a workgroup would hold one point: there one thread takes one CLOUD, writes that cloud's outputs itself, and no
// workspace or finalize launch is needed (the score tensor is a few KB).
#include "common.hpp"

namespace {
constexpr int CE_THREADS = 256;                   // points per workgroup
constexpr int CE_WAVES = CE_THREADS / sonet::WAVE;
constexpr int CE_MAX_C = 256;                     // classes (the confusion table is C x C)
// The gradient's grid: one workgroup per CE_THREADS elements up to this many, a grid-stride loop beyond.  The loop's second trip needs
// more than 2^28 elements (1 GiB of scores): no test of the suite reaches it -- it is correct by reading only.
constexpr int CE_GRAD_MAX_BLOCKS = 1 << 20;

template <typename T> __device__ __forceinline__ T ce_exp(T v);
template <typename T> __device__ __forceinline__ T ce_log(T v);
template <> __device__ __forceinline__ double ce_exp<double>(double v) { return exp(v); }
template <> __device__ __forceinline__ double ce_log<double>(double v) { return log(v); }
template <> __device__ __forceinline__ float ce_exp<float>(float v) { return expf(v); }
template <> __device__ __forceinline__ float ce_log<float>(float v) { return logf(v); }

__device__ __forceinline__ double ce_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // (every lane adds the same pairs: one fixed tree)
    return v;
}

// What one point yields.  p: its first score, stride: elements between two classes.  T = double in the product; float only in the
// variants build's timing record (what float64 costs).
struct CePoint {
    double nll, lse;
    int pred;
    bool t_ok, hit;
};

template <typename T>
__device__ __forceinline__ CePoint ce_point(const float *__restrict__ p, size_t stride, long long t64, int C)
{
    CePoint r;
    r.t_ok = t64 >= 0 && t64 < C;
    const int t = r.t_ok ? (int)t64 : -1;
    // arg-max as torch.max(dim=1) on CPU tensors: first of equal maxima, a NaN beats every number, the first NaN wins.
    // log-sum-exp in the same pass: m the running maximum, S = sum of exp(x - m), rescaled when m moves.
    const float x0 = p[0];
    float best = x0;
    int bi = 0;
    T m = (T)x0, S = (T)1, xt = (T)x0;
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
        const float xf = p[(size_t)c * stride];
        const bool take = xf > best || (xf != xf && best == best);
        best = take ? xf : best;
        bi = take ? c : bi;
        const T x = (T)xf;
        xt = c == t ? x : xt;
        const bool up = x > m;
        const T e = ce_exp<T>(up ? m - x : x - m);
        S = up ? S * e + (T)1 : S + e;
        m = up ? x : m;
    }
    const T logS = ce_log<T>(S);
    r.lse = (double)(m + logS);
    r.nll = r.t_ok ? (double)((m - xt) + logS) : 0.0;     // two non-negative terms
    r.pred = bi;
    r.hit = r.t_ok && bi == t;
    return r;
}

template <typename T>
__global__ __launch_bounds__(CE_THREADS) void ce_loss_kernel(const float *__restrict__ score, const int64_t *__restrict__ target,
                                                              double *__restrict__ lse, int32_t *__restrict__ pred,
                                                              unsigned long long *__restrict__ confusion, double *__restrict__ nll_part,
                                                              int32_t *__restrict__ cnt_part, int C, int N)
{
    __shared__ double s_nll[CE_WAVES];
    __shared__ int s_ok[CE_WAVES], s_bad[CE_WAVES];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = blockIdx.x * CE_THREADS + tid;
    double nll = 0.0;
    bool ok = false, oob = false;
    if (n < N) {
        const size_t pt = (size_t)b * N + n;
        const long long t64 = target[pt];
        const CePoint r = ce_point<T>(score + (size_t)b * C * N + n, (size_t)N, t64, C);
        if (lse) lse[pt] = r.lse;
        if (pred) pred[pt] = r.pred;
        if (confusion && r.t_ok) atomicAdd(&confusion[(size_t)t64 * C + r.pred], 1ULL);
        nll = r.nll;
        ok = r.hit;
        oob = !r.t_ok;
    }
    const int lane = tid & (sonet::WAVE - 1), wave = tid / sonet::WAVE;
    const int n_ok = __popcll(__ballot(ok)), n_oob = __popcll(__ballot(oob));
    const double wsum = ce_wave_sum(nll);
    if (lane == 0) {
        s_nll[wave] = wsum;
        s_ok[wave] = n_ok;
        s_bad[wave] = n_oob;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = s_nll[0];
        int a_ok = s_ok[0], a_bad = s_bad[0];
#pragma unroll
        for (int w = 1; w < CE_WAVES; ++w) {
            acc += s_nll[w];
            a_ok += s_ok[w];
            a_bad += s_bad[w];
        }
        const size_t o = (size_t)b * gridDim.x + blockIdx.x;
        nll_part[o] = acc;
        cnt_part[2 * o] = a_ok;
        cnt_part[2 * o + 1] = a_bad;
    }
}

// One thread per cloud: the workgroup partials in index order.
__global__ __launch_bounds__(64) void ce_loss_finalize_kernel(const double *__restrict__ nll_part, const int32_t *__restrict__ cnt_part,
                                                              int nblk, double *__restrict__ nll_sum, int32_t *__restrict__ correct,
                                                              int32_t *__restrict__ bad, int B)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double acc = 0.0;
    int a_ok = 0, a_bad = 0;
    for (int k = 0; k < nblk; ++k) {
        const size_t o = (size_t)b * nblk + k;
        acc += nll_part[o];
        a_ok += cnt_part[2 * o];
        a_bad += cnt_part[2 * o + 1];
    }
    nll_sum[b] = acc;
    correct[b] = a_ok;
    bad[b] = a_bad;
}

// N == 1: one thread per cloud, its C scores contiguous.
template <typename T>
__global__ __launch_bounds__(CE_THREADS) void ce_loss_rows_kernel(const float *__restrict__ score, const int64_t *__restrict__ target,
                                                                   double *__restrict__ lse, int32_t *__restrict__ pred,
                                                                   unsigned long long *__restrict__ confusion, double *__restrict__ nll_sum,
                                                                   int32_t *__restrict__ correct, int32_t *__restrict__ bad, int B, int C)
{
    const size_t b = (size_t)blockIdx.x * CE_THREADS + threadIdx.x;
    if (b >= (size_t)B) return;
    const long long t64 = target[b];
    const CePoint r = ce_point<T>(score + b * C, (size_t)1, t64, C);
    if (lse) lse[b] = r.lse;
    if (pred) pred[b] = r.pred;
    if (confusion && r.t_ok) atomicAdd(&confusion[(size_t)t64 * C + r.pred], 1ULL);
    nll_sum[b] = r.nll;
    correct[b] = r.hit ? 1 : 0;
    bad[b] = r.t_ok ? 0 : 1;
}

// One thread per ELEMENT of the flat B x C x N tensor (coalesced for every N, N == 1 included); a grid-stride loop beyond
// CE_GRAD_MAX_BLOCKS workgroups.  float64 after the loads, rounded once.
__global__ __launch_bounds__(CE_THREADS) void ce_grad_kernel(const float *__restrict__ score, const int64_t *__restrict__ target,
                                                              const double *__restrict__ lse, const float *__restrict__ gout, double scale,
                                                              float *__restrict__ grad, size_t total, int C, int N)
{
    const double g = (double)gout[0];
    const size_t step = (size_t)gridDim.x * CE_THREADS;
    for (size_t i = (size_t)blockIdx.x * CE_THREADS + threadIdx.x; i < total; i += step) {
        const size_t bc = i / (size_t)N;
        const int n = (int)(i - bc * (size_t)N);
        const size_t b = bc / (size_t)C;
        const int c = (int)(bc - b * (size_t)C);
        const size_t pt = b * (size_t)N + n;
        const long long t64 = target[pt];
        float out = 0.f;                                                  // a bad target: zeros for the whole point
        if (t64 >= 0 && t64 < C) {
            const double p = exp((double)score[i] - lse[pt]);
            out = (float)((p - (c == (int)t64 ? 1.0 : 0.0)) * g * scale);
        }
        grad[i] = out;
    }
}

int ce_check(const char *what, const void *score, const void *target, int B, int C, int N)
{
    SONET_REQUIRE(score && target, "%s: NULL pointer", what);
    SONET_REQUIRE((uintptr_t)score % 4 == 0 && (uintptr_t)target % 8 == 0, "%s: score must be 4-byte and target 8-byte aligned", what);
    SONET_REQUIRE(B > 0 && C > 0 && N > 0, "%s: non-positive size (B=%d C=%d N=%d)", what, B, C, N);
    if (C > CE_MAX_C) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: C=%d > %d", what, C, CE_MAX_C);
    if ((long long)B * N >= (1LL << 31)) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B*N=%lld >= 2^31", what, (long long)B * N);
    if (N > 1 && B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B=%d > 65535 with N > 1", what, B);
    return SONET_OK;
}

template <typename T>
int ce_loss_launch(const char *what, const float *score, const int64_t *target, double *lse, double *nll_sum, int32_t *pred,
                   int32_t *correct, int32_t *bad, int64_t *confusion, void *ws, int B, int C, int N, sonet_stream_t stream)
{
    if (int e = ce_check(what, score, target, B, C, N)) return e;
    SONET_REQUIRE(nll_sum && correct && bad && ws, "%s: NULL pointer", what);
    SONET_REQUIRE((uintptr_t)nll_sum % 8 == 0 && (uintptr_t)lse % 8 == 0, "%s: lse and nll_sum must be 8-byte aligned", what);
    SONET_REQUIRE((uintptr_t)confusion % 8 == 0 && (uintptr_t)ws % 8 == 0, "%s: confusion and ws must be 8-byte aligned", what);
    hipStream_t st = sonet::as_stream(stream);
    unsigned long long *conf = reinterpret_cast<unsigned long long *>(confusion);
    if (N == 1) {
        hipLaunchKernelGGL(ce_loss_rows_kernel<T>, dim3(sonet::ceil_div(B, CE_THREADS)), dim3(CE_THREADS), 0, st, score, target, lse, pred,
                           conf, nll_sum, correct, bad, B, C);
        return sonet::launched(what);
    }
    const int nblk = (int)sonet::ceil_div64(N, CE_THREADS);
    double *nll_part = reinterpret_cast<double *>(ws);
    int32_t *cnt_part = reinterpret_cast<int32_t *>(nll_part + (size_t)B * nblk);
    hipLaunchKernelGGL(ce_loss_kernel<T>, dim3(nblk, B), dim3(CE_THREADS), 0, st, score, target, lse, pred, conf, nll_part, cnt_part, C, N);
    hipLaunchKernelGGL(ce_loss_finalize_kernel, dim3(sonet::ceil_div(B, 64)), dim3(64), 0, st, nll_part, cnt_part, nblk, nll_sum, correct,
                       bad, B);
    return sonet::launched(what);
}
}  // namespace

extern "C" int sonet_ce_max_c(void) { return CE_MAX_C; }
extern "C" int sonet_ce_block_points(void) { return CE_THREADS; }

extern "C" size_t sonet_ce_loss_ws_size(int B, int C, int N)
{
    if (B <= 0 || C <= 0 || N <= 0) return 0;
    if (N == 1) return 16;                                            // (unused there; never an empty allocation)
    return (size_t)B * (size_t)sonet::ceil_div64(N, CE_THREADS) * (sizeof(double) + 2 * sizeof(int32_t));
}

extern "C" int sonet_ce_loss_f32(const float *score, const int64_t *target, double *lse, double *nll_sum, int32_t *pred, int32_t *correct,
                                 int32_t *bad, int64_t *confusion, void *ws, int B, int C, int N, sonet_stream_t stream)
{
    return ce_loss_launch<double>("sonet_ce_loss_f32", score, target, lse, nll_sum, pred, correct, bad, confusion, ws, B, C, N, stream);
}

#ifdef SONET_VARIANTS
// The same launches with float32 expf / logf after the load: a timing record of what the float64 arithmetic costs (tools/bench_ce_loss.py).
extern "C" int sonet_ce_loss_f32_sp(const float *score, const int64_t *target, double *lse, double *nll_sum, int32_t *pred,
                                    int32_t *correct, int32_t *bad, int64_t *confusion, void *ws, int B, int C, int N, sonet_stream_t stream)
{
    return ce_loss_launch<float>("sonet_ce_loss_f32_sp", score, target, lse, nll_sum, pred, correct, bad, confusion, ws, B, C, N, stream);
}
#endif

extern "C" int sonet_ce_grad_f32(const float *score, const int64_t *target, const double *lse, const float *gout, double scale,
                                 float *grad, int B, int C, int N, sonet_stream_t stream)
{
    const char *what = "sonet_ce_grad_f32";
    if (int e = ce_check(what, score, target, B, C, N)) return e;
    SONET_REQUIRE(lse && gout && grad, "%s: NULL pointer", what);
    SONET_REQUIRE((uintptr_t)lse % 8 == 0, "%s: lse must be 8-byte aligned", what);
    const size_t total = (size_t)B * C * N;
    const long long blocks = sonet::ceil_div64((long long)total, CE_THREADS);
    hipLaunchKernelGGL(ce_grad_kernel, dim3((unsigned)(blocks < CE_GRAD_MAX_BLOCKS ? blocks : CE_GRAD_MAX_BLOCKS)), dim3(CE_THREADS), 0,
                       sonet::as_stream(stream), score, target, lse, gout, scale, grad, total, C, N);
    return sonet::launched(what);
}
