// seg_metrics.hip -- part-segmentation metrics from ONE read of the score tensor: predicted part per point, per-cloud correct
// count, NLL sum, per-part intersection / prediction / ground-truth counts and the mean IoU of the cloud's category.
//
// Replaces the host step of the reference's test loop (part-seg/train.py:87-104 with models/losses.py:119-189): torch.max over
// the class scores, a device-to-host copy of the whole B x C x N score tensor and a Python double loop over clouds and parts.
//
// One thread per point, SM_THREADS points per workgroup, blockIdx.y = cloud.  The loop over the C scores of a point reads
// score[b][c][n]: consecutive lanes read consecutive addresses.  Everything integer goes through LDS bins and integer atomics
// (any order gives the same counts); the NLL is summed in float64 in a fixed order -- lanes by an xor tree, the waves of a
// workgroup in wave order, the workgroups of a cloud in index order by the finalize launch.  No floating-point atomics.
#include "common.hpp"

namespace {
constexpr int SM_THREADS = 256;                   // points per workgroup
constexpr int SM_WAVES = SM_THREADS / sonet::WAVE;
constexpr int SM_MAX_C = 256;                     // LDS bins: 3 x 256 x 4 bytes

// The counters are accumulated with atomics: zeroed by a kernel of this entry's own (one launch for the five arrays; kernels, not
// memset nodes, for the reason given at sonet::zero_words).
__global__ __launch_bounds__(256) void seg_metrics_zero_kernel(int32_t *__restrict__ correct, int32_t *__restrict__ bad,
                                                                int32_t *__restrict__ inter, int32_t *__restrict__ pred_cnt,
                                                                int32_t *__restrict__ gt_cnt, int B, int C)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < B) {
        correct[t] = 0;
        bad[t] = 0;
    }
    if (t < B * C) {
        inter[t] = 0;
        pred_cnt[t] = 0;
        gt_cnt[t] = 0;
    }
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // (every lane adds the same pairs: one fixed tree)
    return v;
}

__global__ __launch_bounds__(SM_THREADS) void seg_metrics_kernel(const float *__restrict__ score, const int64_t *__restrict__ seg,
                                                                  int32_t *__restrict__ pred_out, int32_t *__restrict__ correct,
                                                                  int32_t *__restrict__ inter, int32_t *__restrict__ pred_cnt,
                                                                  int32_t *__restrict__ gt_cnt, int32_t *__restrict__ bad,
                                                                  double *__restrict__ nll_part, int C, int N)
{
    __shared__ int s_pred[SM_MAX_C], s_gt[SM_MAX_C], s_inter[SM_MAX_C];
    __shared__ int s_correct, s_bad;
    __shared__ double s_nll[SM_WAVES];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = blockIdx.x * SM_THREADS + tid;
    for (int i = tid; i < C; i += SM_THREADS) {
        s_pred[i] = 0;
        s_gt[i] = 0;
        s_inter[i] = 0;
    }
    if (tid == 0) {
        s_correct = 0;
        s_bad = 0;
    }
    __syncthreads();
    const bool valid = n < N;
    double nll = 0.0;
    bool ok = false, oob = false;
    if (valid) {
        const float *p = score + (size_t)b * C * N + n;
        const long long t64 = seg[(size_t)b * N + n];
        const bool t_ok = t64 >= 0 && t64 < C;
        const int t = t_ok ? (int)t64 : -1;
        // arg-max as torch.max(dim=1) on CPU tensors: first of equal maxima, a NaN beats every number, the first NaN wins.
        // log-sum-exp in the same pass: m is the running maximum, r = sum of exp(x - m) WITHOUT the maximum's own 1, rescaled when
        // m moves.  nll = lse - x[t] = (m - x[t]) + log1p(r): two non-negative terms, so a confident point (nll << |m|) keeps its
        // relative precision, which m + log(1 + r) - x[t] would lose to cancellation.
        float best = p[0];
        int bi = 0;
        float m = best, r = 0.f, xt = best;
#pragma unroll 4
        for (int c = 1; c < C; ++c) {
            const float x = p[(size_t)c * N];
            const bool take = x > best || (x != x && best == best);
            best = take ? x : best;
            bi = take ? c : bi;
            xt = c == t ? x : xt;
            const bool up = x > m;
            const float e = expf(up ? m - x : x - m);
            r = up ? r * e + e : r + e;
            m = up ? x : m;
        }
        const float nll_f = (m - xt) + log1pf(r);
        if (pred_out) pred_out[(size_t)b * N + n] = bi;
        ok = t_ok && bi == t;
        oob = !t_ok;
        nll = t_ok ? (double)nll_f : 0.0;
        atomicAdd(&s_pred[bi], 1);
        if (t_ok) atomicAdd(&s_gt[t], 1);
        if (ok) atomicAdd(&s_inter[bi], 1);
    }
    const int lane = tid & (sonet::WAVE - 1), wave = tid / sonet::WAVE;
    const int n_ok = __popcll(__ballot(ok)), n_oob = __popcll(__ballot(oob));
    const double wsum = wave_sum_f64(nll);
    if (lane == 0) {
        if (n_ok) atomicAdd(&s_correct, n_ok);
        if (n_oob) atomicAdd(&s_bad, n_oob);
        s_nll[wave] = wsum;
    }
    __syncthreads();
    for (int i = tid; i < C; i += SM_THREADS) {
        const size_t o = (size_t)b * C + i;
        if (s_pred[i]) atomicAdd(&pred_cnt[o], s_pred[i]);
        if (s_gt[i]) atomicAdd(&gt_cnt[o], s_gt[i]);
        if (s_inter[i]) atomicAdd(&inter[o], s_inter[i]);
    }
    if (tid == 0) {
        if (s_correct) atomicAdd(&correct[b], s_correct);
        if (s_bad) atomicAdd(&bad[b], s_bad);
        double acc = s_nll[0];
#pragma unroll
        for (int w = 1; w < SM_WAVES; ++w) acc += s_nll[w];
        nll_part[(size_t)b * gridDim.x + blockIdx.x] = acc;
    }
}

// One thread per cloud: the NLL partials in workgroup order, the IoU of the cloud's parts in ascending order -- float64, the
// operations of models/losses.py:162-185 in their order: 1.0 for an empty union, else inter / (union + 0.0001); sum; / parts.
__global__ __launch_bounds__(64) void seg_metrics_finalize_kernel(const int64_t *__restrict__ label, const int32_t *__restrict__ part_offsets,
                                                                  int n_cat, const int32_t *__restrict__ inter,
                                                                  const int32_t *__restrict__ pred_cnt, const int32_t *__restrict__ gt_cnt,
                                                                  const double *__restrict__ nll_part, int nblk, double *__restrict__ nll_sum,
                                                                  double *__restrict__ iou, int32_t *__restrict__ bad, int B, int C)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double nan = __builtin_nan("");
    int nbad = bad[b];
    double acc = 0.0;
    for (int k = 0; k < nblk; ++k) acc += nll_part[(size_t)b * nblk + k];
    const long long lab = label[b];
    double v = nan;
    bool lab_ok = lab >= 0 && lab < n_cat;
    if (lab_ok) {
        const int lo = part_offsets[lab], hi = part_offsets[lab + 1];
        lab_ok = lo >= 0 && hi <= C && lo < hi;              // (a table the caller did not check: no read outside the bins)
        if (lab_ok) {
            double sum = 0.0;
            for (int p = lo; p < hi; ++p) {
                const size_t o = (size_t)b * C + p;
                const int in = inter[o], un = pred_cnt[o] + gt_cnt[o] - in;
                sum += un == 0 ? 1.0 : (double)in / ((double)un + 0.0001);
            }
            v = sum / (double)(hi - lo);
        }
    }
    if (!lab_ok) ++nbad;
    iou[b] = v;
    nll_sum[b] = nbad ? nan : acc;
    bad[b] = nbad;
}
}  // namespace

extern "C" size_t sonet_seg_metrics_ws_size(int B, int C, int N)
{
    if (B <= 0 || C <= 0 || N <= 0) return 0;
    return (size_t)B * (size_t)sonet::ceil_div64(N, SM_THREADS) * sizeof(double);
}

extern "C" int sonet_seg_metrics_f32(const float *score, const int64_t *seg, const int64_t *label, const int32_t *part_offsets,
                                     int n_cat, int32_t *pred_out, int32_t *correct, double *nll_sum, int32_t *inter,
                                     int32_t *pred_cnt, int32_t *gt_cnt, double *iou, int32_t *bad, void *ws, int B, int C, int N,
                                     sonet_stream_t stream)
{
    const char *what = "sonet_seg_metrics_f32";
    SONET_REQUIRE(score && seg && label && part_offsets && correct && nll_sum && inter && pred_cnt && gt_cnt && iou && bad && ws,
                  "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && N > 0, "%s: non-positive size (B=%d C=%d N=%d)", what, B, C, N);
    SONET_REQUIRE(n_cat > 0, "%s: n_cat=%d must be positive", what, n_cat);
    if (C > SM_MAX_C) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: C=%d > %d", what, C, SM_MAX_C);
    if (B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B=%d > 65535", what, B);
    hipStream_t st = sonet::as_stream(stream);
    const int nblk = (int)sonet::ceil_div64(N, SM_THREADS);
    hipLaunchKernelGGL(seg_metrics_zero_kernel, dim3(sonet::ceil_div(B * C, 256)), dim3(256), 0, st, correct, bad, inter, pred_cnt,
                       gt_cnt, B, C);
    hipLaunchKernelGGL(seg_metrics_kernel, dim3(nblk, B), dim3(SM_THREADS), 0, st, score, seg, pred_out, correct, inter, pred_cnt,
                       gt_cnt, bad, reinterpret_cast<double *>(ws), C, N);
    hipLaunchKernelGGL(seg_metrics_finalize_kernel, dim3(sonet::ceil_div(B, 64)), dim3(64), 0, st, label, part_offsets, n_cat, inter,
                       pred_cnt, gt_cnt, reinterpret_cast<const double *>(ws), nblk, nll_sum, iou, bad, B, C);
    return sonet::launched(what);
}
