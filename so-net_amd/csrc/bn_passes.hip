// bn_passes.hip -- the element-wise passes of training-mode BatchNorm + ReLU around the GEMMs (training, configs 2 / 5), f32 and bf16 storage.
//
// Forward (models/layers.py:60-70, 282-296: conv1d -> F.batch_norm -> relu):
//   statistics   per channel sum and sum of squares over (b, l) in f64 -> mean, biased variance (+ the BatchNorm rider, common.hpp)
//   normalise    y = act(x * scale[c] + shift[c]), out of place (raw stays for the backward) or in place
// Backward, replacing the autograd graph of the same three operators: two passes over (gy, raw) instead of ~20 element-wise aten launches
//   pass 1  per channel:  s1 = sum gy*mask,  s2 = sum gy*mask*raw      (f64 accumulation, as the forward statistics)
//   pass 2  g_raw = a[c] * (gy*mask) + b[c] * raw + c0[c]
// with mask = (fma(raw, scale[c], shift[c]) > 0) when the layer has a ReLU (bit-identical to the forward's affine: affine_act / relu_masked /
// bn_bwd_apply of device.hpp are the ONE copy of the per-element arithmetic), else 1.  The coefficient kernels turn (s1, s2) into (a, b, c0)
//   a = gamma*invstd,  b = -a*invstd*sg/n,  c0 = -a*s1/n - b*mean,  sg = invstd*(s2 - mean*s1)
// (the usual  gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)) ), for a constant affine a = scale, b = c0 = 0.
// The GEMMs themselves (dgrad = W^T g_raw on the pointmlp kernels, wgrad = g_raw x^T) are launched by the host.
//
// Every [B][C][L] pass exists in up to three flavours, chosen by the host (launch_stats / launch_rowwise below):
//   vec     16 bytes per lane and access (4 f32 / 8 bf16): rows and pointers 16-byte aligned -- the flavour the training step runs
//   pair    bf16 only: one dword = two elements per lane (L even, pointers 4-byte aligned)
//   scalar  one element per lane: everything else
// Also here: the three node-broadcast forms of the normalise pass (node_add_affine_act, node_gather_lead_affine_act f32 / bf16).
#include "common.hpp"

#include <hip/hip_runtime.h>

namespace {

constexpr int BW_THREADS = 256;

// T below: storage type of the [B][C][L] tensors (float, or uint16_t = bfloat16 bits: values widened, arithmetic in f32 / f64, results
// rounded to nearest-even bf16).

// The tail of the scalar statistics kernels: the workgroup's two f64 sums -- wave shuffle, one LDS pair per wave, the waves added in
// order by thread 0 -- into ws[c] and ws[C + c] with one pair of f64 atomics.
template <int THREADS>
__device__ __forceinline__ void block_sum2_atomic(double s1, double s2, double *__restrict__ ws, int c, int C)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    __shared__ double red[2][THREADS / 64];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, a2 = 0.0;
        for (int w = 0; w < THREADS / 64; ++w) { a += red[0][w]; a2 += red[1][w]; }
        unsafeAtomicAdd(&ws[c], a);
        unsafeAtomicAdd(&ws[C + c], a2);
    }
}

// Scalar statistics, grid (chunks, C): each workgroup reduces one chunk of one channel's flat (b, l) index, every term carried in f64.
//   RAW:  (sum of gy * mask, sum of gy * mask * raw), the backward's pass 1;
//   !RAW: (sum, sum of squares) of gy, the forward statistics (raw, scale, shift unused).
// RAW is a template argument, not a test of the pointer: tested at run time inside the element loop the f32 kernel measured 12 % slower
// than the two kernels it replaces (docs/findings.md).  PAIR (bf16 only): one dword = two elements per lane.
template <typename T, bool PAIR, bool RAW>
__global__ __launch_bounds__(BW_THREADS) void stats_scalar_kernel(const T *__restrict__ gy, const T *__restrict__ raw,
                                                                   const float *__restrict__ scale, const float *__restrict__ shift,
                                                                   int relu, int B, int C, int L, double *__restrict__ ws)
{
    static_assert(!PAIR || sizeof(T) == 2, "pairs are two bf16 values in a dword");
    const int c = blockIdx.y;
    constexpr int V = PAIR ? 2 : 1;
    const int Lv = L / V;
    const long long per_c = (long long)B * Lv;
    const long long chunk = (per_c + gridDim.x - 1) / gridDim.x;
    const long long beg = (long long)blockIdx.x * chunk, end = min(per_c, beg + chunk);
    const float sc = RAW ? scale[c] : 0.f, sh = RAW ? shift[c] : 0.f;
    double s1 = 0.0, s2 = 0.0;
    for (long long t = beg + threadIdx.x; t < end; t += BW_THREADS) {
        const long long b = t / Lv;
        const long long o = (b * C + c) * (long long)L + (t - b * Lv) * V;
        float g[V], r[V];
        if constexpr (PAIR) {
            const unsigned dg = *reinterpret_cast<const unsigned *>(gy + o);
            g[0] = bf_lo(dg); g[1] = bf_hi(dg);
            if constexpr (RAW) { const unsigned dr = *reinterpret_cast<const unsigned *>(raw + o); r[0] = bf_lo(dr); r[1] = bf_hi(dr); }
        } else {
            g[0] = ld_f32(gy, o);
            if constexpr (RAW) r[0] = ld_f32(raw, o);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if constexpr (RAW) {
                const float gv = relu_masked(g[v], r[v], sc, sh, relu);
                s1 += (double)gv;
                s2 += (double)gv * (double)r[v];
            } else {
                s1 += (double)g[v];
                s2 += (double)g[v] * (double)g[v];
            }
        }
    }
    block_sum2_atomic<BW_THREADS>(s1, s2, ws, c, C);
}

__global__ __launch_bounds__(256) void bwd_ws_zero_kernel(double *ws, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) ws[i] = 0.0;
}

// (sum, sum of squares) -> mean, biased variance; with a BatchNorm rider (common.hpp) also what bn_fwd_coeffs_kernel and
// bn_running_update_kernel below compute from them, operation for operation
__global__ __launch_bounds__(256) void stats_finalize_kernel(const double *__restrict__ ws, int C, double inv_n,
                                                             float *__restrict__ mean, float *__restrict__ var, const sonet::BnRider rd)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double m = ws[c] * inv_n;
    double v = ws[C + c] * inv_n - m * m;
    if (v < 0.0) v = 0.0;
    mean[c] = (float)m;
    var[c] = (float)v;
    if (rd.gamma != nullptr) {
        const float mf = (float)m, vf = (float)v;
        const float is = 1.0f / __fsqrt_rn(vf + rd.eps);
        const float s_ = rd.gamma[c] * is;
        rd.invstd[c] = is;
        rd.sc[c] = s_;
        rd.sh[c] = rd.beta[c] - mf * s_;
        if (rd.rmean != nullptr) {
            const float mo = rd.momentum;
            rd.rmean[c] = __fmaf_rn(mf, mo, __fmul_rn(rd.rmean[c], 1.0f - mo));
            rd.rvar[c] = __fmaf_rn(__fmul_rn(vf, rd.unbias), mo, __fmul_rn(rd.rvar[c], 1.0f - mo));
        }
    }
}

// y = act(y * scale[c] + shift[c]) in place over the flat index: another access pattern than the row kernels (no row per workgroup, the
// channel from a division per element), so a kernel of its own
__global__ __launch_bounds__(256) void channel_affine_act_kernel(float *__restrict__ y, const float *__restrict__ scale,
                                                                  const float *__restrict__ shift, int relu, int C, int L,
                                                                  long long total)
{
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int c = (int)((t / L) % C);
        y[t] = affine_act(y[t], scale[c], shift[c], relu);
    }
}

// Scalar row kernel, grid (rows, ysplit): one workgroup row = one (b, c) row of L elements, the coefficients are wave-uniform.
//   MODE 0: out = act(raw * scale + shift) (forward normalise + ReLU; gy, ca, cb, cc unused);
//   MODE 1: out = a * (gy * mask) + b * raw + c0 with mask from (raw, scale, shift) (backward apply).
// PAIR (bf16 only): one dword = two elements per lane.
template <int MODE, typename T, bool PAIR>
__global__ __launch_bounds__(256) void rowwise_kernel(const T *__restrict__ gy, const T *__restrict__ raw,
                                                       const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                       const float *__restrict__ ca, const float *__restrict__ cb,
                                                       const float *__restrict__ cc, T *__restrict__ out, int C, int L)
{
    static_assert(!PAIR || sizeof(T) == 2, "pairs are two bf16 values in a dword");
    const long long row = blockIdx.x;
    const int c = (int)(row % C);
    const float sc = scale[c], sh = shift[c];
    const float a = MODE == 1 ? ca[c] : 0.f, b = MODE == 1 ? cb[c] : 0.f, c0 = MODE == 1 ? cc[c] : 0.f;
    const T *r = raw + row * L, *g = MODE == 1 ? gy + row * L : nullptr;
    T *o = out + row * L;
    auto f = [&](float rv, float gv) {
        if constexpr (MODE == 0) return affine_act(rv, sc, sh, relu);
        else return bn_bwd_apply(gv, rv, sc, sh, relu, a, b, c0);
    };
    if constexpr (PAIR) {
        const int Lv = L >> 1;
        for (int t = blockIdx.y * 256 + threadIdx.x; t < Lv; t += gridDim.y * 256) {
            const unsigned dr = reinterpret_cast<const unsigned *>(r)[t];
            const unsigned dg = MODE == 1 ? reinterpret_cast<const unsigned *>(g)[t] : 0u;
            reinterpret_cast<unsigned *>(o)[t] = cvt_pk_bf16(f(bf_lo(dr), bf_lo(dg)), f(bf_hi(dr), bf_hi(dg)));
        }
    } else {
        for (int t = blockIdx.y * 256 + threadIdx.x; t < L; t += gridDim.y * 256) {
            const float v = f(ld_f32(r, t), MODE == 1 ? ld_f32(g, t) : 0.f);
            if constexpr (sizeof(T) == 4) o[t] = v;
            else o[t] = (uint16_t)(cvt_pk_bf16(v, 0.f) & 0xFFFFu);      // (st_rne converts (v, v): the same bf16 from another instruction)
        }
    }
}

// y = act((t + z[b][c][ids[b][l]]) * scale[c] + shift[c]) in place: the per-node block of a layer whose input concatenates
// per-point and per-node (broadcast back) channels is computed once per node and added here (segmenter layer 1,
// models/networks.py:296-326).  One workgroup per (b, c) row; the row's M node values sit in LDS.
__global__ __launch_bounds__(256) void node_add_affine_act_kernel(float *__restrict__ t, const float *__restrict__ z,
                                                                   const int32_t *__restrict__ ids, const float *__restrict__ scale,
                                                                   const float *__restrict__ shift, int relu, int C, int L, int M)
{
    extern __shared__ float zrow[];
    const long long row = blockIdx.x;
    const int c = (int)(row % C);
    const long long b = row / C;
    for (int m = threadIdx.x; m < M; m += 256) zrow[m] = z[row * M + m];
    __syncthreads();
    const float sc = scale[c], sh = shift[c];
    float *tr = t + row * L;
    const int32_t *id = ids + b * L;
    for (int l = blockIdx.y * 256 + threadIdx.x; l < L; l += gridDim.y * 256) {
        const int m = id[l];
        tr[l] = affine_act(tr[l] + ((unsigned)m < (unsigned)M ? zrow[m] : 0.f), sc, sh, relu);
    }
}

// out[b][c][l] = act((z[b][c][gidx[b][l]] + sum_i wl[c][i] * lead[b][i][l]) * scale[c] + shift[c]):  a layer over GATHERED node
// features plus a few per-column channels (KNNModule layer 1: 384 gathered + 3 de-centred coordinate channels over K * M
// columns, models/layers.py:313-350) is linear in the features, so W_f . x is computed ONCE per node (z, M columns instead of
// K * M: one ninth of the MFMAs at K = 9) and gathered here; the NL <= 4 lead channels are exact f32 fmas in channel order.
// One workgroup per (cloud, 8 channels): gidx / lead are read once per 8 output rows, the 8 node rows sit in LDS.
constexpr int NGL_CH = 8, NGL_THREADS = 128;
// T: storage type of z and out (float, or uint16_t = bfloat16 bits: values widened, arithmetic in f32, one rounding on the store)
template <typename T>
__global__ __launch_bounds__(NGL_THREADS) void node_gather_lead_kernel(const T *__restrict__ z, const int32_t *__restrict__ gidx,
                                                                        const float *__restrict__ lead, const float *__restrict__ wl,
                                                                        const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                                        T *__restrict__ out, int C, int L, int M, int NL)
{
    extern __shared__ float zs[];                                 // [NGL_CH][M] | coef[NGL_CH][6] (w0..w3, scale, shift)
    float *coef = zs + NGL_CH * M;
    const int cb = blockIdx.x * NGL_CH;
    const long long b = blockIdx.y;
    const int nch = min(NGL_CH, C - cb);
    for (int i = threadIdx.x; i < nch * M; i += NGL_THREADS) zs[i] = ld_f32(z, ((long long)b * C + cb) * M + i);
    if (threadIdx.x < nch) {
        const int c = cb + threadIdx.x;
        for (int i = 0; i < 4; ++i) coef[threadIdx.x * 6 + i] = i < NL ? wl[c * NL + i] : 0.f;
        coef[threadIdx.x * 6 + 4] = scale[c];
        coef[threadIdx.x * 6 + 5] = shift[c];
    }
    __syncthreads();
    const int32_t *g = gidx + b * L;
    const float *ld = lead + b * (long long)NL * L;
    T *ob = out + ((long long)b * C + cb) * L;
    const int L4 = (L + 3) >> 2;
    const bool vec = (L & 3) == 0;
    // a thread owns a quad of columns: node ids and lead channels are read once and serve the 8 channel rows
    for (int q = threadIdx.x; q < L4; q += NGL_THREADS) {
        const int l = q * 4;
        int m[4];
        float d[4][4];
        if (vec) {
            const int4 mv = *reinterpret_cast<const int4 *>(g + l);
            m[0] = mv.x; m[1] = mv.y; m[2] = mv.z; m[3] = mv.w;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 dv = i < NL ? *reinterpret_cast<const float4 *>(ld + (long long)i * L + l) : make_float4(0.f, 0.f, 0.f, 0.f);
                d[i][0] = dv.x; d[i][1] = dv.y; d[i][2] = dv.z; d[i][3] = dv.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int le = l + e < L ? l + e : L - 1;
                m[e] = g[le];
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i][e] = i < NL ? ld[(long long)i * L + le] : 0.f;
            }
        }
        for (int c = 0; c < nch; ++c) {
            const float *cf = coef + c * 6;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = (unsigned)m[e] < (unsigned)M ? zs[c * M + m[e]] : 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) a = __fmaf_rn(cf[i], d[i][e], a);      // (absent lead channels: + 0 * 0, exact)
                a = __fmaf_rn(a, cf[4], cf[5]);
                v[e] = (relu && a < 0.f) ? 0.f : a;
            }
            T *o = ob + (long long)c * L + l;
            if (vec) st4_rne(o, v);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (l + e < L) st_rne(o, e, v[e]);
            }
        }
    }
}

// per-channel coefficient kernels (C threads): replace a dozen C-element aten launches per layer
__global__ __launch_bounds__(256) void bn_fwd_coeffs_kernel(const float *__restrict__ mean, const float *__restrict__ var,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             float eps, int C, float *__restrict__ invstd,
                                                             float *__restrict__ sc, float *__restrict__ sh)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float is = 1.0f / __fsqrt_rn(var[c] + eps);          // torch.rsqrt(var + eps) to 1 ulp; only the product below is used
    const float s = gamma[c] * is;
    invstd[c] = is;
    sc[c] = s;
    sh[c] = beta[c] - mean[c] * s;
}

// F.batch_norm's running-statistics update (models/layers.py:60-70 via MyBatchNorm*): r = r*(1-m) + m*stat, the variance
// entering unbiased (var * n/(n-1)).  One launch instead of four C-element aten launches per BatchNorm layer and step.
__global__ __launch_bounds__(256) void bn_running_update_kernel(float *__restrict__ rmean, float *__restrict__ rvar,
                                                                 const float *__restrict__ mean, const float *__restrict__ var,
                                                                 float m, float unbias, int C)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    rmean[c] = __fmaf_rn(mean[c], m, __fmul_rn(rmean[c], 1.0f - m));
    rvar[c] = __fmaf_rn(__fmul_rn(var[c], unbias), m, __fmul_rn(rvar[c], 1.0f - m));
}

__global__ __launch_bounds__(256) void bn_bwd_coeffs_kernel(const double *__restrict__ sums, const float *__restrict__ mean,
                                                             const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                             double n, int C, float *__restrict__ a, float *__restrict__ b,
                                                             float *__restrict__ c0, float *__restrict__ g_gamma,
                                                             float *__restrict__ g_beta)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double s1 = sums[c], s2 = sums[C + c], m = (double)mean[c], is = (double)invstd[c];
    const double sg = is * (s2 - m * s1);                       // sum gy*mask*xhat
    const double av = (double)gamma[c] * is;
    const double bv = -av * is * sg / n;
    a[c] = (float)av;
    b[c] = (float)bv;
    c0[c] = (float)(-av * s1 / n - bv * m);
    g_gamma[c] = (float)sg;
    g_beta[c] = (float)s1;
}

// ---- 16 bytes per lane -------------------------------------------------------------------------------------------------------------
// The element-wise passes of the training step (normalise + ReLU of the forward, the two passes of the BatchNorm / ReLU backward) are
// pure streams over [B][C][L] tensors; with 4-byte accesses per lane they ran at 3.0-4.3 TB/s (and the statistics pass paid a 64-bit
// division per element for its flat index).  Same arithmetic per element, 16 bytes per lane and access (4 f32 / 8 bf16), one (b, c) row
// segment per workgroup: used whenever the rows are 16-byte aligned (L % 4 == 0 resp. L % 8 == 0); the scalar kernels above remain for the rest.
__device__ __forceinline__ uint4 nt_load16(const uint4 *p) {
    const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(p));
    return make_uint4(v[0], v[1], v[2], v[3]);
}
template <bool BF> struct VecIO;
template <> struct VecIO<false> {                              // f32: 4 elements per 16 bytes
    static constexpr int N = 4;
    static __device__ __forceinline__ void unpack(const uint4 &d, float (&v)[4]) {
        v[0] = __uint_as_float(d.x); v[1] = __uint_as_float(d.y); v[2] = __uint_as_float(d.z); v[3] = __uint_as_float(d.w);
    }
    static __device__ __forceinline__ uint4 pack(const float (&v)[4]) {
        return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    }
};
template <> struct VecIO<true> {                               // bf16: 8 elements per 16 bytes
    static constexpr int N = 8;
    static __device__ __forceinline__ void unpack(const uint4 &d, float (&v)[8]) {
        v[0] = bf_lo(d.x); v[1] = bf_hi(d.x); v[2] = bf_lo(d.y); v[3] = bf_hi(d.y);
        v[4] = bf_lo(d.z); v[5] = bf_hi(d.z); v[6] = bf_lo(d.w); v[7] = bf_hi(d.w);
    }
    static __device__ __forceinline__ uint4 pack(const float (&v)[8]) {
        return make_uint4(cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7]));
    }
};

// MODE 0: out = act(x * scale + shift); MODE 1: out = a * (gy * mask) + b * raw + c0 (as rowwise_kernel).  grid (rows, ysplit)
template <int MODE, bool BF>
__global__ __launch_bounds__(256) void rowwise_vec_kernel(const uint4 *__restrict__ gy, const uint4 *__restrict__ raw,
                                                           const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                           const float *__restrict__ ca, const float *__restrict__ cb,
                                                           const float *__restrict__ cc, uint4 *__restrict__ out, int C, int Lv)
{
    constexpr int N = VecIO<BF>::N;
    const long long row = blockIdx.x;
    const int c = (int)(row % C);
    const float sc = scale[c], sh = shift[c];
    const float a = MODE == 1 ? ca[c] : 0.f, b = MODE == 1 ? cb[c] : 0.f, c0 = MODE == 1 ? cc[c] : 0.f;
    const uint4 *r = raw + row * Lv, *g = MODE == 1 ? gy + row * Lv : nullptr;
    uint4 *o = out + row * Lv;
    for (int t = blockIdx.y * 256 + threadIdx.x; t < Lv; t += gridDim.y * 256) {
        float rv[N], gv[N], ov[N];
        VecIO<BF>::unpack(nt_load16(r + t), rv);
        if constexpr (MODE == 1) VecIO<BF>::unpack(nt_load16(g + t), gv);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            if constexpr (MODE == 0) ov[e] = affine_act(rv[e], sc, sh, relu);
            else ov[e] = bn_bwd_apply(gv[e], rv[e], sc, sh, relu, a, b, c0);
        }
        o[t] = VecIO<BF>::pack(ov);
    }
}

// per-channel (sum of gy * mask, sum of gy * mask * raw), or with raw == nullptr (sum of gy, sum of gy^2): grid (segments, C, B);
// f64 accumulation per access as below, one pair of f64 atomics per workgroup
constexpr int SV_BG = 8;                       // clouds per workgroup of the statistics pass
template <bool BF>
__global__ __launch_bounds__(256) void stats_vec_kernel(const uint4 *__restrict__ gy, const uint4 *__restrict__ raw,
                                                         const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                         int B, int bg /*clouds per workgroup*/, int C, int Lv, double *__restrict__ ws)
{
    constexpr int N = VecIO<BF>::N;
    const int c = blockIdx.y;
    const float sc = raw ? scale[c] : 0.f, sh = raw ? shift[c] : 0.f;
    double s1 = 0.0, s2 = 0.0;
    // a workgroup walks its segment of the channel's row in bg (= SV_BG on big launches) clouds: one wave reduction + one pair of f64 atomics per ~240 KB
    // instead of per 30 KB (a workgroup per (segment, channel, cloud) ran at 3.0 TB/s on the bf16 step's tensors)
    for (int bb = blockIdx.z * bg; bb < min(B, (int)(blockIdx.z + 1) * bg); ++bb) {
    const long long row = (long long)bb * C + c;
    const uint4 *g = gy + row * Lv, *r = raw ? raw + row * Lv : nullptr;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < Lv; t += gridDim.x * 256) {
        float gv[N], rv[N];
        VecIO<BF>::unpack(nt_load16(g + t), gv);
        if (raw) VecIO<BF>::unpack(nt_load16(r + t), rv);
        // the N values of one access are summed in f32 (pairwise), then carried in f64: N x fewer f64 operations (they run at half the
        // f32 rate and were what bounded the bf16 pass: 3.0 TB/s), error <= N 2^-24 of one access's partial
        float p1[N], p2[N];
#pragma unroll
        for (int e = 0; e < N; ++e) {
            if (raw) {
                p1[e] = relu_masked(gv[e], rv[e], sc, sh, relu);
                p2[e] = p1[e] * rv[e];
            } else {
                p1[e] = gv[e];
                p2[e] = gv[e] * gv[e];
            }
        }
#pragma unroll
        for (int w = N / 2; w > 0; w >>= 1)
#pragma unroll
            for (int e = 0; e < w; ++e) { p1[e] += p1[e + w]; p2[e] += p2[e + w]; }
        s1 += (double)p1[0];
        s2 += (double)p2[0];
    }
    }
    // (not block_sum2_atomic: the four waves are combined PAIRWISE here, another summation order than the scalar kernels' chain --
    //  the sums the bit-identity tests and the training step see depend on it, so it stays)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    __shared__ double red[2][4];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsafeAtomicAdd(&ws[c], (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
        unsafeAtomicAdd(&ws[C + c], (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    }
}

}  // namespace

// ---- host: which flavour a shape gets -----------------------------------------------------------------------------------------------
static bool vec_ok(int L, int elem_bytes, const void *p0, const void *p1, const void *p2)
{
    return ((long long)L * elem_bytes) % 16 == 0 && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) == 0;
}
static bool bf_pair_ok(int L, const void *p0, const void *p1, const void *p2)
{
    return (L % 2 == 0) && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 3) == 0;
}
// workgroups per channel of the scalar statistics kernels: one per 16384 elements, 1 .. 64
static int stats_chunks(int B, int L)
{
    const int chunks = (int)sonet::ceil_div64((long long)B * L, 16384);
    return chunks < 1 ? 1 : (chunks > 64 ? 64 : chunks);
}
// gridDim.y of the scalar row kernels: one workgroup per 2048 elements of a row, at most `cap` (0: no cap)
static int row_ysplit(int L, int cap)
{
    const int ys = sonet::ceil_div(L, 256 * 8);
    return ys < 1 ? 1 : (cap > 0 && ys > cap ? cap : ys);
}

// One row pass (MODE as rowwise_kernel; MODE 0: gy, a, b, c0 are NULL) over `rows` = B C rows: vec, else (bf16) pair, else scalar.
// ycap: the cap of the scalar / pair grid's y (the vec grid is always capped at 16).
template <int MODE, typename T>
static void launch_rowwise(const T *gy, const T *raw, const float *scale, const float *shift, int relu, const float *a, const float *b,
                           const float *c0, T *out, long long rows, int C, int L, int ycap, hipStream_t st)
{
    constexpr bool BF = sizeof(T) == 2;
    if (vec_ok(L, sizeof(T), gy, raw, out)) {
        const int Lv = (int)((long long)L * sizeof(T) / 16);
        int ys = sonet::ceil_div(Lv, 256 * 4);
        ys = ys < 1 ? 1 : (ys > 16 ? 16 : ys);
        hipLaunchKernelGGL((rowwise_vec_kernel<MODE, BF>), dim3((unsigned)rows, (unsigned)ys), dim3(256), 0, st, reinterpret_cast<const uint4 *>(gy),
                           reinterpret_cast<const uint4 *>(raw), scale, shift, relu, a, b, c0, reinterpret_cast<uint4 *>(out), C, Lv);
        return;
    }
    const dim3 grid((unsigned)rows, (unsigned)row_ysplit(L, ycap));
    if constexpr (BF) {
        if (bf_pair_ok(L, gy, raw, out)) {
            hipLaunchKernelGGL((rowwise_kernel<MODE, T, true>), grid, dim3(256), 0, st, gy, raw, scale, shift, relu, a, b, c0, out, C, L);
            return;
        }
    }
    hipLaunchKernelGGL((rowwise_kernel<MODE, T, false>), grid, dim3(256), 0, st, gy, raw, scale, shift, relu, a, b, c0, out, C, L);
}

// One statistics pass into sums[2 C] (zeroed by the caller; raw, scale, shift NULL: sum and sum of squares of gy): vec when `vec`
// allows it and the grid's z fits, else (bf16) pair, else scalar.
template <typename T>
static void launch_stats(const T *gy, const T *raw, const float *scale, const float *shift, int relu, int B, int C, int L, double *sums,
                         bool vec, hipStream_t st)
{
    constexpr bool BF = sizeof(T) == 2;
    if (vec && vec_ok(L, sizeof(T), gy, raw, nullptr) && B <= 65535) {
        const int Lv = (int)((long long)L * sizeof(T) / 16);
        int seg = sonet::ceil_div(Lv, 256 * 4);
        seg = seg < 1 ? 1 : (seg > 8 ? 8 : seg);
        // (small launches keep one cloud per workgroup: the grid must still fill the chip)
        const int bg = (long long)seg * C * sonet::ceil_div(B, SV_BG) >= 2048 ? SV_BG : 1;
        hipLaunchKernelGGL((stats_vec_kernel<BF>), dim3((unsigned)seg, (unsigned)C, (unsigned)sonet::ceil_div(B, bg)), dim3(256), 0, st,
                           reinterpret_cast<const uint4 *>(gy), reinterpret_cast<const uint4 *>(raw), scale, shift, relu, B, bg, C, Lv, sums);
        return;
    }
    const dim3 grid(stats_chunks(B, L), C);
    auto scalar = [&](auto pair, auto has_raw) {
        hipLaunchKernelGGL((stats_scalar_kernel<T, pair.value, has_raw.value>), grid, dim3(BW_THREADS), 0, st, gy, raw, scale, shift, relu, B, C, L, sums);
    };
    auto by_raw = [&](auto pair) { if (raw) scalar(pair, bool_c<true>{}); else scalar(pair, bool_c<false>{}); };
    if constexpr (BF) {
        if (bf_pair_ok(L, gy, raw, nullptr)) return by_raw(bool_c<true>{});
    }
    by_raw(bool_c<false>{});
}

static void launch_zero_sums(double *sums, int C, hipStream_t st)
{
    hipLaunchKernelGGL(bwd_ws_zero_kernel, dim3(sonet::ceil_div(2 * C, 256)), dim3(256), 0, st, sums, 2 * C);
}
static void launch_finalize(const double *sums, int B, int C, int L, float *mean, float *var, hipStream_t st)
{
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(sonet::ceil_div(C, 256)), dim3(256), 0, st, sums, C, 1.0 / ((double)B * L), mean, var,
                       sonet::take_bn_rider());
}

// ---- entry points: the f32 and the bf16 twin of a pass check and refuse differently, and the recorded dispatch (tests/golden/launch, section
// "bn passes") holds every difference below; each is DELIBERATELY kept as it is, not an oversight to be unified ----

extern "C" int sonet_channel_stats_f32(const float *y, int B, int C, int L, double *stat_ws, float *mean,
                                       float *var_biased, sonet_stream_t stream)
{
    const char *what = "sonet_channel_stats_f32";
    SONET_REQUIRE(y && stat_ws && mean && var_biased, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0, "%s: non-positive size", what);
    if (C > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: C=%d > 65535", what, C);      // (f32: a refusal of its own; bf16: part of "bad size")
    hipStream_t st = sonet::as_stream(stream);
    if (hipMemsetAsync(stat_ws, 0, (size_t)2 * C * sizeof(double), st) != hipSuccess)            // (f32: a memset; every other pass: the zeroing kernel)
        return sonet::fail(SONET_ERR_LAUNCH, "%s: hipMemsetAsync failed", what);
    launch_stats<float>(y, nullptr, nullptr, nullptr, 0, B, C, L, stat_ws, /*vec=*/false, st);   // (no 16-byte path: bn_passes_ref.stats_tol holds it to the scalar arithmetic)
    launch_finalize(stat_ws, B, C, L, mean, var_biased, st);
    return sonet::launched(what);
}

extern "C" int sonet_channel_stats_bf16(const uint16_t *y, int B, int C, int L, double *sums, float *mean, float *var, sonet_stream_t stream)
{
    const char *what = "sonet_channel_stats_bf16";
    SONET_REQUIRE(y && sums && mean && var, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && C <= 65535, "%s: bad size", what);
    hipStream_t st = sonet::as_stream(stream);
    launch_zero_sums(sums, C, st);
    launch_stats<uint16_t>(y, nullptr, nullptr, nullptr, 0, B, C, L, sums, true, st);
    launch_finalize(sums, B, C, L, mean, var, st);
    return sonet::launched(what);
}

extern "C" int sonet_pointwise_bwd_stats_f32(const float *gy, const float *raw, const float *scale, const float *shift,
                                             int relu, int B, int C, int L, double *sums, sonet_stream_t stream)
{
    const char *what = "sonet_pointwise_bwd_stats_f32";
    SONET_REQUIRE(gy && raw && scale && shift && sums, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && C <= 65535, "%s: bad size B=%d C=%d L=%d", what, B, C, L);   // (f32 names the sizes, bf16 does not)
    hipStream_t st = sonet::as_stream(stream);
    launch_zero_sums(sums, C, st);
    launch_stats<float>(gy, raw, scale, shift, relu, B, C, L, sums, true, st);
    return sonet::launched(what);
}

extern "C" int sonet_pointwise_bwd_stats_bf16(const uint16_t *gy, const uint16_t *raw, const float *scale, const float *shift,
                                              int relu, int B, int C, int L, double *sums, sonet_stream_t stream)
{
    const char *what = "sonet_pointwise_bwd_stats_bf16";
    SONET_REQUIRE(gy && raw && scale && shift && sums, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && C <= 65535, "%s: bad size", what);
    hipStream_t st = sonet::as_stream(stream);
    launch_zero_sums(sums, C, st);
    launch_stats<uint16_t>(gy, raw, scale, shift, relu, B, C, L, sums, true, st);
    return sonet::launched(what);
}

// (the scalar f32 row grids are uncapped in y, the bf16 ones stop at 16: they part at L > 32768.  "Too many rows" is an invalid argument
//  in f32 -- inside "bad size" for the forward pass -- and SONET_ERR_UNSUPPORTED in bf16.)
constexpr int ROW_YCAP_F32 = 0, ROW_YCAP_BF16 = 16;

extern "C" int sonet_pointwise_bwd_apply_f32(const float *gy, const float *raw, const float *scale, const float *shift, int relu,
                                             const float *a, const float *b, const float *c0, float *g_raw,
                                             int B, int C, int L, sonet_stream_t stream)
{
    const char *what = "sonet_pointwise_bwd_apply_f32";
    SONET_REQUIRE(gy && raw && scale && shift && a && b && c0 && g_raw, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0, "%s: bad size B=%d C=%d L=%d", what, B, C, L);
    const long long rows = (long long)B * C;
    SONET_REQUIRE(rows <= 2147483647LL, "%s: too many rows", what);
    launch_rowwise<1, float>(gy, raw, scale, shift, relu, a, b, c0, g_raw, rows, C, L, ROW_YCAP_F32, sonet::as_stream(stream));
    return sonet::launched(what);
}

extern "C" int sonet_pointwise_bwd_apply_bf16(const uint16_t *gy, const uint16_t *raw, const float *scale, const float *shift, int relu,
                                              const float *a, const float *b, const float *c0, uint16_t *g_raw, int B, int C, int L,
                                              sonet_stream_t stream)
{
    const char *what = "sonet_pointwise_bwd_apply_bf16";
    SONET_REQUIRE(gy && raw && scale && shift && a && b && c0 && g_raw, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0, "%s: bad size", what);
    const long long rows = (long long)B * C;
    if (rows > 0x7FFFFFFFll) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: too many rows", what);
    launch_rowwise<1, uint16_t>(gy, raw, scale, shift, relu, a, b, c0, g_raw, rows, C, L, ROW_YCAP_BF16, sonet::as_stream(stream));
    return sonet::launched(what);
}

extern "C" int sonet_channel_affine_act_out_f32(const float *x, const float *scale, const float *shift, int relu, float *y,
                                                int B, int C, int L, sonet_stream_t stream)
{
    const char *what = "sonet_channel_affine_act_out_f32";
    SONET_REQUIRE(x && scale && shift && y, "%s: NULL pointer", what);
    const long long rows = (long long)B * C;
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && rows <= 2147483647LL, "%s: bad size B=%d C=%d L=%d", what, B, C, L);
    launch_rowwise<0, float>(nullptr, x, scale, shift, relu, nullptr, nullptr, nullptr, y, rows, C, L, ROW_YCAP_F32, sonet::as_stream(stream));
    return sonet::launched(what);
}

extern "C" int sonet_channel_affine_act_out_bf16(const uint16_t *x, const float *scale, const float *shift, int relu, uint16_t *y,
                                                 int B, int C, int L, sonet_stream_t stream)
{
    const char *what = "sonet_channel_affine_act_out_bf16";
    SONET_REQUIRE(x && scale && shift && y, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0, "%s: bad size", what);
    const long long rows = (long long)B * C;
    if (rows > 0x7FFFFFFFll) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: too many rows", what);
    launch_rowwise<0, uint16_t>(nullptr, x, scale, shift, relu, nullptr, nullptr, nullptr, y, rows, C, L, ROW_YCAP_BF16, sonet::as_stream(stream));
    return sonet::launched(what);
}

extern "C" int sonet_channel_affine_act_f32(float *y, const float *scale, const float *shift, int relu,
                                            int B, int C, int L, sonet_stream_t stream)
{
    const char *what = "sonet_channel_affine_act_f32";
    SONET_REQUIRE(y && scale && shift, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0, "%s: non-positive size", what);
    const long long total = (long long)B * C * L;
    long long blocks = sonet::ceil_div64(total, 256);
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(channel_affine_act_kernel, dim3((unsigned)blocks), dim3(256), 0, sonet::as_stream(stream),
                       y, scale, shift, relu, C, L, total);
    return sonet::launched(what);
}

extern "C" int sonet_bn_fwd_coeffs_f32(const float *mean, const float *var, const float *gamma, const float *beta, float eps, int C,
                                       float *invstd, float *scale, float *shift, sonet_stream_t stream)
{
    const char *what = "sonet_bn_fwd_coeffs_f32";
    SONET_REQUIRE(mean && var && gamma && beta && invstd && scale && shift, "%s: NULL pointer", what);
    SONET_REQUIRE(C > 0, "%s: bad size C=%d", what, C);
    hipLaunchKernelGGL(bn_fwd_coeffs_kernel, dim3(sonet::ceil_div(C, 256)), dim3(256), 0, sonet::as_stream(stream),
                       mean, var, gamma, beta, eps, C, invstd, scale, shift);
    return sonet::launched(what);
}

extern "C" int sonet_bn_running_update_f32(float *running_mean, float *running_var, const float *mean, const float *var,
                                          float momentum, float unbias, int C, sonet_stream_t stream)
{
    const char *what = "sonet_bn_running_update_f32";
    SONET_REQUIRE(running_mean && running_var && mean && var, "%s: NULL pointer", what);
    SONET_REQUIRE(C > 0, "%s: bad size C=%d", what, C);
    hipLaunchKernelGGL(bn_running_update_kernel, dim3(sonet::ceil_div(C, 256)), dim3(256), 0, sonet::as_stream(stream),
                       running_mean, running_var, mean, var, momentum, unbias, C);
    return sonet::launched(what);
}

extern "C" int sonet_bn_bwd_coeffs_f32(const double *sums, const float *mean, const float *invstd, const float *gamma, double n, int C,
                                       float *a, float *b, float *c0, float *g_gamma, float *g_beta, sonet_stream_t stream)
{
    const char *what = "sonet_bn_bwd_coeffs_f32";
    SONET_REQUIRE(sums && mean && invstd && gamma && a && b && c0 && g_gamma && g_beta, "%s: NULL pointer", what);
    SONET_REQUIRE(C > 0 && n > 0, "%s: bad size C=%d", what, C);
    hipLaunchKernelGGL(bn_bwd_coeffs_kernel, dim3(sonet::ceil_div(C, 256)), dim3(256), 0, sonet::as_stream(stream),
                       sums, mean, invstd, gamma, n, C, a, b, c0, g_gamma, g_beta);
    return sonet::launched(what);
}

extern "C" int sonet_node_add_affine_act_f32(float *t, const float *z, const int32_t *min_idx_i32, const float *scale,
                                             const float *shift, int relu, int B, int C, int L, int M, sonet_stream_t stream)
{
    const char *what = "sonet_node_add_affine_act_f32";
    SONET_REQUIRE(t && z && min_idx_i32 && scale && shift, "%s: NULL pointer", what);
    const long long rows = (long long)B * C;
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && M > 0 && M <= 8192 && rows <= 2147483647LL, "%s: bad size B=%d C=%d L=%d M=%d", what, B, C, L, M);
    int gy = sonet::ceil_div(L, 256 * 8);
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(node_add_affine_act_kernel, dim3((unsigned)rows, gy), dim3(256), (size_t)M * sizeof(float),
                       sonet::as_stream(stream), t, z, min_idx_i32, scale, shift, relu, C, L, M);
    return sonet::launched(what);
}

// node_gather_lead_kernel takes its quad path on L % 4 == 0 alone: 16-byte loads of gidx and lead, a 16-byte (f32) / 8-byte (bf16) store
static bool ngl_aligned(int L, int NL, const void *gidx, const void *lead, const void *out, unsigned out_align)
{
    if ((L & 3) != 0) return true;
    return (reinterpret_cast<uintptr_t>(gidx) & 15) == 0 && (NL == 0 || (reinterpret_cast<uintptr_t>(lead) & 15) == 0) &&
           (reinterpret_cast<uintptr_t>(out) & (out_align - 1)) == 0;
}

extern "C" int sonet_node_gather_lead_affine_act_f32(const float *z, const int32_t *gidx, const float *lead, const float *wl,
                                                     const float *scale, const float *shift, int relu, float *out,
                                                     int B, int C, int L, int M, int NL, sonet_stream_t stream)
{
    const char *what = "sonet_node_gather_lead_affine_act_f32";
    SONET_REQUIRE(z && gidx && scale && shift && out && (NL == 0 || (lead && wl)), "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && B <= 65535 && C > 0 && L > 0 && M > 0 && M <= 1024 && NL >= 0 && NL <= 4, "%s: bad size B=%d C=%d L=%d M=%d NL=%d", what, B, C, L, M, NL);
    SONET_REQUIRE(ngl_aligned(L, NL, gidx, lead, out, 16), "%s: gidx, lead and out must be 16-byte aligned when L %% 4 == 0 (misaligned)", what);
    hipLaunchKernelGGL(node_gather_lead_kernel<float>, dim3((unsigned)sonet::ceil_div(C, NGL_CH), (unsigned)B), dim3(NGL_THREADS), (size_t)NGL_CH * (M + 6) * sizeof(float),
                       sonet::as_stream(stream), z, gidx, lead, wl, scale, shift, relu, out, C, L, M, NL);
    return sonet::launched(what);
}

/* bf16 storage of z and out (bfloat16 bit patterns); lead, wl, scale, shift f32 */
extern "C" int sonet_node_gather_lead_affine_act_bf16(const uint16_t *z, const int32_t *gidx, const float *lead, const float *wl,
                                                      const float *scale, const float *shift, int relu, uint16_t *out,
                                                      int B, int C, int L, int M, int NL, sonet_stream_t stream)
{
    const char *what = "sonet_node_gather_lead_affine_act_bf16";
    SONET_REQUIRE(z && gidx && scale && shift && out && (NL == 0 || (lead && wl)), "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && B <= 65535 && C > 0 && L > 0 && M > 0 && M <= 1024 && NL >= 0 && NL <= 4, "%s: bad size B=%d C=%d L=%d M=%d NL=%d", what, B, C, L, M, NL);
    SONET_REQUIRE(ngl_aligned(L, NL, gidx, lead, out, 8), "%s: gidx and lead must be 16-byte, out 8-byte aligned when L %% 4 == 0 (misaligned)", what);
    hipLaunchKernelGGL(node_gather_lead_kernel<uint16_t>, dim3((unsigned)sonet::ceil_div(C, NGL_CH), (unsigned)B), dim3(NGL_THREADS), (size_t)NGL_CH * (M + 6) * sizeof(float),
                       sonet::as_stream(stream), z, gidx, lead, wl, scale, shift, relu, out, C, L, M, NL);
    return sonet::launched(what);
}
