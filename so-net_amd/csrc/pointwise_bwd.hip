// pointwise_bwd.hip -- backward of act(BN(W x + b)) around the GEMMs (training, configs 2 / 5).
//
// Replaces the autograd graph the reference builds for models/layers.py:282-296 (conv1d -> F.batch_norm ->
// relu): two passes over (gy, raw) instead of ~20 element-wise aten launches over B x C x L tensors.
//   pass 1  per channel:  s1 = sum gy*mask,  s2 = sum gy*mask*raw      (f64 accumulation, as channel_stats)
//   pass 2  g_raw = a[c] * (gy*mask) + b[c] * raw + c0[c]
// with mask = (fma(raw, scale[c], shift[c]) > 0) when the layer has a ReLU (bit-identical to the forward's
// affine), else 1.  The host turns (s1, s2) into (a, b, c0) -- for training BatchNorm
//   a = gamma*invstd,  b = -a*invstd*sg/n,  c0 = -a*s1/n - b*mean,  sg = invstd*(s2 - mean*s1)
// (the usual  gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)) ), for a constant affine a = scale, b = c0 = 0.
// The GEMMs themselves (dgrad = W^T g_raw on the pointmlp kernels, wgrad = g_raw x^T) are launched by the host.
#include "common.hpp"

#include <hip/hip_runtime.h>

namespace {

constexpr int BW_THREADS = 256;

__global__ __launch_bounds__(BW_THREADS) void bwd_stats_kernel(const float *__restrict__ gy, const float *__restrict__ raw,
                                                                const float *__restrict__ scale, const float *__restrict__ shift,
                                                                int relu, int B, int C, int L, double *__restrict__ ws)
{
    const int c = blockIdx.y;
    const long long per_c = (long long)B * L;
    const long long chunk = (per_c + gridDim.x - 1) / gridDim.x;
    const long long beg = (long long)blockIdx.x * chunk, end = min(per_c, beg + chunk);
    const float sc = scale[c], sh = shift[c];
    double s1 = 0.0, s2 = 0.0;
    for (long long t = beg + threadIdx.x; t < end; t += BW_THREADS) {
        const long long b = t / L;
        const long long o = (b * C + c) * (long long)L + (t - b * L);
        const float r = raw[o];
        float g = gy[o];
        if (relu && !(__fmaf_rn(r, sc, sh) > 0.f)) g = 0.f;
        s1 += (double)g;
        s2 += (double)g * (double)r;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    __shared__ double red[2][BW_THREADS / 64];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, a2 = 0.0;
        for (int w = 0; w < BW_THREADS / 64; ++w) { a += red[0][w]; a2 += red[1][w]; }
        unsafeAtomicAdd(&ws[c], a);
        unsafeAtomicAdd(&ws[C + c], a2);
    }
}

__global__ __launch_bounds__(256) void bwd_ws_zero_kernel(double *ws, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) ws[i] = 0.0;
}

// one workgroup row = one (b, c) row of L elements: coefficients are wave-uniform
__global__ __launch_bounds__(256) void bwd_apply_kernel(const float *__restrict__ gy, const float *__restrict__ raw,
                                                         const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                         const float *__restrict__ ca, const float *__restrict__ cb,
                                                         const float *__restrict__ cc, float *__restrict__ out, int C, int L)
{
    const long long row = blockIdx.x;
    const int c = (int)(row % C);
    const float sc = scale[c], sh = shift[c], a = ca[c], b = cb[c], c0 = cc[c];
    const float *g = gy + row * L, *r = raw + row * L;
    float *o = out + row * L;
    for (int t = blockIdx.y * 256 + threadIdx.x; t < L; t += gridDim.y * 256) {
        const float rv = r[t];
        float gv = g[t];
        if (relu && !(__fmaf_rn(rv, sc, sh) > 0.f)) gv = 0.f;
        o[t] = __fmaf_rn(a, gv, __fmaf_rn(b, rv, c0));
    }
}

__global__ __launch_bounds__(256) void affine_act_out_kernel(const float *__restrict__ x, const float *__restrict__ scale,
                                                              const float *__restrict__ shift, int relu, float *__restrict__ y,
                                                              int C, int L)
{
    const long long row = blockIdx.x;
    const int c = (int)(row % C);
    const float sc = scale[c], sh = shift[c];
    const float *xi = x + row * L;
    float *yo = y + row * L;
    for (int t = blockIdx.y * 256 + threadIdx.x; t < L; t += gridDim.y * 256) {
        float v = __fmaf_rn(xi[t], sc, sh);
        if (relu) v = (v < 0.f) ? 0.f : v;
        yo[t] = v;
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
        float v = tr[l] + ((unsigned)m < (unsigned)M ? zrow[m] : 0.f);
        v = __fmaf_rn(v, sc, sh);
        if (relu) v = (v < 0.f) ? 0.f : v;
        tr[l] = v;
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

// ---- bf16 twins of the element-wise passes (BASELINE configs[1]: bf16 training): same arithmetic in f32 / f64 on values
// widened from bf16, results rounded to nearest-even bf16.  Two elements (one dword) per lane when the rows are dword aligned.
__device__ __forceinline__ float bf_lo(unsigned d) { return __uint_as_float(d << 16); }
__device__ __forceinline__ float bf_hi(unsigned d) { return __uint_as_float(d & 0xFFFF0000u); }

// grid (chunks, C) as bwd_stats_kernel / channel_stats_kernel; raw == nullptr: plain statistics of gy (sum, sum of squares)
template <bool PAIR>
__global__ __launch_bounds__(BW_THREADS) void bwd_stats_bf16_kernel(const uint16_t *__restrict__ gy, const uint16_t *__restrict__ raw,
                                                                     const float *__restrict__ scale, const float *__restrict__ shift,
                                                                     int relu, int B, int C, int L, double *__restrict__ ws)
{
    const int c = blockIdx.y;
    constexpr int V = PAIR ? 2 : 1;
    const int Lv = L / V;
    const long long per_c = (long long)B * Lv;
    const long long chunk = (per_c + gridDim.x - 1) / gridDim.x;
    const long long beg = (long long)blockIdx.x * chunk, end = min(per_c, beg + chunk);
    const float sc = raw ? scale[c] : 0.f, sh = raw ? shift[c] : 0.f;
    double s1 = 0.0, s2 = 0.0;
    for (long long t = beg + threadIdx.x; t < end; t += BW_THREADS) {
        const long long b = t / Lv;
        const long long o = (b * C + c) * (long long)L + (t - b * Lv) * V;
        float g[V], r[V];
        if constexpr (PAIR) {
            const unsigned dg = *reinterpret_cast<const unsigned *>(gy + o);
            g[0] = bf_lo(dg); g[1] = bf_hi(dg);
            if (raw) { const unsigned dr = *reinterpret_cast<const unsigned *>(raw + o); r[0] = bf_lo(dr); r[1] = bf_hi(dr); }
        } else {
            g[0] = ld_f32(gy, o);
            if (raw) r[0] = ld_f32(raw, o);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (raw) {
                float gv = g[v];
                if (relu && !(__fmaf_rn(r[v], sc, sh) > 0.f)) gv = 0.f;
                s1 += (double)gv;
                s2 += (double)gv * (double)r[v];
            } else {
                s1 += (double)g[v];
                s2 += (double)g[v] * (double)g[v];
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    __shared__ double red[2][BW_THREADS / 64];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, a2 = 0.0;
        for (int w = 0; w < BW_THREADS / 64; ++w) { a += red[0][w]; a2 += red[1][w]; }
        unsafeAtomicAdd(&ws[c], a);
        unsafeAtomicAdd(&ws[C + c], a2);
    }
}

// one workgroup row = one (b, c) row.  MODE 0: out = act(x * scale + shift) (forward normalise + ReLU);
// MODE 1: out = a * (gy * mask) + b * raw + c0 with mask from (raw, scale, shift) (backward apply).
template <int MODE, bool PAIR>
__global__ __launch_bounds__(256) void rowwise_bf16_kernel(const uint16_t *__restrict__ gy, const uint16_t *__restrict__ raw,
                                                            const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                            const float *__restrict__ ca, const float *__restrict__ cb,
                                                            const float *__restrict__ cc, uint16_t *__restrict__ out, int C, int L)
{
    const long long row = blockIdx.x;
    const int c = (int)(row % C);
    const float sc = scale[c], sh = shift[c];
    const float a = MODE == 1 ? ca[c] : 0.f, b = MODE == 1 ? cb[c] : 0.f, c0 = MODE == 1 ? cc[c] : 0.f;
    const uint16_t *r = raw + row * L, *g = MODE == 1 ? gy + row * L : nullptr;
    uint16_t *o = out + row * L;
    auto f = [&](float rv, float gv) {
        if constexpr (MODE == 0) {
            float v = __fmaf_rn(rv, sc, sh);
            if (relu) v = (v < 0.f) ? 0.f : v;
            return v;
        } else {
            if (relu && !(__fmaf_rn(rv, sc, sh) > 0.f)) gv = 0.f;
            return __fmaf_rn(a, gv, __fmaf_rn(b, rv, c0));
        }
    };
    if constexpr (PAIR) {
        const int Lv = L >> 1;
        for (int t = blockIdx.y * 256 + threadIdx.x; t < Lv; t += gridDim.y * 256) {
            const unsigned dr = reinterpret_cast<const unsigned *>(r)[t];
            const unsigned dg = MODE == 1 ? reinterpret_cast<const unsigned *>(g)[t] : 0u;
            reinterpret_cast<unsigned *>(o)[t] = cvt_pk_bf16(f(bf_lo(dr), bf_lo(dg)), f(bf_hi(dr), bf_hi(dg)));
        }
    } else {
        for (int t = blockIdx.y * 256 + threadIdx.x; t < L; t += gridDim.y * 256)
            o[t] = (uint16_t)(cvt_pk_bf16(f(ld_f32(r, t), MODE == 1 ? ld_f32(g, t) : 0.f), 0.f) & 0xFFFFu);
    }
}

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
    if (rd.gamma != nullptr) {                                  // (BatchNorm rider: bn_fwd_coeffs_kernel + bn_running_update_kernel below, operation for operation)
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

}  // namespace


namespace {
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

// MODE 0: out = act(x * scale + shift); MODE 1: out = a * (gy * mask) + b * raw + c0 (as rowwise_bf16_kernel / bwd_apply_kernel).  grid (rows, ysplit)
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
            if constexpr (MODE == 0) {
                float v = __fmaf_rn(rv[e], sc, sh);
                if (relu) v = (v < 0.f) ? 0.f : v;
                ov[e] = v;
            } else {
                float gg = gv[e];
                if (relu && !(__fmaf_rn(rv[e], sc, sh) > 0.f)) gg = 0.f;
                ov[e] = __fmaf_rn(a, gg, __fmaf_rn(b, rv[e], c0));
            }
        }
        o[t] = VecIO<BF>::pack(ov);
    }
}

// per-channel (sum of gy * mask, sum of gy * mask * raw), or with raw == nullptr (sum of gy, sum of gy^2): grid (segments, C, B);
// f64 accumulation per element as in the scalar kernels, one pair of f64 atomics per workgroup
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
                float gg = gv[e];
                if (relu && !(__fmaf_rn(rv[e], sc, sh) > 0.f)) gg = 0.f;
                p1[e] = gg;
                p2[e] = gg * rv[e];
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

static bool vec_ok(int L, int elem_bytes, const void *p0, const void *p1, const void *p2)
{
    return ((long long)L * elem_bytes) % 16 == 0 && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) == 0;
}
template <int MODE, bool BF>
static void launch_rowwise_vec(const void *gy, const void *raw, const float *scale, const float *shift, int relu, const float *a, const float *b,
                               const float *c0, void *out, long long rows, int C, int L, hipStream_t st)
{
    const int Lv = (int)((long long)L * (BF ? 2 : 4) / 16);
    int ys = sonet::ceil_div(Lv, 256 * 4);
    ys = ys < 1 ? 1 : (ys > 16 ? 16 : ys);
    hipLaunchKernelGGL((rowwise_vec_kernel<MODE, BF>), dim3((unsigned)rows, (unsigned)ys), dim3(256), 0, st, reinterpret_cast<const uint4 *>(gy),
                       reinterpret_cast<const uint4 *>(raw), scale, shift, relu, a, b, c0, reinterpret_cast<uint4 *>(out), C, Lv);
}
template <bool BF>
static void launch_stats_vec(const void *gy, const void *raw, const float *scale, const float *shift, int relu, int B, int C, int L, double *sums,
                             hipStream_t st)
{
    const int Lv = (int)((long long)L * (BF ? 2 : 4) / 16);
    int seg = sonet::ceil_div(Lv, 256 * 4);
    seg = seg < 1 ? 1 : (seg > 8 ? 8 : seg);
    // (small launches keep one cloud per workgroup: the grid must still fill the chip)
    const int bg = (long long)seg * C * sonet::ceil_div(B, SV_BG) >= 2048 ? SV_BG : 1;
    hipLaunchKernelGGL((stats_vec_kernel<BF>), dim3((unsigned)seg, (unsigned)C, (unsigned)sonet::ceil_div(B, bg)), dim3(256), 0, st,
                       reinterpret_cast<const uint4 *>(gy), reinterpret_cast<const uint4 *>(raw), scale, shift, relu, B, bg, C, Lv, sums);
}
}  // namespace

static bool bf_pair_ok(int L, const void *p0, const void *p1, const void *p2)
{
    return (L % 2 == 0) && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 3) == 0;
}

// bf16 twins (raw bfloat16 bit patterns [B][C][L]); sums / coefficients stay f64 / f32 exactly as in the f32 entry points.
// sonet_channel_stats_bf16: raw == NULL in the stats kernel -> (sum, sum of squares) -> mean, biased variance.
extern "C" int sonet_pointwise_bwd_stats_bf16(const uint16_t *gy, const uint16_t *raw, const float *scale, const float *shift,
                                              int relu, int B, int C, int L, double *sums, sonet_stream_t stream)
{
    const char *what = "sonet_pointwise_bwd_stats_bf16";
    SONET_REQUIRE(gy && raw && scale && shift && sums, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && C <= 65535, "%s: bad size", what);
    hipStream_t st = sonet::as_stream(stream);
    hipLaunchKernelGGL(bwd_ws_zero_kernel, dim3(sonet::ceil_div(2 * C, 256)), dim3(256), 0, st, sums, 2 * C);
    const long long per_c = (long long)B * L;
    int chunks = (int)sonet::ceil_div64(per_c, 16384);
    chunks = chunks < 1 ? 1 : (chunks > 64 ? 64 : chunks);
    if (vec_ok(L, 2, gy, raw, nullptr) && B <= 65535) launch_stats_vec<true>(gy, raw, scale, shift, relu, B, C, L, sums, st);
    else if (bf_pair_ok(L, gy, raw, nullptr)) hipLaunchKernelGGL(bwd_stats_bf16_kernel<true>, dim3(chunks, C), dim3(BW_THREADS), 0, st, gy, raw, scale, shift, relu, B, C, L, sums);
    else hipLaunchKernelGGL(bwd_stats_bf16_kernel<false>, dim3(chunks, C), dim3(BW_THREADS), 0, st, gy, raw, scale, shift, relu, B, C, L, sums);
    return sonet::launched(what);
}

extern "C" int sonet_channel_stats_bf16(const uint16_t *y, int B, int C, int L, double *sums, float *mean, float *var, sonet_stream_t stream)
{
    const char *what = "sonet_channel_stats_bf16";
    SONET_REQUIRE(y && sums && mean && var, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && C <= 65535, "%s: bad size", what);
    hipStream_t st = sonet::as_stream(stream);
    hipLaunchKernelGGL(bwd_ws_zero_kernel, dim3(sonet::ceil_div(2 * C, 256)), dim3(256), 0, st, sums, 2 * C);
    const long long per_c = (long long)B * L;
    int chunks = (int)sonet::ceil_div64(per_c, 16384);
    chunks = chunks < 1 ? 1 : (chunks > 64 ? 64 : chunks);
    if (vec_ok(L, 2, y, nullptr, nullptr) && B <= 65535) launch_stats_vec<true>(y, nullptr, nullptr, nullptr, 0, B, C, L, sums, st);
    else if (bf_pair_ok(L, y, nullptr, nullptr)) hipLaunchKernelGGL(bwd_stats_bf16_kernel<true>, dim3(chunks, C), dim3(BW_THREADS), 0, st, y, (const uint16_t *)nullptr, (const float *)nullptr, (const float *)nullptr, 0, B, C, L, sums);
    else hipLaunchKernelGGL(bwd_stats_bf16_kernel<false>, dim3(chunks, C), dim3(BW_THREADS), 0, st, y, (const uint16_t *)nullptr, (const float *)nullptr, (const float *)nullptr, 0, B, C, L, sums);
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(sonet::ceil_div(C, 256)), dim3(256), 0, st, sums, C, 1.0 / ((double)B * L), mean, var, sonet::take_bn_rider());
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
    int ysplit = sonet::ceil_div(L, 256 * 8);
    ysplit = ysplit < 1 ? 1 : (ysplit > 16 ? 16 : ysplit);
    dim3 grid((unsigned)rows, (unsigned)ysplit);
    if (vec_ok(L, 2, gy, raw, g_raw)) launch_rowwise_vec<1, true>(gy, raw, scale, shift, relu, a, b, c0, g_raw, rows, C, L, sonet::as_stream(stream));
    else if (bf_pair_ok(L, gy, raw, g_raw)) hipLaunchKernelGGL((rowwise_bf16_kernel<1, true>), grid, dim3(256), 0, sonet::as_stream(stream), gy, raw, scale, shift, relu, a, b, c0, g_raw, C, L);
    else hipLaunchKernelGGL((rowwise_bf16_kernel<1, false>), grid, dim3(256), 0, sonet::as_stream(stream), gy, raw, scale, shift, relu, a, b, c0, g_raw, C, L);
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
    int ysplit = sonet::ceil_div(L, 256 * 8);
    ysplit = ysplit < 1 ? 1 : (ysplit > 16 ? 16 : ysplit);
    dim3 grid((unsigned)rows, (unsigned)ysplit);
    if (vec_ok(L, 2, x, y, nullptr)) launch_rowwise_vec<0, true>(nullptr, x, scale, shift, relu, nullptr, nullptr, nullptr, y, rows, C, L, sonet::as_stream(stream));
    else if (bf_pair_ok(L, x, y, nullptr)) hipLaunchKernelGGL((rowwise_bf16_kernel<0, true>), grid, dim3(256), 0, sonet::as_stream(stream), (const uint16_t *)nullptr, x, scale, shift, relu, (const float *)nullptr, (const float *)nullptr, (const float *)nullptr, y, C, L);
    else hipLaunchKernelGGL((rowwise_bf16_kernel<0, false>), grid, dim3(256), 0, sonet::as_stream(stream), (const uint16_t *)nullptr, x, scale, shift, relu, (const float *)nullptr, (const float *)nullptr, (const float *)nullptr, y, C, L);
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

extern "C" int sonet_pointwise_bwd_stats_f32(const float *gy, const float *raw, const float *scale, const float *shift,
                                             int relu, int B, int C, int L, double *sums, sonet_stream_t stream)
{
    const char *what = "sonet_pointwise_bwd_stats_f32";
    SONET_REQUIRE(gy && raw && scale && shift && sums, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && C <= 65535, "%s: bad size B=%d C=%d L=%d", what, B, C, L);
    hipStream_t st = sonet::as_stream(stream);
    hipLaunchKernelGGL(bwd_ws_zero_kernel, dim3(sonet::ceil_div(2 * C, 256)), dim3(256), 0, st, sums, 2 * C);
    const long long per_c = (long long)B * L;
    int chunks = (int)sonet::ceil_div64(per_c, 16384);
    if (chunks < 1) chunks = 1;
    if (chunks > 64) chunks = 64;
    if (vec_ok(L, 4, gy, raw, nullptr) && B <= 65535) launch_stats_vec<false>(gy, raw, scale, shift, relu, B, C, L, sums, st);
    else hipLaunchKernelGGL(bwd_stats_kernel, dim3(chunks, C), dim3(BW_THREADS), 0, st, gy, raw, scale, shift, relu, B, C, L, sums);
    return sonet::launched(what);
}

extern "C" int sonet_pointwise_bwd_apply_f32(const float *gy, const float *raw, const float *scale, const float *shift, int relu,
                                             const float *a, const float *b, const float *c0, float *g_raw,
                                             int B, int C, int L, sonet_stream_t stream)
{
    const char *what = "sonet_pointwise_bwd_apply_f32";
    SONET_REQUIRE(gy && raw && scale && shift && a && b && c0 && g_raw, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && L > 0, "%s: bad size B=%d C=%d L=%d", what, B, C, L);
    const long long rows = (long long)B * C;
    SONET_REQUIRE(rows <= 2147483647LL, "%s: too many rows", what);
    int gx = sonet::ceil_div(L, 256 * 8);
    if (gx < 1) gx = 1;
    if (vec_ok(L, 4, gy, raw, g_raw)) launch_rowwise_vec<1, false>(gy, raw, scale, shift, relu, a, b, c0, g_raw, rows, C, L, sonet::as_stream(stream));
    else hipLaunchKernelGGL(bwd_apply_kernel, dim3((unsigned)rows, gx), dim3(256), 0, sonet::as_stream(stream),
                            gy, raw, scale, shift, relu, a, b, c0, g_raw, C, L);
    return sonet::launched(what);
}

extern "C" int sonet_channel_affine_act_out_f32(const float *x, const float *scale, const float *shift, int relu, float *y,
                                                int B, int C, int L, sonet_stream_t stream)
{
    const char *what = "sonet_channel_affine_act_out_f32";
    SONET_REQUIRE(x && scale && shift && y, "%s: NULL pointer", what);
    const long long rows = (long long)B * C;
    SONET_REQUIRE(B > 0 && C > 0 && L > 0 && rows <= 2147483647LL, "%s: bad size B=%d C=%d L=%d", what, B, C, L);
    int gx = sonet::ceil_div(L, 256 * 8);
    if (gx < 1) gx = 1;
    if (vec_ok(L, 4, x, y, nullptr)) launch_rowwise_vec<0, false>(nullptr, x, scale, shift, relu, nullptr, nullptr, nullptr, y, rows, C, L, sonet::as_stream(stream));
    else hipLaunchKernelGGL(affine_act_out_kernel, dim3((unsigned)rows, gx), dim3(256), 0, sonet::as_stream(stream),
                            x, scale, shift, relu, y, C, L);
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

// ---- mean over the k copies of a point (segmenter head, models/networks.py:331-336) ----------------------------------------------
// out[r][n] = c * ((h[r][n] + h[r][N + n]) + h[r][2 N + n]),  h [rows][k N], c = 1/3 (k = 3) or 0.5 (k = 2), k = 1: copy -- the
// reference's own order of the adds and the single multiplication, so the result is bit-identical to the three aten launches it
// replaces (split + add + add + mul: ~0.1 ms of the segmenter's 1.9 ms at 64 x 256 x 3 x 1024).
namespace {
__global__ __launch_bounds__(256) void chunk_mean_kernel(const float *__restrict__ h, float *__restrict__ out, long long rows, int N, int k, float c)
{
    const long long r = blockIdx.y;
    const float *hr = h + r * (long long)k * N;
    float *orow = out + r * N;
    const bool vec = (N & 3) == 0 && ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    if (vec) {
        const float4 *h4 = reinterpret_cast<const float4 *>(hr);
        float4 *o4 = reinterpret_cast<float4 *>(orow);
        const int N4 = N >> 2;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < N4; i += gridDim.x * 256) {
            float4 s = h4[i];
            for (int kk = 1; kk < k; ++kk) {
                const float4 v = h4[(long long)kk * N4 + i];
                s.x = __fadd_rn(s.x, v.x); s.y = __fadd_rn(s.y, v.y); s.z = __fadd_rn(s.z, v.z); s.w = __fadd_rn(s.w, v.w);
            }
            if (k > 1) { s.x = __fmul_rn(c, s.x); s.y = __fmul_rn(c, s.y); s.z = __fmul_rn(c, s.z); s.w = __fmul_rn(c, s.w); }
            o4[i] = s;
        }
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
            float s = hr[i];
            for (int kk = 1; kk < k; ++kk) s = __fadd_rn(s, hr[(long long)kk * N + i]);
            orow[i] = k > 1 ? __fmul_rn(c, s) : s;
        }
    }
}
}  // namespace

extern "C" int sonet_chunk_mean_f32(const float *h, float *out, long long rows, int N, int k, sonet_stream_t stream)
{
    const char *what = "sonet_chunk_mean_f32";
    SONET_REQUIRE(h && out, "%s: NULL pointer", what);
    SONET_REQUIRE(rows > 0 && N > 0 && k >= 1, "%s: bad size", what);
    if (rows > 65535 * 32768ll || k > 3) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: rows=%lld k=%d", what, rows, k);
    if (rows > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: more than 65535 rows", what);
    const int gx = sonet::ceil_div(N, 1024) < 1 ? 1 : (sonet::ceil_div(N, 1024) > 8 ? 8 : sonet::ceil_div(N, 1024));
    hipLaunchKernelGGL(chunk_mean_kernel, dim3((unsigned)gx, (unsigned)rows), dim3(256), 0, sonet::as_stream(stream), h, out, rows, N, k,
                       k == 3 ? (float)(1.0 / 3.0) : 0.5f);
    return sonet::launched(what);
}

// ---- sparse dgrad of the pooled last layer ---------------------------------------------------
// In the classifier / autoencoder the only consumer of first_pn_out = W4 . [x1; x2] + b is the per-node max-pool
// (models/networks.py:180-185), so d loss / d first_pn_out has exactly M non-zeros per (b, c) row -- at the arg-max
// positions.  Instead of scattering them into a dense B x 384 x kN tensor and running a dense W4^T GEMM over it
// (234x more MACs than needed at N = 5000), the entries are bucketed by 64-column tile and every tile accumulates
//     g_x[b][:, l] += g[b][c][m] * W4[c][:]      for its entries (c, m) -> l
// in LDS, then writes its 320 x 64 block with coalesced stores (the [C][L] layout makes a direct scatter of the 320-vectors
// uncoalesced in both directions).  Entries of a tile are sorted by (column, channel) before they are applied, so the
// result does not depend on the order the bucket atomics happened to take.
namespace {

constexpr int PD_TL = 128;                     // columns per tile: 256-byte (bf16) / 512-byte (f32) row segments on the way out.  (Round 3: 32
                                               // columns x all 320 channels -- 64-byte bf16 row pieces, every one a partial cache line.)
constexpr int PD_CH = 40;                      // input channels per workgroup (blockIdx.z): 41 KB of accumulators
constexpr int PD_CQ = 4;                       // thread groups per channel: group q owns column quarter q of the tile ...
constexpr int PD_SB = PD_TL / PD_CQ;           // ... = one 32-column bucket of the entry lists (~52 entries at the benchmark shape)
constexpr int PD_WB = 16;                      // W rows requested before the first fma (64 -- a whole bucket in one round trip -- measured slower)
constexpr int PD_SQ = 128;                     // entries per group sorted in LDS at a time (more: further rounds, still in global rank order)

constexpr int PB_Q = 4;                        // workgroups per cloud: each owns a quarter of the bucket range (one per cloud left 3/4 of the chip idle)
__global__ __launch_bounds__(1024) void pooled_bucket_kernel(const int32_t *__restrict__ pos, const float *__restrict__ g,
                                                            int E, int L, int ntile, int32_t *__restrict__ tile_off,
                                                            uint32_t *__restrict__ ent_key, float *__restrict__ ent_val)
{
    extern __shared__ int sm_i[];                // cnt[nbq] | off[nbq + 1]   (nbq = buckets per workgroup)
    __shared__ int qtot[PB_Q];
    const int nbq = (ntile + PB_Q - 1) / PB_Q;
    int *cnt = sm_i, *off = sm_i + nbq;
    const int b = blockIdx.x, q = blockIdx.y;
    const int t0 = q * nbq, nb = max(0, min(ntile, t0 + nbq) - t0);              // this workgroup's buckets [t0, t0 + nb)
    const int32_t *pb = pos + (size_t)b * E;
    for (int t = threadIdx.x; t < nbq; t += 1024) cnt[t] = 0;
    if (threadIdx.x < PB_Q) qtot[threadIdx.x] = 0;
    __syncthreads();
    // pass 1: counts of the own buckets; entries per quarter (every workgroup counts all four: its base offset is the sum of the
    // quarters before it -- no exchange between workgroups), a thread's four counts meet in its wave first
    int mine[PB_Q];
#pragma unroll
    for (int k = 0; k < PB_Q; ++k) mine[k] = 0;
    for (int e = threadIdx.x; e < E; e += 1024) {
        const int l = pb[e];
        if ((unsigned)l >= (unsigned)L) continue;
        const int t = l / PD_SB, qq = t / nbq;
#pragma unroll
        for (int k = 0; k < PB_Q; ++k) mine[k] += (qq == k);
        if (qq == q) atomicAdd(&cnt[t - t0], 1);
    }
#pragma unroll
    for (int k = 0; k < PB_Q; ++k) {
        int v = mine[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&qtot[k], v);
    }
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int k = 0; k < PB_Q; ++k) base += k < q ? qtot[k] : 0;
    if (nb <= 1024) {
        // exclusive scan of the bucket counts by the whole workgroup (Hillis-Steele in LDS; one thread walking the buckets with an LDS
        // round trip each was a fifth of the kernel)
        const int t = threadIdx.x;
        if (t < nb) off[t + 1] = cnt[t];
        if (t == 0) off[0] = 0;
        __syncthreads();
        for (int d = 1; d < nb; d <<= 1) {
            const int v = (t < nb && t >= d) ? off[t + 1 - d] : 0;
            __syncthreads();
            if (t < nb) off[t + 1] += v;
            __syncthreads();
        }
        if (t < nb) cnt[t] = 0;
    } else if (threadIdx.x == 0) {
        int acc = 0;
        for (int t = 0; t < nb; ++t) { off[t] = acc; acc += cnt[t]; cnt[t] = 0; }
        off[nb] = acc;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nb; t += 1024) tile_off[(size_t)b * (ntile + 1) + t0 + t] = base + off[t];
    if (threadIdx.x == 0 && t0 + nb == ntile && nb > 0) tile_off[(size_t)b * (ntile + 1) + ntile] = base + off[nb];
    for (int e = threadIdx.x; e < E; e += 1024) {
        const int l = pb[e];
        if ((unsigned)l >= (unsigned)L) continue;
        const int t = l / PD_SB;
        if (t < t0 || t >= t0 + nb) continue;
        const int p = base + off[t - t0] + atomicAdd(&cnt[t - t0], 1);
        // sort key (column, entry id); entry id = c * M + m, the consumer recovers the channel as id / M
        ent_key[(size_t)b * E + p] = ((uint32_t)(l - t * PD_SB) << 20) | (uint32_t)e;
        ent_val[(size_t)b * E + p] = g[(size_t)b * E + e];
    }
}

// One wave per 32-column bucket: its entries sorted by (column, entry id) -- the keys are distinct -- into skey.  A histogram over the 32
// columns, the entries scattered into their column's segment of an LDS list (any order), every entry ranked among the entries of ITS
// column: position = segment start + rank.  nq * (entries of a column) compares instead of the nq * nq of a rank over the whole bucket
// -- on node-sorted columns (the f32-class training forward) a small node drops its 384 entries into one or two buckets, and ranking
// every entry against the whole bucket in every (bucket, channel slab) workgroup was 0.77 of the dgrad kernel's 1.73 ms there (0.34 of
// 1.23 ms in the original column order: tools/bench_pooled_sorted.py).  Buckets beyond PS_CAP entries: ranks over the whole bucket from
// global memory.  Either way one fixed order.
constexpr int PS_CAP = 2048;
__global__ __launch_bounds__(64) void pooled_sort_kernel(const int32_t *__restrict__ tile_off, const uint32_t *__restrict__ ent_key,
                                                         uint32_t *__restrict__ skey, int E, int nbucket)
{
    __shared__ int colcnt[PD_SB], segstart[PD_SB], cursor[PD_SB];
    __shared__ uint32_t tmp[PS_CAP];
    const int sb = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int beg = tile_off[(size_t)b * (nbucket + 1) + sb];
    const int nq = tile_off[(size_t)b * (nbucket + 1) + sb + 1] - beg;
    const uint32_t *kb = ent_key + (size_t)b * E + beg;
    uint32_t *out = skey + (size_t)b * E + beg;
    if (nq > PS_CAP) {
        for (int e = lane; e < nq; e += 64) {
            const uint32_t key = kb[e];
            int rank = 0;
            for (int t = 0; t < nq; ++t) rank += kb[t] < key;
            out[rank] = key;
        }
        return;
    }
    if (lane < PD_SB) colcnt[lane] = 0;
    __syncthreads();
    for (int e = lane; e < nq; e += 64) atomicAdd(&colcnt[kb[e] >> 20], 1);
    __syncthreads();
    if (lane < PD_SB) {
        int s0 = 0;
        for (int c = 0; c < lane; ++c) s0 += colcnt[c];
        segstart[lane] = s0;
        cursor[lane] = s0;
    }
    __syncthreads();
    for (int e = lane; e < nq; e += 64) {
        const uint32_t key = kb[e];
        tmp[atomicAdd(&cursor[key >> 20], 1)] = key;
    }
    __syncthreads();
    for (int t = lane; t < nq; t += 64) {
        const uint32_t key = tmp[t];
        const int col = (int)(key >> 20);
        const int s0 = segstart[col], s1 = s0 + colcnt[col];
        int rank = 0;
        for (int u = s0; u < s1; ++u) rank += tmp[u] < key;
        out[s0 + rank] = key;
    }
}

template <typename TO>
__global__ __launch_bounds__(PD_CH * PD_CQ) void pooled_dgrad_kernel(const int32_t *__restrict__ tile_off, const uint32_t *__restrict__ ent_key,
                                                           const float *__restrict__ ent_val, const float *__restrict__ g_pooled /*[B][E]: the entries' values by id*/,
                                                           const float *__restrict__ W,
                                                           int E, int M, int Cin, int C1, int L, int nbucket,
                                                           TO *__restrict__ gx1, TO *__restrict__ gx2, int abl /*experiments (variants build): 1 no stores, 2 no accumulation, 4 no sort*/)
{
    extern __shared__ float sm_f[];              // acc[PD_TL][PD_CH + 1] | per group: keys, vals, wrow [PD_SQ] each
    constexpr int ld = PD_CH + 1;
    float *acc = sm_f;
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, nth = blockDim.x;
    const int i = tid % PD_CH, q = tid / PD_CH;                             // channel ch0 + i, column quarter q
    uint32_t *keys = reinterpret_cast<uint32_t *>(sm_f + PD_TL * ld) + q * 3 * PD_SQ;
    float *vals = reinterpret_cast<float *>(keys + PD_SQ);
    int *wrow = reinterpret_cast<int *>(keys + 2 * PD_SQ);
    __shared__ int nq_all[PD_CQ];
    const int ch0 = blockIdx.z * PD_CH, nch = min(PD_CH, Cin - ch0);        // this workgroup's input channels
    for (int t = tid; t < PD_TL * ld; t += nth) acc[t] = 0.f;
    const int sb = tile * PD_CQ + q;                                        // this group's bucket (32 columns)
    const int beg = sb < nbucket ? tile_off[(size_t)b * (nbucket + 1) + sb] : 0;
    const int nq = sb < nbucket ? tile_off[(size_t)b * (nbucket + 1) + sb + 1] - beg : 0;
    const uint32_t *kb = ent_key + (size_t)b * E + beg;
    const float *vb = ent_val + (size_t)b * E + beg;
    const float *gb = g_pooled + (size_t)b * E;
    if (i == 0) nq_all[q] = nq;
    __syncthreads();
    int nmax = 0;
#pragma unroll
    for (int t = 0; t < PD_CQ; ++t) nmax = max(nmax, nq_all[t]);
    // The group's bucket arrives SORTED by (column, entry id) (pooled_sort_kernel below: once per bucket instead of once per (bucket,
    // channel slab)), so the order of the fma chain of an accumulator is fixed whatever order the bucket atomics took; thread (i, q)
    // applies the group's entries to channel ch0 + i (no two threads touch the same accumulator).  Rounds of PD_SQ consecutive entries: a
    // column that continues in the next round resumes from the stored value.
    (void)vb;
    for (int base = 0; base < nmax; base += PD_SQ) {
        const int n = min(PD_SQ, max(0, nq - base));
        __syncthreads();                                                    // the previous round's lists are consumed
        for (int t = i; t < n; t += PD_CH) {
            const uint32_t key = kb[base + t];
            const int id = (int)(key & 0xFFFFFu);
            keys[t] = (key >> 20) + (uint32_t)(q * PD_SB);                  // column inside the tile
            vals[t] = gb[id];
            wrow[t] = (id / M) * Cin + ch0;                                 // (per entry, once: the division per (entry, thread) was half of the kernel in round 2)
        }
        __syncthreads();
        if (i < nch && n > 0 && !(abl & 2)) {
            // the W rows of PD_WB entries (the PD_CH threads of a group read 320 consecutive bytes per entry, L2-resident) are requested
            // before their first fma
            // The entries are sorted by column: the fma chain of a column runs in a REGISTER and is written when the column changes (an
            // LDS read-add-write per entry serialises on the LDS latency -- hipcc cannot tell that two accumulators differ; this was most
            // of the kernel's time).  Same chain, same order, same bits.  (Rank mode: a column that continues from the previous round
            // resumes from the stored value; the accumulators start at zero, so resuming is always right.)
            int cur = (int)keys[0];
            float sum = acc[cur * ld + i];
            for (int e0 = 0; e0 < n; e0 += PD_WB) {
                float wv[PD_WB];
#pragma unroll
                for (int t = 0; t < PD_WB; ++t) {
                    const int e = e0 + t < n ? e0 + t : n - 1;
                    wv[t] = W[(size_t)wrow[e] + i];
                }
#pragma unroll
                for (int t = 0; t < PD_WB; ++t) {
                    if (e0 + t < n) {
                        const int col = (int)keys[e0 + t];
                        if (col != cur) {
                            acc[cur * ld + i] = sum;
                            cur = col;
                            sum = acc[cur * ld + i];
                        }
                        sum = __fmaf_rn(vals[e0 + t], wv[t], sum);
                    }
                }
            }
            acc[cur * ld + i] = sum;
        }
    }
    __syncthreads();
    if (abl & 1) return;
    const int l0 = tile * PD_TL;
    if (sizeof(TO) == 2 && (L & 1) == 0) {
        // bf16 output, even L: two columns per thread, one 4-byte store -- 64 consecutive threads write the 256 bytes of a row segment
        for (int idx = tid; idx < nch * (PD_TL / 2); idx += nth) {
            const int r = idx / (PD_TL / 2), col = (idx - r * (PD_TL / 2)) * 2;
            if (l0 + col >= L) continue;                        // (L even: col + 1 is inside too)
            const unsigned pk = cvt_pk_bf16(acc[col * ld + r], acc[(col + 1) * ld + r]);
            const int ch = ch0 + r;
            TO *dst = ch < C1 ? gx1 + ((size_t)b * C1 + ch) * L + l0 + col : gx2 + ((size_t)b * (Cin - C1) + (ch - C1)) * L + l0 + col;
            *reinterpret_cast<unsigned *>(dst) = pk;
        }
        return;
    }
    for (int idx = tid; idx < nch * PD_TL; idx += nth) {        // coalesced: consecutive threads along the columns of one channel
        const int r = idx / PD_TL, col = idx - r * PD_TL;
        if (l0 + col >= L) continue;
        const float v = acc[col * ld + r];
        const int ch = ch0 + r;
        if (ch < C1) st_rne(gx1, ((size_t)b * C1 + ch) * L + l0 + col, v);
        else st_rne(gx2, ((size_t)b * (Cin - C1) + (ch - C1)) * L + l0 + col, v);
    }
}

// Four channels per thread (Cin a multiple of 4).  The accumulate loop of the kernel above is bound by instruction issue, not by latency: per
// (entry, channel) three LDS reads, an address, a global load, a compare and one fma.  Here thread (i4, q, s) owns channels 4 i4 .. 4 i4 + 3 of the
// columns [8 s, 8 s + 8) of quarter q: the same per-entry overhead (one 16-byte LDS read, one 16-byte load of W) feeds four fmas, and the
// sixteen sub-ranges of a tile (their entry counts differ less than the four quarters') share the wave's loop trips.  Same entries in the same
// (column, entry id) order per accumulator: the same bits as the kernel above.
constexpr int PD4_LD = PD_CH + 4;              // accumulator row pitch: 16-byte aligned groups of four channels
constexpr int PD4_WB = 8;                      // entries (a W float4 each) requested before the first fma
#ifdef SONET_VARIANTS   // (the column-owned form: replaced by the entry-balanced kernel below, kept as the bit-exact twin of the one-channel kernel)
template <typename TO>
__global__ __launch_bounds__(PD_CH * PD_CQ) void pooled_dgrad4_kernel(const int32_t *__restrict__ tile_off, const uint32_t *__restrict__ skey,
                                                            const float *__restrict__ g_pooled, const float *__restrict__ W,
                                                            int E, int M, int Cin, int C1, int L, int nbucket,
                                                            TO *__restrict__ gx1, TO *__restrict__ gx2)
{
    extern __shared__ __attribute__((aligned(16))) float sm_f4[];       // acc[PD_TL][PD4_LD] | per quarter: uint4 ent[PD_SQ] (column, value bits, W row offset, -)
    constexpr int ld = PD4_LD;
    float *acc = sm_f4;
    uint4 *ent_all = reinterpret_cast<uint4 *>(sm_f4 + PD_TL * ld);
    __shared__ int nq_all[PD_CQ], subcnt[PD_CQ][4];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, nth = blockDim.x;
    const int q = tid / PD_CH, tq = tid - q * PD_CH;                        // column quarter, thread inside it
    const int sub = tq / 10, i4 = tq - sub * 10;                            // 8-column sub-range, channel quad
    uint4 *ent = ent_all + q * PD_SQ;
    const int ch0 = blockIdx.z * PD_CH, nch = min(PD_CH, Cin - ch0);
    for (int t = tid; t < PD_TL * ld; t += nth) acc[t] = 0.f;
    const int sb = tile * PD_CQ + q;
    const int beg = sb < nbucket ? tile_off[(size_t)b * (nbucket + 1) + sb] : 0;
    const int nq = sb < nbucket ? tile_off[(size_t)b * (nbucket + 1) + sb + 1] - beg : 0;
    const uint32_t *kb = skey + (size_t)b * E + beg;
    const float *gb = g_pooled + (size_t)b * E;
    if (tq == 0) nq_all[q] = nq;
    __syncthreads();
    int nmax = 0;
#pragma unroll
    for (int t = 0; t < PD_CQ; ++t) nmax = max(nmax, nq_all[t]);
    for (int base = 0; base < nmax; base += PD_SQ) {
        const int n = min(PD_SQ, max(0, nq - base));
        __syncthreads();                                                    // the previous round's list is consumed
        if (tq < 4) subcnt[q][tq] = 0;
        __syncthreads();
        for (int t = tq; t < n; t += PD_CH) {
            const uint32_t key = kb[base + t];
            const int id = (int)(key & 0xFFFFFu), colq = (int)(key >> 20);
            ent[t] = make_uint4((unsigned)(colq + q * PD_SB), __float_as_uint(gb[id]), (unsigned)((id / M) * Cin + ch0), 0u);
            atomicAdd(&subcnt[q][colq >> 3], 1);
        }
        __syncthreads();
        int lo = 0;
        for (int t = 0; t < sub; ++t) lo += subcnt[q][t];
        const int cnt = subcnt[q][sub];
        if (4 * i4 < nch && cnt > 0) {
            // (sorted by column: the chains of a column run in registers and are written when the column changes; a column that continues
            //  from the previous round resumes from the stored value -- the accumulators start at zero)
            int cur = (int)ent[lo].x;
            float4 sum = *reinterpret_cast<const float4 *>(acc + cur * ld + 4 * i4);
            for (int e0 = 0; e0 < cnt; e0 += PD4_WB) {
                uint4 en[PD4_WB];
                float4 wv[PD4_WB];
#pragma unroll
                for (int t = 0; t < PD4_WB; ++t) {
                    en[t] = ent[lo + (e0 + t < cnt ? e0 + t : cnt - 1)];
                    wv[t] = *reinterpret_cast<const float4 *>(W + (size_t)en[t].z + 4 * i4);
                }
#pragma unroll
                for (int t = 0; t < PD4_WB; ++t) {
                    if (e0 + t < cnt) {
                        const int col = (int)en[t].x;
                        if (col != cur) {
                            *reinterpret_cast<float4 *>(acc + cur * ld + 4 * i4) = sum;
                            cur = col;
                            sum = *reinterpret_cast<const float4 *>(acc + cur * ld + 4 * i4);
                        }
                        const float v = __uint_as_float(en[t].y);
                        sum.x = __fmaf_rn(v, wv[t].x, sum.x);
                        sum.y = __fmaf_rn(v, wv[t].y, sum.y);
                        sum.z = __fmaf_rn(v, wv[t].z, sum.z);
                        sum.w = __fmaf_rn(v, wv[t].w, sum.w);
                    }
                }
            }
            *reinterpret_cast<float4 *>(acc + cur * ld + 4 * i4) = sum;
        }
    }
    __syncthreads();
    const int l0 = tile * PD_TL;
    if (sizeof(TO) == 2 && (L & 1) == 0) {
        for (int idx = tid; idx < nch * (PD_TL / 2); idx += nth) {
            const int r = idx / (PD_TL / 2), col = (idx - r * (PD_TL / 2)) * 2;
            if (l0 + col >= L) continue;
            const unsigned pk = cvt_pk_bf16(acc[col * ld + r], acc[(col + 1) * ld + r]);
            const int ch = ch0 + r;
            TO *dst = ch < C1 ? gx1 + ((size_t)b * C1 + ch) * L + l0 + col : gx2 + ((size_t)b * (Cin - C1) + (ch - C1)) * L + l0 + col;
            *reinterpret_cast<unsigned *>(dst) = pk;
        }
        return;
    }
    for (int idx = tid; idx < nch * PD_TL; idx += nth) {
        const int r = idx / PD_TL, col = idx - r * PD_TL;
        if (l0 + col >= L) continue;
        const float v = acc[col * ld + r];
        const int ch = ch0 + r;
        if (ch < C1) st_rne(gx1, ((size_t)b * C1 + ch) * L + l0 + col, v);
        else st_rne(gx2, ((size_t)b * (Cin - C1) + (ch - C1)) * L + l0 + col, v);
    }
}
#endif  // SONET_VARIANTS

// Entry-balanced form (the product's kernel).  In the column-owned form a wave's loop runs as long as its fullest 8-column sub-range (mean 13 entries, a long tail: a small
// node drops its 384 entries on a handful of columns).  Here the tile's sorted list -- its four buckets are consecutive in `skey` -- is staged
// as ONE list, PD5_R entries per round, and cut into sixteen chunks of equal LENGTH, one per group of ten threads (four channels each): every
// lane of the workgroup runs the same number of entries (+- 1).  A column that straddles a chunk boundary: the later chunk starts from zero
// for it and leaves its partial sum in `head`; after the round the first such chunk of a run on one column adds the run's partial sums to
// the accumulator in chunk order -- a fixed order, so the result is reproducible run to run (it differs from the column-owned kernels in the
// last bit where a column was cut: another association of the same sum).
constexpr int PD_SPARSE_KERNEL = 5;           // input widths that are multiples of 4 (the variants build can ask for 4: SONET_PD_KERNEL)
constexpr int PD5_R = 384;                     // entries per round (LDS: five workgroups per CU)
constexpr int PD5_G = 16;                      // chunks = groups of ten threads
// TAIL (f32 outputs): what used to follow the launch rides on its store.
//  * col0 / pos0: every channel of an EMPTY node gathers position 0 (models/networks.py:185) -- those entries are one dense mat-vec per cloud
//    (the caller's), whose result lands on ONE column, pos0[b]: added by the thread that stores that column (two scatter_add launches less,
//    and the tensors are final when the launch is over, which the next item needs).
//  * sraw / ssc / ssh / spart: gx2 is gy of the layer that produced x2; when that layer handed its RAW output on (normalise-on-load: the
//    raw tensor IS x2) its BatchNorm-backward sums -- per channel sum of gy * mask and of gy * mask * raw, what
//    sonet_pointwise_bwd_stats_f32 reads (gy, raw) once more for -- are taken from the tile while it is stored: the launch reads raw
//    (1 GB at 64 x 256 x 15000) instead of a pass reading gy AND raw.  A 32-column block of a channel is a half wave: five shuffles per
//    quantity, block sums through the LDS in a fixed order, one (double, double) per (cloud, tile, channel), summed by pd_sums_finalize_kernel.
struct PdTail {
    const float *col0;                    // [B][Cin] or NULL
    const int32_t *pos0;                  // [B]
    const float *sraw;                    // [B][Cin - C1][L] or NULL
    const float *ssc, *ssh;               // [Cin - C1]
    int srelu;
    double *spart;                        // [B * gridDim.x][Cin - C1][2]
};

__global__ __launch_bounds__(256) void pd_sums_finalize_kernel(const double *__restrict__ partial, int n, int C, double *__restrict__ sums)
{
    __shared__ double r1[256], r2[256];
    const int c = blockIdx.x, t = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int k = t; k < n; k += 256) {
        const double *p = partial + ((size_t)k * C + c) * 2;
        s1 += p[0];
        s2 += p[1];
    }
    r1[t] = s1;
    r2[t] = s2;
    __syncthreads();
#pragma unroll
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) { r1[t] += r1[t + off]; r2[t] += r2[t + off]; }
        __syncthreads();
    }
    if (t == 0) { sums[c] = r1[0]; sums[C + c] = r2[0]; }
}

template <typename TO, bool TAIL = false>
__global__ __launch_bounds__(PD_CH * PD_CQ) void pooled_dgrad5_kernel(const int32_t *__restrict__ tile_off, const uint32_t *__restrict__ skey,
                                                            const float *__restrict__ g_pooled, const float *__restrict__ W,
                                                            int E, int M, int Cin, int C1, int L, int nbucket,
                                                            TO *__restrict__ gx1, TO *__restrict__ gx2, const PdTail tail)
{
    static_assert(!TAIL || sizeof(TO) == 4, "the tail exists for f32 outputs");
    extern __shared__ __attribute__((aligned(16))) float sm_f5[];       // acc[PD_TL][PD4_LD] | head[PD5_G][PD_CH] | uint4 ent[PD5_R]
    constexpr int ld = PD4_LD;
    static_assert(PD_CH * PD_CQ == PD5_G * 10 && PD_CH == 40, "sixteen groups of ten threads, four channels each");
    float *acc = sm_f5;
    float *head = sm_f5 + PD_TL * ld;
    uint4 *ent = reinterpret_cast<uint4 *>(head + PD5_G * PD_CH);
    __shared__ int headcol[PD5_G];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, nth = blockDim.x;
    const int grp = tid / 10, i4 = tid - grp * 10;
    const int ch0 = blockIdx.z * PD_CH, nch = min(PD_CH, Cin - ch0);
    for (int t = tid; t < PD_TL * ld; t += nth) acc[t] = 0.f;
    const int32_t *to = tile_off + (size_t)b * (nbucket + 1);
    int bo[PD_CQ + 1];
#pragma unroll
    for (int t = 0; t <= PD_CQ; ++t) bo[t] = to[min(tile * PD_CQ + t, nbucket)];
    const int beg = bo[0], N = bo[PD_CQ] - beg;
    const uint32_t *kb = skey + (size_t)b * E + beg;
    const float *gb = g_pooled + (size_t)b * E;
    for (int base = 0; base < N; base += PD5_R) {
        const int n = min(PD5_R, N - base);
        __syncthreads();                                                    // the accumulators are zeroed / the previous round is merged
        for (int t = tid; t < n; t += nth) {
            const int e = beg + base + t;
            const uint32_t key = kb[base + t];
            const int id = (int)(key & 0xFFFFFu);
            const int q = (e >= bo[1]) + (e >= bo[2]) + (e >= bo[3]);      // the bucket of the tile this entry sits in
            ent[t] = make_uint4((unsigned)((int)(key >> 20) + q * PD_SB), __float_as_uint(gb[id]), (unsigned)((id / M) * Cin + ch0), 0u);
        }
        __syncthreads();
        // chunk grp: the first n % 16 chunks take one entry more (the non-empty chunks are the first ones)
        const int per = n / PD5_G, rem = n - per * PD5_G;
        const int lo = grp * per + min(grp, rem), cnt = per + (grp < rem ? 1 : 0);
        const bool cont = cnt > 0 && lo > 0 && ent[lo - 1].x == ent[lo].x;  // my first column began in the chunk before
        if (i4 == 0) headcol[grp] = cont ? (int)ent[lo].x : -1;
        if (4 * i4 < nch && cnt > 0) {
            int cur = (int)ent[lo].x;
            bool in_head = cont;
            float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!in_head) sum = *reinterpret_cast<const float4 *>(acc + cur * ld + 4 * i4);
            for (int e0 = 0; e0 < cnt; e0 += PD4_WB) {
                uint4 en[PD4_WB];
                float4 wv[PD4_WB];
#pragma unroll
                for (int t = 0; t < PD4_WB; ++t) {
                    en[t] = ent[lo + (e0 + t < cnt ? e0 + t : cnt - 1)];
                    wv[t] = *reinterpret_cast<const float4 *>(W + (size_t)en[t].z + 4 * i4);
                }
#pragma unroll
                for (int t = 0; t < PD4_WB; ++t) {
                    if (e0 + t < cnt) {
                        const int col = (int)en[t].x;
                        if (col != cur) {
                            *reinterpret_cast<float4 *>(in_head ? head + grp * PD_CH + 4 * i4 : acc + cur * ld + 4 * i4) = sum;
                            in_head = false;
                            cur = col;
                            sum = *reinterpret_cast<const float4 *>(acc + cur * ld + 4 * i4);
                        }
                        const float v = __uint_as_float(en[t].y);
                        sum.x = __fmaf_rn(v, wv[t].x, sum.x);
                        sum.y = __fmaf_rn(v, wv[t].y, sum.y);
                        sum.z = __fmaf_rn(v, wv[t].z, sum.z);
                        sum.w = __fmaf_rn(v, wv[t].w, sum.w);
                    }
                }
            }
            *reinterpret_cast<float4 *>(in_head ? head + grp * PD_CH + 4 * i4 : acc + cur * ld + 4 * i4) = sum;
        }
        __syncthreads();
        // the cut columns: the first chunk of a run of partial sums on one column adds the run, in chunk order
        if (4 * i4 < nch && grp > 0) {
            const int hc = headcol[grp];
            if (hc >= 0 && headcol[grp - 1] != hc) {
                float4 s = *reinterpret_cast<const float4 *>(acc + hc * ld + 4 * i4);
                for (int g = grp; g < PD5_G && headcol[g] == hc; ++g) {
                    const float4 hv = *reinterpret_cast<const float4 *>(head + g * PD_CH + 4 * i4);
                    s.x += hv.x; s.y += hv.y; s.z += hv.z; s.w += hv.w;
                }
                *reinterpret_cast<float4 *>(acc + hc * ld + 4 * i4) = s;
            }
        }
    }
    __syncthreads();
    const int l0 = tile * PD_TL;
    if constexpr (TAIL) {
        // units of (channel r, 32-column block): one per half wave and step; `head` is free now: block sums [160][2]
        float *ust = head;
        const int hw = tid >> 5, ln = tid & 31;
        const int p0 = tail.col0 ? tail.pos0[b] : -1;
        const int C2 = Cin - C1;
        float *g1 = reinterpret_cast<float *>(gx1), *g2 = reinterpret_cast<float *>(gx2);
        // (eight units at a time: the loads of a batch -- accumulator rows from the LDS, raw and its coefficients from memory -- are all
        //  requested before the first store; one unit per trip left every trip waiting for its own load: 1.74 ms against 1.0 ms apart)
        for (int k0 = 0; k0 < 32; k0 += 8) {
            float v[8], rw[8], sc[8], sh[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int u = hw + 5 * (k0 + t), r = u >> 2, blk = u & 3;
                const int col = blk * 32 + ln, l = l0 + col, ch = ch0 + r;
                const bool ok = r < nch && l < L;
                v[t] = ok ? acc[col * ld + r] : 0.f;
                if (ok && l == p0) v[t] = v[t] + tail.col0[(size_t)b * Cin + ch];
                const bool st = ok && ch >= C1 && tail.sraw != nullptr;
                rw[t] = st ? tail.sraw[((size_t)b * C2 + (ch - C1)) * L + l] : 0.f;
                sc[t] = st ? tail.ssc[ch - C1] : 0.f;
                sh[t] = st ? tail.ssh[ch - C1] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int u = hw + 5 * (k0 + t), r = u >> 2, blk = u & 3;
                const int col = blk * 32 + ln, l = l0 + col, ch = ch0 + r;
                const bool ok = r < nch && l < L;
                float s1 = 0.f, s2 = 0.f;
                if (ok) {
                    if (ch < C1) g1[((size_t)b * C1 + ch) * L + l] = v[t];
                    else {
                        g2[((size_t)b * C2 + (ch - C1)) * L + l] = v[t];
                        if (tail.sraw) {
                            float gm = v[t];
                            if (tail.srelu && !(__fmaf_rn(rw[t], sc[t], sh[t]) > 0.f)) gm = 0.f;
                            s1 = gm;
                            s2 = gm * rw[t];
                        }
                    }
                }
                if (tail.sraw) {
                    s1 = row32_sum(s1);
                    s2 = row32_sum(s2);
                    if (ln == 0) { ust[2 * u] = s1; ust[2 * u + 1] = s2; }
                }
            }
        }
        if (tail.sraw) {
            __syncthreads();
            if (tid < nch && ch0 + tid >= C1) {
                double a = 0.0, q = 0.0;
#pragma unroll
                for (int blk = 0; blk < 4; ++blk) { a += (double)ust[2 * (tid * 4 + blk)]; q += (double)ust[2 * (tid * 4 + blk) + 1]; }
                double *dst = tail.spart + (((size_t)b * gridDim.x + tile) * C2 + (ch0 + tid - C1)) * 2;
                dst[0] = a;
                dst[1] = q;
            }
        }
        return;
    }
    if (sizeof(TO) == 2 && (L & 1) == 0) {
        for (int idx = tid; idx < nch * (PD_TL / 2); idx += nth) {
            const int r = idx / (PD_TL / 2), col = (idx - r * (PD_TL / 2)) * 2;
            if (l0 + col >= L) continue;
            const unsigned pk = cvt_pk_bf16(acc[col * ld + r], acc[(col + 1) * ld + r]);
            const int ch = ch0 + r;
            TO *dst = ch < C1 ? gx1 + ((size_t)b * C1 + ch) * L + l0 + col : gx2 + ((size_t)b * (Cin - C1) + (ch - C1)) * L + l0 + col;
            *reinterpret_cast<unsigned *>(dst) = pk;
        }
        return;
    }
    for (int idx = tid; idx < nch * PD_TL; idx += nth) {
        const int r = idx / PD_TL, col = idx - r * PD_TL;
        if (l0 + col >= L) continue;
        const float v = acc[col * ld + r];
        const int ch = ch0 + r;
        if (ch < C1) st_rne(gx1, ((size_t)b * C1 + ch) * L + l0 + col, v);
        else st_rne(gx2, ((size_t)b * (Cin - C1) + (ch - C1)) * L + l0 + col, v);
    }
}

// ---- the same dgrad on the matrix cores (bf16 training path) -------------------------------------------------------------
// g_x[:, tile] = W^T (320 x 384) . G (384 x 64 columns), G the tile of the never-built dense gradient: the workgroup zeroes a 48 KB
// bf16 image of G^T in LDS, drops the tile's entries into it (in this model a (channel, column) pair occurs at most once -- node m's
// arg-max of channel c -- so nothing depends on the order the bucket atomics took; repeated pairs add up in bf16) and runs the dense product: A =
// the bf16 pack of W^T (the layer kernels' A-fragment order, streamed from L2 three chunks ahead), B = G^T rows from LDS.  The two
// 32-column MFMA tiles of a wave are the even and the odd columns, so cvt_pk(acc_even, acc_odd) is the dword to store (as in
// pointmlp_bf16.hip).  g and W are rounded to bf16 (the dense bf16 dgrad of the other layers does the same); products exact, f32
// accumulate.  0.85 -> ... ms at 64 x 384 x 64 entries, 15000 columns (the scalar kernel above: sort 0.17 + W rows from L2 0.40 +
// stores 0.18 + 0.10, profiles/r04w_pooled_dgrad_ablation.log).
constexpr int PM_TL = 64;                      // columns per workgroup (two 32-column buckets)
constexpr int PM_PITCH = 784;                  // bytes per G^T row: 384 channels x 2 + 16 (196 words = 4 mod 64 banks: 16-byte reads of 16 rows tile the banks)

template <int NMT, int CH /*64-column halves per workgroup: 1 or 2*/>
__global__ __launch_bounds__(128 * CH) void pooled_dgrad_mfma_kernel(const int32_t *__restrict__ tile_off, const uint32_t *__restrict__ ent_key,
                                                                const float *__restrict__ ent_val, const uint4 *__restrict__ Wtp,
                                                                int E, int M, int C, int KC, int C1, int C2, int L, int nbucket,
                                                                uint16_t *__restrict__ gx1, uint16_t *__restrict__ gx2)
{
    constexpr int NR = 32 * CH;                  // G^T rows (column pairs) per parity
    extern __shared__ uint4 pm_lds[];            // Ge[NR][PM_PITCH] | Go[NR][PM_PITCH]: G^T of the even / odd columns, channels contiguous
    unsigned char *Ge = reinterpret_cast<unsigned char *>(pm_lds), *Go = Ge + NR * PM_PITCH;
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mhalf = wave & 1, chalf = wave >> 1;                          // cin tiles [mhalf NMT, ...), columns [64 chalf, 64 chalf + 64) of the tile
    const int n = lane & 31, h = lane >> 5;
    for (int t = tid; t < 2 * NR * PM_PITCH / 16; t += 128 * CH) pm_lds[t] = make_uint4(0u, 0u, 0u, 0u);
    const int sb0 = tile * 2 * CH;
    const int32_t *off = tile_off + (size_t)b * (nbucket + 1);
    int bnd[2 * CH + 1];
#pragma unroll
    for (int k = 0; k <= 2 * CH; ++k) bnd[k] = off[min(sb0 + k, nbucket)];
    // A fragments of the first chunks: on their way while the tile is built.  (With CH = 2 the two waves of a cin half request the same
    // fragments a few hundred cycles apart: the second request is an L1 hit, and W^T crosses the L2 once per 128 columns.)
    const uint4 *wt = Wtp + ((size_t)(mhalf * NMT) * KC) * 64 + lane;
    uint4 A[3][NMT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) A[s][mt] = wt[((size_t)mt * KC + min(s, KC - 1)) * 64];
    __syncthreads();
    for (int e = bnd[0] + tid; e < bnd[2 * CH]; e += 128 * CH) {
        const uint32_t key = ent_key[(size_t)b * E + e];
        int bk = 0;
#pragma unroll
        for (int k = 1; k < 2 * CH; ++k) bk += e >= bnd[k];
        const int l = (int)(key >> 20) + 32 * bk, c = (int)(key & 0xFFFFFu) / M;
        // (a compare-and-swap on the dword that holds the channel pair: two channels of a column share it, and a (channel, column) pair
        //  that does occur twice -- not in this model -- adds up instead of being overwritten, in arrival order)
        unsigned *wd = reinterpret_cast<unsigned *>(((l & 1) ? Go : Ge) + (l >> 1) * PM_PITCH + (c >> 1) * 4);
        const int sh = (c & 1) * 16;
        const float g = ent_val[(size_t)b * E + e];
        unsigned old = *wd, assumed;
        do {
            assumed = old;
            const float cur = __uint_as_float(((assumed >> sh) & 0xFFFFu) << 16);
            const unsigned nb = cvt_pk_bf16(cur + g, 0.f) & 0xFFFFu;
            old = atomicCAS(wd, assumed, (assumed & ~(0xFFFFu << sh)) | (nb << sh));
        } while (old != assumed);
    }
    __syncthreads();

    f32x16 acc[NMT][2];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[mt][0][r] = 0.f; acc[mt][1][r] = 0.f; }
    const unsigned char *be = Ge + (32 * chalf + n) * PM_PITCH + h * 16, *bo = Go + (32 * chalf + n) * PM_PITCH + h * 16;
#define PM_STEP(kc, s)                                                                                          \
    if ((kc) < KC) {                                                                                            \
        const int kn = min((kc) + 2, KC - 1);                                                                   \
        _Pragma("unroll") for (int mt = 0; mt < NMT; ++mt) A[((s) + 2) % 3][mt] = wt[((size_t)mt * KC + kn) * 64]; \
        const bf16x8 Be = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(be + (kc) * 32));         \
        const bf16x8 Bo = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(bo + (kc) * 32));         \
        _Pragma("unroll") for (int mt = 0; mt < NMT; ++mt) {                                                    \
            const bf16x8 Av = __builtin_bit_cast(bf16x8, A[s][mt]);                                             \
            acc[mt][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Av, Be, acc[mt][0], 0, 0, 0);                  \
            acc[mt][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Av, Bo, acc[mt][1], 0, 0, 0);                  \
        }                                                                                                       \
    }
    for (int kc = 0; kc < KC; kc += 3) {
        PM_STEP(kc, 0)
        PM_STEP(kc + 1, 1)
        PM_STEP(kc + 2, 2)
    }
#undef PM_STEP

    if constexpr (CH == 2) {
        // 128-column tiles: the output goes through LDS (the G^T image is finished with) and leaves as 16 bytes per lane, 256-byte row
        // segments.  (As dword stores -- 32 lanes x 4 bytes per row and instruction, every segment a partial cache line on 30000-byte
        // rows -- the store phase ran at the ~1.6 TB/s of the staged bf16 layer kernel's epilogue.)
        constexpr int OP = 272;                                           // bytes per output row in LDS: 128 columns x 2 + 16
        unsigned char *ot = reinterpret_cast<unsigned char *>(pm_lds);
        __syncthreads();                                                  // every wave has read its last B fragment
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = (mhalf * NMT + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                *reinterpret_cast<unsigned *>(ot + ci * OP + (64 * chalf + 2 * n) * 2) = cvt_pk_bf16(acc[mt][0][r], acc[mt][1][r]);
            }
        __syncthreads();
        const int l0 = tile * (PM_TL * CH);
        const int piece = tid & 15;                                       // 8 columns
        const bool vec = (L & 7) == 0;                                    // row starts 16-byte aligned
        for (int ci = tid >> 4; ci < C1 + C2; ci += (128 * CH) >> 4) {
            const int c0 = l0 + 8 * piece;
            if (c0 >= L) continue;
            uint16_t *dst = ci < C1 ? gx1 + ((size_t)b * C1 + ci) * L + c0 : gx2 + ((size_t)b * C2 + (ci - C1)) * L + c0;
            const uint4 v = *reinterpret_cast<const uint4 *>(ot + ci * OP + piece * 16);
            if (vec && c0 + 8 <= L) {
                *reinterpret_cast<uint4 *>(dst) = v;
            } else {                                                      // (L even: whole dwords)
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + 2 * e < L) reinterpret_cast<unsigned *>(dst)[e] = w[e];
            }
        }
    } else {
    const int col = tile * (PM_TL * CH) + 64 * chalf + 2 * n;          // (L even: col + 1 is inside when col is)
    if (col < L) {
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = (mhalf * NMT + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (ci >= C1 + C2) continue;
                const unsigned pk = cvt_pk_bf16(acc[mt][0][r], acc[mt][1][r]);
                uint16_t *dst = ci < C1 ? gx1 + ((size_t)b * C1 + ci) * L + col : gx2 + ((size_t)b * C2 + (ci - C1)) * L + col;
                *reinterpret_cast<unsigned *>(dst) = pk;
            }
        }
    }
    }
}

}  // namespace

extern "C" size_t sonet_pooled_dgrad_ws_size(int B, int C, int M, int L)
{
    if (B <= 0 || C <= 0 || M <= 0 || L <= 0) return 0;
    const size_t E = (size_t)C * M, nbucket = (size_t)sonet::ceil_div(L, PD_SB);
    return (size_t)B * (E * 12 + (nbucket + 1) * 4);            // bucket lists (key, value), the sorted keys, bucket offsets
}

// Sparse wgrad of the pooled last layer: the gradient of first_pn_out exists only at the C*M gathered positions of a
// cloud, so  g_W[c][ci] = sum over (b, m) of g[b][c][m] * x[b][ci][pos[b][c][m]]  -- 24,576 x Ci MACs per cloud instead of
// a dense [C x L] x [L x Ci] GEMM over a tensor that is 99.6 % zeros (and that then need not be built at all).
// One workgroup per (cloud, PW_R input-channel rows): the rows sit in LDS (coalesced load; the column gathers of x that
// make a direct scatter formulation uncoalesced become LDS reads), thread <-> output channel c keeps its M entries in
// registers (g and pos come TRANSPOSED, [B][M][C], so that loading them is coalesced) and applies them to PW_G row pairs.
// Per-cloud partials out[b][c][ci]; the caller sums over b (fixed order: deterministic).
constexpr int PW_ROWS = 16;                                  // x rows per workgroup (the entries are loaded once for all of them)
template <typename TX> struct PwR { static constexpr int value = sizeof(TX) == 4 ? 1 : 2; };   // rows resident in LDS at a time: 60 KB either way at
                                                             // 15000 columns (bf16 pairs, single f32 rows) -- two workgroups per CU
constexpr int PW_M = 64;                                     // entries per output channel kept in registers (M <= PW_M)
constexpr int PW_T = 768;                                    // threads: two per output channel (C <= 384), each with half of the M entries
// xs / xh (f32 rows only): x holds the RAW output of a BatchNorm layer; the copy into LDS applies act(raw * xs[ci] + xh[ci]) -- what
// sonet_channel_affine_act_f32 would have stored -- so the gathers see the normalised activations that were never written.
template <typename TX>
__global__ __launch_bounds__(PW_T) void pooled_wgrad_kernel(const float *__restrict__ g, const int32_t *__restrict__ pos,
                                                            const TX *__restrict__ x, int C, int M, int Ci, int L,
                                                            float *__restrict__ out, const float *__restrict__ xs = nullptr,
                                                            const float *__restrict__ xh = nullptr, int xrelu = 0)
{
    // rows in the storage type: bf16 rows stay bf16 in LDS (widened on the read) -- 60 KB per pair of 15000-column rows instead of 120,
    // so two workgroups share a CU and one multiplies while the other loads (round 3 widened on the way in: one workgroup per CU,
    // load -> barrier -> multiply -> barrier in sequence).  The multiply is instruction-bound (an LDS read and an fma per entry and
    // row): two threads per channel, 32 entries each, the halves meet in LDS (a + b: one order).
    constexpr int PW_R = PwR<TX>::value, PW_G = PW_ROWS / PW_R;
    extern __shared__ __attribute__((aligned(16))) unsigned char rows_raw[];           // [PW_R][L] of TX | comb[PW_T / 2][PW_R] f32
    TX *rows = reinterpret_cast<TX *>(rows_raw);
    float *comb = reinterpret_cast<float *>(rows_raw + (((size_t)PW_R * L * sizeof(TX) + 15) & ~(size_t)15));
    const int b = blockIdx.y;
    const int c = threadIdx.x % (PW_T / 2), half = threadIdx.x / (PW_T / 2);   // C <= PW_T / 2 (checked by the launcher)
    constexpr int MH = PW_M / 2;
    float gv[MH];
    int pv[MH];
#pragma unroll
    for (int m = 0; m < MH; ++m) {
        const int mm = half * MH + m;
        const bool ok = mm < M && c < C;
        gv[m] = ok ? g[((size_t)b * M + mm) * C + c] : 0.f;
        const int p = ok ? pos[((size_t)b * M + mm) * C + c] : -1;
        pv[m] = (unsigned)p < (unsigned)L ? p : -1;
    }
    auto widen = [](TX v) -> float {
        if constexpr (sizeof(TX) == 4) return v;
        else return __uint_as_float((unsigned)v << 16);
    };
    for (int gi = 0; gi < PW_G; ++gi) {
        const int ci0 = (blockIdx.x * PW_G + gi) * PW_R;
        if (ci0 >= Ci) break;
        const int nr = min(PW_R, Ci - ci0);
        const TX *xb = x + ((size_t)b * Ci + ci0) * L;
        __syncthreads();                                                  // the previous pair has been consumed
        const size_t nbytes = (size_t)nr * L * sizeof(TX);
        bool copied = false;
        if constexpr (sizeof(TX) == 4) {
            if (xs != nullptr) {                                          // (PW_R == 1: the row is channel ci0)
                const float sc = xs[ci0], sh = xh[ci0];
                auto act = [&](float v) { v = __fmaf_rn(v, sc, sh); return (xrelu && v < 0.f) ? 0.f : v; };
                if ((nbytes & 15) == 0 && ((size_t)xb & 15) == 0) {
                    const float4 *x4 = reinterpret_cast<const float4 *>(xb);
                    float4 *r4 = reinterpret_cast<float4 *>(rows);
                    for (int i = threadIdx.x; i < (int)(nbytes >> 4); i += blockDim.x) {
                        const float4 t = x4[i];
                        r4[i] = make_float4(act(t.x), act(t.y), act(t.z), act(t.w));
                    }
                } else {
                    for (int i = threadIdx.x; i < nr * L; i += blockDim.x) rows[i] = act(xb[i]);
                }
                copied = true;
            }
        }
        if constexpr (sizeof(TX) == 2) {
            // bf16 rows (PW_R == 2: channels ci0, ci0 + 1) sit INTERLEAVED in LDS, one dword per column = (row ci0 | row ci0 + 1 << 16): an entry
            // costs ONE LDS read for both rows (round 6; two 2-byte reads before -- the multiply is bound by its LDS reads).  The values and
            // the order of the fmas are unchanged: bit-identical sums.  With xs / xh the rows are normalised on the way in: act(raw * xs + xh)
            // in f32, ReLU, one round-to-nearest-even back to bf16 -- sonet_channel_affine_act_out_bf16's arithmetic.
            const float s0 = xs ? xs[ci0] : 1.f, h0 = xs ? xh[ci0] : 0.f;
            const float s1 = (xs && nr > 1) ? xs[ci0 + 1] : 1.f, h1 = (xs && nr > 1) ? xh[ci0 + 1] : 0.f;
            auto act16 = [&](unsigned v, bool second) -> unsigned {
                if (xs == nullptr) return v;
                float f = __fmaf_rn(__uint_as_float(v << 16), second ? s1 : s0, second ? h1 : h0);
                if (xrelu && f < 0.f) f = 0.f;
                return cvt_pk_bf16(f, 0.f) & 0xFFFFu;
            };
            unsigned *pairs = reinterpret_cast<unsigned *>(rows_raw);
            const uint16_t *x0 = reinterpret_cast<const uint16_t *>(xb), *x1r = x0 + L;
            if ((L & 7) == 0 && ((size_t)xb & 15) == 0) {
                const uint4 *a4 = reinterpret_cast<const uint4 *>(x0), *b4 = reinterpret_cast<const uint4 *>(x1r);
                uint4 *p4 = reinterpret_cast<uint4 *>(pairs);
                for (int i = threadIdx.x; i < (L >> 3); i += blockDim.x) {          // eight columns of both rows per thread
                    const uint4 ta = a4[i];
                    const uint4 tb = nr > 1 ? b4[i] : make_uint4(0u, 0u, 0u, 0u);
                    const unsigned da[4] = {ta.x, ta.y, ta.z, ta.w}, db[4] = {tb.x, tb.y, tb.z, tb.w};
                    unsigned o[8];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        o[2 * k] = act16(da[k] & 0xFFFFu, false) | ((nr > 1 ? act16(db[k] & 0xFFFFu, true) : 0u) << 16);
                        o[2 * k + 1] = act16(da[k] >> 16, false) | ((nr > 1 ? act16(db[k] >> 16, true) : 0u) << 16);
                    }
                    p4[2 * i] = make_uint4(o[0], o[1], o[2], o[3]);
                    p4[2 * i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
                }
            } else {
                for (int i = threadIdx.x; i < L; i += blockDim.x)
                    pairs[i] = act16((unsigned)x0[i], false) | ((nr > 1 ? act16((unsigned)x1r[i], true) : 0u) << 16);
            }
            copied = true;
        }
        if (copied) {
        } else if ((nbytes & 15) == 0 && ((size_t)xb & 15) == 0) {
            const uint4 *x4 = reinterpret_cast<const uint4 *>(xb);
            uint4 *r4 = reinterpret_cast<uint4 *>(rows);
            for (int i = threadIdx.x; i < (int)(nbytes >> 4); i += blockDim.x) r4[i] = x4[i];
        } else {
            for (int i = threadIdx.x; i < nr * L; i += blockDim.x) rows[i] = xb[i];
        }
        __syncthreads();
        float acc[PW_R];
#pragma unroll
        for (int r = 0; r < PW_R; ++r) acc[r] = 0.f;
        if (c < C) {
#pragma unroll
            for (int m = 0; m < MH; ++m) {
                if (pv[m] >= 0) {
                    if constexpr (sizeof(TX) == 2) {
                        const unsigned d = reinterpret_cast<const unsigned *>(rows_raw)[pv[m]];      // (row ci0 | row ci0 + 1 << 16) of this column
                        acc[0] = __fmaf_rn(gv[m], bf_lo(d), acc[0]);
                        if (nr > 1) acc[1] = __fmaf_rn(gv[m], bf_hi(d), acc[1]);
                    } else {
                        acc[0] = __fmaf_rn(gv[m], widen(rows[pv[m]]), acc[0]);
                    }
                }
            }
            if (half == 1) {
#pragma unroll
                for (int r = 0; r < PW_R; ++r) comb[c * PW_R + r] = acc[r];
            }
        }
        __syncthreads();
        if (c < C && half == 0)
            for (int r = 0; r < nr; ++r) out[((size_t)b * C + c) * Ci + ci0 + r] = acc[r] + comb[c * PW_R + r];
    }
}

template <typename TX>
static int pooled_wgrad_impl(const char *what, const float *g_pooled, const int32_t *pos, const TX *x, int B, int C, int M, int Ci, int L,
                             float *gw_partial, sonet_stream_t stream, const float *xs = nullptr, const float *xh = nullptr, int xrelu = 0)
{
    SONET_REQUIRE(g_pooled && pos && x && gw_partial, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && M > 0 && Ci > 0 && L > 0 && B <= 65535, "%s: bad size B=%d C=%d M=%d Ci=%d L=%d", what, B, C, M, Ci, L);
    if (C > 384 || M > PW_M) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: C=%d > 384 or M=%d > %d", what, C, M, PW_M);
    constexpr int PW_R = PwR<TX>::value;
    const size_t lds = (((size_t)PW_R * L * sizeof(TX) + 15) & ~(size_t)15) + (size_t)(PW_T / 2) * PW_R * sizeof(float);
    if (lds > 152 * 1024) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: L=%d rows do not fit LDS", what, L);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(pooled_wgrad_kernel<TX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return sonet::fail(SONET_ERR_LAUNCH, "%s: cannot reserve %zu bytes of LDS", what, lds);
    hipLaunchKernelGGL(pooled_wgrad_kernel<TX>, dim3((unsigned)sonet::ceil_div(Ci, PW_ROWS), (unsigned)B), dim3(PW_T), lds, sonet::as_stream(stream),
                       g_pooled, pos, x, C, M, Ci, L, gw_partial, xs, xh, xrelu);
    return sonet::launched(what);
}

/* sonet_pooled_wgrad_f32 when x is the RAW output of a BatchNorm layer (normalise-on-load, see sonet_pointmlp_h3_stats_xaff_f32): the rows
 * are normalised on their way into the LDS: x = act(raw * xs[ci] + xh[ci]); xs, xh [Ci]. */
extern "C" int sonet_pooled_wgrad_xaff_f32(const float *g_pooled, const int32_t *pos, const float *x, int B, int C, int M, int Ci, int L,
                                           float *gw_partial, const float *xs, const float *xh, int xrelu, sonet_stream_t stream)
{
    SONET_REQUIRE(xs && xh, "sonet_pooled_wgrad_xaff_f32: NULL pointer");
    return pooled_wgrad_impl<float>("sonet_pooled_wgrad_xaff_f32", g_pooled, pos, x, B, C, M, Ci, L, gw_partial, stream, xs, xh, xrelu);
}

extern "C" int sonet_pooled_wgrad_f32(const float *g_pooled, const int32_t *pos, const float *x, int B, int C, int M, int Ci, int L,
                                      float *gw_partial, sonet_stream_t stream)
{
    return pooled_wgrad_impl<float>("sonet_pooled_wgrad_f32", g_pooled, pos, x, B, C, M, Ci, L, gw_partial, stream);
}

/* x as bfloat16 bit patterns (the bf16 training path keeps its activations in bf16); everything else as above */
extern "C" int sonet_pooled_wgrad_xbf16(const float *g_pooled, const int32_t *pos, const uint16_t *x, int B, int C, int M, int Ci, int L,
                                        float *gw_partial, sonet_stream_t stream)
{
    return pooled_wgrad_impl<uint16_t>("sonet_pooled_wgrad_xbf16", g_pooled, pos, x, B, C, M, Ci, L, gw_partial, stream);
}

/* ... when x is the RAW (bf16) output of a BatchNorm layer (bf16 training with normalise-on-load, see sonet_pointmlp_bf16_stats_xaff): the rows
 * are normalised on their way into the LDS, x = bf16(act(raw * xs[ci] + xh[ci])); xs, xh [Ci]. */
extern "C" int sonet_pooled_wgrad_xaff_xbf16(const float *g_pooled, const int32_t *pos, const uint16_t *x, int B, int C, int M, int Ci, int L,
                                             float *gw_partial, const float *xs, const float *xh, int xrelu, sonet_stream_t stream)
{
    SONET_REQUIRE(xs && xh, "sonet_pooled_wgrad_xaff_xbf16: NULL pointer");
    return pooled_wgrad_impl<uint16_t>("sonet_pooled_wgrad_xaff_xbf16", g_pooled, pos, x, B, C, M, Ci, L, gw_partial, stream, xs, xh, xrelu);
}

template <typename TO>
static int pooled_dgrad_impl(const char *what, const float *g_pooled, const int32_t *pos, const float *W, int B, int C, int M, int C1, int C2,
                             int L, void *ws, TO *gx1, TO *gx2, sonet_stream_t stream, const PdTail *tail = nullptr, double *tail_sums = nullptr)
{
    SONET_REQUIRE(g_pooled && pos && W && ws && gx1, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && M > 0 && C1 > 0 && C2 >= 0 && L > 0, "%s: non-positive size", what);
    SONET_REQUIRE((C2 == 0) == (gx2 == nullptr), "%s: gx2 and C2 disagree", what);
    const int Cin = C1 + C2, E = C * M, ntile = sonet::ceil_div(L, PD_TL), nbucket = sonet::ceil_div(L, PD_SB);
    if ((long long)C * M >= (1 << 20) || B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: C*M=%d entries per cloud (max 2^20)", what, E);
    const size_t lds2 = ((size_t)PD_TL * (PD_CH + 1) + (size_t)PD_CQ * 3 * PD_SQ) * 4;
    if ((size_t)(2 * nbucket + 1) * 4 > 64 * 1024) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: L=%d too large for the bucket counters", what, L);
    uint32_t *ent_key = reinterpret_cast<uint32_t *>(ws);
    float *ent_val = reinterpret_cast<float *>(ent_key + (size_t)B * E);
    uint32_t *skey = reinterpret_cast<uint32_t *>(ent_val + (size_t)B * E);
    int32_t *tile_off = reinterpret_cast<int32_t *>(skey + (size_t)B * E);
    hipStream_t st = sonet::as_stream(stream);
    int abl = 0;
    if (const char *e = sonet::knob("SONET_PD_ABL")) abl = atoi(e);
    hipLaunchKernelGGL(pooled_bucket_kernel, dim3(B, PB_Q), dim3(1024), (size_t)(2 * sonet::ceil_div(nbucket, PB_Q) + 1) * 4, st, pos, g_pooled, E, L, nbucket, tile_off, ent_key, ent_val);
    if (!(abl & 4)) hipLaunchKernelGGL(pooled_sort_kernel, dim3(nbucket, B), dim3(64), 0, st, tile_off, ent_key, skey, E, nbucket);
    int one = 0;
    if (const char *e = sonet::knob("SONET_PD_ONE")) one = atoi(e);     // (variants build: 1 = the one-channel-per-thread kernel)
    int which = PD_SPARSE_KERNEL;
    if (const char *e = sonet::knob("SONET_PD_KERNEL")) which = atoi(e);   // (variants build: 4 = column-owned sub-ranges, 5 = equal-length chunks)
    if (tail && !(Cin % 4 == 0 && abl == 0 && !one && which == 5 && sizeof(TO) == 4))
        return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: the tail needs f32 outputs and C1 + C2 a multiple of 4", what);
    if (Cin % 4 == 0 && abl == 0 && !one && which == 5) {
        const size_t lds5 = (size_t)PD_TL * PD4_LD * 4 + (size_t)PD5_G * PD_CH * 4 + (size_t)PD5_R * 16;
#ifdef SONET_VARIANTS
        if (tail) {
            if constexpr (sizeof(TO) == 4) {
                hipLaunchKernelGGL((pooled_dgrad5_kernel<TO, true>), dim3(ntile, B, sonet::ceil_div(Cin, PD_CH)), dim3(PD_CH * PD_CQ), lds5, st, tile_off, skey, g_pooled, W, E, M,
                                   Cin, C1, L, nbucket, gx1, gx2 ? gx2 : gx1, *tail);
                if (tail->sraw) hipLaunchKernelGGL(pd_sums_finalize_kernel, dim3((unsigned)C2), dim3(256), 0, st, tail->spart, B * ntile, C2, tail_sums);
                return sonet::launched(what);
            }
        }
#endif
        hipLaunchKernelGGL(pooled_dgrad5_kernel<TO>, dim3(ntile, B, sonet::ceil_div(Cin, PD_CH)), dim3(PD_CH * PD_CQ), lds5, st, tile_off, skey, g_pooled, W, E, M, Cin, C1,
                           L, nbucket, gx1, gx2 ? gx2 : gx1, PdTail{nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr});
        return sonet::launched(what);
    }
#ifdef SONET_VARIANTS
    if (Cin % 4 == 0 && abl == 0 && !one && which == 4) {
        const size_t lds4 = (size_t)PD_TL * PD4_LD * 4 + (size_t)PD_CQ * PD_SQ * 16;
        hipLaunchKernelGGL(pooled_dgrad4_kernel<TO>, dim3(ntile, B, sonet::ceil_div(Cin, PD_CH)), dim3(PD_CH * PD_CQ), lds4, st, tile_off, skey, g_pooled, W, E, M, Cin, C1,
                           L, nbucket, gx1, gx2 ? gx2 : gx1);
        return sonet::launched(what);
    }
#endif
    hipLaunchKernelGGL(pooled_dgrad_kernel<TO>, dim3(ntile, B, sonet::ceil_div(Cin, PD_CH)), dim3(PD_CH * PD_CQ), lds2, st, tile_off, (abl & 4) ? ent_key : skey, ent_val, g_pooled, W, E, M, Cin, C1,
                       L, nbucket, gx1, gx2 ? gx2 : gx1, abl);
    return sonet::launched(what);
}

extern "C" int sonet_pooled_dgrad_f32(const float *g_pooled, const int32_t *pos, const float *W, int B, int C, int M, int C1, int C2,
                                      int L, void *ws, float *gx1, float *gx2, sonet_stream_t stream)
{
    return pooled_dgrad_impl<float>("sonet_pooled_dgrad_f32", g_pooled, pos, W, B, C, M, C1, C2, L, ws, gx1, gx2, stream);
}

#ifdef SONET_VARIANTS
// (variants build only: riding on the store of the sparse input gradient measured slower than the launches it replaces, docs/findings.md R5.14)
extern "C" size_t sonet_pooled_dgrad_tail_ws_size(int B, int C2, int L)
{
    if (B <= 0 || C2 <= 0 || L <= 0) return 0;
    return (size_t)B * sonet::ceil_div(L, PD_TL) * C2 * 2 * sizeof(double);
}

/* sonet_pooled_dgrad_f32 with what used to follow it riding on the store (C1 + C2 a multiple of 4):
 *  col0 [B][C1 + C2], pos0 [B] (both or neither): gx[b][:, pos0[b]] += col0[b] -- the dense part of the gradient (the entries of empty nodes all
 *    gather one column, models/networks.py:185; the caller computes their mat-vec);
 *  sraw [B][C2][L], ssc, ssh [C2], srelu, tail_ws (sonet_pooled_dgrad_tail_ws_size bytes), sums [2 C2] (all or none, C2 > 0): gx2 is gy of the
 *    BatchNorm (+ ReLU) layer whose RAW output is sraw; sums[0 .. C2) = sum over (b, l) of gy * mask, sums[C2 .. 2 C2) = sum of gy * mask * raw,
 *    mask = !srelu || raw * ssc + ssh > 0 -- the sums sonet_pointwise_bwd_stats_f32 computes from one more pass over (gy, raw); fixed order. */
extern "C" int sonet_pooled_dgrad_tail_f32(const float *g_pooled, const int32_t *pos, const float *W, int B, int C, int M, int C1, int C2,
                                           int L, void *ws, float *gx1, float *gx2, const float *col0, const int32_t *pos0,
                                           const float *sraw, const float *ssc, const float *ssh, int srelu, void *tail_ws, double *sums,
                                           sonet_stream_t stream)
{
    const char *what = "sonet_pooled_dgrad_tail_f32";
    SONET_REQUIRE((col0 == nullptr) == (pos0 == nullptr), "%s: col0 and pos0 come together", what);
    SONET_REQUIRE((sraw == nullptr) == (tail_ws == nullptr) && (sraw == nullptr) == (sums == nullptr) && (!sraw || (ssc && ssh && C2 > 0 && gx2)),
                  "%s: the sums need sraw, ssc, ssh, a workspace, the output and a second panel", what);
    const PdTail t = {col0, pos0, sraw, ssc, ssh, srelu, reinterpret_cast<double *>(tail_ws)};
    return pooled_dgrad_impl<float>(what, g_pooled, pos, W, B, C, M, C1, C2, L, ws, gx1, gx2, stream, &t, sums);
}
#endif /* SONET_VARIANTS */

/* gradients written as bfloat16 bit patterns (f32 accumulation in LDS as above, one rounding on the store) */
extern "C" int sonet_pooled_dgrad_obf16(const float *g_pooled, const int32_t *pos, const float *W, int B, int C, int M, int C1, int C2,
                                        int L, void *ws, uint16_t *gx1, uint16_t *gx2, sonet_stream_t stream)
{
    return pooled_dgrad_impl<uint16_t>("sonet_pooled_dgrad_obf16", g_pooled, pos, W, B, C, M, C1, C2, L, ws, gx1, gx2, stream);
}

/* The same gradient on the matrix cores: wt_pack = sonet_pointmlp_bf16_pack of W^T ([C1 + C2][C], i.e. Cin = C, Cout = C1 + C2 padded
 * to 32-row tiles); g and W rounded to bf16, f32 accumulate; L even, C a multiple of 16, (C1 + C2) / 32 tiles even and <= 12, C <= 384. */
extern "C" int sonet_pooled_dgrad_mfma_bf16(const float *g_pooled, const int32_t *pos, const void *wt_pack, int B, int C, int M, int C1, int C2,
                                            int L, void *ws, uint16_t *gx1, uint16_t *gx2, sonet_stream_t stream)
{
    const char *what = "sonet_pooled_dgrad_mfma_bf16";
    SONET_REQUIRE(g_pooled && pos && wt_pack && ws && gx1, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && M > 0 && C1 > 0 && C2 >= 0 && L > 0, "%s: non-positive size", what);
    SONET_REQUIRE((C2 == 0) == (gx2 == nullptr), "%s: gx2 and C2 disagree", what);
    const int Cin = C1 + C2, E = C * M, CT = sonet::ceil_div(Cin, 32), nbucket = sonet::ceil_div(L, PD_SB);
    if ((L & 1) || C % 16 || C * 2 + 16 > PM_PITCH || (CT & 1) || CT > 12 || (long long)C * M >= (1 << 20) || B > 65535 ||
        (size_t)(2 * nbucket + 1) * 4 > 64 * 1024 || ((reinterpret_cast<uintptr_t>(gx1) | reinterpret_cast<uintptr_t>(gx2)) & 3))
        return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: shape B=%d C=%d M=%d C1=%d C2=%d L=%d not supported", what, B, C, M, C1, C2, L);
    uint32_t *ent_key = reinterpret_cast<uint32_t *>(ws);
    float *ent_val = reinterpret_cast<float *>(ent_key + (size_t)B * E);
    int32_t *tile_off = reinterpret_cast<int32_t *>(ent_val + (size_t)B * E);
    hipStream_t st = sonet::as_stream(stream);
    hipLaunchKernelGGL(pooled_bucket_kernel, dim3(B, PB_Q), dim3(1024), (size_t)(2 * sonet::ceil_div(nbucket, PB_Q) + 1) * 4, st, pos, g_pooled, E, L, nbucket, tile_off, ent_key, ent_val);
    // 128-column workgroups (four waves, one per CU: W^T crosses the L2 once per 128 columns) on big launches, 64-column ones otherwise
    int ch = (long long)B * sonet::ceil_div(L, 2 * PM_TL) >= 2048 ? 2 : 1;
    if (const char *e = sonet::knob("SONET_PM_CH")) { const int v = atoi(e); if (v == 1 || v == 2) ch = v; }
    const int ntile_l = sonet::ceil_div(L, PM_TL * ch);
    size_t lds = (size_t)2 * 32 * ch * PM_PITCH;
    if (ch == 2 && (size_t)CT * 32 * 272 > lds) lds = (size_t)CT * 32 * 272;          // (the output tile reuses the image)
    const uint4 *wtp = reinterpret_cast<const uint4 *>(wt_pack);
    uint16_t *g2 = gx2 ? gx2 : gx1;
#define PM_LAUNCH1(NN, CC) do { if (const int rc_ = sonet::launch_lds_once<&pooled_dgrad_mfma_kernel<NN, CC>, 128 * 1024>(what, dim3(ntile_l, B), dim3(128 * CC), lds, st, \
                tile_off, ent_key, ent_val, wtp, E, M, C, C / 16, C1, C2, L, nbucket, gx1, g2)) return rc_; } while (0)
#define PM_LAUNCH(NN) do { if (ch == 2) PM_LAUNCH1(NN, 2); else PM_LAUNCH1(NN, 1); } while (0)
    switch (CT / 2) {
        case 1: PM_LAUNCH(1); break;
        case 2: PM_LAUNCH(2); break;
        case 3: PM_LAUNCH(3); break;
        case 4: PM_LAUNCH(4); break;
        case 5: PM_LAUNCH(5); break;
        default: PM_LAUNCH(6); break;
    }
#undef PM_LAUNCH1
#undef PM_LAUNCH
    return sonet::launched(what);
}

// ---- small-batch fully connected layer (classifier / decoder heads in eval mode) --------------------------------------
// y[b][o] = act((sum_k x[b][k] * W[o][k]) * scale[o] + shift[o]),  x [B][Cin], W [Cout][Cin] (nn.Linear layout), exact f32
// fma chains.  MyLinear (models/layers.py:123-166) on a B x C feature: three of these (1024 -> 512 -> 256 -> 40)
// replace ~12 aten launches (GEMM + bias, batch-norm transform, clamp).
namespace {
// The layer is a latency problem (67 MFLOP at B = 64, three of them in a row): the work is cut into many small workgroups and
// every memory request of a thread is in flight before its first fma.  One workgroup = FC_ROWS = 16 rows x FC_OC = 8 outputs;
// thread (row, ks) owns every 16th float4 of its row (the 16 ks lanes of a row read 256 consecutive bytes), its 8 weight rows
// sit in LDS in the order the lanes walk k (ws[k % 4][k / 4][8]: the 16 lanes of an LDS read touch consecutive 32-byte slots);
// the 16 k slices of a row meet in LDS and are summed in a fixed order.  1024 -> 512 at B = 64: 256 workgroups.
// (Round 1: 64 rows x 2-4 outputs per workgroup, every lane reading its own row -- 64 cache lines per load instruction -- and
// each workgroup pulling all of x: 22 us.  A version that staged x through LDS in chunks, 64 workgroups: 29-34 us, one wave per
// SIMD waiting for each chunk.)
constexpr int FC_ROWS = 16, FC_OC = 8, FC_KS = 16, FC_MAXJ = 16;   // FC_MAXJ float4 per thread and pass: 1024 columns
template <bool MULTI /*Cin > 1024: more than one pass*/>
__global__ __launch_bounds__(256) void linear_act_kernel(const float *__restrict__ x, const float *__restrict__ W,
                                                          const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                          float *__restrict__ y, int B, int Cin, int Cout, int nj /*float4 per thread*/)
{
    extern __shared__ __attribute__((aligned(16))) float fc_lds[];   // ws[4][K4][8] | part[16][16][8]
    const int K4 = nj * FC_KS;                                    // padded Cin / 4
    float *ws = fc_lds;
    float *part = ws + (size_t)4 * K4 * FC_OC;
    const int ks = threadIdx.x & 15, rr = threadIdx.x >> 4;
    const int o0 = blockIdx.x * FC_OC, row = blockIdx.y * FC_ROWS + rr;
    const bool vec = (Cin & 3) == 0;
    // x first: the requests travel while the weights are staged.  A pass covers FC_MAXJ float4 per thread = 1024 columns; wider layers
    // (Cin up to 4096: the weights of all passes sit in LDS) run the pass loop again with the accumulators kept.
    float4 xv[FC_MAXJ];
    auto fetch = [&](int j0) {
#pragma unroll
        for (int j = 0; j < FC_MAXJ; ++j) {
            xv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int k = ((j0 + j) * FC_KS + ks) * 4;
            if (j0 + j < nj && row < B && k < Cin) {
                const float *src = x + (size_t)row * Cin + k;
                if (vec) xv[j] = *reinterpret_cast<const float4 *>(src);
                else {
                    xv[j].x = src[0];
                    if (k + 1 < Cin) xv[j].y = src[1];
                    if (k + 2 < Cin) xv[j].z = src[2];
                    if (k + 3 < Cin) xv[j].w = src[3];
                }
            }
        }
    };
    fetch(0);
    // weights: float4 along k, eight requests per thread in flight at a time; zero past Cin / Cout
    for (int i0 = 0; i0 < FC_OC * K4; i0 += 8 * 256) {
        float4 wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 256 + (int)threadIdx.x, q = i / K4, k = (i - q * K4) * 4;
            wv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < FC_OC * K4 && o0 + q < Cout && k < Cin) {
                const float *src = W + (size_t)(o0 + q) * Cin + k;
                if (vec) wv[u] = *reinterpret_cast<const float4 *>(src);
                else {
                    wv[u].x = src[0];
                    if (k + 1 < Cin) wv[u].y = src[1];
                    if (k + 2 < Cin) wv[u].z = src[2];
                    if (k + 3 < Cin) wv[u].w = src[3];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 256 + (int)threadIdx.x, q = i / K4, k4 = i - q * K4;
            if (i < FC_OC * K4) {
                ws[(0 * K4 + k4) * FC_OC + q] = wv[u].x;
                ws[(1 * K4 + k4) * FC_OC + q] = wv[u].y;
                ws[(2 * K4 + k4) * FC_OC + q] = wv[u].z;
                ws[(3 * K4 + k4) * FC_OC + q] = wv[u].w;
            }
        }
    }
    __syncthreads();
    float acc[FC_OC];
#pragma unroll
    for (int q = 0; q < FC_OC; ++q) acc[q] = 0.f;
    for (int j0 = 0; j0 < (MULTI ? nj : 1); j0 += FC_MAXJ) {   // (single pass: straight-line code, measured 1.6 us faster on 1024 -> 512)
        if (MULTI && j0 > 0) fetch(j0);
#pragma unroll
        for (int j = 0; j < FC_MAXJ; ++j) {
            if (j0 + j < nj) {
                const float xe[4] = {xv[j].x, xv[j].y, xv[j].z, xv[j].w};
                const float4 *wp = reinterpret_cast<const float4 *>(ws + (size_t)((j0 + j) * FC_KS + ks) * FC_OC);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float4 w0 = wp[(size_t)e * K4 * 2], w1 = wp[(size_t)e * K4 * 2 + 1];
                    acc[0] = __fmaf_rn(xe[e], w0.x, acc[0]); acc[1] = __fmaf_rn(xe[e], w0.y, acc[1]);
                    acc[2] = __fmaf_rn(xe[e], w0.z, acc[2]); acc[3] = __fmaf_rn(xe[e], w0.w, acc[3]);
                    acc[4] = __fmaf_rn(xe[e], w1.x, acc[4]); acc[5] = __fmaf_rn(xe[e], w1.y, acc[5]);
                    acc[6] = __fmaf_rn(xe[e], w1.z, acc[6]); acc[7] = __fmaf_rn(xe[e], w1.w, acc[7]);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < FC_OC; ++q) part[(rr * FC_KS + ks) * FC_OC + q] = acc[q];
    __syncthreads();
    if (threadIdx.x < FC_ROWS * FC_OC) {
        const int r2 = threadIdx.x >> 3, q = threadIdx.x & 7;
        const int o = o0 + q, row2 = blockIdx.y * FC_ROWS + r2;
        if (o < Cout && row2 < B) {
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < FC_KS; ++t) sum += part[(r2 * FC_KS + t) * FC_OC + q];
            float v = __fmaf_rn(sum, scale[o], shift[o]);
            if (relu) v = (v < 0.f) ? 0.f : v;
            y[(size_t)row2 * Cout + o] = v;
        }
    }
}
}  // namespace

extern "C" int sonet_linear_act_f32(const float *x, const float *W, const float *scale, const float *shift, int relu, float *y,
                                    int B, int Cin, int Cout, sonet_stream_t stream)
{
    const char *what = "sonet_linear_act_f32";
    SONET_REQUIRE(x && W && scale && shift && y, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && Cin > 0 && Cout > 0, "%s: non-positive size", what);
    // (the kernel reads x and W with 16-byte loads whenever Cin % 4 == 0: the rows then start on a 16-byte boundary iff the bases do)
    SONET_REQUIRE((Cin & 3) != 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W)) & 15) == 0,
                  "%s: x and W must be 16-byte aligned when Cin %% 4 == 0 (misaligned)", what);
    const int rows = sonet::ceil_div(B, FC_ROWS);
    if (rows > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B=%d too large", what, B);
    const int nj = sonet::ceil_div(Cin, 4 * FC_KS);
    if (Cin > 4096) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: Cin=%d too large (max 4096: the workgroup's 8 weight rows sit in LDS)", what, Cin);
    const size_t lds = ((size_t)4 * nj * FC_KS * FC_OC + FC_ROWS * FC_KS * FC_OC) * sizeof(float);
    dim3 grid(sonet::ceil_div(Cout, FC_OC), rows), block(256);
    hipStream_t st = sonet::as_stream(stream);
    static bool raised = false;                                   // (dynamic LDS above 64 KiB has to be asked for: Cin > 1792)
    if (lds > 64 * 1024 && !raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&linear_act_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(&linear_act_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024) != hipSuccess)
            return sonet::fail(SONET_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit", what);
        raised = true;
    }
    if (nj > FC_MAXJ) hipLaunchKernelGGL(linear_act_kernel<true>, grid, block, lds, st, x, W, scale, shift, relu, y, B, Cin, Cout, nj);
    else              hipLaunchKernelGGL(linear_act_kernel<false>, grid, block, lds, st, x, W, scale, shift, relu, y, B, Cin, Cout, nj);
    return sonet::launched(what);
}
