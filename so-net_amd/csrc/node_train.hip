// node_train.hip -- node-level pieces of the TRAINING step that ran on aten (rocprofv3 of the bf16 step: _scatter_gather_elementwise 0.23 ms,
// reduce_kernel<MaxOps> 0.18 ms, fills and the index expansion of torch.gather's backward):
//   * max over the last dimension WITH the arg-max (first maximum, as torch.max documents) and its backward -- the max over the K'
//     neighbours of KNNModule (models/layers.py:350-365: torch.max(dim=3)) and over the M nodes (models/networks.py:197);
//   * the backward of the neighbour gather (models/operations.py:38-54): gx[b][c][m] = sum over the (m', k) with knn_I[b][m'][k] == m of
//     g[b][c][m'][k], as a GATHER over per-cloud inverse lists (fixed summation order: bitwise reproducible; aten scatter-adds atomically);
//   * the same for the segmenter's back-broadcast of node-level maps to the point copies (models/segmenter.py:96-98): gx[b][c][m] = sum
//     of g[b][c][j] over the columns j whose node is m, in ascending j.
#include "common.hpp"

namespace {

// store of a value that came from storage of the same type (or 0): exact, so bf16 TRUNCATES -- not the rounding store st_rne (device.hpp)
__device__ __forceinline__ void st_exact(float *p, long long i, float v) { p[i] = v; }
__device__ __forceinline__ void st_exact(uint16_t *p, long long i, float v) { p[i] = (uint16_t)(__float_as_uint(v) >> 16); }

// one thread per row of K contiguous values: value and index of the FIRST maximum; a NaN wins (the first one), as torch.max
template <typename T>
__global__ __launch_bounds__(256) void lastdim_argmax_kernel(const T *__restrict__ x, T *__restrict__ out, int32_t *__restrict__ idx, int K, long long rows)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const long long base = r * K;
    float m = ld_f32(x, base);
    int mi = 0;
    for (int k = 1; k < K; ++k) {
        const float v = ld_f32(x, base + k);
        if (v > m || (v != v && m == m)) { m = v; mi = k; }
    }
    st_exact(out, r, m);
    idx[r] = mi;
}

// gx[r][k] = (k == idx[r]) ? g[r] : 0 : the whole row is written (no separate fill)
template <typename T>
__global__ __launch_bounds__(256) void lastdim_max_bwd_kernel(const T *__restrict__ g, const int32_t *__restrict__ idx, T *__restrict__ gx, int K, long long rows)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float gv = ld_f32(g, r);
    const int mi = idx[r];
    const long long base = r * K;
    for (int k = 0; k < K; ++k) st_exact(gx, base + k, k == mi ? gv : 0.f);
}

// inverse neighbour lists of one cloud: off[b][m] .. off[b][m+1] index into list[b][.] = the entries e = m' * K + k (ascending) whose
// neighbour is node m.  One workgroup per cloud, thread m owns node m (M <= 1024); entries with an index outside [0, M) belong to nobody.
__global__ __launch_bounds__(1024) void knn_inverse_kernel(const long long *__restrict__ knn_I, int M, int K, int32_t *__restrict__ off, int32_t *__restrict__ list)
{
    __shared__ int cnt[1025];
    extern __shared__ int Is[];                  // the cloud's E indices (out of range: -1).  Every thread walks all of them twice: straight
                                                 // from global memory that was 1152 dependent loads per thread, 87 us of the training step
    const int b = blockIdx.x, m = threadIdx.x;
    const long long *I = knn_I + (long long)b * M * K;
    const int E = M * K;
    for (int e = m; e < E; e += blockDim.x) {
        const long long i = I[e];
        Is[e] = (i >= 0 && i < M) ? (int)i : -1;
    }
    __syncthreads();
    int n = 0;
    if (m < M)
        for (int e = 0; e < E; ++e) n += (Is[e] == m);
    cnt[m] = m < M ? n : 0;
    __syncthreads();
    if (m == 0) {
        int acc = 0;
        for (int i = 0; i < M; ++i) { const int c = cnt[i]; cnt[i] = acc; acc += c; }
        cnt[M] = acc;
    }
    __syncthreads();
    // (M + 1 offsets from at most 1024 threads: at M == 1024 thread 0 also writes the closing one)
    for (int i = m; i <= M; i += blockDim.x) off[(long long)b * (M + 1) + i] = cnt[i];
    if (m < M) {
        int w = cnt[m];
        int32_t *L = list + (long long)b * E;
        for (int e = 0; e < E; ++e)
            if (Is[e] == m) L[w++] = e;
    }
}

// one thread per (b, c, m): the sum of its list's entries of g[b][c][.], in list order, f32 accumulation
template <typename T>
__global__ __launch_bounds__(256) void knn_gather_bwd_kernel(const T *__restrict__ g, const int32_t *__restrict__ off, const int32_t *__restrict__ list,
                                                              float *__restrict__ gx, int C, int M, int K, long long total)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int m = (int)(t % M);
    const long long bc = t / M;
    const int b = (int)(bc / C);
    const int32_t *o = off + (long long)b * (M + 1);
    const int32_t *L = list + (long long)b * M * K;
    const long long base = bc * (long long)M * K;
    float s = 0.f;
    for (int i = o[m]; i < o[m + 1]; ++i) s += ld_f32(g, base + L[i]);
    gx[t] = s;
}

// inverse node lists of one cloud: off[b][m] .. off[b][m+1] index into list[b][.] = the columns j (ascending) with ids[b][j] == m.  One
// workgroup per cloud, thread m owns node m (M <= 1024); the ids pass through LDS in chunks (every thread reads every id: broadcast);
// ids outside [0, M) belong to nobody.
constexpr int NGB_CHUNK = 8192;
__global__ __launch_bounds__(1024) void node_inverse_kernel(const int32_t *__restrict__ ids, int M, int L, int32_t *__restrict__ off,
                                                            int32_t *__restrict__ list)
{
    __shared__ int cnt[1025];
    __shared__ int Is[NGB_CHUNK];
    const int b = blockIdx.x, m = threadIdx.x;
    const int32_t *I = ids + (long long)b * L;
    int n = 0;
    for (int c0 = 0; c0 < L; c0 += NGB_CHUNK) {
        const int len = min(NGB_CHUNK, L - c0);
        __syncthreads();
        for (int e = m; e < len; e += blockDim.x) Is[e] = I[c0 + e];
        __syncthreads();
        if (m < M)
            for (int e = 0; e < len; ++e) n += (Is[e] == m);
    }
    cnt[m] = m < M ? n : 0;
    __syncthreads();
    if (m == 0) {
        int acc = 0;
        for (int i = 0; i < M; ++i) { const int c = cnt[i]; cnt[i] = acc; acc += c; }
        cnt[M] = acc;
    }
    __syncthreads();
    for (int i = m; i <= M; i += blockDim.x) off[(long long)b * (M + 1) + i] = cnt[i];
    int w = m < M ? cnt[m] : 0;
    int32_t *Lst = list + (long long)b * L;
    for (int c0 = 0; c0 < L; c0 += NGB_CHUNK) {
        const int len = min(NGB_CHUNK, L - c0);
        __syncthreads();
        for (int e = m; e < len; e += blockDim.x) Is[e] = I[c0 + e];
        __syncthreads();
        if (m < M)
            for (int e = 0; e < len; ++e)
                if (Is[e] == m) Lst[w++] = c0 + e;
    }
}

// one thread per (b, c, m): the sum of g[b][c][j] over its list, in list (= ascending column) order, f32 accumulation
template <typename T>
__global__ __launch_bounds__(256) void node_gather_bwd_kernel(const T *__restrict__ g, const int32_t *__restrict__ off, const int32_t *__restrict__ list,
                                                              float *__restrict__ gx, int C, int M, int L, long long total)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int m = (int)(t % M);
    const long long bc = t / M;
    const int b = (int)(bc / C);
    const int32_t *o = off + (long long)b * (M + 1);
    const int32_t *Lst = list + (long long)b * L;
    const long long base = bc * (long long)L;
    float s = 0.f;
    for (int i = o[m]; i < o[m + 1]; ++i) s += ld_f32(g, base + Lst[i]);
    gx[t] = s;
}

// The BatchNorm / ReLU backward of a layer (rowwise_kernel<1, float, false> of bn_passes.hip: bn_bwd_apply, operation for operation) and the per-node sums of what
// it stores in ONE pass over (gy, raw): the gradient of a per-node addend (segmenter layer 1 in its node-wise form) is the sum of
// g_raw over every node's columns, and a second launch would read the stored tensor again.  A workgroup owns ANS_ROWS channel rows of
// one cloud and walks them in tiles of ANS_TILE columns: g_raw is computed, stored and kept in LDS; then one thread per (row, node)
// adds the node's columns of the tile -- the next entries of its inverse list, which ascends -- to the partial sum it carries from tile
// to tile: one f32 chain per (b, c, m) in ascending column order, the bits of node_gather_bwd_kernel.  A pair p = row * M + m is always
// served by thread p % ANS_THREADS, so its partial sum and list cursor need no barrier of their own.
constexpr int ANS_ROWS = 4, ANS_TILE = 1024, ANS_THREADS = 256;
template <bool VEC>
__global__ __launch_bounds__(ANS_THREADS) void bwd_apply_nodesum_kernel(const float *__restrict__ gy, const float *__restrict__ raw,
                                                                         const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                                         const float *__restrict__ ca, const float *__restrict__ cb,
                                                                         const float *__restrict__ cc, const int32_t *__restrict__ off,
                                                                         const int32_t *__restrict__ list, float *__restrict__ out,
                                                                         float *__restrict__ gz, int C, int L, int M, int row_groups)
{
    extern __shared__ float ans_lds[];
    float *tile = ans_lds;                                    // [ANS_ROWS][ANS_TILE] g_raw of the current tile
    float *psum = tile + ANS_ROWS * ANS_TILE;                 // [ANS_ROWS * M] partial sums
    int *cur = reinterpret_cast<int *>(psum + (size_t)ANS_ROWS * M);     // [ANS_ROWS * M] next list entry of the pair
    const size_t b = blockIdx.x / (unsigned)row_groups;
    const int c_first = (int)(blockIdx.x % (unsigned)row_groups) * ANS_ROWS;
    const int nrows = min(ANS_ROWS, C - c_first);
    const int32_t *o = off + b * (size_t)(M + 1);
    const int32_t *lst = list + b * (size_t)L;
    const int npairs = nrows * M;
    for (int p = threadIdx.x; p < npairs; p += ANS_THREADS) {
        psum[p] = 0.f;
        cur[p] = o[p % M];
    }
    float sc[ANS_ROWS], sh[ANS_ROWS], a[ANS_ROWS], bb[ANS_ROWS], c0[ANS_ROWS];
#pragma unroll
    for (int r = 0; r < ANS_ROWS; ++r) {
        const int c = min(c_first + r, C - 1);
        sc[r] = scale[c]; sh[r] = shift[c]; a[r] = ca[c]; bb[r] = cb[c]; c0[r] = cc[c];
    }
    const size_t row0 = (b * (size_t)C + (size_t)c_first) * (size_t)L;
    for (int t0 = 0; t0 < L; t0 += ANS_TILE) {
        const int tlen = min(ANS_TILE, L - t0);
        __syncthreads();                                      // (the walk over the previous tile is over)
#pragma unroll
        for (int r = 0; r < ANS_ROWS; ++r) {
            if (r >= nrows) break;
            const size_t base = row0 + (size_t)r * (size_t)L + (size_t)t0;
            if constexpr (VEC) {                              // (L % 4 == 0 and 16-byte aligned operands: so is every row and tile)
                for (int i = threadIdx.x * 4; i < tlen; i += ANS_THREADS * 4) {
                    const float4 rv = *reinterpret_cast<const float4 *>(raw + base + i);
                    const float4 gv = *reinterpret_cast<const float4 *>(gy + base + i);
                    const float rr[4] = {rv.x, rv.y, rv.z, rv.w};
                    float gg[4] = {gv.x, gv.y, gv.z, gv.w};
                    float ov[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (relu && !(__fmaf_rn(rr[e], sc[r], sh[r]) > 0.f)) gg[e] = 0.f;
                        ov[e] = __fmaf_rn(a[r], gg[e], __fmaf_rn(bb[r], rr[e], c0[r]));
                    }
                    const float4 o4 = make_float4(ov[0], ov[1], ov[2], ov[3]);
                    *reinterpret_cast<float4 *>(out + base + i) = o4;
                    *reinterpret_cast<float4 *>(tile + r * ANS_TILE + i) = o4;
                }
            } else {
                for (int i = threadIdx.x; i < tlen; i += ANS_THREADS) {
                    const float rv = raw[base + i];
                    const float ov = bn_bwd_apply(gy[base + i], rv, sc[r], sh[r], relu, a[r], bb[r], c0[r]);
                    out[base + i] = ov;
                    tile[r * ANS_TILE + i] = ov;
                }
            }
        }
        __syncthreads();
        const int tend = t0 + tlen;
        for (int p = threadIdx.x; p < npairs; p += ANS_THREADS) {
            const int r = p / M, m = p - r * M;
            const int end = o[m + 1];
            const float *tr = tile + r * ANS_TILE;            // (every column read lies in [t0, tend): the list ascends)
            int k = cur[p];
            float s = psum[p];
            bool more = true;
            while (more && k < end) {
                // four list entries per round trip (clamped to the node's own range), added strictly in list order
                int col[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) col[e] = lst[min(k + e, end - 1)];
                const int n = min(4, end - k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (more && e < n) {
                        if (col[e] < tend) { s += tr[col[e] - t0]; ++k; }
                        else more = false;
                    }
                }
            }
            psum[p] = s;
            cur[p] = k;
        }
    }
    for (int p = threadIdx.x; p < npairs; p += ANS_THREADS) {
        const int r = p / M, m = p - r * M;
        gz[(b * (size_t)C + (size_t)(c_first + r)) * (size_t)M + (size_t)m] = psum[p];
    }
}

}  // namespace

template <typename T>
static int argmax_impl(const char *what, const T *x, T *out, int32_t *idx, long long rows, int K, sonet_stream_t stream)
{
    SONET_REQUIRE(x && out && idx, "%s: NULL pointer", what);
    SONET_REQUIRE(rows > 0 && K > 0, "%s: bad size", what);
    const long long blocks = sonet::ceil_div64(rows, 256);
    if (blocks > 0x7FFFFFFFll) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: too large", what);
    hipLaunchKernelGGL(lastdim_argmax_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, sonet::as_stream(stream), x, out, idx, K, rows);
    return sonet::launched(what);
}
template <typename T>
static int maxbwd_impl(const char *what, const T *g, const int32_t *idx, T *gx, long long rows, int K, sonet_stream_t stream)
{
    SONET_REQUIRE(g && gx && idx, "%s: NULL pointer", what);
    SONET_REQUIRE(rows > 0 && K > 0, "%s: bad size", what);
    const long long blocks = sonet::ceil_div64(rows, 256);
    if (blocks > 0x7FFFFFFFll) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: too large", what);
    hipLaunchKernelGGL(lastdim_max_bwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, sonet::as_stream(stream), g, idx, gx, K, rows);
    return sonet::launched(what);
}

extern "C" int sonet_lastdim_argmax_f32(const float *x, float *out, int32_t *idx, long long rows, int K, sonet_stream_t stream)
{
    return argmax_impl("sonet_lastdim_argmax_f32", x, out, idx, rows, K, stream);
}
extern "C" int sonet_lastdim_argmax_bf16(const uint16_t *x, uint16_t *out, int32_t *idx, long long rows, int K, sonet_stream_t stream)
{
    return argmax_impl("sonet_lastdim_argmax_bf16", x, out, idx, rows, K, stream);
}
extern "C" int sonet_lastdim_max_bwd_f32(const float *g, const int32_t *idx, float *gx, long long rows, int K, sonet_stream_t stream)
{
    return maxbwd_impl("sonet_lastdim_max_bwd_f32", g, idx, gx, rows, K, stream);
}
extern "C" int sonet_lastdim_max_bwd_bf16(const uint16_t *g, const int32_t *idx, uint16_t *gx, long long rows, int K, sonet_stream_t stream)
{
    return maxbwd_impl("sonet_lastdim_max_bwd_bf16", g, idx, gx, rows, K, stream);
}

extern "C" size_t sonet_knn_gather_bwd_ws_size(int B, int M, int K)
{
    if (B <= 0 || M <= 0 || K <= 0) return 0;
    return ((size_t)B * (M + 1) + (size_t)B * M * K) * sizeof(int32_t);
}

template <typename T>
static int gather_bwd_impl(const char *what, const T *g, const int64_t *knn_I, float *gx, void *ws, int B, int C, int M, int K, sonet_stream_t stream)
{
    SONET_REQUIRE(g && knn_I && gx && ws, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && M > 0 && K > 0, "%s: bad size", what);
    if (M > 1024) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: M=%d > 1024", what, M);
    int32_t *off = reinterpret_cast<int32_t *>(ws), *list = off + (size_t)B * (M + 1);
    hipStream_t s = sonet::as_stream(stream);
    if ((size_t)M * K * 4 > 56 * 1024) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: M*K=%d indices do not fit the LDS", what, M * K);
    hipLaunchKernelGGL(knn_inverse_kernel, dim3((unsigned)B), dim3(1024), (size_t)M * K * 4, s, reinterpret_cast<const long long *>(knn_I), M, K, off, list);
    const long long total = (long long)B * C * M;
    hipLaunchKernelGGL(knn_gather_bwd_kernel<T>, dim3((unsigned)sonet::ceil_div64(total, 256)), dim3(256), 0, s, g, off, list, gx, C, M, K, total);
    return sonet::launched(what);
}
extern "C" int sonet_knn_gather_bwd_f32(const float *g, const int64_t *knn_I, float *gx, void *ws, int B, int C, int M, int K, sonet_stream_t stream)
{
    return gather_bwd_impl("sonet_knn_gather_bwd_f32", g, knn_I, gx, ws, B, C, M, K, stream);
}
extern "C" int sonet_knn_gather_bwd_bf16(const uint16_t *g, const int64_t *knn_I, float *gx, void *ws, int B, int C, int M, int K, sonet_stream_t stream)
{
    return gather_bwd_impl("sonet_knn_gather_bwd_bf16", g, knn_I, gx, ws, B, C, M, K, stream);
}

extern "C" size_t sonet_node_gather_bwd_ws_size(int B, int M, int L)
{
    if (B <= 0 || M <= 0 || L <= 0) return 0;
    return ((size_t)B * (M + 1) + (size_t)B * L) * sizeof(int32_t);
}

template <typename T>
static int node_gather_bwd_impl(const char *what, const T *g, const int32_t *ids, float *gx, void *ws, int B, int C, int M, int L,
                                sonet_stream_t stream)
{
    SONET_REQUIRE(g && ids && gx && ws, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && M > 0 && L > 0, "%s: bad size", what);
    if (M > 1024) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: M=%d > 1024", what, M);
    const long long total = (long long)B * C * M;
    if (sonet::ceil_div64(total, 256) > 0x7FFFFFFFll) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: too large", what);
    int32_t *off = reinterpret_cast<int32_t *>(ws), *list = off + (size_t)B * (M + 1);
    hipStream_t s = sonet::as_stream(stream);
    hipLaunchKernelGGL(node_inverse_kernel, dim3((unsigned)B), dim3(1024), 0, s, ids, M, L, off, list);
    hipLaunchKernelGGL(node_gather_bwd_kernel<T>, dim3((unsigned)sonet::ceil_div64(total, 256)), dim3(256), 0, s, g, off, list, gx, C, M, L, total);
    return sonet::launched(what);
}
extern "C" int sonet_node_gather_bwd_f32(const float *g, const int32_t *ids, float *gx, void *ws, int B, int C, int M, int L, sonet_stream_t stream)
{
    return node_gather_bwd_impl("sonet_node_gather_bwd_f32", g, ids, gx, ws, B, C, M, L, stream);
}
extern "C" int sonet_node_gather_bwd_bf16(const uint16_t *g, const int32_t *ids, float *gx, void *ws, int B, int C, int M, int L, sonet_stream_t stream)
{
    return node_gather_bwd_impl("sonet_node_gather_bwd_bf16", g, ids, gx, ws, B, C, M, L, stream);
}

extern "C" size_t sonet_pointwise_bwd_apply_nodesum_ws_size(int B, int M, int L)
{
    return sonet_node_gather_bwd_ws_size(B, M, L);               // the inverse lists of node_inverse_kernel
}

extern "C" int sonet_pointwise_bwd_apply_nodesum_tile(void) { return ANS_TILE; }

/* sonet_pointwise_bwd_apply_f32 and sonet_node_gather_bwd_f32 of what it stores, in one pass over (gy, raw): g_raw [B][C][L] and
 * gz[b][c][m] = the sum of g_raw[b][c][l] over the columns with ids[b][l] == m in ascending column order (one f32 chain), the bits of
 * the two launches.  No atomics, no host synchronisation. */
extern "C" int sonet_pointwise_bwd_apply_nodesum_f32(const float *gy, const float *raw, const float *scale, const float *shift, int relu,
                                                     const float *a, const float *b, const float *c0, const int32_t *ids, int M,
                                                     float *g_raw, float *gz, void *ws, int B, int C, int L, sonet_stream_t stream)
{
    const char *what = "sonet_pointwise_bwd_apply_nodesum_f32";
    SONET_REQUIRE(gy && raw && scale && shift && a && b && c0 && ids && g_raw && gz && ws, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && M > 0 && L > 0, "%s: bad size B=%d C=%d M=%d L=%d", what, B, C, M, L);
    if (M > 1024) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: M=%d > 1024", what, M);
    const int row_groups = sonet::ceil_div(C, ANS_ROWS);
    const long long nwg = (long long)B * row_groups;
    if (nwg > 0x7FFFFFFFll) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: too large", what);
    int32_t *off = reinterpret_cast<int32_t *>(ws), *list = off + (size_t)B * (M + 1);
    hipStream_t s = sonet::as_stream(stream);
    hipLaunchKernelGGL(node_inverse_kernel, dim3((unsigned)B), dim3(1024), 0, s, ids, M, L, off, list);
    const size_t lds = ((size_t)ANS_ROWS * ANS_TILE + 2 * (size_t)ANS_ROWS * M) * sizeof(float);      // <= 48 KiB at M = 1024
    const bool vec = L % 4 == 0 && (((uintptr_t)gy | (uintptr_t)raw | (uintptr_t)g_raw) & 15) == 0;
    if (vec) hipLaunchKernelGGL(bwd_apply_nodesum_kernel<true>, dim3((unsigned)nwg), dim3(ANS_THREADS), lds, s, gy, raw, scale, shift, relu,
                                a, b, c0, off, list, g_raw, gz, C, L, M, row_groups);
    else     hipLaunchKernelGGL(bwd_apply_nodesum_kernel<false>, dim3((unsigned)nwg), dim3(ANS_THREADS), lds, s, gy, raw, scale, shift, relu,
                                a, b, c0, off, list, g_raw, gz, C, L, M, row_groups);
    return sonet::launched(what);
}
