// retrieval.hip -- class-restricted ranked neighbour lists: for every query shape the members of its own class, ascending by the
// Euclidean distance of their feature rows, the first `top` of them.
//
// Replaces the neighbour stage of the reference's retrieval evaluation (shrec16/test.py:68-99): per test shape one Python iteration
// of torch.eq + torch.nonzero over all labels, a gathered K x 55 matrix, torch.norm, torch.sort and two device-to-host copies.
//
// Prologue (five small launches): labels (given, or the arg-max of the feature row by torch.max's CPU rule) and their histogram;
// an exclusive scan of the histogram; one workgroup per non-empty class compacts the class's gallery indices in ascending order (a
// stable counting sort: the position of a shape inside its class list is the number of earlier shapes of that class -- ballots and
// a running count, no arrival order anywhere); the features re-laid class-sorted and channel-major, so that the lanes of a wave read
// consecutive class members of one channel.
// Hot path (one launch, one workgroup per query): 64-bit keys (bits of d2, position in the class list) formed in LDS, sorted there
// by a bitonic network, the first min(K, top) written out.  A class larger than one LDS load is consumed in chunks with the best
// `top` carried: the key order is total, so the list is the one a single sort of everything gives.  The Q x K distance matrix never
// exists in HBM.  Integer atomics only (the histogram and the bad count): two runs give the same bits.
#include "common.hpp"
#include <type_traits>

namespace {
constexpr int RT_THREADS = 256;
constexpr int RT_WAVES = RT_THREADS / sonet::WAVE;
constexpr int RT_HOT_THREADS = 256;                // threads of a query's workgroup
constexpr int RT_CHUNK = 2048;                     // keys one workgroup sorts in LDS at a time (docs/findings.md, "Retrieval lists")
constexpr int RT_MAX_TOP = 1024;
constexpr int RT_MAX_D = 1024;
constexpr int RT_MAX_LABEL = 65535;
constexpr int RT_BINS = RT_MAX_LABEL + 1;          // ws: hist [RT_BINS] | off [RT_BINS] | lab [N] | order [N] | featT [D][N]
constexpr unsigned RT_NAN = 0x7FC00000u;           // every NaN d2 becomes this pattern: after +inf (0x7F800000) in the key order
constexpr unsigned long long RT_PAD = ~0ull;       // padding key: after every real key

int chunk_keys()
{
    int ck = RT_CHUNK;
    if (const char *e = sonet::knob("SONET_RETRIEVAL_CHUNK")) {          // (variants build only: the sweep of tools/bench_retrieval.py)
        const int v = atoi(e);
        if (v >= 2 * RT_MAX_TOP && v <= 16384 && (v & (v - 1)) == 0) ck = v;
    }
    return ck;
}

int hot_threads()
{
    if (const char *e = sonet::knob("SONET_RETRIEVAL_THREADS")) {        // (variants build only)
        const int v = atoi(e);
        if (v == 256 || v == 512 || v == 1024) return v;
    }
    return RT_HOT_THREADS;
}

__global__ __launch_bounds__(256) void retrieval_zero_kernel(int32_t *__restrict__ hist, int32_t *__restrict__ bad, int n_label)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n_label) hist[t] = 0;
    if (t == 0) bad[0] = 0;
}

// One thread per shape.  lab[j] = the label used, -1 when it is outside [0, n_label).
__global__ __launch_bounds__(64) void retrieval_label_kernel(const float *__restrict__ feat, const int64_t *__restrict__ label,
                                                             int32_t *__restrict__ lab, int32_t *__restrict__ label_out,
                                                             int32_t *__restrict__ hist, int32_t *__restrict__ bad, int n_label, int N,
                                                             int D)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    bool oob = false;
    if (j < N) {
        int l;
        if (label) {
            const long long v = label[j];
            l = v >= 0 && v < n_label ? (int)v : -1;
        } else {
            // torch.max(dim=1) on CPU tensors: first of equal maxima, a NaN beats every number, the first NaN wins
            const float *p = feat + (size_t)j * D;
            float best = p[0];
            l = 0;
            for (int c = 1; c < D; ++c) {
                const float x = p[c];
                const bool take = x > best || (x != x && best == best);
                best = take ? x : best;
                l = take ? c : l;
            }
            if (l >= n_label) l = -1;                        // (n_label == D is required: never taken)
        }
        lab[j] = l;
        if (label_out) label_out[j] = l;
        if (l >= 0) atomicAdd(&hist[l], 1);
        oob = l < 0;
    }
    const int n_oob = __popcll(__ballot(oob));
    if (n_oob && (threadIdx.x & (sonet::WAVE - 1)) == 0) atomicAdd(bad, n_oob);
}

// off[c] = hist[0] + .. + hist[c - 1], off[n_label] = shapes with a good label.  One workgroup.
__global__ __launch_bounds__(1024) void retrieval_scan_kernel(const int32_t *__restrict__ hist, int32_t *__restrict__ off, int n_label)
{
    __shared__ int part[1024];
    const int tid = threadIdx.x, per = (n_label + 1023) / 1024;
    const int lo = min(tid * per, n_label), hi = min(lo + per, n_label);
    int s = 0;
    for (int c = lo; c < hi; ++c) s += hist[c];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 1024; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
        }
        off[n_label] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int c = lo; c < hi; ++c) {
        off[c] = run;
        run += hist[c];
    }
}

// One workgroup per class: its members in ascending gallery index (torch.nonzero's order).  order[off[c] + p] = the class's p-th
// member; p is "the position of j inside the class list" of the keys.
__global__ __launch_bounds__(RT_THREADS) void retrieval_compact_kernel(const int32_t *__restrict__ lab, const int32_t *__restrict__ hist,
                                                                       const int32_t *__restrict__ off, int32_t *__restrict__ order, int N)
{
    __shared__ int wcnt[RT_WAVES];
    const int c = blockIdx.x, K = hist[c];
    if (K == 0) return;
    const int base = off[c], tid = threadIdx.x, lane = tid & (sonet::WAVE - 1), wave = tid / sonet::WAVE;
    int run = 0;
    for (int j0 = 0; j0 < N && run < K; j0 += RT_THREADS) {
        const int j = j0 + tid;
        const bool m = j < N && lab[j] == c;
        const unsigned long long b = __ballot(m);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        int before = run, total = run;
#pragma unroll
        for (int w = 0; w < RT_WAVES; ++w) {
            before += w < wave ? wcnt[w] : 0;
            total += wcnt[w];
        }
        if (m) order[base + before + __popcll(b & ((1ull << lane) - 1ull))] = j;
        run = total;
        __syncthreads();
    }
}

// featT[c][s] = feat[order[s]][c] for the n_good = off[n_label] sorted slots: a 64 x 64 tile through LDS, both sides coalesced.
__global__ __launch_bounds__(RT_THREADS) void retrieval_relay_kernel(const float *__restrict__ feat, const int32_t *__restrict__ order,
                                                                     const int32_t *__restrict__ n_good_p, float *__restrict__ featT,
                                                                     int N, int D)
{
    __shared__ float tile[64][65];
    const int n_good = n_good_p[0];
    const int s0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    if (s0 >= n_good) return;
    const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
    for (int r = row; r < 64; r += RT_WAVES) {
        const int s = s0 + r, c = c0 + lane;
        if (s < n_good && c < D) tile[r][lane] = feat[(size_t)order[s] * D + c];
    }
    __syncthreads();
    for (int r = row; r < 64; r += RT_WAVES) {
        const int c = c0 + r, s = s0 + lane;
        if (c < D && s < n_good) featT[(size_t)c * N + s] = tile[lane][r];
    }
}

// d2 of the query row (LDS) and the class member at sorted slot s: c ascending, every operation rounded to f32, accumulator from +0.
__device__ __forceinline__ unsigned d2_bits(const float *__restrict__ q, const float *__restrict__ col, size_t N, int D)
{
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < D; ++c) {
        const float t = __fsub_rn(q[c], col[(size_t)c * N]);
        acc = __fadd_rn(acc, __fmul_rn(t, t));
    }
    return acc != acc ? RT_NAN : __float_as_uint(acc);
}

__device__ __forceinline__ void compare_exchange(unsigned long long *buf, int i, int j, int k)
{
    const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
    const unsigned long long a = buf[lo], b = buf[hi];
    if ((a > b) == ((lo & k) == 0)) {
        buf[lo] = b;
        buf[hi] = a;
    }
}

// Bitonic network over P keys (a power of two), T threads, thread t owning the pairs t, t + T, ...  The stages with a stride above 64
// end in a workgroup barrier.  At strides 64 .. 1 the 64 pairs of a wave stay inside one block of 128 keys, which no other wave touches:
// those stages run back to back per block, ordered by the wave's own in-order LDS queue, and one barrier closes them.
template <int T>
__device__ __forceinline__ void bitonic_sort(unsigned long long *buf, int P, int tid)
{
    for (int k = 2; k <= P; k <<= 1) {
        int j = k >> 1;
        for (; j > 64; j >>= 1) {
            for (int i = tid; i < (P >> 1); i += T) compare_exchange(buf, i, j, k);
            __syncthreads();
        }
        for (int i = tid; i < (P >> 1); i += T) {
            for (int jj = j; jj > 0; jj >>= 1) {
                compare_exchange(buf, i, jj, k);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}

template <int T>
__global__ __launch_bounds__(T) void retrieval_lists_kernel(
    const float *__restrict__ feat, const float *__restrict__ featT, const int64_t *__restrict__ ids, const int32_t *__restrict__ query,
    const int32_t *__restrict__ lab, const int32_t *__restrict__ hist, const int32_t *__restrict__ off, const int32_t *__restrict__ order,
    int top, int CK, int64_t *__restrict__ nn_id, float *__restrict__ nn_dist, int32_t *__restrict__ nn_pos, int32_t *__restrict__ count,
    int32_t *__restrict__ bad, int N, int D)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *buf = reinterpret_cast<unsigned long long *>(smem);            // [CK]
    float *q = reinterpret_cast<float *>(smem + (size_t)CK * sizeof(unsigned long long));   // [D]
    const int qi = blockIdx.x, tid = threadIdx.x;
    const int i = query ? query[qi] : qi;
    const bool i_ok = i >= 0 && i < N;
    const int l = i_ok ? lab[i] : -1;
    int cnt = 0, base = 0;
    if (l >= 0) {
        const int K = hist[l];
        base = off[l];
        for (int c = tid; c < D; c += T) q[c] = feat[(size_t)i * D + c];
        __syncthreads();
        int done = 0;
        while (done < K) {
            const int n_new = min(K - done, CK - cnt), n = cnt + n_new;
            for (int t = tid; t < n_new; t += T) {
                const int p = done + t;
                buf[cnt + t] = ((unsigned long long)d2_bits(q, featT + base + p, (size_t)N, D) << 32) | (unsigned)p;
            }
            int P = 2;
            while (P < n) P <<= 1;
            for (int t = n + tid; t < P; t += T) buf[t] = RT_PAD;
            __syncthreads();
            bitonic_sort<T>(buf, P, tid);
            done += n_new;
            cnt = min(n, top);
        }
    } else if (!i_ok && tid == 0) {
        atomicAdd(bad, 1);
    }
    const size_t o = (size_t)qi * top;
    for (int r = tid; r < top; r += T) {
        long long id = -1;
        int p = -1;
        float d = __uint_as_float(0x7F800000u);
        if (r < cnt) {
            const unsigned long long key = buf[r];
            const unsigned bits = (unsigned)(key >> 32);
            p = (int)(unsigned)key;
            const int j = order[base + p];
            id = ids ? ids[j] : (long long)j;
            d = bits == RT_NAN ? __uint_as_float(RT_NAN) : sqrtf(__uint_as_float(bits));
        }
        nn_id[o + r] = id;
        nn_dist[o + r] = d;
        if (nn_pos) nn_pos[o + r] = p;
    }
    if (tid == 0) count[qi] = cnt;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
}  // namespace

extern "C" int sonet_retrieval_chunk_keys(void) { return chunk_keys(); }

extern "C" size_t sonet_retrieval_ws_size(int N, int D, int Q, int top)
{
    if (N <= 0 || D <= 0 || Q <= 0 || top <= 0) return 0;
    return align16((size_t)2 * RT_BINS * 4 + (size_t)2 * N * 4) + (size_t)N * D * 4;
}

extern "C" int sonet_retrieval_lists_f32(const float *feat, const int64_t *label, const int64_t *ids, const int32_t *query, int n_label,
                                         int top, int64_t *nn_id, float *nn_dist, int32_t *nn_pos, int32_t *count, int32_t *label_out,
                                         int32_t *bad, void *ws, int N, int D, int Q, sonet_stream_t stream)
{
    const char *what = "sonet_retrieval_lists_f32";
    SONET_REQUIRE(feat && nn_id && nn_dist && count && bad && ws, "%s: NULL pointer", what);
    SONET_REQUIRE(N > 0 && D > 0 && Q > 0, "%s: non-positive size (N=%d D=%d Q=%d)", what, N, D, Q);
    SONET_REQUIRE(top >= 1 && top <= RT_MAX_TOP, "%s: top=%d outside [1, %d]", what, top, RT_MAX_TOP);
    SONET_REQUIRE(n_label >= 1 && n_label <= RT_MAX_LABEL, "%s: n_label=%d outside [1, %d]", what, n_label, RT_MAX_LABEL);
    SONET_REQUIRE(label || n_label == D, "%s: labels derived from the features need n_label == D, got n_label=%d D=%d", what, n_label, D);
    SONET_REQUIRE(query || Q == N, "%s: without a query list Q must be N, got Q=%d N=%d", what, Q, N);
    SONET_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "%s: ws must be 4-byte aligned", what);
    if (N >= (1 << 24)) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: N=%d >= 2^24", what, N);
    if (D > RT_MAX_D) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: D=%d > %d", what, D, RT_MAX_D);
    hipStream_t st = sonet::as_stream(stream);
    int32_t *hist = reinterpret_cast<int32_t *>(ws), *off = hist + RT_BINS, *lab = off + RT_BINS, *order = lab + N;
    float *featT = reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + align16((size_t)2 * RT_BINS * 4 + (size_t)2 * N * 4));
    const int CK = chunk_keys();
    const size_t lds = (size_t)CK * sizeof(unsigned long long) + (size_t)D * sizeof(float);
    hipLaunchKernelGGL(retrieval_zero_kernel, dim3(sonet::ceil_div(n_label, 256)), dim3(256), 0, st, hist, bad, n_label);
    hipLaunchKernelGGL(retrieval_label_kernel, dim3(sonet::ceil_div(N, 64)), dim3(64), 0, st, feat, label, lab, label_out, hist, bad,
                       n_label, N, D);
    hipLaunchKernelGGL(retrieval_scan_kernel, dim3(1), dim3(1024), 0, st, hist, off, n_label);
    hipLaunchKernelGGL(retrieval_compact_kernel, dim3(n_label), dim3(RT_THREADS), 0, st, lab, hist, off, order, N);
    hipLaunchKernelGGL(retrieval_relay_kernel, dim3(sonet::ceil_div(N, 64), sonet::ceil_div(D, 64)), dim3(RT_THREADS), 0, st, feat, order,
                       off + n_label, featT, N, D);
    auto hot = [&](auto tt) {
        constexpr int T = decltype(tt)::value;
        if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(retrieval_lists_kernel<T>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return sonet::fail(SONET_ERR_LAUNCH, "%s: LDS", what);
        hipLaunchKernelGGL(retrieval_lists_kernel<T>, dim3(Q), dim3(T), lds, st, feat, featT, ids, query, lab, hist, off, order, top, CK,
                           nn_id, nn_dist, nn_pos, count, bad, N, D);
        return (int)SONET_OK;
    };
    int rc;
    switch (hot_threads()) {
    case 1024: rc = hot(std::integral_constant<int, 1024>{}); break;
    case 512: rc = hot(std::integral_constant<int, 512>{}); break;
    default: rc = hot(std::integral_constant<int, 256>{}); break;
    }
    if (rc != SONET_OK) return rc;
    return sonet::launched(what);
}
