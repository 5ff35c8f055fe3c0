// batch.hip -- training / test batch assembly on gfx950 (the per-step half of the data path): subsample + augment B clouds of a
// device-resident dataset in ONE launch, then the node self-kNN (sonet_knn_self_f32) as a second launch on the same stream.
//
// Replaces the DataLoader item of the reference (data/modelnet_shrec_loader.py:193-271, data/shapenet_loader.py:131-198,
// data/augmentation.py) and its collate.  One workgroup per output slot b (source cloud s = idx[b], n_s points, CSR offsets):
//   1. subsample  modelnet / shrec: N of n_s without replacement (N > n_s is an argument error, as np.random.choice raises);
//                 shapenet: N < n_s without replacement, otherwise all n_s in order and N - n_s more uniformly WITH replacement.
//                 Without replacement = the N smallest (key, index) pairs, key = a Philox draw per source point, found by an LDS
//                 radix select (8-bit digits, at most four histogram passes; the keys are recomputed in every pass, never stored, so
//                 n_s is bounded only by int32) and compacted in SOURCE order.  The random mode therefore emits the chosen points
//                 in ascending source index, the reference in np.random.choice's order: the network only sees the points through
//                 point-wise layers and max-pools, so the order does not change what it computes.  Replay mode takes the chosen
//                 indices as given, in their order.
//   2. augment    (train mode only) in float64, one rounding to float32 at the store, the reference's order and conventions
//                 (row vectors, x @ R): horizontal rotation, perturbation rotation, jitter, scale, shift (flags and recipe decide).
//   3. store      pc / sn [B][3][N] f32, node [B][3][M] f32, chosen [B][N] i64 (global source index).
// Random numbers: Philox4x32-10, key = seed, counter = (step, b, stream, element) -- include/sonet_hip.h has the whole mapping.  The
// draws of slot b depend on (seed, step, b) only.  Replay mode: the caller's draws replace the generator and run the same code below.
#include "common.hpp"
#include <math.h>

namespace {

constexpr int AB_THREADS = 256;
constexpr int AB_WAVES = AB_THREADS / sonet::WAVE;
constexpr int AB_SCALARS = SONET_BATCH_DRAW_SCALARS;

// ---- Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) ----------------------------------------------------------------
__device__ __forceinline__ uint4 philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ unsigned word(const uint4 &w, int q) { return q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w; }

constexpr double TWO_M32 = 2.3283064365386963e-10;       // 2^-32
constexpr double TWO_PI = 6.283185307179586;              // 2 * pi (double), = np.pi * 2 exactly

__device__ __forceinline__ double unit(unsigned w) { return (double)w * TWO_M32; }           // [0, 1)
// three standard normals from one Philox block: Box-Muller on (w0, w1) -> z0 = r cos t, z1 = r sin t; on (w2, w3) -> z2 = r cos t
__device__ __forceinline__ void normals3(const uint4 &w, double z[3]) {
    const double ra = sqrt(-2.0 * log(((double)w.x + 1.0) * TWO_M32)), ta = TWO_PI * unit(w.y);
    const double rb = sqrt(-2.0 * log(((double)w.z + 1.0) * TWO_M32)), tb = TWO_PI * unit(w.w);
    z[0] = ra * cos(ta); z[1] = ra * sin(ta); z[2] = rb * cos(tb);
}

__device__ __forceinline__ double clip(double v, double c) { return fmin(fmax(v, -c), c); }     // np.clip(v, -c, c)

// row vector times a 3x3 matrix (np.dot(x, R)), products summed left to right
__device__ __forceinline__ void rowmul(double p[3], const double *R) {
    const double a = p[0], b = p[1], c = p[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = (a * R[j] + b * R[3 + j]) + c * R[6 + j];
}
// 3x3 product A @ B
__device__ void matmul3(const double *A, const double *Bm, double *C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * Bm[j] + A[3 * i + 1] * Bm[3 + j]) + A[3 * i + 2] * Bm[6 + j];
}

struct SlotState {                  // per-slot values shared by the workgroup (LDS)
    long long o0;                   // global offset of the source cloud
    int n_s, ok, s;
    double Rh[9], Rp[9], scale, shift[3];
    unsigned hist[256];
    unsigned sel_digit, sel_below, sel_cnt;
    unsigned wsum[AB_WAVES];
};

// exclusive block scan of v (all threads take part); *total = the block sum
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned *wsum, unsigned *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                              // the previous call's readers are done with wsum
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < AB_WAVES; ++i) {
        before += i < w ? wsum[i] : 0u;
        all += wsum[i];
    }
    *total = all;
    return before + inc - v;
}

struct Args {
    const float *src; long long P; const int64_t *off; int S; const float *nodes_src; const int64_t *idx;
    int B, N, M, K, flags; unsigned k0, k1, step;
    const int64_t *replay_idx; const double *replay_draws; double *draws_out;
    float *pc, *sn, *node; int64_t *chosen, *knn_I; int32_t *bad;
};

// one output point: source point i (local) of the slot's cloud -> output column j, augmented (train) or copied (test)
__device__ __forceinline__ void emit_point(const Args &a, const SlotState &st, int b, int j, long long i) {
    const size_t N = (size_t)a.N;
    const size_t D = AB_SCALARS + 6 * N + 3 * (size_t)a.M;
    float *pcb = a.pc + (size_t)b * 3 * N, *snb = a.sn + (size_t)b * 3 * N;
    if (i < 0 || i >= st.n_s) {                                   // only a replayed index can be out of range
        if (a.bad) a.bad[b] = 1;
        a.chosen[(size_t)b * N + j] = -1;
        for (int c = 0; c < 3; ++c) { pcb[c * N + j] = __builtin_nanf(""); snb[c * N + j] = __builtin_nanf(""); }
        return;
    }
    const long long g = st.o0 + i;
    a.chosen[(size_t)b * N + j] = g;
    double p[3], n[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] = a.src[c * a.P + g]; n[c] = a.src[(3 + c) * a.P + g]; }
    if (a.flags & SONET_BATCH_TRAIN) {
        double zp[3], zn[3];
        if (a.replay_draws) {
            const double *r = a.replay_draws + (size_t)b * D + AB_SCALARS + 3 * (size_t)j;
#pragma unroll
            for (int c = 0; c < 3; ++c) { zp[c] = r[c]; zn[c] = r[3 * N + c]; }
        } else {
            normals3(philox(a.step, (unsigned)b, 3u, (unsigned)j, a.k0, a.k1), zp);
            normals3(philox(a.step, (unsigned)b, 4u, (unsigned)j, a.k0, a.k1), zn);
        }
        if (a.draws_out) {
            double *o = a.draws_out + (size_t)b * D + AB_SCALARS + 3 * (size_t)j;
#pragma unroll
            for (int c = 0; c < 3; ++c) { o[c] = zp[c]; o[3 * N + c] = zn[c]; }
        }
        if (a.flags & SONET_BATCH_ROT_HORIZONTAL) { rowmul(p, st.Rh); rowmul(n, st.Rh); }
        if (a.flags & SONET_BATCH_ROT_PERTURBATION) { rowmul(p, st.Rp); rowmul(n, st.Rp); }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[c] = clip(0.01 * zp[c], 0.05) + p[c];
            n[c] = clip(0.01 * zn[c], 0.05) + n[c];
            p[c] = p[c] * st.scale;
            n[c] = n[c] * st.scale;
            if (a.flags & SONET_BATCH_TRANSLATION) p[c] = p[c] + st.shift[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { pcb[c * N + j] = (float)p[c]; snb[c * N + j] = (float)n[c]; }
}

__global__ __launch_bounds__(AB_THREADS) void assemble_batch_kernel(Args a)
{
    __shared__ SlotState st;
    const int tid = threadIdx.x;
    const size_t N = (size_t)a.N, M = (size_t)a.M;
    const size_t D = AB_SCALARS + 6 * N + 3 * M;
    const bool train = (a.flags & SONET_BATCH_TRAIN) != 0, shapenet = (a.flags & SONET_BATCH_SHAPENET) != 0;

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        // ---- the slot: source cloud, validity (device data is checked here; the host checks what it can see before the launch)
        if (tid == 0) {
            const long long s = a.idx[b];
            int ok = s >= 0 && s < a.S;
            long long o0 = 0, n_s = 0;
            if (ok) {
                o0 = a.off[s];
                n_s = a.off[s + 1] - o0;
                ok = o0 >= 0 && n_s >= 1 && n_s <= 0x7FFFFFFF && a.off[s + 1] <= a.P && (shapenet || (long long)a.N <= n_s);
            }
            st.ok = ok; st.s = ok ? (int)s : 0; st.o0 = ok ? o0 : 0; st.n_s = ok ? (int)n_s : 0;
            if (a.bad) a.bad[b] = ok ? 0 : 1;
            // per-slot draws: u (horizontal angle), 3 raw perturbation normals, scale, 3 shifts
            double d[AB_SCALARS];
            if (a.replay_draws) {
                for (int q = 0; q < AB_SCALARS; ++q) d[q] = a.replay_draws[(size_t)b * D + q];
            } else {
                const uint4 w0 = philox(a.step, (unsigned)b, 2u, 0u, a.k0, a.k1);
                const uint4 w2 = philox(a.step, (unsigned)b, 2u, 2u, a.k0, a.k1);
                d[0] = unit(w0.x);
                normals3(philox(a.step, (unsigned)b, 2u, 1u, a.k0, a.k1), d + 1);
                d[4] = 0.8 + (1.2 - 0.8) * unit(w0.y);
                d[5] = -0.1 + (0.1 - -0.1) * unit(w2.x);
                d[6] = -0.1 + (0.1 - -0.1) * unit(w2.y);
                d[7] = -0.1 + (0.1 - -0.1) * unit(w2.z);
            }
            if (a.draws_out && train)
                for (int q = 0; q < AB_SCALARS; ++q) a.draws_out[(size_t)b * D + q] = d[q];
            // rotate_point_cloud_with_normal_som: angle = uniform() * 2 * pi, [[c,0,s],[0,1,0],[-s,0,c]]
            const double ang = d[0] * 2 * M_PI, ch = cos(ang), sh = sin(ang);
            const double Rh[9] = {ch, 0, sh, 0, 1, 0, -sh, 0, ch};
            // rotate_perturbation_point_cloud_with_normal_som: angles = clip(0.06 * randn(3), +-0.18), R = Rz @ (Ry @ Rx)
            const double x = clip(0.06 * d[1], 0.18), y = clip(0.06 * d[2], 0.18), z = clip(0.06 * d[3], 0.18);
            const double Rx[9] = {1, 0, 0, 0, cos(x), -sin(x), 0, sin(x), cos(x)};
            const double Ry[9] = {cos(y), 0, sin(y), 0, 1, 0, -sin(y), 0, cos(y)};
            const double Rz[9] = {cos(z), -sin(z), 0, sin(z), cos(z), 0, 0, 0, 1};
            double Ryx[9];
            matmul3(Ry, Rx, Ryx);
            matmul3(Rz, Ryx, st.Rp);
            for (int q = 0; q < 9; ++q) st.Rh[q] = Rh[q];
            st.scale = d[4];
            st.shift[0] = d[5]; st.shift[1] = d[6]; st.shift[2] = d[7];
        }
        __syncthreads();
        float *pcb = a.pc + (size_t)b * 3 * N, *snb = a.sn + (size_t)b * 3 * N, *ndb = a.node + (size_t)b * 3 * M;
        const int n_s = st.n_s;

        if (!st.ok) {                                             // a bad slot: NaN points and nodes, chosen -1
            for (size_t j = tid; j < N; j += AB_THREADS) {
                a.chosen[(size_t)b * N + j] = -1;
                for (int c = 0; c < 3; ++c) { pcb[c * N + j] = __builtin_nanf(""); snb[c * N + j] = __builtin_nanf(""); }
            }
            for (size_t m = tid; m < M; m += AB_THREADS) {
                for (int c = 0; c < 3; ++c) ndb[c * M + m] = __builtin_nanf("");
                if (a.K == 1) a.knn_I[(size_t)b * M + m] = (int64_t)m;
            }
            __syncthreads();
            continue;
        }

        // ---- 1 + 2 + 3 for the points
        if (a.replay_idx) {
            for (int j = tid; j < a.N; j += AB_THREADS) emit_point(a, st, b, j, a.replay_idx[(size_t)b * N + j]);
        } else if (shapenet && a.N >= n_s) {
            // all n_s points in order, then N - n_s uniform draws with replacement: index = (w * n_s) >> 32
            for (int j = tid; j < a.N; j += AB_THREADS) {
                long long i = j;
                if (j >= n_s) {
                    const unsigned e = (unsigned)(j - n_s);
                    const unsigned w = word(philox(a.step, (unsigned)b, 1u, e >> 2, a.k0, a.k1), e & 3);
                    i = (long long)(((unsigned long long)w * (unsigned)n_s) >> 32);
                }
                emit_point(a, st, b, j, i);
            }
        } else {
            // radix select of the N-th smallest key (ties by index): key of point i = word i & 3 of philox(step, b, 0, i >> 2)
            const int ne = (n_s + 3) >> 2;
            unsigned prefix = 0u, pmask = 0u, kk = (unsigned)a.N, keq = 0xFFFFFFFFu;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                for (int h = tid; h < 256; h += AB_THREADS) st.hist[h] = 0u;
                __syncthreads();
                for (int e = tid; e < ne; e += AB_THREADS) {
                    const uint4 w = philox(a.step, (unsigned)b, 0u, (unsigned)e, a.k0, a.k1);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const unsigned key = word(w, q);
                        if (4 * e + q < n_s && (key & pmask) == prefix) atomicAdd(&st.hist[(key >> shift) & 255u], 1u);
                    }
                }
                __syncthreads();
                if (tid < 64) {                                   // wave 0: the first digit whose inclusive count reaches kk
                    unsigned c[4], sum = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) { c[q] = st.hist[4 * tid + q]; sum += c[q]; }
                    unsigned inc = sum;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned t = __shfl_up(inc, o, 64);
                        if (tid >= o) inc += t;
                    }
                    unsigned run = inc - sum;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (run < kk && run + c[q] >= kk) { st.sel_digit = 4 * tid + q; st.sel_below = run; st.sel_cnt = c[q]; }
                        run += c[q];
                    }
                }
                __syncthreads();
                const unsigned dgt = st.sel_digit, below = st.sel_below, cnt = st.sel_cnt;
                prefix |= dgt << shift;
                pmask |= 255u << shift;
                kk -= below;
                if (cnt == kk) { prefix |= ~pmask; pmask = 0xFFFFFFFFu; break; }    // the whole bucket is taken: no tie rule needed
                if (pass == 3) keq = kk;                         // kk of the keys equal to prefix are taken, lowest index first
            }
            // compaction in source order: take key < T, and key == T while fewer than keq of them were taken
            const unsigned T = prefix;
            unsigned base = 0u, eqbase = 0u;
            const int rounds = (ne + AB_THREADS - 1) / AB_THREADS;
            for (int r = 0; r < rounds; ++r) {
                const int e = r * AB_THREADS + tid;
                uint4 w = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
                if (e < ne) w = philox(a.step, (unsigned)b, 0u, (unsigned)e, a.k0, a.k1);
                unsigned lt = 0u, eq = 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned key = word(w, q);
                    const bool live = e < ne && 4 * e + q < n_s;
                    lt |= (live && key < T) ? 1u << q : 0u;
                    eq |= (live && key == T) ? 1u << q : 0u;
                }
                unsigned take = lt;
                if (keq != 0xFFFFFFFFu) {                         // wave-uniform: only after four passes with a split bucket
                    unsigned eqtot;
                    unsigned er = eqbase + block_scan(__builtin_popcount(eq), st.wsum, &eqtot);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (eq & (1u << q)) { if (er < keq) take |= 1u << q; ++er; }
                    eqbase += eqtot;
                } else {
                    take |= eq;
                }
                unsigned tot;
                unsigned pos = base + block_scan(__builtin_popcount(take), st.wsum, &tot);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if ((take & (1u << q)) && pos < (unsigned)a.N) emit_point(a, st, b, (int)pos++, 4LL * e + q);
                base += tot;
            }
        }

        // ---- nodes (file layout [S][M][3]) -> [B][3][M]
        const float *ns = a.nodes_src + (size_t)st.s * M * 3;
        for (size_t m = tid; m < M; m += AB_THREADS) {
            double v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = ns[3 * m + c];
            if (train) {
                double z[3];
                if (a.replay_draws) {
                    const double *r = a.replay_draws + (size_t)b * D + AB_SCALARS + 6 * N + 3 * m;
#pragma unroll
                    for (int c = 0; c < 3; ++c) z[c] = r[c];
                } else {
                    normals3(philox(a.step, (unsigned)b, 5u, (unsigned)m, a.k0, a.k1), z);
                }
                if (a.draws_out) {
                    double *o = a.draws_out + (size_t)b * D + AB_SCALARS + 6 * N + 3 * m;
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c] = z[c];
                }
                if (a.flags & SONET_BATCH_ROT_HORIZONTAL) rowmul(v, st.Rh);
                if (a.flags & SONET_BATCH_ROT_PERTURBATION) rowmul(v, st.Rp);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    v[c] = clip(0.04 * z[c], 0.1) + v[c];
                    v[c] = v[c] * st.scale;
                    if (a.flags & SONET_BATCH_TRANSLATION) v[c] = v[c] + st.shift[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) ndb[c * M + m] = (float)v[c];
            if (a.K == 1) a.knn_I[(size_t)b * M + m] = (int64_t)m;     // som_k < 2: arange(M) as M x 1
        }
        __syncthreads();                                          // st is rewritten by the next slot of this workgroup
    }
}

}  // namespace

extern "C" int sonet_assemble_batch_f32(const float *src, long long P, const int64_t *offsets, int S, const float *nodes_src,
                                        const int64_t *idx, int B, int N, int M, int K, int flags, long long seed,
                                        long long step, const int64_t *replay_idx, const double *replay_draws,
                                        double *draws_out, float *pc, float *sn, float *node, int64_t *chosen, int64_t *knn_I,
                                        int32_t *bad, sonet_stream_t stream)
{
    const char *what = "sonet_assemble_batch_f32";
    SONET_REQUIRE(src && offsets && nodes_src && idx && pc && sn && node && chosen && knn_I, "%s: NULL pointer", what);
    SONET_REQUIRE(P > 0 && S > 0 && B > 0 && N > 0 && M > 0, "%s: P=%lld S=%d B=%d N=%d M=%d must be >= 1", what, P, S, B, N, M);
    SONET_REQUIRE((flags & ~SONET_BATCH_FLAG_MASK) == 0, "%s: unknown flag bits 0x%x", what, flags & ~SONET_BATCH_FLAG_MASK);
    SONET_REQUIRE(!(flags & SONET_BATCH_SHAPENET) ||
                      !(flags & (SONET_BATCH_ROT_HORIZONTAL | SONET_BATCH_ROT_PERTURBATION | SONET_BATCH_TRANSLATION)),
                  "%s: the shapenet recipe has no rotation or shift (flags 0x%x)", what, flags);
    SONET_REQUIRE(K >= 1 && K <= M, "%s: K=%d must be in [1, M=%d]", what, K, M);
    if (K > SONET_BATCH_MAX_K) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: K=%d > %d", what, K, SONET_BATCH_MAX_K);
    SONET_REQUIRE((size_t)B * N * 3 < ((size_t)1 << 40) && (size_t)B * M * 3 < ((size_t)1 << 40), "%s: batch too large", what);
    Args a{src, P, offsets, S, nodes_src, idx, B, N, M, K, flags, (unsigned)(unsigned long long)seed, (unsigned)((unsigned long long)seed >> 32), (unsigned)(unsigned long long)step,
           replay_idx, replay_draws, draws_out, pc, sn, node, chosen, knn_I, bad};
    hipStream_t st = sonet::as_stream(stream);
    const unsigned grid = (unsigned)(B < 65536 ? B : 65536);
    hipLaunchKernelGGL(assemble_batch_kernel, dim3(grid), dim3(AB_THREADS), 0, st, a);
    const int rc = sonet::launched(what);
    if (rc != SONET_OK || K == 1) return rc;
    return sonet_knn_self_f32(node, knn_I, B, M, K, stream);      // the node table of the loaders, on the augmented nodes
}
