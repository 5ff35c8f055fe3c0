// som_train.hip -- SOM training (BatchSOM.optimize, util/som.py:295-366): T iterations for B clouds in ONE launch on gfx950.
//
// The reference runs an iteration as ~10 tensor ops over B x 3 x N x M and B x 3 x M x rows x cols temporaries; the repository's
// batch_update restates it as som_assign + som_group + two M x M products (~8 launches per iteration, 640 per optimize).  Here one
// workgroup owns one cloud for the whole schedule: its nodes, per-node counts / sums and cluster means live in LDS, the points are
// copied to LDS once when they fit (otherwise re-read from L2 every iteration), and the only global traffic per iteration is the
// schedule's weight table w_t [M][M] (shared by every cloud, L2-resident) and one f32 learning rate.  Nothing waits on another
// workgroup: a cloud's whole dependency chain is inside its workgroup, clouds are taken in a grid-stride loop.
//
// Iteration t (three barriers):
//   assign  d = (dx*dx + dy*dy) + dz*dz, separate f32 multiplies / adds (two points per packed v_pk_* operation, each lane rounded on
//           its own), nodes visited in ascending id with strict '<': ties go to the lowest id (torch.min's first minimum);
//   reduce  per-node count (u32) and coordinate sums as 64-bit FIXED-POINT integers (LDS integer atomics): integer addition is
//           associative, so the sums -- and everything after them -- do not depend on the order the atomics arrive in.  The scale
//           2^S is chosen per cloud from its largest |coordinate| so that N terms cannot overflow; the quantisation step is
//           2^-(61 - ceil(log2 N)) of that magnitude (2^-48 at N = 5000), far below an f32 ulp of the cluster mean;
//           mean_i = (float)sum_i / ((float)count_i + 1e-5f) (f32 division, as som_group), r_i = count_i > 0;
//   update  node_j += sum_i ((mean_i - node_j) * r_i * w_t[i][j] * lr_t) from the OLD nodes (Jacobi, util/som.py:339-352), the
//           i-sum in ascending i, one thread per node.
#include "common.hpp"

namespace {

constexpr int ST_THREADS = 1024;
constexpr int ST_MAX_NODES = SONET_SOM_TRAIN_MAX_NODES;
constexpr int ST_MAX_POINTS = SONET_SOM_TRAIN_MAX_POINTS;
constexpr size_t ST_LDS_MAX = 160 * 1024;



__host__ __device__ inline size_t st_node_bytes(int M) {         // nodes | means | sums | counts | max word, padded to 16 B
    return ((size_t)M * (2 * sizeof(float4) + 3 * sizeof(unsigned long long) + sizeof(unsigned)) + 16 + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t st_point_bytes(int N) { return (size_t)((N + 3) & ~3) * 3 * sizeof(float); }

// the nearest node of four points (two packed pairs, one LDS broadcast read per node), ties to the lowest id
__device__ __forceinline__ void nearest4(const float4 *__restrict__ nodes, int M, const float4 X, const float4 Y, const float4 Z, int id[4]) {
    const f32x2_t xa{X.x, X.y}, ya{Y.x, Y.y}, za{Z.x, Z.y}, xb{X.z, X.w}, yb{Y.z, Y.w}, zb{Z.z, Z.w};
    float b0 = __builtin_inff(), b1 = b0, b2 = b0, b3 = b0;
    int j0 = 0, j1 = 0, j2 = 0, j3 = 0;
#pragma unroll 2
    for (int m = 0; m < M; ++m) {
        const float4 nd = nodes[m];
        const f32x2_t dxa = xa - nd.x, dya = ya - nd.y, dza = za - nd.z;
        const f32x2_t dxb = xb - nd.x, dyb = yb - nd.y, dzb = zb - nd.z;
        const f32x2_t da = (dxa * dxa + dya * dya) + dza * dza;     // -ffp-contract=off: no FMA, each lane rounded like sqdist (som.hip)
        const f32x2_t db = (dxb * dxb + dyb * dyb) + dzb * dzb;
        if (da.x < b0) { b0 = da.x; j0 = m; }
        if (da.y < b1) { b1 = da.y; j1 = m; }
        if (db.x < b2) { b2 = db.x; j2 = m; }
        if (db.y < b3) { b3 = db.y; j3 = m; }
    }
    id[0] = j0; id[1] = j1; id[2] = j2; id[3] = j3;
}

__device__ __forceinline__ unsigned long long fixq(float v, double scale) {
    return (unsigned long long)__double2ll_rn((double)v * scale);     // exact product (power of two), one rounding to the grid
}

// LDS (dynamic): float4 nodes[M] | float4 mean[M] (.w = r) | u64 sums[3][M] | u32 cnt[M] | u32 amax (16 B) | [points x, y, z [Np] each]
template <bool RESIDENT>
// (four waves per SIMD, one 16-wave workgroup per CU: measured fastest of {4, 8} waves per SIMD x {1, 2}-node unroll x points
//  resident up to 80 / 160 KB -- bit-identical results; docs/findings.md)
__global__ __launch_bounds__(ST_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void som_train_kernel(
    const float *__restrict__ x, const float *__restrict__ node0, int node0_shared, const float *__restrict__ w,
    const float *__restrict__ lr, int T, int B, int N, int M, float *__restrict__ node_out, bool vec)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *nodes = reinterpret_cast<float4 *>(smem);
    float4 *mean = nodes + M;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(mean + M);
    unsigned *cnt = reinterpret_cast<unsigned *>(sums + 3 * M);
    unsigned *amax = cnt + M;
    float *pts = reinterpret_cast<float *>(smem + st_node_bytes(M));
    const int tid = threadIdx.x;
    const int Np = (N + 3) & ~3;
    const int nq = Np >> 2;
    float *lx = pts, *ly = pts + Np, *lz = pts + 2 * (size_t)Np;

    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const float *xb = x + (size_t)b * 3 * N;
        const float *nb = node0 + (node0_shared ? (size_t)0 : (size_t)b * 3 * M);
        if (tid == 0) *amax = 0u;
        for (int m = tid; m < M; m += ST_THREADS) {
            nodes[m] = make_float4(nb[m], nb[M + m], nb[2 * M + m], 0.f);
            sums[m] = 0ull; sums[M + m] = 0ull; sums[2 * M + m] = 0ull;
            cnt[m] = 0u;
        }
        __syncthreads();
        // one pass over the cloud: the LDS copy (padding = 0) and the largest |coordinate| (bit patterns of non-negative floats order
        // like their values)
        unsigned am = 0u;
        for (int n = tid; n < Np; n += ST_THREADS) {
            float a = 0.f, c = 0.f, e = 0.f;
            if (n < N) { a = xb[n]; c = xb[N + n]; e = xb[2 * (size_t)N + n]; }
            if (RESIDENT) { lx[n] = a; ly[n] = c; lz[n] = e; }
            am = max(am, max(__float_as_uint(fabsf(a)), max(__float_as_uint(fabsf(c)), __float_as_uint(fabsf(e)))));
        }
        atomicMax(amax, am);
        __syncthreads();
        int ex = 0;
        const float mx = __uint_as_float(*amax);
        if (mx > 0.f && mx <= 3.4e38f) frexpf(mx, &ex);                  // mx < 2^ex
        const int L = N > 1 ? 32 - __clz(N - 1) : 0;                      // N <= 2^L
        const int S = 61 - ex - L;                                        // |q| <= 2^(61-L), |sum| <= 2^61
        const double scale = ldexp(1.0, S), unscale = ldexp(1.0, -S);

        for (int t = 0; t < T; ++t) {
            // ---- assign + fixed-point accumulation, four consecutive points per thread and pass
            for (int q = tid; q < nq; q += ST_THREADS) {
                const int n0 = 4 * q;
                float4 X, Y, Z;
                if (RESIDENT) {
                    X = *reinterpret_cast<const float4 *>(lx + n0);
                    Y = *reinterpret_cast<const float4 *>(ly + n0);
                    Z = *reinterpret_cast<const float4 *>(lz + n0);
                } else if (vec) {                                           // rows 16-B aligned: N % 4 == 0, x aligned
                    X = *reinterpret_cast<const float4 *>(xb + n0);
                    Y = *reinterpret_cast<const float4 *>(xb + N + n0);
                    Z = *reinterpret_cast<const float4 *>(xb + 2 * (size_t)N + n0);
                } else {
                    X = make_float4(xb[n0], 0.f, 0.f, 0.f);
                    Y = make_float4(xb[N + n0], 0.f, 0.f, 0.f);
                    Z = make_float4(xb[2 * (size_t)N + n0], 0.f, 0.f, 0.f);
                    if (n0 + 1 < N) { X.y = xb[n0 + 1]; Y.y = xb[N + n0 + 1]; Z.y = xb[2 * (size_t)N + n0 + 1]; }
                    if (n0 + 2 < N) { X.z = xb[n0 + 2]; Y.z = xb[N + n0 + 2]; Z.z = xb[2 * (size_t)N + n0 + 2]; }
                    if (n0 + 3 < N) { X.w = xb[n0 + 3]; Y.w = xb[N + n0 + 3]; Z.w = xb[2 * (size_t)N + n0 + 3]; }
                }
                int id[4];
                nearest4(nodes, M, X, Y, Z, id);
                const float px[4] = {X.x, X.y, X.z, X.w}, py[4] = {Y.x, Y.y, Y.z, Y.w}, pz[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (n0 + p < N) {
                        atomicAdd(&cnt[id[p]], 1u);
                        atomicAdd(&sums[id[p]], fixq(px[p], scale));
                        atomicAdd(&sums[M + id[p]], fixq(py[p], scale));
                        atomicAdd(&sums[2 * M + id[p]], fixq(pz[p], scale));
                    }
                }
            }
            __syncthreads();
            // ---- cluster means (networks.py:140-142 arithmetic), accumulators cleared for the next iteration
            for (int m = tid; m < M; m += ST_THREADS) {
                const unsigned c = cnt[m];
                const float sx = (float)((double)(long long)sums[m] * unscale);
                const float sy = (float)((double)(long long)sums[M + m] * unscale);
                const float sz = (float)((double)(long long)sums[2 * M + m] * unscale);
                mean[m] = make_float4(cluster_mean(sx, (float)c), cluster_mean(sy, (float)c), cluster_mean(sz, (float)c), c > 0u ? 1.f : 0.f);
                sums[m] = 0ull; sums[M + m] = 0ull; sums[2 * M + m] = 0ull;
                cnt[m] = 0u;
            }
            __syncthreads();
            // ---- Jacobi update: node j reads only its own old value and the means, so it is written in place
            const float lrt = lr[t];
            const float *wt = w + (size_t)t * M * M;
            for (int j = tid; j < M; j += ST_THREADS) {
                const float4 nj = nodes[j];
                float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll 8
                for (int i = 0; i < M; ++i) {
                    const float4 mi = mean[i];
                    const float wl = wt[(size_t)i * M + j];
                    ax = __fadd_rn(ax, __fmul_rn(__fmul_rn(__fmul_rn(__fsub_rn(mi.x, nj.x), mi.w), wl), lrt));
                    ay = __fadd_rn(ay, __fmul_rn(__fmul_rn(__fmul_rn(__fsub_rn(mi.y, nj.y), mi.w), wl), lrt));
                    az = __fadd_rn(az, __fmul_rn(__fmul_rn(__fmul_rn(__fsub_rn(mi.z, nj.z), mi.w), wl), lrt));
                }
                nodes[j] = make_float4(__fadd_rn(nj.x, ax), __fadd_rn(nj.y, ay), __fadd_rn(nj.z, az), 0.f);
            }
            __syncthreads();
        }
        float *ob = node_out + (size_t)b * 3 * M;
        for (int m = tid; m < M; m += ST_THREADS) {
            const float4 nd = nodes[m];
            ob[m] = nd.x; ob[M + m] = nd.y; ob[2 * M + m] = nd.z;
        }
        __syncthreads();                                                  // LDS is reused by the next cloud of this workgroup
    }
}

}  // namespace

extern "C" int sonet_som_train_f32(const float *x, const float *node0, int node0_shared, const float *w, const float *lr,
                                   int T, int B, int N, int M, float *node_out, sonet_stream_t stream)
{
    const char *what = "sonet_som_train_f32";
    SONET_REQUIRE(x && node0 && node_out, "%s: NULL pointer", what);
    SONET_REQUIRE(T == 0 || (w && lr), "%s: NULL w / lr with T=%d", what, T);
    SONET_REQUIRE(B > 0 && N > 0 && M > 0 && T >= 0, "%s: B=%d N=%d M=%d must be >= 1, T=%d >= 0", what, B, N, M, T);
    SONET_REQUIRE(M <= ST_MAX_NODES, "%s: M=%d > %d nodes", what, M, ST_MAX_NODES);
    SONET_REQUIRE(N <= ST_MAX_POINTS, "%s: N=%d > %d points", what, N, ST_MAX_POINTS);
    const size_t lds_nodes = st_node_bytes(M), lds_res = lds_nodes + st_point_bytes(N);
    const bool resident = lds_res <= ST_LDS_MAX;
    const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const size_t lds = resident ? lds_res : lds_nodes;
    const unsigned grid = (unsigned)(B < 65536 ? B : 65536);
    hipStream_t st = sonet::as_stream(stream);
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(&som_train_kernel<true>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)ST_LDS_MAX) != hipSuccess)
        return sonet::fail(SONET_ERR_LAUNCH, "%s: cannot raise the LDS limit", what);
    if (resident)
        hipLaunchKernelGGL(som_train_kernel<true>, dim3(grid), dim3(ST_THREADS), lds, st, x, node0, node0_shared, w, lr, T, B, N, M, node_out, vec);
    else
        hipLaunchKernelGGL(som_train_kernel<false>, dim3(grid), dim3(ST_THREADS), lds, st, x, node0, node0_shared, w, lr, T, B, N, M, node_out, vec);
    return sonet::launched(what);
}
