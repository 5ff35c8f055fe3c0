// chamfer.hip -- exact 1-nearest-neighbour search for the Chamfer loss ("next" row), and the loss itself as one
// fused launch (search, robust_norm elements, per-cloud float64 sums) with its own gradient kernel.
//
// Replaces the per-sample faiss GpuIndexFlatL2 build + search + host round trip of
// models/losses.py:220-235, 260-276.  One thread per query point; the database cloud is streamed
// through LDS in tiles of 1024 points (float4, broadcast reads), the same (dx*dx+dy*dy)+dz*dz
// arithmetic as som_assign, ascending j with strict '<' so ties keep the lowest database index.
#include "common.hpp"

namespace {
constexpr int CH_THREADS = 256;
constexpr int CH_TILE = 1024;

// Two database points per step in packed f32 (v_pk_add_f32 / v_pk_mul_f32: each lane of a pair is an IEEE single operation, so the
// distances are the bits of the scalar form): the tile holds PAIRS -- (x0, x1, y0, y1) and (z0, z1) -- and the 8 arithmetic operations of a
// pair cost 8 instructions instead of 16; the two compare / select steps stay scalar and in order (ascending j, strict '<').

// The search loop, one copy for both kernels: the database cloud dbb [3][Nd] goes through the two LDS arrays in tiles of CH_TILE
// points; every thread of the workgroup must call it (barriers inside), a thread without a query passes any finite point.
// Returns the index of the nearest database point: ascending j, strict '<' (ties keep the lowest index; a row of NaN distances
// keeps index 0).  The result is always inside [0, Nd).
__device__ __forceinline__ int chamfer_search(const float *__restrict__ dbb, int Nd, float px, float py, float pz,
                                              float4 *__restrict__ txy, float2 *__restrict__ tz)
{
    const f32x2_t PX = {px, px}, PY = {py, py}, PZ = {pz, pz};
    float best = __builtin_inff();
    int bi = 0;
    for (int t0 = 0; t0 < Nd; t0 += CH_TILE) {
        const int cnt = min(CH_TILE, Nd - t0);
        const int npair = (cnt + 1) >> 1;
        __syncthreads();
        for (int t = threadIdx.x; t < npair; t += CH_THREADS) {
            const int j0 = t0 + 2 * t, j1 = j0 + 1;
            const bool has1 = 2 * t + 1 < cnt;
            // (an odd tail: the second point of the last pair is a copy of the first -- its distance is equal, never strictly smaller)
            const int jb = has1 ? j1 : j0;
            txy[t] = make_float4(dbb[j0], dbb[jb], dbb[Nd + j0], dbb[Nd + jb]);
            tz[t] = make_float2(dbb[2 * (size_t)Nd + j0], dbb[2 * (size_t)Nd + jb]);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < npair; ++t) {
            const float4 a = txy[t];
            const float2 c = tz[t];
            const f32x2_t X = {a.x, a.y}, Y = {a.z, a.w}, Z = {c.x, c.y};
            const f32x2_t dx = PX - X, dy = PY - Y, dz = PZ - Z;
            const f32x2_t d = (dx * dx + dy * dy) + dz * dz;         // (-ffp-contract=off: no fused multiply-add)
            const bool lt0 = d[0] < best;
            best = lt0 ? d[0] : best;
            bi = lt0 ? t0 + 2 * t : bi;
            const bool lt1 = d[1] < best;
            best = lt1 ? d[1] : best;
            bi = lt1 ? t0 + 2 * t + 1 : bi;
        }
    }
    return bi;
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_nn_kernel(const float *__restrict__ q, const float *__restrict__ db,
                                                                 int32_t *__restrict__ nn, int Nq, int Nd)
{
    __shared__ float4 txy[CH_TILE / 2];                          // (x0, x1, y0, y1) of database points 2 t, 2 t + 1
    __shared__ float2 tz[CH_TILE / 2];                           // (z0, z1)
    const int b = blockIdx.y;
    const int i = blockIdx.x * CH_THREADS + threadIdx.x;
    const float *qb = q + (size_t)b * 3 * Nq, *dbb = db + (size_t)b * 3 * Nd;
    const bool valid = i < Nq;
    const float px = valid ? qb[i] : 0.f, py = valid ? qb[Nq + i] : 0.f, pz = valid ? qb[2 * (size_t)Nq + i] : 0.f;
    const int bi = chamfer_search(dbb, Nd, px, py, pz, txy, tz);
    if (valid) nn[(size_t)b * Nq + i] = bi;
}

// ---- the fused loss (models/losses.py:237-290 without the host): search, robust_norm element and per-cloud sums in one launch ----
// blockIdx.x < ceil(M / 256): the predicted -> gt direction (queries = predicted points, database = gt); the other workgroups: gt ->
// predicted.  The element is computed from the coordinates of the CHOSEN neighbour, not from the running minimum: a query with a NaN
// coordinate has minimum +inf and index 0, and its element is NaN as in the reference.  A workgroup adds its elements in float64 --
// lanes by an xor tree, waves in wave order -- and writes one partial; chamfer_loss_sums_kernel adds a (cloud, direction)'s partials in
// ascending order.  No floating-point atomics.
constexpr int CH_WAVES = CH_THREADS / sonet::WAVE;

__device__ __forceinline__ double ch_wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // (every lane adds the same pairs: one fixed tree)
    return v;
}

// robust_norm (models/losses.py:17-27) of sel - q: every operation rounded to f32, the root correctly rounded
__device__ __forceinline__ float chamfer_element(float sx, float sy, float sz, float qx, float qy, float qz)
{
    const float dx = __fsub_rn(sx, qx), dy = __fsub_rn(sy, qy), dz = __fsub_rn(sz, qz);
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return sqrtf(__fadd_rn(s, 1e-8f));          // (the correctly rounded sequence at the library's flags; __fsqrt_rn is the bare v_sqrt_f32 here)
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_loss_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                   int32_t *__restrict__ nn_pg, int32_t *__restrict__ nn_gp,
                                                                   float *__restrict__ elem_fwd, float *__restrict__ elem_bwd,
                                                                   double *__restrict__ part, int M, int N)
{
    __shared__ float4 txy[CH_TILE / 2];
    __shared__ float2 tz[CH_TILE / 2];
    __shared__ double s_sum[CH_WAVES];
    const int b = blockIdx.y;
    const int nblk_f = (M + CH_THREADS - 1) / CH_THREADS;
    const bool fwd = (int)blockIdx.x < nblk_f;                   // (uniform over the workgroup)
    const int blk = fwd ? blockIdx.x : blockIdx.x - nblk_f;
    const int Nq = fwd ? M : N, Nd = fwd ? N : M;
    const float *qb = (fwd ? pred : gt) + (size_t)b * 3 * Nq, *dbb = (fwd ? gt : pred) + (size_t)b * 3 * Nd;
    int32_t *nn = fwd ? nn_pg : nn_gp;
    float *elem = fwd ? elem_fwd : elem_bwd;
    const int i = blk * CH_THREADS + threadIdx.x;
    const bool valid = i < Nq;
    const float px = valid ? qb[i] : 0.f, py = valid ? qb[Nq + i] : 0.f, pz = valid ? qb[2 * (size_t)Nq + i] : 0.f;
    const int bi = chamfer_search(dbb, Nd, px, py, pz, txy, tz);          // in [0, Nd)
    double e64 = 0.0;
    if (valid) {
        const float e = chamfer_element(dbb[bi], dbb[Nd + bi], dbb[2 * (size_t)Nd + bi], px, py, pz);
        if (nn) nn[(size_t)b * Nq + i] = bi;
        if (elem) elem[(size_t)b * Nq + i] = e;
        e64 = (double)e;
    }
    const double wsum = ch_wave_sum_f64(e64);
    if ((threadIdx.x & (sonet::WAVE - 1)) == 0) s_sum[threadIdx.x / sonet::WAVE] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = s_sum[0];
#pragma unroll
        for (int w = 1; w < CH_WAVES; ++w) acc += s_sum[w];
        part[(size_t)b * gridDim.x + blockIdx.x] = acc;
    }
}

// one thread per (cloud, direction): sums [B][2] from the workgroup partials [B][nblk_f + nblk_b], ascending
__global__ __launch_bounds__(64) void chamfer_loss_sums_kernel(const double *__restrict__ part, double *__restrict__ sums, int B,
                                                                int nblk_f, int nblk_b)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= 2 * B) return;
    const int b = t >> 1, dir = t & 1;
    const double *p = part + (size_t)b * (nblk_f + nblk_b) + (dir ? nblk_f : 0);
    const int n = dir ? nblk_b : nblk_f;
    double acc = p[0];
    for (int k = 1; k < n; ++k) acc += p[k];
    sums[t] = acc;
}

// ---- gradient of the two loss terms with respect to the predicted cloud, at the caller's neighbour indices ----
// One thread per predicted point m.  Its own term first (the predicted -> gt direction), then the gt side of the cloud streams through
// LDS in tiles of CH_TILE entries -- (nn_gp[n], gt[:, n], elem_bwd[n]) -- and the thread adds the term of every n whose index is m, in
// ascending n: B * M * N integer compares, what one search direction costs.  Differences of f32 coordinates are exact in float64;
// the sums are float64, rounded to f32 once.  An index outside its range contributes nothing and is never an address; such entries
// are counted in *bad (the gt side by the first workgroup of each cloud only: every workgroup of the cloud reads all of it).
__global__ __launch_bounds__(CH_THREADS) void chamfer_grad_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                   const int32_t *__restrict__ nn_pg, const int32_t *__restrict__ nn_gp,
                                                                   const float *__restrict__ elem_fwd, const float *__restrict__ elem_bwd,
                                                                   const float *__restrict__ gscale, float *__restrict__ dpred,
                                                                   int32_t *__restrict__ bad, double bm, double bn, int M, int N)
{
    __shared__ float4 tg[CH_TILE];                               // (x, y, z, element) of gt point t0 + t
    __shared__ int tidx[CH_TILE];                                // nn_gp of that point, -1 for one outside [0, M)
    __shared__ int s_bad;
    const int b = blockIdx.y;
    const int m = blockIdx.x * CH_THREADS + threadIdx.x;
    const bool valid = m < M;
    const float *pb = pred + (size_t)b * 3 * M, *gb = gt + (size_t)b * 3 * N;
    if (threadIdx.x == 0) s_bad = 0;
    const double cf = (double)gscale[0] / bm, cb = (double)gscale[1] / bn;        // gf / (B M), gb / (B N)
    const float px = valid ? pb[m] : 0.f, py = valid ? pb[M + m] : 0.f, pz = valid ? pb[2 * (size_t)M + m] : 0.f;
    double ax = 0.0, ay = 0.0, az = 0.0;
    int nbad = 0;
    if (valid) {
        const int j = nn_pg[(size_t)b * M + m];
        if (j >= 0 && j < N) {
            const double e = (double)elem_fwd[(size_t)b * M + m];
            ax = cf * ((double)px - (double)gb[j]) / e;
            ay = cf * ((double)py - (double)gb[N + j]) / e;
            az = cf * ((double)pz - (double)gb[2 * (size_t)N + j]) / e;
        } else {
            nbad = 1;
        }
    }
    for (int t0 = 0; t0 < N; t0 += CH_TILE) {
        const int cnt = min(CH_TILE, N - t0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += CH_THREADS) {
            const int n = t0 + t;
            const int j = nn_gp[(size_t)b * N + n];
            const bool ok = j >= 0 && j < M;
            if (!ok && blockIdx.x == 0) ++nbad;
            tidx[t] = ok ? j : -1;
            tg[t] = make_float4(gb[n], gb[N + n], gb[2 * (size_t)N + n], elem_bwd[(size_t)b * N + n]);
        }
        __syncthreads();
        if (valid) {
#pragma unroll 4
            for (int t = 0; t < cnt; ++t) {
                if (tidx[t] == m) {
                    const float4 g = tg[t];
                    const double e = (double)g.w;
                    ax += cb * ((double)px - (double)g.x) / e;
                    ay += cb * ((double)py - (double)g.y) / e;
                    az += cb * ((double)pz - (double)g.z) / e;
                }
            }
        }
    }
    if (valid) {
        float *o = dpred + (size_t)b * 3 * M;
        o[m] = (float)ax;
        o[M + m] = (float)ay;
        o[2 * (size_t)M + m] = (float)az;
    }
    if (nbad) atomicAdd(&s_bad, nbad);
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) atomicAdd(bad, s_bad);
}
#ifdef SONET_VARIANTS   // (a measured-slower record: variants build only, tools/ + tests/variants)
// ---- both directions in ONE sweep of the distance matrix (models/losses.py:255 and :262 together) -----------------------------
// One thread per point of cloud A (the larger one: more workgroups); cloud B goes through LDS in tiles.  d(a_i, b_j) is
// computed once: the row minimum (a_i's nearest b) is a register update as above; the column minimum (b_j's nearest a) is a
// packed 64-bit key (distance bits << 32 | i) in an LDS bin per b_j -- every lane reads the bin (one broadcast ds_read_b64) and
// only a record-breaker issues the ds_min_u64, as in index_max.  Distances are >= 0, so their bit patterns order like the
// values; equal distances order by the smaller i: exactly "ascending i, strict <".  (dx)^2 == (-dx)^2 bit for bit, so the
// column result equals a separate b -> a launch.  Bins go to memory by atomicMin on the same keys (one per bin, tile and
// workgroup); a NaN distance has a key above +inf and never wins against a finite one; an all-NaN column keeps index 0.
// MEASURED (profiles/r02l_chamfer.log, 1280 x 5000 points): 8.66 ms at B = 64 against 0.34 ms for two one-direction launches,
// which already run at 0.67 of the vector-issue roof (22 lane-ops per pair) -- the dependent LDS read and the divergent branch
// per pair stall a loop that is otherwise pure register arithmetic.  The loss (models/losses.py) therefore keeps the two
// launches; this entry point stays as the tested record of the experiment (identical indices).
constexpr int C2_TILE = 2048;
constexpr unsigned long long C2_INIT = 0x7F800000FFFFFFFFull;          // (+inf, i = 2^32 - 1): what "no candidate yet" compares as

__global__ __launch_bounds__(CH_THREADS) void chamfer_nn2_kernel(const float *__restrict__ a, const float *__restrict__ bdb,
                                                                  int32_t *__restrict__ nn_a, unsigned long long *__restrict__ colkey,
                                                                  int Na, int Nb)
{
    __shared__ float4 tile[C2_TILE];
    __shared__ unsigned long long bins[C2_TILE];
    const int b = blockIdx.y;
    const int i = blockIdx.x * CH_THREADS + threadIdx.x;
    const float *ab = a + (size_t)b * 3 * Na, *bb = bdb + (size_t)b * 3 * Nb;
    const bool valid = i < Na;
    const float px = valid ? ab[i] : 0.f, py = valid ? ab[Na + i] : 0.f, pz = valid ? ab[2 * (size_t)Na + i] : 0.f;
    float best = __builtin_inff();
    int bi = 0;
    for (int t0 = 0; t0 < Nb; t0 += C2_TILE) {
        const int cnt = min(C2_TILE, Nb - t0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += CH_THREADS) {
            tile[t] = make_float4(bb[t0 + t], bb[Nb + t0 + t], bb[2 * (size_t)Nb + t0 + t], 0.f);
            bins[t] = C2_INIT;
        }
        __syncthreads();
        if (valid) {
#pragma unroll 4
            for (int t = 0; t < cnt; ++t) {
                const float4 p = tile[t];
                const float dx = __fsub_rn(px, p.x), dy = __fsub_rn(py, p.y), dz = __fsub_rn(pz, p.z);
                const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                const bool lt = d < best;
                best = lt ? d : best;
                bi = lt ? t0 + t : bi;
                const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
                if (key < bins[t]) atomicMin(&bins[t], key);
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += CH_THREADS) {
            const unsigned long long k = bins[t];
            if (k < C2_INIT) atomicMin(colkey + (size_t)b * Nb + t0 + t, k);
        }
    }
    if (valid) nn_a[(size_t)b * Na + i] = bi;
}

__global__ __launch_bounds__(256) void chamfer_nn2_finalize_kernel(const unsigned long long *__restrict__ colkey, int32_t *__restrict__ nn_b, long long n)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const unsigned long long k = colkey[t];
    nn_b[t] = k < C2_INIT ? (int32_t)(unsigned)(k & 0xFFFFFFFFull) : 0;
}
#endif  // SONET_VARIANTS
}  // namespace

#ifdef SONET_VARIANTS
extern "C" size_t sonet_chamfer_nn2_ws_size(int B, int Na, int Nb)
{
    if (B <= 0 || Na <= 0 || Nb <= 0) return 0;
    return (size_t)B * (size_t)(Na > Nb ? Nb : Na) * 8;
}

extern "C" int sonet_chamfer_nn2_f32(const float *pa, const float *pb, int32_t *nn_ab, int32_t *nn_ba, void *ws, int B, int Na, int Nb,
                                     sonet_stream_t stream)
{
    const char *what = "sonet_chamfer_nn2_f32";
    SONET_REQUIRE(pa && pb && nn_ab && nn_ba && ws, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && Na > 0 && Nb > 0, "%s: non-positive size", what);
    if (B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B=%d > 65535", what, B);
    hipStream_t st = sonet::as_stream(stream);
    // threads over the larger cloud, LDS tiles over the smaller one
    const bool swap = Nb > Na;
    const float *big = swap ? pb : pa, *small = swap ? pa : pb;
    int32_t *nn_big = swap ? nn_ba : nn_ab, *nn_small = swap ? nn_ab : nn_ba;
    const int Nbig = swap ? Nb : Na, Nsmall = swap ? Na : Nb;
    unsigned long long *colkey = reinterpret_cast<unsigned long long *>(ws);
    if (hipMemsetAsync(colkey, 0xFF, (size_t)B * Nsmall * 8, st) != hipSuccess) return sonet::fail(SONET_ERR_LAUNCH, "%s: memset failed", what);
    hipLaunchKernelGGL(chamfer_nn2_kernel, dim3(sonet::ceil_div(Nbig, CH_THREADS), B), dim3(CH_THREADS), 0, st, big, small, nn_big, colkey, Nbig, Nsmall);
    const long long n = (long long)B * Nsmall;
    hipLaunchKernelGGL(chamfer_nn2_finalize_kernel, dim3((unsigned)sonet::ceil_div64(n, 256)), dim3(256), 0, st, colkey, nn_small, n);
    return sonet::launched(what);
}
#endif  // SONET_VARIANTS

extern "C" int sonet_chamfer_nn_f32(const float *q, const float *db, int32_t *nn, int B, int Nq, int Nd,
                                    sonet_stream_t stream)
{
    const char *what = "sonet_chamfer_nn_f32";
    SONET_REQUIRE(q && db && nn, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && Nq > 0 && Nd > 0, "%s: non-positive size", what);
    if (B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B=%d > 65535", what, B);
    hipLaunchKernelGGL(chamfer_nn_kernel, dim3(sonet::ceil_div(Nq, CH_THREADS), B), dim3(CH_THREADS), 0,
                       sonet::as_stream(stream), q, db, nn, Nq, Nd);
    return sonet::launched(what);
}

extern "C" size_t sonet_chamfer_loss_ws_size(int B, int M, int N)
{
    if (B <= 0 || M <= 0 || N <= 0) return 0;
    return (size_t)B * (size_t)(sonet::ceil_div64(M, CH_THREADS) + sonet::ceil_div64(N, CH_THREADS)) * sizeof(double);
}

extern "C" int sonet_chamfer_loss_f32(const float *pred, const float *gt, int32_t *nn_pg, int32_t *nn_gp, float *elem_fwd,
                                      float *elem_bwd, double *sums, void *ws, int B, int M, int N, sonet_stream_t stream)
{
    const char *what = "sonet_chamfer_loss_f32";
    SONET_REQUIRE(pred && gt && sums && ws, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && M > 0 && N > 0, "%s: non-positive size (B=%d M=%d N=%d)", what, B, M, N);
    if (B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B=%d > 65535", what, B);
    hipStream_t st = sonet::as_stream(stream);
    const int nblk_f = sonet::ceil_div(M, CH_THREADS), nblk_b = sonet::ceil_div(N, CH_THREADS);
    double *part = reinterpret_cast<double *>(ws);
    hipLaunchKernelGGL(chamfer_loss_kernel, dim3(nblk_f + nblk_b, B), dim3(CH_THREADS), 0, st, pred, gt, nn_pg, nn_gp, elem_fwd,
                       elem_bwd, part, M, N);
    hipLaunchKernelGGL(chamfer_loss_sums_kernel, dim3(sonet::ceil_div(2 * B, 64)), dim3(64), 0, st, part, sums, B, nblk_f, nblk_b);
    return sonet::launched(what);
}

extern "C" int sonet_chamfer_grad_f32(const float *pred, const float *gt, const int32_t *nn_pg, const int32_t *nn_gp,
                                      const float *elem_fwd, const float *elem_bwd, const float *gscale, float *dpred, int32_t *bad,
                                      int B, int M, int N, sonet_stream_t stream)
{
    const char *what = "sonet_chamfer_grad_f32";
    SONET_REQUIRE(pred && gt && nn_pg && nn_gp && elem_fwd && elem_bwd && gscale && dpred && bad, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && M > 0 && N > 0, "%s: non-positive size (B=%d M=%d N=%d)", what, B, M, N);
    if (B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B=%d > 65535", what, B);
    hipStream_t st = sonet::as_stream(stream);
    if (int rc = sonet::zero_words(bad, 4, st)) return rc;
    hipLaunchKernelGGL(chamfer_grad_kernel, dim3(sonet::ceil_div(M, CH_THREADS), B), dim3(CH_THREADS), 0, st, pred, gt, nn_pg, nn_gp,
                       elem_fwd, elem_bwd, gscale, dpred, bad, (double)B * (double)M, (double)B * (double)N, M, N);
    return sonet::launched(what);
}
