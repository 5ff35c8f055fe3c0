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

// ---- the loss pyramid of one autoencoder step (models/autoencoder.py:83-98): up to three predicted clouds against ONE gt cloud ------
// chamfer_pyramid_loss_kernel is chamfer_loss_kernel with the level picked by the workgroup index: per cloud, level l owns the
// workgroups [blk0, blk0 + nblk_f + nblk_b) -- predicted -> gt first, then gt -> predicted, 256 consecutive queries each -- so every
// index, element and float64 partial is the one chamfer_loss_kernel forms for that level alone, and the sums kernel adds a
// (cloud, level, direction)'s partials in the same ascending order.
constexpr int PYR_LEVELS = 3;
constexpr int PYR_THREADS = 1024;                                // the gradient kernel's workgroup
constexpr int PYR_MAX_N = 8192;                                  // gt points: one cloud's keys are sorted in one LDS array
constexpr int PYR_MAX_M = 65535;                                 // predicted points: m sits in the upper 16 bits of a key, 0xFFFF is "no owner"
constexpr unsigned PYR_NO_OWNER = 0xFFFFFFFFu;

struct PyrLossLevel {
    const float *pred;
    int32_t *nn_pg, *nn_gp;
    float *elem_fwd, *elem_bwd;
    int M, blk0, nblk_f;
};
struct PyrLossArgs {
    PyrLossLevel lv[PYR_LEVELS];
};

__global__ __launch_bounds__(CH_THREADS) void chamfer_pyramid_loss_kernel(const PyrLossArgs a, const float *__restrict__ gt,
                                                                           double *__restrict__ part, int L, int N)
{
    __shared__ float4 txy[CH_TILE / 2];
    __shared__ float2 tz[CH_TILE / 2];
    __shared__ double s_sum[CH_WAVES];
    const int b = blockIdx.y;
    PyrLossLevel v = a.lv[0];                                    // (uniform over the workgroup: kernel arguments and blockIdx)
    if (L > 1 && (int)blockIdx.x >= a.lv[1].blk0) v = a.lv[1];
    if (L > 2 && (int)blockIdx.x >= a.lv[2].blk0) v = a.lv[2];
    const int M = v.M;
    const int rel = (int)blockIdx.x - v.blk0;
    const bool fwd = rel < v.nblk_f;
    const int blk = fwd ? rel : rel - v.nblk_f;
    const int Nq = fwd ? M : N, Nd = fwd ? N : M;
    const float *qb = (fwd ? v.pred : gt) + (size_t)b * 3 * Nq, *dbb = (fwd ? gt : v.pred) + (size_t)b * 3 * Nd;
    int32_t *nn = fwd ? v.nn_pg : v.nn_gp;
    float *elem = fwd ? v.elem_fwd : v.elem_bwd;
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

struct PyrSumsArgs {
    int blk0[PYR_LEVELS], nblk_f[PYR_LEVELS];
};

// one thread per (cloud, level, direction): sums [B][L][2] from the workgroup partials [B][nblk], ascending
__global__ __launch_bounds__(64) void chamfer_pyramid_sums_kernel(const PyrSumsArgs a, const double *__restrict__ part,
                                                                   double *__restrict__ sums, int B, int L, int nblk, int nblk_b)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= 2 * B * L) return;
    const int dir = t & 1, l = (t >> 1) % L, b = (t >> 1) / L;
    const int blk0 = l == 0 ? a.blk0[0] : l == 1 ? a.blk0[1] : a.blk0[2];
    const int nblk_f = l == 0 ? a.nblk_f[0] : l == 1 ? a.nblk_f[1] : a.nblk_f[2];
    const double *p = part + (size_t)b * nblk + blk0 + (dir ? nblk_f : 0);
    const int n = dir ? nblk_b : nblk_f;
    double acc = p[0];
    for (int k = 1; k < n; ++k) acc += p[k];
    sums[t] = acc;
}

// ---- gradient of every level in one launch, from stable inverse lists instead of an M x N compare --------------------------------
// One workgroup per (cloud, level).  The keys (nn_gp[n] << 16) | n of the cloud's gt points are sorted in LDS (the bitonic network of
// retrieval.hip on 32-bit keys; n makes every key distinct, so the order is total: ascending owner m, then ascending n -- the order
// chamfer_grad_kernel meets the terms of m in).  An entry outside [0, M) gets the key PYR_NO_OWNER, which sorts behind every owner,
// is counted and is never an address.  A thread then takes predicted points m = tid, tid + 1024, ...: its own forward term first,
// then a binary search for the first key of m and a walk to the last one.  B (M + N) terms and N log^2 N compare-exchanges per level,
// the arithmetic of chamfer_grad_kernel term for term: the same bits.
__device__ __forceinline__ void pyr_compare_exchange(unsigned *buf, int i, int j, int k)
{
    const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
    const unsigned a = buf[lo], b = buf[hi];
    if ((a > b) == ((lo & k) == 0)) {
        buf[lo] = b;
        buf[hi] = a;
    }
}

// P keys (a power of two), thread t owning the pairs t, t + PYR_THREADS, ...: the stages with a stride above 64 end in a workgroup
// barrier; at strides 64 .. 1 the 64 pairs of a wave stay inside one block of 128 keys that no other wave touches, so those stages run
// back to back in the wave's own in-order LDS queue and one barrier closes them.
__device__ __forceinline__ void pyr_bitonic_sort(unsigned *buf, int P, int tid)
{
    for (int k = 2; k <= P; k <<= 1) {
        int j = k >> 1;
        for (; j > 64; j >>= 1) {
            for (int i = tid; i < (P >> 1); i += PYR_THREADS) pyr_compare_exchange(buf, i, j, k);
            __syncthreads();
        }
        for (int i = tid; i < (P >> 1); i += PYR_THREADS) {
            for (int jj = j; jj > 0; jj >>= 1) {
                pyr_compare_exchange(buf, i, jj, k);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}

struct PyrGradLevel {
    const float *pred;
    const int32_t *nn_pg, *nn_gp;
    const float *elem_fwd, *elem_bwd;
    float *dpred;
    int M;
};
struct PyrGradArgs {
    PyrGradLevel lv[PYR_LEVELS];
};

__global__ __launch_bounds__(PYR_THREADS) void chamfer_pyramid_grad_kernel(const PyrGradArgs a, const float *__restrict__ gt,
                                                                            const float *__restrict__ gscale, int32_t *__restrict__ bad,
                                                                            int B, int N, int P)
{
    __shared__ unsigned keys[PYR_MAX_N];
    __shared__ int s_bad;
    const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const PyrGradLevel v = l == 0 ? a.lv[0] : l == 1 ? a.lv[1] : a.lv[2];
    const int M = v.M;
    const float *pb = v.pred + (size_t)b * 3 * M, *gb = gt + (size_t)b * 3 * N;
    if (tid == 0) s_bad = 0;
    int nbad = 0;
    for (int n = tid; n < P; n += PYR_THREADS) {                 // (P <= PYR_MAX_N; the tail [N, P) is padding)
        unsigned key = PYR_NO_OWNER;
        if (n < N) {
            const int j = v.nn_gp[(size_t)b * N + n];
            if (j >= 0 && j < M) key = ((unsigned)j << 16) | (unsigned)n;
            else ++nbad;
        }
        keys[n] = key;
    }
    __syncthreads();
    pyr_bitonic_sort(keys, P, tid);
    const double cf = (double)gscale[2 * l] / ((double)B * (double)M), cb = (double)gscale[2 * l + 1] / ((double)B * (double)N);
    for (int m = tid; m < M; m += PYR_THREADS) {
        const float px = pb[m], py = pb[M + m], pz = pb[2 * (size_t)M + m];
        double ax = 0.0, ay = 0.0, az = 0.0;
        const int j = v.nn_pg[(size_t)b * M + m];
        if (j >= 0 && j < N) {
            const double e = (double)v.elem_fwd[(size_t)b * M + m];
            ax = cf * ((double)px - (double)gb[j]) / e;
            ay = cf * ((double)py - (double)gb[N + j]) / e;
            az = cf * ((double)pz - (double)gb[2 * (size_t)N + j]) / e;
        } else {
            ++nbad;
        }
        const unsigned first = (unsigned)m << 16;                // the smallest key m can own
        int lo = 0, hi = N;                                      // (keys [0, N): every real entry; the padding sorts behind them)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < first) lo = mid + 1;
            else hi = mid;
        }
        for (int i = lo; i < N; ++i) {
            const unsigned key = keys[i];
            if ((key >> 16) != (unsigned)m) break;
            const int n = (int)(key & 0xFFFFu);                  // < N: only entries with n < N carry an owner
            const double e = (double)v.elem_bwd[(size_t)b * N + n];
            ax += cb * ((double)px - (double)gb[n]) / e;
            ay += cb * ((double)py - (double)gb[N + n]) / e;
            az += cb * ((double)pz - (double)gb[2 * (size_t)N + n]) / e;
        }
        float *o = v.dpred + (size_t)b * 3 * M;
        o[m] = (float)ax;
        o[M + m] = (float)ay;
        o[2 * (size_t)M + m] = (float)az;
    }
    if (nbad) atomicAdd(&s_bad, nbad);
    __syncthreads();
    if (tid == 0 && s_bad) atomicAdd(bad + l, s_bad);
}
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

// ---- the loss pyramid: every level and both directions in one launch, every level's gradient in one more ------------------------------
extern "C" int sonet_chamfer_pyramid_max_n(void) { return PYR_MAX_N; }
extern "C" int sonet_chamfer_pyramid_max_m(void) { return PYR_MAX_M; }

namespace {
// what both entries ask of the sizes; M may be NULL only when the caller's own check has failed already
int pyramid_sizes(const char *what, int B, int L, const int *M, int N)
{
    SONET_REQUIRE(L >= 1 && L <= PYR_LEVELS, "%s: L=%d outside 1..%d", what, L, PYR_LEVELS);
    SONET_REQUIRE(M, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && N > 0, "%s: non-positive size (B=%d N=%d)", what, B, N);
    for (int l = 0; l < L; ++l) SONET_REQUIRE(M[l] > 0, "%s: non-positive size (M[%d]=%d)", what, l, M[l]);
    if (B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B=%d > 65535", what, B);
    if (N > PYR_MAX_N) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: N=%d > %d", what, N, PYR_MAX_N);
    for (int l = 0; l < L; ++l)
        if (M[l] > PYR_MAX_M) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: M[%d]=%d > %d", what, l, M[l], PYR_MAX_M);
    return SONET_OK;
}
}  // namespace

extern "C" size_t sonet_chamfer_pyramid_ws_size(int B, int L, int M0, int M1, int M2, int N)
{
    const int M[PYR_LEVELS] = {M0, M1, M2};
    if (B <= 0 || L < 1 || L > PYR_LEVELS || N <= 0) return 0;
    long long nblk = 0;
    for (int l = 0; l < L; ++l) {
        if (M[l] <= 0) return 0;
        nblk += sonet::ceil_div64(M[l], CH_THREADS) + sonet::ceil_div64(N, CH_THREADS);
    }
    return (size_t)B * (size_t)nblk * sizeof(double);
}

extern "C" int sonet_chamfer_pyramid_loss_f32(const float *const *pred, const float *gt, int32_t *const *nn_pg, int32_t *const *nn_gp,
                                              float *const *elem_fwd, float *const *elem_bwd, double *sums, void *ws, int B, int L,
                                              const int *M, int N, sonet_stream_t stream)
{
    const char *what = "sonet_chamfer_pyramid_loss_f32";
    if (int rc = pyramid_sizes(what, B, L, M, N)) return rc;
    SONET_REQUIRE(pred && gt && sums && ws, "%s: NULL pointer", what);
    for (int l = 0; l < L; ++l) SONET_REQUIRE(pred[l], "%s: NULL pointer (pred[%d])", what, l);
    hipStream_t st = sonet::as_stream(stream);
    const int nblk_b = sonet::ceil_div(N, CH_THREADS);
    PyrLossArgs a = {};
    PyrSumsArgs s = {};
    int nblk = 0;
    for (int l = 0; l < L; ++l) {
        PyrLossLevel &v = a.lv[l];
        v.pred = pred[l];
        v.nn_pg = nn_pg ? nn_pg[l] : nullptr;
        v.nn_gp = nn_gp ? nn_gp[l] : nullptr;
        v.elem_fwd = elem_fwd ? elem_fwd[l] : nullptr;
        v.elem_bwd = elem_bwd ? elem_bwd[l] : nullptr;
        v.M = M[l];
        v.blk0 = s.blk0[l] = nblk;
        v.nblk_f = s.nblk_f[l] = sonet::ceil_div(M[l], CH_THREADS);
        nblk += v.nblk_f + nblk_b;
    }
    double *part = reinterpret_cast<double *>(ws);
    hipLaunchKernelGGL(chamfer_pyramid_loss_kernel, dim3(nblk, B), dim3(CH_THREADS), 0, st, a, gt, part, L, N);
    hipLaunchKernelGGL(chamfer_pyramid_sums_kernel, dim3(sonet::ceil_div(2 * B * L, 64)), dim3(64), 0, st, s, part, sums, B, L, nblk,
                       nblk_b);
    return sonet::launched(what);
}

extern "C" int sonet_chamfer_pyramid_grad_f32(const float *const *pred, const float *gt, const int32_t *const *nn_pg,
                                              const int32_t *const *nn_gp, const float *const *elem_fwd, const float *const *elem_bwd,
                                              const float *gscale, float *const *dpred, int32_t *bad, int B, int L, const int *M, int N,
                                              sonet_stream_t stream)
{
    const char *what = "sonet_chamfer_pyramid_grad_f32";
    if (int rc = pyramid_sizes(what, B, L, M, N)) return rc;
    SONET_REQUIRE(pred && gt && nn_pg && nn_gp && elem_fwd && elem_bwd && gscale && dpred && bad, "%s: NULL pointer", what);
    PyrGradArgs a = {};
    for (int l = 0; l < L; ++l) {
        SONET_REQUIRE(pred[l] && nn_pg[l] && nn_gp[l] && elem_fwd[l] && elem_bwd[l] && dpred[l], "%s: NULL pointer (level %d)", what, l);
        a.lv[l] = PyrGradLevel{pred[l], nn_pg[l], nn_gp[l], elem_fwd[l], elem_bwd[l], dpred[l], M[l]};
    }
    hipStream_t st = sonet::as_stream(stream);
    if (int rc = sonet::zero_words(bad, 4 * (size_t)L, st)) return rc;
    int P = 2;                                                   // the sort's extent: the power of two at or above N
    while (P < N) P <<= 1;
    hipLaunchKernelGGL(chamfer_pyramid_grad_kernel, dim3(L, B), dim3(PYR_THREADS), 0, st, a, gt, gscale, bad, B, N, P);
    return sonet::launched(what);
}
