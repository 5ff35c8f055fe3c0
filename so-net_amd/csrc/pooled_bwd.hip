// pooled_bwd.hip -- backward of the pooled last layer of the first PointNet (training) over the arg-max positions of the per-node max-pool.
//   the blocks     pd_key / pd_key_col / pd_key_id (the sort key of an entry), pd_bounds (a tile's bucket boundaries), pd_entry (the staged
//                  record of an entry), pd_chain4 (the fma chains of a column-owned four-channel thread), pd_out / pd_store_tile (the way out);
//                  pooled_dgrad5_kernel and pooled_wgrad_kernel, the pair of every training step, keep their own spelling (docs/findings.md)
//   the lists      pooled_bucket_kernel (entries into 32-column buckets), pooled_sort_kernel (each bucket by (column, entry id))
//   sparse dgrad   pooled_dgrad_kernel (one channel per thread: any width), pooled_dgrad4_kernel (four channels, column-owned: variants build,
//                  the bit-exact twin of the former), pooled_dgrad5_kernel (four channels, entry-balanced: the product's; <TAIL>: the
//                  measured-slower riders on its store, variants build) with pd_sums_finalize_kernel
//   dense tile     pooled_dgrad_mfma_kernel (bf16 output: the tile of the never-built gradient times W^T on the matrix cores)
//   sparse wgrad   pooled_wgrad_kernel
//   host           PdWs (the workspace), pd_check (what both dgrad launchers check first), the entry points
#include "common.hpp"

#include <hip/hip_runtime.h>

// ---- sparse dgrad of the pooled last layer ---------------------------------------------------
// In the classifier / autoencoder the only consumer of first_pn_out = W4 . [x1; x2] + b is the per-node max-pool
// (models/networks.py:180-185), so d loss / d first_pn_out has exactly M non-zeros per (b, c) row -- at the arg-max
// positions.  Instead of scattering them into a dense B x 384 x kN tensor and running a dense W4^T GEMM over it
// (234x more MACs than needed at N = 5000), the entries are bucketed by 32-column quarter of a 128-column tile and every tile accumulates
//     g_x[b][:, l] += g[b][c][m] * W4[c][:]      for its entries (c, m) -> l
// in LDS, 40 input channels per workgroup, then writes its 40 x 128 block with coalesced stores (the [C][L] layout makes a direct scatter
// of the 320-vectors uncoalesced in both directions).  The entries of a bucket are sorted by (column, entry id) before they are applied, so
// the result does not depend on the order the bucket atomics happened to take.
namespace {

constexpr int PD_TL = 128;                     // columns per tile: 256-byte (bf16) / 512-byte (f32) row segments on the way out.  (Round 3: 32
                                               // columns x all 320 channels -- 64-byte bf16 row pieces, every one a partial cache line.)
constexpr int PD_CH = 40;                      // input channels per workgroup (blockIdx.z): 41 KB of accumulators
constexpr int PD_CQ = 4;                       // thread groups per channel: group q owns column quarter q of the tile ...
constexpr int PD_SB = PD_TL / PD_CQ;           // ... = one 32-column bucket of the entry lists (~52 entries at the benchmark shape)
constexpr int PD_WB = 16;                      // W rows requested before the first fma (64 -- a whole bucket in one round trip -- measured slower)
constexpr int PD_SQ = 128;                     // entries per group sorted in LDS at a time (more: further rounds, still in global rank order)

// The sort key of an entry: (column inside its bucket, entry id), distinct per entry; entry id = c * M + m, the consumer recovers the
// channel as id / M.  The launchers refuse C * M >= PD_KEY_IDS.
constexpr int PD_KEY_BITS = 20;
constexpr long long PD_KEY_IDS = 1ll << PD_KEY_BITS;
__device__ __forceinline__ uint32_t pd_key(int col, int id) { return ((uint32_t)col << PD_KEY_BITS) | (uint32_t)id; }
__device__ __forceinline__ int pd_key_col(uint32_t key) { return (int)(key >> PD_KEY_BITS); }
__device__ __forceinline__ int pd_key_id(uint32_t key) { return (int)(key & (uint32_t)(PD_KEY_IDS - 1)); }

// bnd[0 .. N]: where the N consecutive buckets from sb0 on begin and end in cloud b's entry list (buckets past the last one are empty)
template <int N>
__device__ __forceinline__ void pd_bounds(const int32_t *__restrict__ tile_off, int b, int nbucket, int sb0, int (&bnd)[N + 1])
{
    const int32_t *to = tile_off + (size_t)b * (nbucket + 1);
#pragma unroll
    for (int t = 0; t <= N; ++t) bnd[t] = to[min(sb0 + t, nbucket)];
}

// channel ch of cloud b on its way out: its row of the first panel (C1 channels) or of the second (the other Cin - C1)
template <typename TO>
__device__ __forceinline__ TO *pd_out(TO *gx1, TO *gx2, int b, int ch, int C1, int Cin, int L)
{
    return ch < C1 ? gx1 + ((size_t)b * C1 + ch) * L : gx2 + ((size_t)b * (Cin - C1) + (ch - C1)) * L;
}

// The accumulators acc[PD_TL][ld] of tile `tile`, channels [ch0, ch0 + nch), to the output; one rounding for bf16.
template <typename TO>
__device__ __forceinline__ void pd_store_tile(const float *acc, int ld, int tile, int b, int ch0, int nch, int C1, int Cin, int L, TO *gx1, TO *gx2)
{
    const int tid = threadIdx.x, nth = blockDim.x, l0 = tile * PD_TL;
    if (sizeof(TO) == 2 && (L & 1) == 0) {
        // bf16 output, even L: two columns per thread, one 4-byte store -- 64 consecutive threads write the 256 bytes of a row segment
        for (int idx = tid; idx < nch * (PD_TL / 2); idx += nth) {
            const int r = idx / (PD_TL / 2), col = (idx - r * (PD_TL / 2)) * 2;
            if (l0 + col >= L) continue;                        // (L even: col + 1 is inside too)
            const unsigned pk = cvt_pk_bf16(acc[col * ld + r], acc[(col + 1) * ld + r]);
            *reinterpret_cast<unsigned *>(pd_out(gx1, gx2, b, ch0 + r, C1, Cin, L) + l0 + col) = pk;
        }
        return;
    }
    for (int idx = tid; idx < nch * PD_TL; idx += nth) {        // coalesced: consecutive threads along the columns of one channel
        const int r = idx / PD_TL, col = idx - r * PD_TL;
        if (l0 + col >= L) continue;
        st_rne(pd_out(gx1, gx2, b, ch0 + r, C1, Cin, L), l0 + col, acc[col * ld + r]);
    }
}

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
        ent_key[(size_t)b * E + p] = pd_key(l - t * PD_SB, e);
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
    for (int e = lane; e < nq; e += 64) atomicAdd(&colcnt[pd_key_col(kb[e])], 1);
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
        tmp[atomicAdd(&cursor[pd_key_col(key)], 1)] = key;
    }
    __syncthreads();
    for (int t = lane; t < nq; t += 64) {
        const uint32_t key = tmp[t];
        const int col = pd_key_col(key);
        const int s0 = segstart[col], s1 = s0 + colcnt[col];
        int rank = 0;
        for (int u = s0; u < s1; ++u) rank += tmp[u] < key;
        out[s0 + rank] = key;
    }
}

template <typename TO>
__global__ __launch_bounds__(PD_CH * PD_CQ) void pooled_dgrad_kernel(const int32_t *__restrict__ tile_off, const uint32_t *__restrict__ ent_key,
                                                           const float *__restrict__ g_pooled /*[B][E]: the entries' values by id*/,
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
    int bnd[2];                                                             // this group's bucket (32 columns)
    pd_bounds<1>(tile_off, b, nbucket, tile * PD_CQ + q, bnd);
    const int beg = bnd[0], nq = bnd[1] - beg;
    const uint32_t *kb = ent_key + (size_t)b * E + beg;
    const float *gb = g_pooled + (size_t)b * E;
    if (i == 0) nq_all[q] = nq;
    __syncthreads();
    int nmax = 0;
#pragma unroll
    for (int t = 0; t < PD_CQ; ++t) nmax = max(nmax, nq_all[t]);
    // The group's bucket arrives SORTED by (column, entry id) (pooled_sort_kernel above: once per bucket instead of once per (bucket,
    // channel slab)), so the order of the fma chain of an accumulator is fixed whatever order the bucket atomics took; thread (i, q)
    // applies the group's entries to channel ch0 + i (no two threads touch the same accumulator).  Rounds of PD_SQ consecutive entries: a
    // column that continues in the next round resumes from the stored value.
    for (int base = 0; base < nmax; base += PD_SQ) {
        const int n = min(PD_SQ, max(0, nq - base));
        __syncthreads();                                                    // the previous round's lists are consumed
        for (int t = i; t < n; t += PD_CH) {
            const uint32_t key = kb[base + t];
            const int id = pd_key_id(key);
            keys[t] = (uint32_t)(pd_key_col(key) + q * PD_SB);              // column inside the tile
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
    pd_store_tile(acc, ld, tile, b, ch0, nch, C1, Cin, L, gx1, gx2);
}

// The staged record of an entry, 16 bytes: (column inside the tile -- its bucket is quarter q --, value bits, offset of its W row for the
// workgroup's channel slab, -)
__device__ __forceinline__ uint4 pd_entry(uint32_t key, int q, const float *__restrict__ gb, int M, int Cin, int ch0)
{
    const int id = pd_key_id(key);
    return make_uint4((unsigned)(pd_key_col(key) + q * PD_SB), __float_as_uint(gb[id]), (unsigned)((id / M) * Cin + ch0), 0u);
}

// The fma chains of a four-channel thread over its cnt > 0 staged entries ent[0 .. cnt), sorted by column: acc4 / W4 are the accumulator row
// of column 0 and W, both at the thread's channel quad.  PD4_WB entries and their float4 of W are requested before the first fma; the chains
// of a column run in registers and are written when the column changes (a column that continues from an earlier round resumes from the stored
// value -- the accumulators start at zero).  The entry-balanced kernel spells the same loop with a cut column's sum parked in `head`: through
// this helper (a PARK template argument) the pair it runs beside the weight gradient measured slower, docs/findings.md.
constexpr int PD4_LD = PD_CH + 4;              // accumulator row pitch: 16-byte aligned groups of four channels
constexpr int PD4_WB = 8;                      // entries (a W float4 each) requested before the first fma
__device__ __forceinline__ void pd_chain4(const uint4 *ent, int cnt, const float *__restrict__ W4, float *acc4)
{
    constexpr int ld = PD4_LD;
    int cur = (int)ent[0].x;
    float4 sum = *reinterpret_cast<const float4 *>(acc4 + cur * ld);
    for (int e0 = 0; e0 < cnt; e0 += PD4_WB) {
        uint4 en[PD4_WB];
        float4 wv[PD4_WB];
#pragma unroll
        for (int t = 0; t < PD4_WB; ++t) {
            en[t] = ent[e0 + t < cnt ? e0 + t : cnt - 1];
            wv[t] = *reinterpret_cast<const float4 *>(W4 + (size_t)en[t].z);
        }
#pragma unroll
        for (int t = 0; t < PD4_WB; ++t) {
            if (e0 + t < cnt) {
                const int col = (int)en[t].x;
                if (col != cur) {
                    *reinterpret_cast<float4 *>(acc4 + cur * ld) = sum;
                    cur = col;
                    sum = *reinterpret_cast<const float4 *>(acc4 + cur * ld);
                }
                const float v = __uint_as_float(en[t].y);
                sum.x = __fmaf_rn(v, wv[t].x, sum.x);
                sum.y = __fmaf_rn(v, wv[t].y, sum.y);
                sum.z = __fmaf_rn(v, wv[t].z, sum.z);
                sum.w = __fmaf_rn(v, wv[t].w, sum.w);
            }
        }
    }
    *reinterpret_cast<float4 *>(acc4 + cur * ld) = sum;
}

// Four channels per thread (Cin a multiple of 4).  The accumulate loop of the one-channel kernel is bound by instruction issue, not by latency: per
// (entry, channel) three LDS reads, an address, a global load, a compare and one fma.  Here thread (i4, q, s) owns channels 4 i4 .. 4 i4 + 3 of the
// columns [8 s, 8 s + 8) of quarter q: the same per-entry overhead (one 16-byte LDS read, one 16-byte load of W) feeds four fmas, and the
// sixteen sub-ranges of a tile (their entry counts differ less than the four quarters') share the wave's loop trips.  Same entries in the same
// (column, entry id) order per accumulator: the same bits as the one-channel kernel.
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
    int bnd[2];
    pd_bounds<1>(tile_off, b, nbucket, tile * PD_CQ + q, bnd);
    const int beg = bnd[0], nq = bnd[1] - beg;
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
            ent[t] = pd_entry(key, q, gb, M, Cin, ch0);
            atomicAdd(&subcnt[q][pd_key_col(key) >> 3], 1);
        }
        __syncthreads();
        int lo = 0;
        for (int t = 0; t < sub; ++t) lo += subcnt[q][t];
        const int cnt = subcnt[q][sub];
        if (4 * i4 < nch && cnt > 0) pd_chain4(ent + lo, cnt, W + 4 * i4, acc + 4 * i4);
    }
    __syncthreads();
    pd_store_tile(acc, ld, tile, b, ch0, nch, C1, Cin, L, gx1, gx2);
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
            const int id = pd_key_id(key);
            const int q = (e >= bo[1]) + (e >= bo[2]) + (e >= bo[3]);      // the bucket of the tile this entry sits in
            ent[t] = make_uint4((unsigned)(pd_key_col(key) + q * PD_SB), __float_as_uint(gb[id]), (unsigned)((id / M) * Cin + ch0), 0u);
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
                            const float gm = relu_masked(v[t], rw[t], sc[t], sh[t], tail.srelu);
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
    int bnd[2 * CH + 1];
    pd_bounds<2 * CH>(tile_off, b, nbucket, tile * 2 * CH, bnd);
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
        const int l = pd_key_col(key) + PD_SB * bk, c = pd_key_id(key) / M;
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
            uint16_t *dst = pd_out(gx1, gx2, b, ci, C1, C1 + C2, L) + c0;
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
                // (pd_out spelled out: through the helper these 16 NMT unrolled stores measured 2 % slower, docs/findings.md)
                uint16_t *dst = ci < C1 ? gx1 + ((size_t)b * C1 + ci) * L + col : gx2 + ((size_t)b * C2 + (ci - C1)) * L + col;
                *reinterpret_cast<unsigned *>(dst) = pk;
            }
        }
    }
    }
}

// The workspace of the dgrad launchers: the bucket lists (key, value) of B clouds of E entries, the sorted keys, the bucket offsets.  The
// matrix-core launcher sorts nothing and puts the offsets right behind the values (`sorted` false); the size is the same for both.
struct PdWs {
    uint32_t *ent_key;
    float *ent_val;
    uint32_t *skey;
    int32_t *tile_off;
    static size_t bytes(size_t B, size_t E, size_t nbucket) { return B * (E * 12 + (nbucket + 1) * 4); }
    PdWs(void *ws, int B, int E, bool sorted)
        : ent_key(reinterpret_cast<uint32_t *>(ws)), ent_val(reinterpret_cast<float *>(ent_key + (size_t)B * E)),
          skey(reinterpret_cast<uint32_t *>(ent_val + (size_t)B * E)), tile_off(reinterpret_cast<int32_t *>(sorted ? skey + (size_t)B * E : skey)) {}
};

// what both dgrad launchers check first (`w`: the weights or their pack)
int pd_check(const char *what, const void *g_pooled, const void *pos, const void *w, const void *ws, const void *gx1, const void *gx2, int B,
             int C, int M, int C1, int C2, int L)
{
    SONET_REQUIRE(g_pooled && pos && w && ws && gx1, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && C > 0 && M > 0 && C1 > 0 && C2 >= 0 && L > 0, "%s: non-positive size", what);
    SONET_REQUIRE((C2 == 0) == (gx2 == nullptr), "%s: gx2 and C2 disagree", what);
    return SONET_OK;
}

}  // namespace

extern "C" size_t sonet_pooled_dgrad_ws_size(int B, int C, int M, int L)
{
    if (B <= 0 || C <= 0 || M <= 0 || L <= 0) return 0;
    return PdWs::bytes((size_t)B, (size_t)C * M, (size_t)sonet::ceil_div(L, PD_SB));
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
    if (const int rc = pd_check(what, g_pooled, pos, W, ws, gx1, gx2, B, C, M, C1, C2, L)) return rc;
    const int Cin = C1 + C2, E = C * M, ntile = sonet::ceil_div(L, PD_TL), nbucket = sonet::ceil_div(L, PD_SB);
    if ((long long)C * M >= PD_KEY_IDS || B > 65535) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: C*M=%d entries per cloud (max 2^20)", what, E);
    const size_t lds2 = ((size_t)PD_TL * (PD_CH + 1) + (size_t)PD_CQ * 3 * PD_SQ) * 4;
    if ((size_t)(2 * nbucket + 1) * 4 > 64 * 1024) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: L=%d too large for the bucket counters", what, L);
    const PdWs w(ws, B, E, true);
    hipStream_t st = sonet::as_stream(stream);
    int abl = 0;
    if (const char *e = sonet::knob("SONET_PD_ABL")) abl = atoi(e);
    hipLaunchKernelGGL(pooled_bucket_kernel, dim3(B, PB_Q), dim3(1024), (size_t)(2 * sonet::ceil_div(nbucket, PB_Q) + 1) * 4, st, pos, g_pooled, E, L, nbucket, w.tile_off, w.ent_key, w.ent_val);
    if (!(abl & 4)) hipLaunchKernelGGL(pooled_sort_kernel, dim3(nbucket, B), dim3(64), 0, st, w.tile_off, w.ent_key, w.skey, E, nbucket);
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
                hipLaunchKernelGGL((pooled_dgrad5_kernel<TO, true>), dim3(ntile, B, sonet::ceil_div(Cin, PD_CH)), dim3(PD_CH * PD_CQ), lds5, st, w.tile_off, w.skey, g_pooled, W, E, M,
                                   Cin, C1, L, nbucket, gx1, gx2 ? gx2 : gx1, *tail);
                if (tail->sraw) hipLaunchKernelGGL(pd_sums_finalize_kernel, dim3((unsigned)C2), dim3(256), 0, st, tail->spart, B * ntile, C2, tail_sums);
                return sonet::launched(what);
            }
        }
#endif
        hipLaunchKernelGGL(pooled_dgrad5_kernel<TO>, dim3(ntile, B, sonet::ceil_div(Cin, PD_CH)), dim3(PD_CH * PD_CQ), lds5, st, w.tile_off, w.skey, g_pooled, W, E, M, Cin, C1,
                           L, nbucket, gx1, gx2 ? gx2 : gx1, PdTail{nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr});
        return sonet::launched(what);
    }
#ifdef SONET_VARIANTS
    if (Cin % 4 == 0 && abl == 0 && !one && which == 4) {
        const size_t lds4 = (size_t)PD_TL * PD4_LD * 4 + (size_t)PD_CQ * PD_SQ * 16;
        hipLaunchKernelGGL(pooled_dgrad4_kernel<TO>, dim3(ntile, B, sonet::ceil_div(Cin, PD_CH)), dim3(PD_CH * PD_CQ), lds4, st, w.tile_off, w.skey, g_pooled, W, E, M, Cin, C1,
                           L, nbucket, gx1, gx2 ? gx2 : gx1);
        return sonet::launched(what);
    }
#endif
    hipLaunchKernelGGL(pooled_dgrad_kernel<TO>, dim3(ntile, B, sonet::ceil_div(Cin, PD_CH)), dim3(PD_CH * PD_CQ), lds2, st, w.tile_off, (abl & 4) ? w.ent_key : w.skey, g_pooled, W, E, M, Cin, C1,
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
    if (const int rc = pd_check(what, g_pooled, pos, wt_pack, ws, gx1, gx2, B, C, M, C1, C2, L)) return rc;
    const int Cin = C1 + C2, E = C * M, CT = sonet::ceil_div(Cin, 32), nbucket = sonet::ceil_div(L, PD_SB);
    if ((L & 1) || C % 16 || C * 2 + 16 > PM_PITCH || (CT & 1) || CT > 12 || (long long)C * M >= PD_KEY_IDS || B > 65535 ||
        (size_t)(2 * nbucket + 1) * 4 > 64 * 1024 || ((reinterpret_cast<uintptr_t>(gx1) | reinterpret_cast<uintptr_t>(gx2)) & 3))
        return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: shape B=%d C=%d M=%d C1=%d C2=%d L=%d not supported", what, B, C, M, C1, C2, L);
    const PdWs w(ws, B, E, false);
    hipStream_t st = sonet::as_stream(stream);
    hipLaunchKernelGGL(pooled_bucket_kernel, dim3(B, PB_Q), dim3(1024), (size_t)(2 * sonet::ceil_div(nbucket, PB_Q) + 1) * 4, st, pos, g_pooled, E, L, nbucket, w.tile_off, w.ent_key, w.ent_val);
    // 128-column workgroups (four waves, one per CU: W^T crosses the L2 once per 128 columns) on big launches, 64-column ones otherwise
    int ch = (long long)B * sonet::ceil_div(L, 2 * PM_TL) >= 2048 ? 2 : 1;
    if (const char *e = sonet::knob("SONET_PM_CH")) { const int v = atoi(e); if (v == 1 || v == 2) ch = v; }
    const int ntile_l = sonet::ceil_div(L, PM_TL * ch);
    size_t lds = (size_t)2 * 32 * ch * PM_PITCH;
    if (ch == 2 && (size_t)CT * 32 * 272 > lds) lds = (size_t)CT * 32 * 272;          // (the output tile reuses the image)
    const uint4 *wtp = reinterpret_cast<const uint4 *>(wt_pack);
    uint16_t *g2 = gx2 ? gx2 : gx1;
    int rc = SONET_OK;
    with_int_c<1, 2, 3, 4, 5, 6>(CT / 2, [&](auto nmt) {       // (pairs of 32-row tiles per cin half; a count outside the list takes the last)
        auto launch = [&](auto cc) {
            constexpr int NN = decltype(nmt)::value, CC = decltype(cc)::value;
            rc = sonet::launch_lds_once<&pooled_dgrad_mfma_kernel<NN, CC>, 128 * 1024>(what, dim3(ntile_l, B), dim3(128 * CC), lds, st, w.tile_off, w.ent_key,
                                                                                    w.ent_val, wtp, E, M, C, C / 16, C1, C2, L, nbucket, gx1, g2);
        };
        if (ch == 2) launch(int_c<2>{}); else launch(int_c<1>{});
    });
    if (rc) return rc;
    return sonet::launched(what);
}
