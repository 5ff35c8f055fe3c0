// knn_layer.hip -- KNNModule's second layer on an input that never leaves the chip: h1 (the first layer per neighbour copy, knn_h1.hpp) is
// built in LDS as finished MFMA B fragments, multiplied by the layer-2 h3p pack and reduced over each node's K neighbour copies, in ONE
// launch (models/layers.py:319-365).  It replaces sonet_knn_stage_input_p16 + sonet_pointmlp_h3p_gmax (node_stage.hip, pointmlp_h3p.hip)
// where the shape allows it; the planes it writes and the range words it reports are theirs bit for bit:
//   * h1 is the arithmetic of knn_h1_half, the one copy both kernels include;
//   * every accumulator sums its 16-channel chunks in ascending order, the three products of a chunk as (W.lo, X.hi), (W.hi, X.mid),
//     (W.hi, X.hi): the order of pointmlp_h3p_kernel (chunks past Cin / 16 meet the pack's zero padding there and here: they add +0);
//   * the epilogue is that kernel's group-max epilogue (EPI 4): fma(acc, scale / 32, 32 shift), ReLU, nan_max over a node's GK columns
//     left to right, then gmax_p16_store (device.hpp: range, clamp, p16_split2, the two stores), the copy both kernels call.
//
// Shape: a workgroup of four waves takes one 128-column block of the K-level layout (G nodes x GK neighbour copies, node_stage.hip) and
// the whole of Cout.  Wave w owns the output tiles w MT .. w MT + MT - 1 (MT = Cout / 128) across all four 32-column tiles -- a weight
// fragment feeds 6 MFMAs, where the 32-column waves of the layer kernel get 1.5 out of one -- and holds 16 MT accumulator registers per
// column tile, 256 at MT = 4: one workgroup per CU.  The K range runs in stages of 8 chunks (128 channels x 128 columns of h1 = 64 KiB of
// LDS as [chunk][form][half][column] 16-byte vectors: a B fragment is one ds_read_b128, a half wave reads 512 contiguous bytes); two
// stages alternate, the next one is built by all 256 threads (column x half, as knn_stage_input_kernel) while the current one is
// multiplied: one workgroup barrier per stage.  Weight fragments come straight from global memory (the pack is at most 1 MiB and every
// workgroup reads all of it: L2) through a small register ring, three (chunk, tile) steps ahead.  Nothing here is an inline-asm memory
// instruction and no wait is counted by hand: a step (12 MFMAs, one weight request, its share of the build) is branch-free and fenced, so
// that hipcc interleaves the build's vector arithmetic with the MFMAs of the same step.  Measurements: docs/findings.md.
#include "common.hpp"
#include "knn_h1.hpp"

namespace {

constexpr int KL_STAGE = 8;                                    // chunks per stage = the pack's K padding (P_KPAD of pointmlp_h3p.hip)
constexpr int KL_MAXC = 512;                                   // Cin, Cout at most (the coefficient tables are static LDS)
constexpr int KL_WRING = 4;                                    // register slots of the weight-fragment ring; requests run KL_WRING - 1 steps ahead

struct KnnLayerArgs {
    const int4 *rec;                      // [Lp] records of the K-level columns
    const uint4 *zp;                      // P16 planes of z, 1 x Cin x Lm
    const float *wl, *scale1, *shift1;    // layer 1: [Cin][3], [Cin], [Cin]
    const uint4 *Wp;                      // h3p pack of layer 2 [Cout][Cin]
    const float *scale2, *shift2;         // [Cout]
    char *yp;                             // P16 planes 1 x Cout x Lout
    unsigned *rlog;
    long long Lm;
    int relu1, relu2, KC, NS, KCP, CT, Cout, GK, G, ngout, Lout;
    int abl;                              // (variants build) ablations, timing only: 1 = every weight request reads step 0's fragments, 2 = every gather reads column 0
};

struct KnnLayerLds {
    uint4 x[2][KL_STAGE][2][2][128];      // [stage buffer][chunk][form][half][column]; the epilogue stages its tiles here afterwards
    float coef[5][KL_MAXC];               // layer 1's coefficients, [kind][chunk][half][element] (knn_h1_coef)
    float aff[KL_MAXC / 32][2][2][16];    // layer 2's scale / 32 and 32 shift as [tile][half][scale, shift][register]
    unsigned wmax[4];
};
static_assert(sizeof(KnnLayerLds) <= 160 * 1024, "LDS of a CU");
static_assert(4 * 32 * GM_STRIDE * sizeof(float) <= sizeof(uint4) * 2 * KL_STAGE * 2 * 2 * 128, "the epilogue's staging fits the operand buffers");

template <int MT>
__global__ __launch_bounds__(256) void knn_layer2_gmax_kernel(const KnnLayerArgs a)
{
    __shared__ __attribute__((aligned(16))) KnnLayerLds lds;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int blk = (int)blockIdx.x;
    // build side: thread = (column, half) of the block
    const int col = tid & 127, hh = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int4 rcol = a.rec[(long long)blk * 128 + col];
    const KnnCol kcol = knn_col(rcol);
    const int KC = a.KC, Cin = KC * 16;

    for (int t = tid; t < KL_MAXC; t += 256) {
        // slot = chunk, half, element  <->  channel 16 (chunk) + p16_channel(half, element)
        const int c = (t >> 4) * 16 + p16_channel((t >> 3) & 1, t & 7);
#pragma unroll
        for (int kind = 0; kind < 5; ++kind) lds.coef[kind][t] = knn_h1_coef(kind, c < Cin, c, a.wl, a.scale1, a.shift1);
    }
    for (int o = tid; o < a.Cout; o += 256) {
        // (the table makes the epilogue's value 32 x already, like the P16-only epilogues of pointmlp_h3p_kernel; accumulators hold 1024 W.x)
        const int rr = o & 31;
        float *t = &lds.aff[o >> 5][(rr >> 2) & 1][0][(rr & 3) | ((rr >> 3) << 2)];
        t[0] = a.scale2[o] * (32.f / 1024.f);
        t[16] = a.shift2[o] * 32.f;
    }

    RangeAcc xr = {0, 0u};
    const float lo1 = a.relu1 ? 0.f : -65504.f;
    // (plane p = (chunk, form, half) of a P16 tensor with L columns starts at p L; a column without a source gathers column 0 and drops it)
    const uint4 *zbase = a.zp + (long long)hh * a.Lm + (kcol.ok ? rcol.x : 0);

    // Build side, one chunk at a time: the two 16-byte gathers of a chunk (past KC they re-read the last chunk: no branch, the values
    // are dropped below) into one of two register slots, a chunk ahead of the four PAIR units that turn them into h1 (knn_h1_pair:
    // ~30 vector instructions each), and the two 16-byte LDS writes behind the fourth unit.
    uint4 Zh[2], Zm[2];
    unsigned hv4[4], mv4[4];
    // a unit's ten coefficients are read from the table one unit ahead (two register sets): read where they are used, every unit
    // waited for its LDS round trip, five times a step
    f32x2_t creg[2][5];
    auto load_coef = [&](f32x2_t (&c)[5], int kc, int u) {
        const int ci = (kc < KC ? kc : KC - 1) * 16 + hh * 8 + 2 * u;        // (past KC: any table row; the column is forced to zeros)
#pragma unroll
        for (int kind = 0; kind < 5; ++kind) c[kind] = *reinterpret_cast<const f32x2_t *>(&lds.coef[kind][ci]);
    };
    auto gather = [&](int slot, int kc) {
        kc = kc < KC ? kc : KC - 1;
        const uint4 *zq = zbase + (long long)kc * 4 * a.Lm;
#ifdef SONET_VARIANTS
        if (a.abl & 2) zq = a.zp + (long long)hh * a.Lm;
#endif
        Zh[slot] = zq[0];
        Zm[slot] = zq[2 * a.Lm];
    };
    auto build_unit = [&](int slot, const f32x2_t (&c)[5], int kc, int buf, int q, int u) {
        const bool in = kc < KC, live = kcol.ok && in;
        const float *const cf[5] = {reinterpret_cast<const float *>(&c[0]), reinterpret_cast<const float *>(&c[1]), reinterpret_cast<const float *>(&c[2]),
                                    reinterpret_cast<const float *>(&c[3]), reinterpret_cast<const float *>(&c[4])};
        KnnCol kk = kcol;
        kk.valid = kcol.valid && in;
        const unsigned zh = u == 0 ? Zh[slot].x : u == 1 ? Zh[slot].y : u == 2 ? Zh[slot].z : Zh[slot].w;
        const unsigned zm = u == 0 ? Zm[slot].x : u == 1 ? Zm[slot].y : u == 2 ? Zm[slot].z : Zm[slot].w;
        knn_h1_pair<false>(live ? zh : 0u, live ? zm : 0u, cf, kk, lo1, xr, hv4[u], mv4[u]);
        if (u == 3) {
            lds.x[buf][q][0][hh][col] = make_uint4(hv4[0], hv4[1], hv4[2], hv4[3]);
            lds.x[buf][q][1][hh][col] = make_uint4(mv4[0], mv4[1], mv4[2], mv4[3]);
        }
    };

    // Weight fragments: a STEP is one (chunk, tile of this wave) = two 1-KiB coalesced loads (hi, residual form) and 12 MFMAs; steps run
    // chunk-major (step = chunk x MT + tile) through a ring of KL_WRING register slots, requested KL_WRING - 1 steps ahead (a whole
    // chunk's fragments a chunk ahead cost 16 MT registers: at MT = 4 hipcc then ran out of registers and loaded each fragment right in
    // front of its MFMAs; eight slots measured the same as four).  A stage is 8 MT steps, a multiple of the ring: slot = step % KL_WRING.
    const int NS = a.NS, KCT = NS * KL_STAGE;
    const uint4 *wbase = a.Wp + ((size_t)(wave * MT) * a.KCP * 2) * 64 + lane;
    uint4 Wr[KL_WRING][2];
    auto load_w = [&](int kc0, int t) {                        // step t of the stage that starts at chunk kc0 (t may reach into the next one)
        int kc = kc0 + t / MT;
        kc = kc < KCT ? kc : KCT - 1;                          // (past the last chunk: re-read it; the fragments are not used)
        const uint4 *wq = wbase + ((size_t)(t % MT) * a.KCP + kc) * 128;
#ifdef SONET_VARIANTS
        if (a.abl & 1) wq = wbase;
#endif
        Wr[t % KL_WRING][0] = wq[0];
        Wr[t % KL_WRING][1] = wq[64];
    };

    f32x16 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][c][r] = 0.f;

    // B fragments of a chunk: [form][column tile], two register sets -- the next chunk's are read while this one is multiplied
    f16x8 Bf[2][2][4];
    auto read_b = [&](int set, int buf, int q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            Bf[set][0][c] = __builtin_bit_cast(f16x8, lds.x[buf][q][0][h][32 * c + j]);
            Bf[set][1][c] = __builtin_bit_cast(f16x8, lds.x[buf][q][1][h][32 * c + j]);
        }
    };

    // ---- stage 0 is built before the loop; stage s + 1 while stage s is multiplied -------------------------------------------
#pragma unroll
    for (int t = 0; t < KL_WRING - 1; ++t) load_w(0, t);
    {
        // (all 16 gathers of the stage in flight at once, under the table fill: nothing else holds registers yet)
        uint4 Ph[KL_STAGE], Pm[KL_STAGE];
#pragma unroll
        for (int q = 0; q < KL_STAGE; ++q) {
            gather(0, q);
            Ph[q] = Zh[0];
            Pm[q] = Zm[0];
        }
        __syncthreads();                                       // the tables
#pragma unroll
        for (int q = 0; q < KL_STAGE; ++q) {
            Zh[0] = Ph[q];
            Zm[0] = Pm[q];
            f32x2_t c4[4][5];
#pragma unroll
            for (int u = 0; u < 4; ++u) load_coef(c4[u], q, u);
#pragma unroll
            for (int u = 0; u < 4; ++u) build_unit(0, c4[u], q, 0, q, u);
        }
    }
    if (NS > 1) load_coef(creg[0], KL_STAGE, 0);

    // (BUILD = false: the last stage, behind which nothing is left to build -- its own loop body, so that neither body has a branch)
    auto stage = [&](int s, auto build_next) {
        constexpr bool BUILD = decltype(build_next)::value;
        const int buf = s & 1, kc0 = s * KL_STAGE, kn = kc0 + KL_STAGE;
        __syncthreads();                                       // stage s is complete; every wave has left the other buffer
        read_b(0, buf, 0);
        if constexpr (BUILD) gather(0, kn);
        // Chunk q of this stage is multiplied while chunk q of the next stage is built: per step one weight request (KL_WRING - 1 steps ahead),
        // 12 MFMAs and the step's share of the chunk's four pair units.  A scheduling fence per step: what hipcc interleaves, it
        // interleaves inside a step -- left alone it gathered requests and vector work from all over the stage until it ran out of registers.
#pragma unroll
        for (int q = 0; q < KL_STAGE; ++q) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int t = q * MT + mt;
                load_w(kc0, t + KL_WRING - 1);
                if (mt == 0 && q + 1 < KL_STAGE) {
                    read_b((q + 1) & 1, buf, q + 1);
                    if constexpr (BUILD) gather((q + 1) & 1, kn + q + 1);
                }
                const f16x8 wh = __builtin_bit_cast(f16x8, Wr[t % KL_WRING][0]), wm = __builtin_bit_cast(f16x8, Wr[t % KL_WRING][1]);
#pragma unroll
                for (int term = 0; term < 3; ++term)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[mt][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(term == 0 ? wm : wh, Bf[q & 1][term == 1 ? 1 : 0][c], acc[mt][c], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (BUILD && u * MT / 4 == mt) {
                        const int n = q * 4 + u;                             // unit of the stage; the next one may be the next stage's first
                        load_coef(creg[(n + 1) & 1], kn + (n + 1) / 4, (n + 1) % 4);
                        build_unit(q & 1, creg[n & 1], kn + q, buf ^ 1, q, u);
                    }
                // (one wave per SIMD hides about five single-issue instructions behind an MFMA: the step's vector work in threes and fours)
#define KL_GAP2 __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 3, 0); \
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                KL_GAP2 KL_GAP2 KL_GAP2 KL_GAP2 KL_GAP2 KL_GAP2
#undef KL_GAP2
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    for (int s = 0; s + 1 < NS; ++s) stage(s, bool_c<true>{});
    stage(NS - 1, bool_c<false>{});
    __syncthreads();                                           // every wave is done with the operands: the buffers become the epilogue's

    // ---- epilogue: per tile of this wave, 32 rows x 128 columns through LDS, max over each node's GK columns -> P16 planes ----
    float (*gm)[GM_STRIDE] = reinterpret_cast<float (*)[GM_STRIDE]>(reinterpret_cast<char *>(&lds.x[0][0][0][0][0]) + (size_t)wave * (32 * GM_STRIDE * 4));
    RangeAcc yr = {0, 0u};
    const float relu_thr = a.relu2 ? 0.f : -__builtin_inff();  // v < thr ? 0 : v  (a NaN stays a NaN, as torch's ReLU leaves it)
    const float split_lo = a.relu2 ? 0.f : -2047.f;
    // (the lane's coordinates of the reduce side are formed here, behind the loop, from an opaque copy of the thread id: derived before
    // the loop they would be carried through it, and at MT = 4 every vector register in the loop is taken)
    int tid2 = tid;
    asm volatile("" : "+v"(tid2));
    const int je = tid2 & 31, he = (tid2 >> 5) & 1;           // (j and h again)
    const int p = tid2 & 3, g = (tid2 & 63) >> 2;             // reduce side: lane = (element pair of a P16 half, node of the block)
    const long long n_out = (long long)blk * a.G + g;
    const bool node = g < a.G && n_out < a.ngout;
    const float *rbase = &gm[2 * (p & 1) + 8 * (p >> 1)][(g < a.G ? g : 0) * a.GK];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int ct = wave * MT + mt;
        float sc16[16], sh16[16];
        {
            const float4 *t4 = reinterpret_cast<const float4 *>(&lds.aff[ct][he][0][0]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 s4 = t4[u], h4 = t4[4 + u];
                sc16[4 * u] = s4.x; sc16[4 * u + 1] = s4.y; sc16[4 * u + 2] = s4.z; sc16[4 * u + 3] = s4.w;
                sh16[4 * u] = h4.x; sh16[4 * u + 1] = h4.y; sh16[4 * u + 2] = h4.z; sh16[4 * u + 3] = h4.w;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = __fmaf_rn(acc[mt][c][r], sc16[r], sh16[r]);
                gm[(r & 3) + 8 * (r >> 2) + 4 * he][32 * c + je] = v < relu_thr ? 0.f : v;
            }
        // (only this wave reads what it wrote: its LDS operations complete in order, the fences keep hipcc from moving them)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // 16-row chunk qq and half h2 of the tile (qh = 2 qq + h2): two rows x GK columns per lane and qh, each maximum taken left to
        // right; the four qh side by side, so that eight LDS reads are in flight per step
        float m0[4], m1[4];
#pragma unroll
        for (int qh = 0; qh < 4; ++qh) {
            const float *r0 = rbase + (16 * (qh >> 1) + 4 * (qh & 1)) * GM_STRIDE;
            m0[qh] = r0[0];
            m1[qh] = r0[GM_STRIDE];
        }
        for (int k = 1; k < a.GK; ++k) {
#pragma unroll
            for (int qh = 0; qh < 4; ++qh) {
                const float *r0 = rbase + (16 * (qh >> 1) + 4 * (qh & 1)) * GM_STRIDE;
                m0[qh] = nan_max(m0[qh], r0[k]);
                m1[qh] = nan_max(m1[qh], r0[GM_STRIDE + k]);
            }
        }
        if (node) {
#pragma unroll
            for (int qh = 0; qh < 4; ++qh) {
                const int qq = qh >> 1, h2 = qh & 1;
                gmax_p16_store(m0[qh], m1[qh], split_lo, yr, a.yp, ct * 2 + qq, h2, p, (size_t)a.Lout, (size_t)n_out);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    if (a.rlog != nullptr) {
        // what the two launches report: h1's post-activation maximum and the output planes' maximum (word 2), the pack's weight word (word 1)
        const unsigned b1 = range_x32_out(wave_umax(range_act_bits(xr, a.relu1)));
        const unsigned b2 = range_x32_out(wave_umax(range_act_bits(yr, a.relu2)));
        if ((tid2 & 63) == 0) lds.wmax[wave] = b1 > b2 ? b1 : b2;
        __syncthreads();
        if (tid2 == 0) {
            const unsigned m01 = lds.wmax[0] > lds.wmax[1] ? lds.wmax[0] : lds.wmax[1], m23 = lds.wmax[2] > lds.wmax[3] ? lds.wmax[2] : lds.wmax[3];
            const unsigned mx = m01 > m23 ? m01 : m23;
            if (mx > __atomic_load_n(a.rlog + 2, __ATOMIC_RELAXED)) atomicMax(a.rlog + 2, mx);
            if (blk == 0) atomicMax(a.rlog + 1, reinterpret_cast<const unsigned *>(a.Wp + (size_t)a.CT * a.KCP * 128)[0]);
        }
    }
}

}  // namespace

/* KNNModule's first layer per neighbour copy + its second layer + the max over the K neighbours, one launch: what
 * sonet_knn_stage_input_p16 followed by sonet_pointmlp_h3p_gmax (P16 out) computes, bit for bit, without h1 in memory. */
extern "C" int sonet_knn_layer2_gmax_p16(const void *rec, const void *z_p16, const float *wl, const float *scale1, const float *shift1, int relu1,
                                         int B, int M, int K, int Cin, const void *Wp, const float *scale2, const float *shift2, int relu2,
                                         int Cout, int GK, int G, int ngout, int Lout, void *yp, sonet_stream_t stream)
{
    const char *what = "sonet_knn_layer2_gmax_p16";
    SONET_REQUIRE(rec && z_p16 && wl && scale1 && shift1 && Wp && scale2 && shift2 && yp, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && M > 0 && Cin > 0 && Cout > 0 && K >= 1 && K <= 128, "%s: bad size B=%d M=%d Cin=%d Cout=%d K=%d", what, B, M, Cin, Cout, K);
    SONET_REQUIRE(GK == K && G == knn_stage_groups(K) && (long long)ngout == (long long)B * M, "%s: the grouping of the K-level layout is GK=%d G=%d ngout=%d", what,
                  K, knn_stage_groups(K), B * M);
    SONET_REQUIRE(Lout >= ngout, "%s: Lout=%d (the planes' column count) below ngout=%d", what, Lout, ngout);
    if (Cout % 128 != 0 || Cout > KL_MAXC) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: Cout=%d must be a multiple of 128, at most %d", what, Cout, KL_MAXC);
    if (Cin % 16 != 0 || Cin > KL_MAXC) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: Cin=%d must be a multiple of 16, at most %d", what, Cin, KL_MAXC);
    if (G * GK > 128) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: G GK = %d columns exceed a block", what, G * GK);
    const long long Lp = (long long)sonet_knn_stage_columns(B, M, K), Lm = (long long)sonet_node_stage_columns(B, M);
    const long long nblk = Lp / 128;
    const int KC = Cin / 16, NS = sonet::ceil_div(KC, KL_STAGE), KCP = NS * KL_STAGE, CT = Cout / 32;
    if (nblk > 0x7FFFFFFFll || (double)KC * 64.0 * (double)Lm >= 2.0e9 || (double)(Cout / 16) * 64.0 * (double)Lout >= 2.0e9 || (double)CT * KCP * 2048.0 >= 2.0e9)
        return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: a panel exceeds 2 GiB", what);
    KnnLayerArgs a;
    a.rec = reinterpret_cast<const int4 *>(rec); a.zp = reinterpret_cast<const uint4 *>(z_p16); a.wl = wl; a.scale1 = scale1; a.shift1 = shift1;
    a.Wp = reinterpret_cast<const uint4 *>(Wp); a.scale2 = scale2; a.shift2 = shift2; a.yp = static_cast<char *>(yp); a.rlog = sonet::range_log();
    a.Lm = Lm; a.relu1 = relu1; a.relu2 = relu2; a.KC = KC; a.NS = NS; a.KCP = KCP; a.CT = CT; a.Cout = Cout; a.GK = GK; a.G = G; a.ngout = ngout; a.Lout = Lout;
    a.abl = 0;
#ifdef SONET_VARIANTS
    sonet::knob_int("SONET_KL_ABL", &a.abl);
#endif
    with_int_c<1, 2, 3, 4>(Cout / 128, [&](auto mt) {
        hipLaunchKernelGGL((knn_layer2_gmax_kernel<decltype(mt)::value>), dim3((unsigned)nblk), dim3(256), 0, sonet::as_stream(stream), a);
    });
    return sonet::launched(what);
}
