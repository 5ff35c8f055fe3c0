// upconv_bwd.hip -- the input gradient of the decoder's up-convolution as ONE launch per layer (training):
//   y = conv3x3_pad1(upsample2_nearest(x), w),  g = dL/dy [B][Cout][2H][2W]   ->   dx = dL/dx [B][Cin][H][W]
//
// Folded form (upconv.hip): output pixel (2i + py, 2j + px) reads the low-resolution pixels (i - 1 + py + dy, j - 1 + px + dx) with the
// sixteen folded (parity, tap) matrices Wf[py][px][dy][dx] [Cout][Cin].  Transposed: the input pixel (u, v) collects, from the parity plane
// g[:, :, py::2, px::2], the pixel (u + 1 - py - dy, v + 1 - px - dx) -- zeros outside [0, H) x [0, W) --
//       dx = sum over py, px, dy, dx' of  Wf[py][px][dy][dx']^T . shifted(g[:, :, py::2, px::2], 1 - py - dy, 1 - px - dx')
// -- 16 Cout instead of 36 Cout multiplies per input element, and neither the upsampled map nor its gradient ever exists.
//
// Arithmetic: the three-way bf16 split of BOTH operands (pointmlp_x3.hip): six products on v_mfma_f32_32x32x16_bf16, smallest first, f32
// accumulation -- gradients are far below the range of the forward's fp16 split.  The folded weights are summed in float64, rounded to f32
// and split by the pack kernel (split3_pair_w); g is split when it is staged (split3_pair).  Sixteen (parity, tap) products go into ONE
// accumulator set: every DG_FLUSH chunks (16 x 16 x 4 = 1024 products, the forward's chain) it is added to a second set and restarts
// from zero.  No atomics: the result is a function of the operands alone, bit for bit.
//
// Tiling: the forward's flat column axis, c = (b H + i) W + j.  A workgroup (4 waves) owns UP_TP = 128 consecutive columns x one 32-row
// block of Cin; a wave owns 32 columns.  The reduction runs over Cout in chunks of 16 channels, each chunk in two stages, one per py:
//   * the two parity planes (px = 0, 1: one 8-byte load per row) of the columns c0 - W - 1 .. c0 + 127 + W + 1 of the chunk, as three bf16
//     pieces in MFMA B-fragment order; a neighbour in the padding or in another cloud is read from a slot of zeros;
//   * the eight (px, dy, dx) A fragments of the stage (3 KiB each, three pieces) -- except those whose shifted operand lies in the padding
//     for EVERY column of the tile, which are neither read nor multiplied.
// 74 KB of LDS per workgroup: two workgroups per CU.  The next stage's global loads are in flight in registers while this stage's MFMAs run.
#include "upconv_fold.hpp"

namespace {

constexpr int DG_FLUSH = 4;                                // chunks per accumulation chain: 4 x 16 channels x 16 (parity, tap) pairs = 1024 products
constexpr int DG_WIT = 8 * 3 * 64 / UP_THREADS;            // A-fragment uint4 per thread and stage

// ---- weight pack: Wpt[ct][kc][pt][piece][lane] (uint4 = 8 bf16): pt = 8 py + 4 px + 2 dy + dx; row (input channel) ct * 32 + (lane & 31),
// zeros past Cin; reduction channels (of Cout) 16 kc + 8 (lane >> 5) .. + 7; piece = h, m, l of the folded weight (f64 sum rounded to f32).
__global__ __launch_bounds__(256) void upconv_dgrad_pack_kernel(const float *__restrict__ W, uint4 *__restrict__ Wpt, int Cin, int KC, long long total)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;        // ((ct * KC + kc) * 16 + pt) * 64 + lane; total is a multiple of 64
    if (t >= total) return;
    const PackIdx ix = pack_index(t, KC);
    const int lane = ix.lane;
    const FoldRect rect = fold_rect(ix.pt);
    const int c = ix.ct * 32 + (lane & 31), hh = lane >> 5;         // (the forward's pack with the two channel roles exchanged)
    float wf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int o = ix.kc * UP_KC + 8 * hh + e;
        wf[e] = c < Cin ? fold_sum(W + ((long long)o * Cin + c) * 9, rect, [](float) {}) : 0.f;
    }
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) split3_pair_w(wf[2 * p], wf[2 * p + 1], h[p], m[p], l[p]);
    uint4 *dst = Wpt + (ix.r * 3) * 64 + lane;
    dst[0] = make_uint4(h[0], h[1], h[2], h[3]);
    dst[64] = make_uint4(m[0], m[1], m[2], m[3]);
    dst[128] = make_uint4(l[0], l[1], l[2], l[3]);
}

struct DgArgs {
    const float *g;                       // [B][Cout][2H][2W]
    const uint4 *Wpt;                     // the pack above
    float *dx;                            // [B][Cin][H][W]
    int Cin, Cout, H, W, KC, CT, ncols;
};

struct DgLds {
    uint4 wsm[8][3][64];                  // [px, dy, dx][piece][lane] of the stage's py
    uint4 gs[2][3][2][UP_NSLOT + 1];      // [px][piece][K half][staged column], the last slot holds zeros
    unsigned mask;
};
constexpr int DG_LDS = (int)sizeof(DgLds);
static_assert(2 * DG_LDS <= 160 * 1024, "two workgroups per CU");

__global__ __launch_bounds__(UP_THREADS, 2) void upconv3x3_dgrad_kernel(const DgArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dg_lds_raw[];
    DgLds &lds = *reinterpret_cast<DgLds *>(dg_lds_raw);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ct = blockIdx.x % a.CT, cb = blockIdx.x / a.CT;
    const int H = a.H, W = a.W, HW = H * W, Cin = a.Cin, KC = a.KC;
    const int NS = UP_TP + 2 * W + 2;
    const int c0 = cb * UP_TP;

    // this lane's column and the LDS slots of its nine shifted neighbours, k = (sy + 1) * 3 + (sx + 1) (the same text as upconv.hip, kept
    // apart on purpose: docs/findings.md)
    const int c = c0 + wave * 32 + j;
    const bool colvalid = c < a.ncols;
    const int cc = colvalid ? c : 0;
    const int b = cc / HW, pix = cc - b * HW, pi = pix / W, pj = pix - pi * W;
    int off[9];
    unsigned wmask = 0;                   // shifts for which some column of this WAVE has an in-range neighbour
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int sy = k / 3 - 1, sx = k % 3 - 1;
        const bool ok = colvalid && (unsigned)(pi + sy) < (unsigned)H && (unsigned)(pj + sx) < (unsigned)W;
        off[k] = ok ? wave * 32 + j + (W + 1) + sy * W + sx : UP_ZS;
        if (__ballot(ok) != 0ull) wmask |= 1u << k;
    }
    if (tid == 0) lds.mask = 0u;
    if (tid < 12) (&lds.gs[0][0][0][0])[tid * (UP_NSLOT + 1) + UP_ZS] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    if (lane == 0) atomicOr(&lds.mask, wmask);
    __syncthreads();
    const unsigned gmask = lds.mask;      // ... of the WORKGROUP
    unsigned ptmask = 0;                  // (parity, tap) pairs whose weights are needed: pair pt reads the MIRRORED shift (1 - py - dy, 1 - px - dx)
#pragma unroll
    for (int pt = 0; pt < 16; ++pt) {
        const int k = 8 - pair_shift(pt).k();
        if ((gmask >> k) & 1u) ptmask |= 1u << pt;
    }

    // staging items of this thread: (staged column s, K half hq); gsrc = address of (channel 0, row 2 i, column 2 j) of that column, NULL = zeros
    const float *gsrc[UP_XIT];
    int gs_s[UP_XIT], gs_h[UP_XIT];
    const size_t chs = (size_t)4 * HW;                     // channel stride of g
#pragma unroll
    for (int it = 0; it < UP_XIT; ++it) {
        const int q = it * UP_THREADS + tid;
        const int hq = q >= NS ? 1 : 0, s = q - hq * NS;
        const long long cs = (long long)c0 - (W + 1) + s;
        const bool inb = q < 2 * NS && cs >= 0 && cs < a.ncols;
        gs_s[it] = q < 2 * NS ? s : -1;
        gs_h[it] = hq;
        if (inb) {
            const int bs = (int)(cs / HW), ps = (int)(cs - (long long)bs * HW), is = ps / W, js = ps - is * W;
            gsrc[it] = a.g + (size_t)bs * a.Cout * chs + (size_t)(2 * is) * (2 * W) + 2 * js;
        } else {
            gsrc[it] = nullptr;
        }
    }
    const uint4 *wsrc = a.Wpt + (size_t)ct * KC * 16 * 192 + tid;      // + (kc * 16 + 8 py) * 192 + itw * 256

    float2 gr[UP_XIT][8];
    uint4 wr[DG_WIT];
    auto fetch = [&](int st) {            // stage st = 2 kc + py
        const int kc = st >> 1, py = st & 1;
#pragma unroll
        for (int it = 0; it < UP_XIT; ++it) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ch = kc * UP_KC + 8 * gs_h[it] + e;              // < Cout: Cout is a multiple of 32
                gr[it][e] = gsrc[it] != nullptr ? *reinterpret_cast<const float2 *>(gsrc[it] + (size_t)ch * chs + (size_t)py * (2 * W))
                                                : make_float2(0.f, 0.f);
            }
        }
#pragma unroll
        for (int itw = 0; itw < DG_WIT; ++itw) {
            const int pt = 8 * py + (itw * UP_THREADS + tid) / 192;
            wr[itw] = ((ptmask >> pt) & 1u) ? wsrc[((size_t)kc * 16 + 8 * py) * 192 + itw * UP_THREADS] : make_uint4(0u, 0u, 0u, 0u);
        }
    };

    f32x16 acc, tot;
    zero_acc(acc);
    zero_acc(tot);

    const int NST = 2 * KC;
    fetch(0);
    for (int st = 0; st < NST; ++st) {
        const int py = st & 1;
        __syncthreads();                                    // the previous stage's fragment reads are done
#pragma unroll
        for (int it = 0; it < UP_XIT; ++it) {
            if (gs_s[it] >= 0) {
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    unsigned hv[4], mv[4], lv[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float v0 = px == 0 ? gr[it][2 * p].x : gr[it][2 * p].y, v1 = px == 0 ? gr[it][2 * p + 1].x : gr[it][2 * p + 1].y;
                        split3_pair(v0, v1, hv[p], mv[p], lv[p]);
                    }
                    lds.gs[px][0][gs_h[it]][gs_s[it]] = make_uint4(hv[0], hv[1], hv[2], hv[3]);
                    lds.gs[px][1][gs_h[it]][gs_s[it]] = make_uint4(mv[0], mv[1], mv[2], mv[3]);
                    lds.gs[px][2][gs_h[it]][gs_s[it]] = make_uint4(lv[0], lv[1], lv[2], lv[3]);
                }
            }
        }
#pragma unroll
        for (int itw = 0; itw < DG_WIT; ++itw) {
            const int q = itw * UP_THREADS + tid;
            if ((ptmask >> (8 * py + q / 192)) & 1u) (&lds.wsm[0][0][0])[q] = wr[itw];
        }
        __syncthreads();
        if (st + 1 < NST) fetch(st + 1);

#pragma unroll
        for (int ptl = 0; ptl < 8; ++ptl) {
            const int px = ptl >> 2, dy = (ptl >> 1) & 1, dx = ptl & 1;
            const int ky = 2 - py - dy, kx = 2 - px - dx;                  // shift + 1; ky depends on the stage's py: 2 - dy or 1 - dy
            // (off[] must be indexed by a compile-time constant: both values of py are written out)
            const int k0 = (2 - dy) * 3 + kx, k1 = (1 - dy) * 3 + kx;
            const int k = ky * 3 + kx;
            if ((wmask >> k) & 1u) {
                const int o = py == 0 ? off[k0] : off[k1];
                const bf16x8 Bh = __builtin_bit_cast(bf16x8, lds.gs[px][0][h][o]);
                const bf16x8 Bm = __builtin_bit_cast(bf16x8, lds.gs[px][1][h][o]);
                const bf16x8 Bl = __builtin_bit_cast(bf16x8, lds.gs[px][2][h][o]);
                const bf16x8 Ah = __builtin_bit_cast(bf16x8, lds.wsm[ptl][0][lane]);
                const bf16x8 Am = __builtin_bit_cast(bf16x8, lds.wsm[ptl][1][lane]);
                const bf16x8 Al = __builtin_bit_cast(bf16x8, lds.wsm[ptl][2][lane]);
                x3_chain(acc, Ah, Am, Al, Bh, Bm, Bl);
            }
        }
        if (py == 1 && (((st >> 1) % DG_FLUSH) == DG_FLUSH - 1 || st == NST - 1)) flush_chain(tot, acc);
    }

    // epilogue: rows (r, h) of the Cin block that exist, this lane's column
    if (colvalid) {
        float *xb = a.dx + ((size_t)b * Cin + (size_t)ct * 32) * HW + pix;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, h);
            if (ct * 32 + row < Cin) xb[(size_t)row * HW] = tot[r];
        }
    }
}

}  // namespace

extern "C" size_t sonet_upconv3x3_dgrad_pack_size(int Cin, int Cout)
{
    if (!shape_ok(Cin, Cout, 1, 1)) return 0;
    return (size_t)sonet::ceil_div(Cin, 32) * (size_t)(Cout / UP_KC) * 16 * 3072;
}

extern "C" int sonet_upconv3x3_dgrad_pack_f32(const float *W, void *Wpt, int Cin, int Cout, sonet_stream_t stream)
{
    const char *what = "sonet_upconv3x3_dgrad_pack_f32";
    const int KC = Cout / UP_KC;
    const long long total = (long long)sonet::ceil_div(Cin, 32) * KC * 16 * 64;
    const bool aligned = (reinterpret_cast<uintptr_t>(Wpt) & 15) == 0 && (reinterpret_cast<uintptr_t>(W) & 3) == 0;
    if (const int rc = up_pack_check(what, W && Wpt, aligned, Cin, Cout, total)) return rc;
    hipLaunchKernelGGL(upconv_dgrad_pack_kernel, dim3((unsigned)sonet::ceil_div64(total, 256)), dim3(256), 0, sonet::as_stream(stream),
                       W, reinterpret_cast<uint4 *>(Wpt), Cin, KC, total);
    return sonet::launched(what);
}

extern "C" int sonet_upconv3x3_dgrad_f32(const float *g, const void *Wpt, float *dx, int B, int Cin, int Cout, int H, int W, sonet_stream_t stream)
{
    const char *what = "sonet_upconv3x3_dgrad_f32";
    const bool aligned = (reinterpret_cast<uintptr_t>(Wpt) & 15) == 0 && (reinterpret_cast<uintptr_t>(g) & 7) == 0 && (reinterpret_cast<uintptr_t>(dx) & 3) == 0;
    if (const int rc = up_check(what, g && Wpt && dx, aligned, B, Cin, Cout, H, W)) return rc;
    const int CT = sonet::ceil_div(Cin, 32), KC = Cout / UP_KC;
    unsigned nblk;
    DgArgs a;
    if (const int rc = up_grid(what, B, H, W, CT, a.ncols, nblk)) return rc;
    a.g = g;
    a.Wpt = reinterpret_cast<const uint4 *>(Wpt);
    a.dx = dx;
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.KC = KC; a.CT = CT;
    const int rc = sonet::launch_lds_once<upconv3x3_dgrad_kernel, DG_LDS>(what, dim3(nblk), dim3(UP_THREADS), DG_LDS,
                                                                          sonet::as_stream(stream), a);
    if (rc != SONET_OK) return rc;
    return sonet::launched(what);
}
