// upconv.hip -- the decoder's up-convolution as ONE launch per layer (inference):
//   y = act(conv3x3_pad1(upsample2_nearest(x), w) * scale + shift)          (UpConv, models/layers.py:214-240; DecoderConv, models/networks.py:393-431)
//
// Folded form.  A nearest x2 upsample followed by a 3x3 conv (pad 1) is four 2x2 convs on the LOW-resolution map, one per output parity:
// output pixel (2i + py, 2j + px) reads the low-resolution pixels (i - 1 + py + dy, j - 1 + px + dx), dy, dx in {0, 1}, zeros outside
// [0, H) x [0, W), with the weights
//       py = 0:  tap 0 = w[ky=0],            tap 1 = w[ky=1] + w[ky=2]
//       py = 1:  tap 0 = w[ky=0] + w[ky=1],  tap 1 = w[ky=2]                  (the same table in x)
// -- 4/9 of the multiplies, and the upsampled tensor is never written.  A (parity, tap) pair reads the map shifted by
// (sy, sx) = (py + dy - 1, px + dx - 1) in {-1, 0, 1}^2: nine shifted operands feed the sixteen (parity, tap) products.
//
// Arithmetic: the three-term fp16 split of the third-generation point-wise layer (pointmlp_h3p.hip),
//   1024 w x ~= fp16(32 w - Wh) . Xh + Wh . Xm + Wh . Xh,   Wh = fp16(32 w), Xh = fp16(32 x), Xm = fp16(32 x - Xh),
// on v_mfma_f32_32x32x16_f16, smallest term first, f32 accumulation; the factor 1024 leaves through scale / 1024.  The weights are folded
// in float64, rounded to f32 and split by the pack kernel; the activations are clamped to +-2047 and split when they are staged.
// The reduction runs over 4 taps x Cin: every UP_FLUSH chunks (1024 products per parity) the running accumulators are added to a second
// set and restart from zero, so that no f32 chain is longer than that whatever Cin is.
//
// Tiling: the columns of the four GEMMs are the low-resolution pixels of the whole batch on ONE flat axis, c = (b H + i) W + j.  A
// workgroup (4 waves) owns UP_TP = 128 consecutive columns x one 32-row block of Cout x all four parities (4 x 16 accumulator
// registers per lane); a wave owns 32 columns.  Per 16-channel chunk the workgroup stages
//   * the columns c0 - W - 1 .. c0 + 127 + W + 1 of the chunk (the tile and its one-pixel halo on the flat axis) as split fp16 pieces
//     in MFMA B-fragment order; a neighbour that lies in the padding (or past the batch) is read from a slot of zeros -- the nine
//     LDS offsets of a lane are fixed before the loop, so borders cost nothing inside it;
//   * the sixteen (parity, tap) A fragments of its Cout block (2 KiB each) -- except those whose shifted operand lies in the padding for
//     EVERY column of the tile, which are neither read nor multiplied (at 1 x 1: twelve of sixteen).
// The next chunk's global loads are in flight in registers while this chunk's MFMAs run.
#include "upconv_fold.hpp"               // the family's building blocks: shared with upconv_bwd.hip and upconv_wgrad.hip

namespace {

// ---- weight pack: Wp[ct][kc][pt][form][lane] (uint4 = 8 fp16): pt = (py, px, dy, dx) as 8 py + 4 px + 2 dy + dx; row ct * 32 + (lane & 31),
// channels 16 kc + 8 (lane >> 5) .. + 7 (zeros past Cin); form 0 = fp16(32 wf), form 1 = fp16(32 wf - form 0) of the folded weight wf (f64 sum
// rounded to f32).  64-byte trailer: word 0 = bits of the largest magnitude among the weights and their folded sums.
__global__ __launch_bounds__(256) void upconv_pack_kernel(const float *__restrict__ W, uint4 *__restrict__ Wp, int Cin, int KC, long long total,
                                                           unsigned *__restrict__ trailer)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;        // ((ct * KC + kc) * 16 + pt) * 64 + lane; total is a multiple of 64
    if (t >= total) return;
    RangeAcc wr = {0, 0u};
    const PackIdx ix = pack_index(t, KC);
    const int lane = ix.lane;
    const FoldRect rect = fold_rect(ix.pt);
    const int o = ix.ct * UP_CB + (lane & 31), hh = lane >> 5;
    float wf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ix.kc * UP_KC + 8 * hh + e;
        wf[e] = c < Cin ? fold_sum(W + ((long long)o * Cin + c) * 9, rect, [&](float v) { range_track(wr, v, v); }) : 0.f;
    }
    unsigned h[4], m[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        range_track(wr, wf[2 * p], wf[2 * p + 1]);
        p16_split_pair(wf[2 * p], wf[2 * p + 1], h[p], m[p]);
    }
    uint4 *dst = Wp + (ix.r * 2) * 64 + lane;
    dst[0] = make_uint4(h[0], h[1], h[2], h[3]);
    dst[64] = make_uint4(m[0], m[1], m[2], m[3]);
    range_publish(trailer, wave_umax(range_amax_bits(wr)), lane);
}

struct UpArgs {
    const float *x;                       // [B][Cin][H][W]
    const uint4 *Wp;                      // the pack above
    const float *scale, *shift;           // [Cout]
    float *y;                             // [B][Cout][2H][2W]
    unsigned *rlog;                       // range-log slot or NULL (word 0: max |x| bits, word 1: max |w| bits)
    const unsigned *trailer;
    int Cin, Cout, H, W, KC, CT, relu, ncols;
};

__global__ __launch_bounds__(UP_THREADS, 2) void upconv3x3_kernel(const UpArgs a)
{
    struct Lds {
        uint4 wsm[16][2][64];             // [pt][form][lane]
        uint4 xs[2][2][UP_NSLOT + 1];     // [form][K half][staged column], the last slot holds zeros
        unsigned mask;
    };
    __shared__ __attribute__((aligned(16))) Lds lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ct = blockIdx.x % a.CT, cb = blockIdx.x / a.CT;
    const int H = a.H, W = a.W, HW = H * W, Cin = a.Cin, KC = a.KC;
    const int NS = UP_TP + 2 * W + 2;
    const int c0 = cb * UP_TP;

    // this lane's column and the LDS slots of its nine shifted neighbours (the same text as upconv_bwd.hip, kept apart on purpose:
    // docs/findings.md)
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
    if (tid < 4) lds.xs[tid >> 1][tid & 1][UP_ZS] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    if (lane == 0) atomicOr(&lds.mask, wmask);
    __syncthreads();
    const unsigned gmask = lds.mask;      // ... of the WORKGROUP
    unsigned ptmask = 0;                  // (parity, tap) pairs whose weights are needed
#pragma unroll
    for (int pt = 0; pt < 16; ++pt) {
        const int k = pair_shift(pt).k();
        if ((gmask >> k) & 1u) ptmask |= 1u << pt;
    }

    // staging items of this thread: (staged column s, K half hq); xsrc = address of channel 0 of that column, NULL = zeros
    const float *xsrc[UP_XIT];
    int xs_s[UP_XIT], xs_h[UP_XIT];
#pragma unroll
    for (int it = 0; it < UP_XIT; ++it) {
        const int q = it * UP_THREADS + tid;
        const int hq = q >= NS ? 1 : 0, s = q - hq * NS;
        const long long cs = (long long)c0 - (W + 1) + s;
        const bool inb = q < 2 * NS && cs >= 0 && cs < a.ncols;
        xs_s[it] = q < 2 * NS ? s : -1;
        xs_h[it] = hq;
        if (inb) {
            const int bs = (int)(cs / HW), ps = (int)(cs - (long long)bs * HW);
            xsrc[it] = a.x + (size_t)bs * Cin * HW + ps;
        } else {
            xsrc[it] = nullptr;
        }
    }
    const uint4 *wsrc = a.Wp + (size_t)ct * KC * 16 * 128 + tid;       // + (kc * 16 + pt) * 128, pt = 2 itw + (tid >> 7)

    float xr[UP_XIT][8];
    uint4 wr[8];
    auto fetch = [&](int kc) {
#pragma unroll
        for (int it = 0; it < UP_XIT; ++it) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ch = kc * UP_KC + 8 * xs_h[it] + e;
                xr[it][e] = (xsrc[it] != nullptr && ch < Cin) ? xsrc[it][(size_t)ch * HW] : 0.f;
            }
        }
#pragma unroll
        for (int itw = 0; itw < 8; ++itw) {
            const int pt = 2 * itw + (tid >> 7);
            wr[itw] = ((ptmask >> pt) & 1u) ? wsrc[((size_t)kc * 16 + 2 * itw) * 128] : make_uint4(0u, 0u, 0u, 0u);
        }
    };

    f32x16 acc[4], tot[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) { zero_acc(acc[p]); zero_acc(tot[p]); }
    RangeAcc xrng = {0, 0u};

    fetch(0);
    for (int kc = 0; kc < KC; ++kc) {
        __syncthreads();                                    // the previous chunk's fragment reads are done
#pragma unroll
        for (int it = 0; it < UP_XIT; ++it) {
            if (xs_s[it] >= 0) {
                unsigned hv[4], mv[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    range_track(xrng, xr[it][2 * p], xr[it][2 * p + 1]);
                    p16_split_pair(xr[it][2 * p], xr[it][2 * p + 1], hv[p], mv[p]);
                }
                lds.xs[0][xs_h[it]][xs_s[it]] = make_uint4(hv[0], hv[1], hv[2], hv[3]);
                lds.xs[1][xs_h[it]][xs_s[it]] = make_uint4(mv[0], mv[1], mv[2], mv[3]);
            }
        }
#pragma unroll
        for (int itw = 0; itw < 8; ++itw) {
            const int pt = 2 * itw + (tid >> 7);
            if ((ptmask >> pt) & 1u) (&lds.wsm[0][0][0])[itw * UP_THREADS + tid] = wr[itw];
        }
        __syncthreads();
        if (kc + 1 < KC) fetch(kc + 1);

#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if ((wmask >> k) & 1u) {
                const int sy = k / 3, sx = k % 3;                                  // = py + dy, px + dx
                const f16x8 bh = __builtin_bit_cast(f16x8, lds.xs[0][h][off[k]]);
                const f16x8 bm = __builtin_bit_cast(f16x8, lds.xs[1][h][off[k]]);
#pragma unroll
                for (int py = 0; py < 2; ++py) {
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        const int dy = sy - py, dx = sx - px;
                        if (dy < 0 || dy > 1 || dx < 0 || dx > 1) continue;
                        const int p = py * 2 + px, pt = p * 4 + dy * 2 + dx;
                        const f16x8 wh = __builtin_bit_cast(f16x8, lds.wsm[pt][0][lane]);
                        const f16x8 wm = __builtin_bit_cast(f16x8, lds.wsm[pt][1][lane]);
                        acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wm, bh, acc[p], 0, 0, 0);
                        acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bm, acc[p], 0, 0, 0);
                        acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bh, acc[p], 0, 0, 0);
                    }
                }
            }
        }
        if ((kc % UP_FLUSH) == UP_FLUSH - 1 || kc == KC - 1) {
#pragma unroll
            for (int p = 0; p < 4; ++p) flush_chain(tot[p], acc[p]);
        }
    }

    // operand ranges: the activations this workgroup staged (the halo columns are some other workgroup's tile as well), the pack's weights
    if (a.rlog != nullptr) {
        range_publish(a.rlog, wave_umax(range_amax_bits(xrng)), lane);
        if (blockIdx.x == 0 && tid == 0) {
            const unsigned wb = a.trailer[0];
            if (wb > __atomic_load_n(a.rlog + 1, __ATOMIC_RELAXED)) atomicMax(a.rlog + 1, wb);
        }
    }

    // epilogue: rows (r, h) of the Cout block, the column's 2 x 2 output pixels; the two px of a row leave as one 8-byte store
    if (colvalid) {
        const int H2 = 2 * H, W2 = 2 * W;
        float *yb = a.y + ((size_t)b * a.Cout + (size_t)ct * UP_CB) * H2 * W2 + (size_t)(2 * pi) * W2 + 2 * pj;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, h);
            const float sc = a.scale[ct * UP_CB + row] * (1.f / 1024.f), sf = a.shift[ct * UP_CB + row];
            float *yr = yb + (size_t)row * H2 * W2;
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                float v0 = __fmaf_rn(tot[py * 2 + 0][r], sc, sf), v1 = __fmaf_rn(tot[py * 2 + 1][r], sc, sf);
                if (a.relu) {                                                      // (a NaN stays a NaN, as torch's relu)
                    v0 = v0 < 0.f ? 0.f : v0;
                    v1 = v1 < 0.f ? 0.f : v1;
                }
                *reinterpret_cast<float2 *>(yr + (size_t)py * W2) = make_float2(v0, v1);
            }
        }
    }
}

}  // namespace

extern "C" size_t sonet_upconv3x3_pack_size(int Cin, int Cout)
{
    if (!shape_ok(Cin, Cout, 1, 1)) return 0;
    return (size_t)(Cout / UP_CB) * (size_t)sonet::ceil_div(Cin, UP_KC) * 16 * 2048 + 64;
}

extern "C" int sonet_upconv3x3_pack_f32(const float *W, void *Wp, int Cin, int Cout, sonet_stream_t stream)
{
    const char *what = "sonet_upconv3x3_pack_f32";
    const int KC = sonet::ceil_div(Cin, UP_KC);
    const long long total = (long long)(Cout / UP_CB) * KC * 16 * 64;
    if (const int rc = up_pack_check(what, W && Wp, /*aligned: not checked here*/ true, Cin, Cout, total)) return rc;
    unsigned *trailer = reinterpret_cast<unsigned *>(reinterpret_cast<uint4 *>(Wp) + total * 2);
    if (sonet::zero_words(trailer, 64, sonet::as_stream(stream)) != 0) return sonet::fail(SONET_ERR_LAUNCH, "%s: clearing the trailer failed", what);
    hipLaunchKernelGGL(upconv_pack_kernel, dim3((unsigned)sonet::ceil_div64(total, 256)), dim3(256), 0, sonet::as_stream(stream),
                       W, reinterpret_cast<uint4 *>(Wp), Cin, KC, total, trailer);
    return sonet::launched(what);
}

extern "C" int sonet_upconv3x3_f32(const float *x, const void *Wp, const float *scale, const float *shift, int relu, float *y,
                                   int B, int Cin, int Cout, int H, int W, uint32_t *range_log, sonet_stream_t stream)
{
    const char *what = "sonet_upconv3x3_f32";
    const bool aligned = (reinterpret_cast<uintptr_t>(Wp) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 7) == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0;
    if (const int rc = up_check(what, x && Wp && scale && shift && y, aligned, B, Cin, Cout, H, W)) return rc;
    const int CT = Cout / UP_CB, KC = sonet::ceil_div(Cin, UP_KC);
    unsigned nblk;
    UpArgs a;
    if (const int rc = up_grid(what, B, H, W, CT, a.ncols, nblk)) return rc;
    a.x = x;
    a.Wp = reinterpret_cast<const uint4 *>(Wp);
    a.scale = scale;
    a.shift = shift;
    a.y = y;
    a.rlog = range_log;
    a.trailer = reinterpret_cast<const unsigned *>(a.Wp + (size_t)CT * KC * 16 * 128);
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.KC = KC; a.CT = CT; a.relu = relu != 0;
    hipLaunchKernelGGL(upconv3x3_kernel, dim3(nblk), dim3(UP_THREADS), 0, sonet::as_stream(stream), a);
    return sonet::launched(what);
}
