// upconv_wgrad.hip -- the weight gradient of the decoder's up-convolution as TWO small launches per layer (training):
//   y = conv3x3_pad1(upsample2_nearest(x), w),  g = dL/dy [B][Cout][2H][2W],  x [B][Cin][H][W]   ->   dw = dL/dw [Cout][Cin][3][3]
//
// Folded form (upconv.hip): output pixel (2i + py, 2j + px) reads the low-resolution pixels (i - 1 + py + dy, j - 1 + px + dx) with the
// sixteen folded (parity, tap) matrices Wf[py][px][dy][dx] = F(w).  The gradient of a folded matrix is one product over the flat column
// axis c = (b H + i) W + j,
//       dWf[py][px][dy][dx'][o][ci] = sum over c of  g[:, o, py::2, px::2][c] * shifted(x, py + dy - 1, px + dx' - 1)[ci][c]
// (zeros outside [0, H) x [0, W), never another cloud), and the fold is linear, so dw = F^T(dWf): every one of the nine taps is the sum of
// the four folded gradients whose fold range (fold_range) holds its ky and its kx.  Sixteen products over B H W columns instead of
// thirty-six over 4 B H W -- 1/9 of the multiplies --, and neither upsample(x) nor a shifted copy of x is written to memory.
//
// Arithmetic: the three-way bf16 split of BOTH operands (split3_pair), six products on v_mfma_f32_32x32x16_bf16, smallest first, f32
// accumulation: every UW_FLUSH steps (256 products per element: a quarter of the chain the two neighbours allow) the accumulators are added
// to a second set and restart from zero.  No range log: gradients range over f32's exponents.  No atomics.
//
// Decomposition (the model is wgrad_x3.hip: a small output, a long reduction): a workgroup (4 waves) owns 32 output channels x 32 input
// channels x ALL sixteen (parity, tap) pairs over one slice of the column axis; wave w owns the parity (py, px) = (w >> 1, w & 1), i.e. four
// accumulators.  Per step of 16 columns (a lane: one row, 8 consecutive columns):
//   * wave (py, q) loads, of the g rows of py, the columns 4 q .. 4 q + 3 of every lane's eight -- one load gives both px of a row --,
//     splits each value once and publishes its half of the two A fragments (py, px = 0, 1) in LDS;
//   * wave sy + 1 (sy = -1, 0, 1) loads the TEN consecutive values c - 1 + sy W .. c + 8 + sy W of its x row -- a shift is sy W + sx on
//     the flat axis --, splits them once (30 splits per 8-column group instead of 72) and publishes the three shifts sx = -1, 0, 1 as
//     B fragments in LDS, each element zeroed (a select, not a product) where (i + sy, j + sx) leaves the map: row, map and cloud borders;
//   * after one barrier wave (py, px) multiplies the A fragment of its parity with the four B fragments (sy, sx) = (py + dy - 1,
//     px + dx' - 1).
// With W % 4 == 0 and 16-byte aligned operands (deconv3 .. deconv6) the four columns of g are two 16-byte loads and the ten values of x
// two 16-byte loads and two single ones; otherwise element by element -- the same values in the same order, the same bits.
// The LDS fragments are double buffered (one barrier per step, 78 KB of dynamic LDS: two workgroups per CU); the next step's global loads
// are in flight while the MFMAs run.  A
// (parity, tap) pair whose shifted operand is padding for EVERY column (H = 1 or W = 1) is not multiplied: four of sixteen at 1 x 1.
// Columns past B H W, rows past Cin and halo elements before the first / after the last cloud are zeros chosen WITHOUT a load: every
// address formed lies inside g, x or the workspace.
//
// The partial blocks go to ws[slice][pt][Cout][Cpad] (Cpad = Cin rounded up to 32; every element is written, zeros included); the second
// kernel sums the slices in order in float64, applies the four-term F^T sum, rounds once and writes all of dw.  The slice count is a
// function of the shape alone (uw_plan): no device query, the same bits on every part.
#include "upconv_fold.hpp"

namespace {

constexpr int UW_KSTEP = SONET_UPWGRAD_K_STEP;                         // columns per MFMA step
constexpr int UW_FLUSH = SONET_UPWGRAD_FLUSH_COLS / UW_KSTEP;          // steps per accumulation chain
constexpr int UW_SLICE = SONET_UPWGRAD_SLICE_COLS;                     // columns a slice has at least (but for the last)
constexpr int UW_MAXSL = SONET_UPWGRAD_MAX_SLICES;
constexpr int UW_CB = SONET_UPWGRAD_CIN_BLOCK;                         // input channels per workgroup
constexpr size_t UW_WS_CAP = (size_t)64 << 20;                              // more slices than fit in this are not taken
static_assert(UW_KSTEP == 16 && UW_CB == 32 && UW_FLUSH * UW_KSTEP <= 1024, "the kernel is written for these extents");

// pair_shift(8 py + 4 px + q).k() from the wave's (py, px) and q = 2 dy + dx.  (Through pt the kernel's code changes: the MFMA loop keeps
// this form, and the assertion holds it to the header's.)
__host__ __device__ constexpr int uw_shift_k(int py, int px, int q) { return (py + (q >> 1)) * 3 + px + (q & 1); }
constexpr bool uw_shift_k_ok() {
    for (int pt = 0; pt < 16; ++pt)
        if (uw_shift_k(pt >> 3, (pt >> 2) & 1, pt & 3) != pair_shift(pt).k()) return false;
    return true;
}
static_assert(uw_shift_k_ok(), "the weight gradient's shift index is pair_shift's");

struct UwPlan { int OB, CT, nstep, sps, nslice; long long ncols; size_t ws_bytes; };

// slices: one per UW_SLICE columns, at most UW_MAXSL and at most what UW_WS_CAP holds; whole steps per slice, no empty slice
bool uw_plan(int B, int Cin, int Cout, int H, int W, UwPlan &p) {
    if (B < 1 || !shape_ok(Cin, Cout, H, W)) return false;
    p.ncols = (long long)B * H * W;
    if (p.ncols > 0x7FFF0000ll) return false;
    p.OB = Cout / UP_CB;
    p.CT = sonet::ceil_div(Cin, UW_CB);
    p.nstep = (int)sonet::ceil_div64(p.ncols, UW_KSTEP);
    const size_t per = (size_t)16 * Cout * ((size_t)p.CT * UW_CB) * sizeof(float);
    long long want = sonet::ceil_div64(p.ncols, UW_SLICE);
    if (want > UW_MAXSL) want = UW_MAXSL;
    const long long cap = (long long)(UW_WS_CAP / per);
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    p.sps = (int)sonet::ceil_div64(p.nstep, want);
    p.nslice = sonet::ceil_div(p.nstep, p.sps);
    p.ws_bytes = (size_t)p.nslice * per;
    return true;
}

struct UwArgs {
    const float *g;                       // [B][Cout][2H][2W]
    const float *x;                       // [B][Cin][H][W]
    float *part;                          // [nslice][16][Cout][CT * 32]
    int Cin, Cout, H, W, CT, OB, ncols, sps, nstep;
    unsigned pairmask;                    // (parity, tap) pairs with an in-range shifted element somewhere: pt = 8 py + 4 px + 2 dy + dx
};

struct UwLds {
    uint4 xs[2][9][3][64];                // [buffer][(sy + 1) * 3 + sx + 1][piece][lane]: B fragments, 2 x 27 KiB
    uint4 ga[2][4][3][64];                // [buffer][2 py + px][piece][lane]: A fragments, 2 x 12 KiB
};
constexpr int UW_LDS = (int)sizeof(UwLds);
static_assert(2 * UW_LDS <= 160 * 1024, "two workgroups per CU");

// VEC: W % 4 == 0 and g, x 16-byte aligned -- a lane's four columns of g (both px) are two 16-byte loads, its ten values of x two
// 16-byte loads and two single ones.  Otherwise element by element.  The same values in the same order: the same bits.
template <bool VEC>
__global__ __launch_bounds__(UP_THREADS, 2) void upconv3x3_wgrad_kernel(const UwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char uw_lds_raw[];
    UwLds &lds = *reinterpret_cast<UwLds *>(uw_lds_raw);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int py = wave >> 1, px = wave & 1;                       // the parity whose four products this wave accumulates
    const int gq = wave & 1;              // ... and, of the g rows of py, the half (columns 4 gq .. 4 gq + 3 of a lane's eight) it stages
    const int sy = wave - 1;              // waves 0..2 stage the x row of this shift; wave 3 stages none
    const int H = a.H, W = a.W, HW = H * W, Cin = a.Cin, Cout = a.Cout, ncols = a.ncols;
    const int ct = blockIdx.x % a.CT, rest = blockIdx.x / a.CT;
    const int ob = rest % a.OB, sl = rest / a.OB;
    const int st0 = sl * a.sps, st1 = min(a.nstep, st0 + a.sps);
    const int o = ob * UP_CB + i;                                  // < Cout: Cout is a multiple of 32
    const int c = ct * UW_CB + i;
    const bool c_ok = c < Cin;
    const size_t gcs = (size_t)4 * HW;                             // channel stride of g
    const float *grow = a.g + (size_t)o * gcs + (size_t)py * (2 * W);          // + b Cout gcs + 2 i 2 W + 2 j
    const float *xrow = a.x + (size_t)(c_ok ? c : 0) * HW;                      // + b Cin HW + pixel

    float gv[8];                          // [column 0..3][px]
    float xv[10];
    unsigned mk[3];                       // per sx: bit e = the shifted element of column e is inside the map
    auto load = [&](int st) {
        const int d0 = st * UW_KSTEP + 8 * h;                      // this lane's eight columns d0 .. d0 + 7
        const int b = (int)((unsigned)d0 / (unsigned)HW), pix = d0 - b * HW;
        const int ii = (int)((unsigned)pix / (unsigned)W), jj = pix - ii * W;
        {   // g: columns d0 + 4 gq + (0 .. 3), both px of each
            int gb = b, gi = ii, gj = jj;
            if (VEC) {                                             // jj and W are multiples of 4: the four columns share a row
                if (gq) { gj += 4; if (gj == W) { gj = 0; if (++gi == H) { gi = 0; ++gb; } } }
                if (d0 + 4 * gq < ncols) {                         // (ncols is a multiple of 4: all four or none)
                    const float4 *p = reinterpret_cast<const float4 *>(grow + (size_t)gb * Cout * gcs + (size_t)(2 * gi) * (2 * W) + 2 * gj);
                    const float4 t0 = p[0], t1 = p[1];
                    gv[0] = t0.x; gv[1] = t0.y; gv[2] = t0.z; gv[3] = t0.w; gv[4] = t1.x; gv[5] = t1.y; gv[6] = t1.z; gv[7] = t1.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) gv[e] = 0.f;
                }
            } else {
                for (int s = 0; s < 4 * gq; ++s)
                    if (++gj == W) { gj = 0; if (++gi == H) { gi = 0; ++gb; } }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float2 t = make_float2(0.f, 0.f);
                    if (d0 + 4 * gq + e < ncols)
                        t = *reinterpret_cast<const float2 *>(grow + (size_t)gb * Cout * gcs + (size_t)(2 * gi) * (2 * W) + 2 * gj);
                    gv[2 * e] = t.x; gv[2 * e + 1] = t.y;
                    if (++gj == W) { gj = 0; if (++gi == H) { gi = 0; ++gb; } }
                }
            }
        }
        if (wave < 3) {
            int mi = ii, mj = jj;
            mk[0] = mk[1] = mk[2] = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool rowok = d0 + e < ncols && (unsigned)(mi + sy) < (unsigned)H;
                if (rowok && mj >= 1) mk[0] |= 1u << e;
                if (rowok) mk[1] |= 1u << e;
                if (rowok && mj + 1 < W) mk[2] |= 1u << e;
                if (++mj == W) { mj = 0; if (++mi == H) mi = 0; }
            }
            if (VEC) {
                const int fa = d0 + sy * W;                        // a multiple of 4, like HW and ncols: a group of four is in one cloud, or outside
#pragma unroll
                for (int grp = 0; grp < 2; ++grp) {
                    const int f = fa + 4 * grp;
                    const bool inb = c_ok && f >= 0 && f < ncols;
                    const unsigned fb = inb ? (unsigned)f : 0u;
                    const unsigned bb = fb / (unsigned)HW, pp = fb - bb * (unsigned)HW;
                    const float *p = xrow + (size_t)bb * Cin * HW + pp;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (inb) v = *reinterpret_cast<const float4 *>(p);
                    xv[1 + 4 * grp] = v.x; xv[2 + 4 * grp] = v.y; xv[3 + 4 * grp] = v.z; xv[4 + 4 * grp] = v.w;
                    // the value before / after the eight is read by sx = -1 / +1 only from the same row of the same cloud
                    if (grp == 0) xv[0] = (inb && pp > 0u) ? p[-1] : 0.f;
                    else xv[9] = (inb && pp + 4u < (unsigned)HW) ? p[4] : 0.f;
                }
            } else {
                const int f0 = d0 + sy * W - 1;                    // flat column of the first of the ten values (may be -W - 1 .. -1)
                int bb = 0, pp = 0;
                if (f0 > 0) { bb = (int)((unsigned)f0 / (unsigned)HW); pp = f0 - bb * HW; }
#pragma unroll
                for (int t = 0; t < 10; ++t) {
                    const int f = f0 + t;
                    xv[t] = (c_ok && f >= 0 && f < ncols) ? xrow[(size_t)bb * Cin * HW + pp] : 0.f;
                    if (f >= 0 && ++pp == HW) { pp = 0; ++bb; }
                }
            }
        }
    };

    f32x16 acc[4], tot[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { zero_acc(acc[q]); zero_acc(tot[q]); }

    int buf = 0, chain = 0;
    load(st0);
    for (int st = st0; st < st1; ++st) {
        // split what the previous iteration requested, each element once: g -> half of two A fragments, x -> three B fragments, in LDS
#pragma unroll
        for (int pxx = 0; pxx < 2; ++pxx) {
            unsigned h0, m0, l0, h1, m1, l1;
            split3_pair(gv[pxx], gv[2 + pxx], h0, m0, l0);
            split3_pair(gv[4 + pxx], gv[6 + pxx], h1, m1, l1);
            reinterpret_cast<uint2 *>(&lds.ga[buf][2 * py + pxx][0][lane])[gq] = make_uint2(h0, h1);
            reinterpret_cast<uint2 *>(&lds.ga[buf][2 * py + pxx][1][lane])[gq] = make_uint2(m0, m1);
            reinterpret_cast<uint2 *>(&lds.ga[buf][2 * py + pxx][2][lane])[gq] = make_uint2(l0, l1);
        }
        if (wave < 3) {
            unsigned pc[3][5];
#pragma unroll
            for (int q = 0; q < 5; ++q) split3_pair(xv[2 * q], xv[2 * q + 1], pc[0][q], pc[1][q], pc[2][q]);
#pragma unroll
            for (int sxi = 0; sxi < 3; ++sxi) {                    // sx = sxi - 1: column e takes value e + sx + 1 of the ten
                unsigned km[4];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    km[p] = (((mk[sxi] >> (2 * p)) & 1u) ? 0x0000FFFFu : 0u) | (((mk[sxi] >> (2 * p + 1)) & 1u) ? 0xFFFF0000u : 0u);
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    unsigned f[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const unsigned v = sxi == 0 ? pc[t][p] : sxi == 2 ? pc[t][p + 1] : ((pc[t][p] >> 16) | (pc[t][p + 1] << 16));
                        f[p] = v & km[p];
                    }
                    lds.xs[buf][(sy + 1) * 3 + sxi][t][lane] = make_uint4(f[0], f[1], f[2], f[3]);
                }
            }
        }
        __syncthreads();                                           // (the buffer written two steps ago has been read by every wave)
        if (st + 1 < st1) load(st + 1);

        const bf16x8 Ah = __builtin_bit_cast(bf16x8, lds.ga[buf][2 * py + px][0][lane]);
        const bf16x8 Am = __builtin_bit_cast(bf16x8, lds.ga[buf][2 * py + px][1][lane]);
        const bf16x8 Al = __builtin_bit_cast(bf16x8, lds.ga[buf][2 * py + px][2][lane]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {                              // q = 2 dy + dx
            const int pt = 8 * py + 4 * px + q;
            if ((a.pairmask >> pt) & 1u) {
                const int k = uw_shift_k(py, px, q);
                const bf16x8 Bh = __builtin_bit_cast(bf16x8, lds.xs[buf][k][0][lane]);
                const bf16x8 Bm = __builtin_bit_cast(bf16x8, lds.xs[buf][k][1][lane]);
                const bf16x8 Bl = __builtin_bit_cast(bf16x8, lds.xs[buf][k][2][lane]);
                x3_chain(acc[q], Ah, Am, Al, Bh, Bm, Bl);
            }
        }
        if (++chain == UW_FLUSH || st + 1 == st1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) flush_chain(tot[q], acc[q]);
            chain = 0;
        }
        buf ^= 1;
    }

    // partial blocks: rows (r, h) of the Cout block, this lane's input channel -- every element of the padded block, zeros included
    const size_t Cpad = (size_t)a.CT * UW_CB;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int pt = 8 * py + 4 * px + q;
        float *pp = a.part + (((size_t)sl * 16 + pt) * Cout + (size_t)ob * UP_CB) * Cpad + (size_t)ct * UW_CB + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) pp[(size_t)acc_row(r, h) * Cpad] = tot[q][r];
    }
}

// dw[o][c][ky][kx] = sum of the four dWf whose fold ranges hold ky and kx; dWf = the slices added in order.  Float64, one rounding.
// A workgroup: 16 consecutive (o, c) elements x 16 pairs; thread (e, pt) walks the slices, the first 144 threads unfold.
__global__ __launch_bounds__(256) void upconv3x3_wgrad_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw, int Cin, int Cout,
                                                                      int Cpad, int nslice, long long total /*Cout * Cin*/)
{
    __shared__ double sums[16][17];
    const int e = threadIdx.x & 15, pt = threadIdx.x >> 4;
    const long long t = (long long)blockIdx.x * 16 + e;
    double s = 0.0;
    if (t < total) {
        const int o = (int)(t / Cin), c = (int)(t - (long long)o * Cin);
        const float *p = part + ((size_t)pt * Cout + o) * Cpad + c;
        const size_t stride = (size_t)16 * Cout * Cpad;
#pragma unroll 8
        for (int k = 0; k < nslice; ++k) s += (double)p[(size_t)k * stride];
    }
    sums[e][pt] = s;
    __syncthreads();
    if (threadIdx.x < 144) {
        const int e2 = threadIdx.x / 9, k9 = threadIdx.x - 9 * e2;
        const int ky = k9 / 3, kx = k9 - 3 * ky;
        const long long t2 = (long long)blockIdx.x * 16 + e2;
        if (t2 < total) {
            double d = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {                         // q = 8 py + 4 px + 2 dy + dx, in this order
                if (fold_rect(q).holds(ky, kx)) d += sums[e2][q];
            }
            dw[t2 * 9 + k9] = (float)d;
        }
    }
}

}  // namespace

extern "C" size_t sonet_upconv3x3_wgrad_ws_size(int B, int Cin, int Cout, int H, int W)
{
    UwPlan p;
    return uw_plan(B, Cin, Cout, H, W, p) ? p.ws_bytes : 0;
}

extern "C" int sonet_upconv3x3_wgrad_f32(const float *g, const float *x, float *dw, void *ws, int B, int Cin, int Cout, int H, int W,
                                         sonet_stream_t stream)
{
    const char *what = "sonet_upconv3x3_wgrad_f32";
    const bool aligned = (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && (reinterpret_cast<uintptr_t>(g) & 7) == 0 &&
                         (reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(dw) & 3) == 0;
    if (const int rc = up_check(what, g && x && dw && ws, aligned, B, Cin, Cout, H, W)) return rc;
    UwPlan p;
    if (!uw_plan(B, Cin, Cout, H, W, p)) return up_too_many_columns(what, (long long)B * H * W);
    const long long nblk = (long long)p.nslice * p.OB * p.CT, total = (long long)Cout * Cin;
    if (nblk > 0x7FFFFFFFll || sonet::ceil_div64(total, 16) > 0x7FFFFFFFll)
        return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: %d x %d is too large", what, Cout, Cin);
    UwArgs a;
    a.g = g; a.x = x;
    a.part = reinterpret_cast<float *>(ws);
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.CT = p.CT; a.OB = p.OB; a.ncols = (int)p.ncols; a.sps = p.sps; a.nstep = p.nstep;
    a.pairmask = live_pairs(H, W);
    hipStream_t st = sonet::as_stream(stream);
    const bool vec = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
    const int rc = vec ? sonet::launch_lds_once<&upconv3x3_wgrad_kernel<true>, UW_LDS>(what, dim3((unsigned)nblk), dim3(UP_THREADS), UW_LDS, st, a)
                       : sonet::launch_lds_once<&upconv3x3_wgrad_kernel<false>, UW_LDS>(what, dim3((unsigned)nblk), dim3(UP_THREADS), UW_LDS, st, a);
    if (rc != SONET_OK) return rc;
    hipLaunchKernelGGL(upconv3x3_wgrad_reduce_kernel, dim3((unsigned)sonet::ceil_div64(total, 16)), dim3(256), 0, st,
                       reinterpret_cast<const float *>(ws), dw, Cin, Cout, p.CT * UW_CB, p.nslice, total);
    return sonet::launched(what);
}
