// upconv_fold.hpp -- the header of the folded up-convolution family, three users: the forward (upconv.hip), the input gradient
// (upconv_bwd.hip) and the weight gradient (upconv_wgrad.hip).  One copy of each building block: the tile extents of the flat column
// axis; the fold table of the (parity, tap) weights and the shift a pair reads (fold_rect, pair_shift: all three); the pack kernels'
// index decode and folded sum; the accumulation chain's flush (all three); the launchers' argument checks and grid arithmetic.  A lane's
// column with its nine neighbour slots, the workgroup's mask of live shifts and a thread's staging items stay written out in the two
// kernels that use them: as shared blocks they measured slower (docs/findings.md).
#pragma once
#include "common.hpp"

namespace {

constexpr int UP_THREADS = 256;
constexpr int UP_TP = SONET_UPCONV_TILE_PIXELS;            // columns (low-resolution pixels) per workgroup
constexpr int UP_KC = SONET_UPCONV_K_CHUNK;                // channels of the reduction per staged chunk
constexpr int UP_CB = SONET_UPCONV_COUT_BLOCK;             // output channels per workgroup
constexpr int UP_MAXHW = SONET_UPCONV_MAX_HW;
constexpr int UP_NSLOT = UP_TP + 2 * UP_MAXHW + 2;         // staged columns at W = 64
constexpr int UP_ZS = UP_NSLOT;                            // the slot of zeros
constexpr int UP_XIT = (2 * UP_NSLOT + UP_THREADS - 1) / UP_THREADS;      // (column, K half) items per thread
constexpr int UP_FLUSH = 16;                               // forward: chunks per accumulation chain (1024 products)
static_assert(UP_TP == 128 && UP_KC == 16 && UP_CB == 32, "the kernels are written for these extents");

// row of the output block a lane holds in accumulator register r (h = lane >> 5)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- the sixteen (parity, tap) pairs, pt = 8 py + 4 px + 2 dy + dx ---------------------------------------------------------------------
// ky (kx) range a (parity, tap) pair sums: parity 0: {0}, {1, 2}; parity 1: {0, 1}, {2}
__device__ __forceinline__ void fold_range(int par, int tap, int &k0, int &k1) {
    k0 = tap == 0 ? 0 : (par == 0 ? 1 : 2);
    k1 = tap == 0 ? (par == 0 ? 0 : 1) : 2;
}
// the rectangle of the 3 x 3 kernel pair pt sums
struct FoldRect {
    int ky0, ky1, kx0, kx1;
    __device__ __forceinline__ bool holds(int ky, int kx) const { return ky >= ky0 && ky <= ky1 && kx >= kx0 && kx <= kx1; }
};
__device__ __forceinline__ FoldRect fold_rect(int pt) {
    FoldRect f;
    fold_range(pt >> 3, (pt >> 1) & 1, f.ky0, f.ky1);
    fold_range((pt >> 2) & 1, pt & 1, f.kx0, f.kx1);
    return f;
}
// the folded weight of one (output, input) channel pair: the float64 sum of w9[ky][kx] over the rectangle, rounded to f32; see(v) is
// shown every weight read
template <typename See> __device__ __forceinline__ float fold_sum(const float *w9, const FoldRect &f, See see) {
    double s = 0.0;
    for (int ky = f.ky0; ky <= f.ky1; ++ky)
        for (int kx = f.kx0; kx <= f.kx1; ++kx) {
            const float v = w9[ky * 3 + kx];
            see(v);
            s += (double)v;
        }
    return (float)s;
}

// pair pt reads the map shifted by (sy, sx) = (py + dy - 1, px + dx - 1); k() numbers the nine shifts, (sy + 1) * 3 + sx + 1.  The input
// gradient reads the mirrored shift (-sy, -sx): 8 - k().
struct PairShift {
    int sy, sx;
    __host__ __device__ constexpr int k() const { return (sy + 1) * 3 + sx + 1; }
};
__host__ __device__ constexpr PairShift pair_shift(int pt) { return PairShift{(pt >> 3) + ((pt >> 1) & 1) - 1, ((pt >> 2) & 1) + (pt & 1) - 1}; }
// the pairs with an in-range shifted element somewhere in an H x W map (bit pt): the host's form of the kernels' ptmask loops
inline unsigned live_pairs(int H, int W) {
    unsigned m = 0;
    for (int pt = 0; pt < 16; ++pt)
        if ((H > 1 || pair_shift(pt).sy == 0) && (W > 1 || pair_shift(pt).sx == 0)) m |= 1u << pt;
    return m;
}

// ---- the pack kernels: thread t = ((ct * KC + kc) * 16 + pt) * 64 + lane, r = t >> 6 the fragment it writes -----------------------------
struct PackIdx { int lane, pt, kc, ct; long long r; };
__device__ __forceinline__ PackIdx pack_index(long long t, int KC) {
    PackIdx p;
    p.lane = (int)(t & 63);
    p.r = t >> 6;
    p.pt = (int)(p.r & 15);
    const long long r2 = p.r >> 4;
    p.kc = (int)(r2 % KC);
    p.ct = (int)(r2 / KC);
    return p;
}

// ---- the accumulation chain: acc runs for a bounded number of products, then is added to tot and restarts from zero ------------------
__device__ __forceinline__ void zero_acc(f32x16 &v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.f;
}
__device__ __forceinline__ void flush_chain(f32x16 &tot, f32x16 &acc) {
    tot += acc;
    zero_acc(acc);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
bool shape_ok(int Cin, int Cout, int H, int W) {
    return Cin >= 1 && Cout >= UP_CB && Cout % UP_CB == 0 && H >= 1 && H <= UP_MAXHW && W >= 1 && W <= UP_MAXHW;
}

// what every launch of the family checks first, in this order, with these texts
int up_check(const char *what, bool nonnull, bool aligned, int B, int Cin, int Cout, int H, int W) {
    SONET_REQUIRE(nonnull, "%s: NULL pointer", what);
    SONET_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "%s: non-positive size", what);
    SONET_REQUIRE(aligned, "%s: misaligned pointer", what);
    if (!shape_ok(Cin, Cout, H, W))
        return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: needs Cout %% %d == 0 and 1 <= H, W <= %d (got Cout=%d H=%d W=%d)", what, UP_CB, UP_MAXHW,
                           Cout, H, W);
    return SONET_OK;
}
// ... and a pack kernel's launch, of `total` threads
int up_pack_check(const char *what, bool nonnull, bool aligned, int Cin, int Cout, long long total) {
    SONET_REQUIRE(nonnull, "%s: NULL pointer", what);
    SONET_REQUIRE(Cin > 0 && Cout > 0, "%s: non-positive size", what);
    SONET_REQUIRE(aligned, "%s: misaligned pointer", what);
    if (!shape_ok(Cin, Cout, 1, 1)) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: Cout = %d is not a multiple of %d", what, Cout, UP_CB);
    if (sonet::ceil_div64(total, 256) > 0x7FFFFFFFll) return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: %d x %d is too large", what, Cout, Cin);
    return SONET_OK;
}
int up_too_many_columns(const char *what, long long ncols) { return sonet::fail(SONET_ERR_UNSUPPORTED, "%s: B * H * W = %lld is too large", what, ncols); }
// the flat axis of a launch with CT row blocks: its columns and its workgroups, one per UP_TP columns and row block
int up_grid(const char *what, int B, int H, int W, int CT, int &ncols, unsigned &nblk) {
    const long long nc = (long long)B * H * W, nb = sonet::ceil_div64(nc, UP_TP) * CT;
    if (nc > 0x7FFF0000ll || nb > 0x7FFFFFFFll) return up_too_many_columns(what, nc);
    ncols = (int)nc;
    nblk = (unsigned)nb;
    return SONET_OK;
}

}  // namespace
