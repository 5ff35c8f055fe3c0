// upconv_fold.hpp -- what the forward (upconv.hip) and the input gradient (upconv_bwd.hip) of the folded up-convolution share: the tile
// extents of the flat column axis, the fold table of the (parity, tap) weights and the shapes both launches take.
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

// ky (kx) range a (parity, tap) pair sums: parity 0: {0}, {1, 2}; parity 1: {0, 1}, {2}
__device__ __forceinline__ void fold_range(int par, int tap, int &k0, int &k1) {
    k0 = tap == 0 ? 0 : (par == 0 ? 1 : 2);
    k1 = tap == 0 ? (par == 0 ? 0 : 1) : 2;
}

bool shape_ok(int Cin, int Cout, int H, int W) {
    return Cin >= 1 && Cout >= UP_CB && Cout % UP_CB == 0 && H >= 1 && H <= UP_MAXHW && W >= 1 && W <= UP_MAXHW;
}

}  // namespace
