// knn_h1.hpp -- KNNModule's first layer per neighbour copy, one copy of its arithmetic (models/layers.py:319-352 + the first MyConv2d):
//   h1[c][column] = act(scale[c] (z[c][source column] + wl[c][0..2] . d) + shift[c])
// from a column's 16-byte record (source column on the flat M-level axis, the three de-centred coordinates d: knn_stage_prepare_kernel)
// and the pre-split z planes.  Used by the kernel that stores h1 (node_stage.hip, knn_stage_input_kernel) and by the one that builds it in
// LDS as the operand of KNNModule's second layer (knn_layer.hip).  Included behind common.hpp.
#pragma once

// Every power of two rides in a coefficient: the z planes hold 32 z and the split wants 32 h1, so a table keeps 32 w, scale, 32 shift --
// a = 32 z + (32 w) . d is 32 x the reference's sum bit for bit, and act(a * scale + 32 shift) = 32 h1 exactly (powers of two commute with
// the rounding of an fma below overflow, and |32 h1| <= 65504 is the range the split clamps to anyway).
// kind 0..4 of channel c: 32 w0, 32 w1, 32 w2, scale, 32 shift; `in` = the channel exists (a channel that does not reads as zeros).
__device__ __forceinline__ float knn_h1_coef(int kind, bool in, int c, const float *__restrict__ wl, const float *__restrict__ scale,
                                             const float *__restrict__ shift) {
    if (!in) return 0.f;
    return kind < 3 ? 32.f * wl[c * 3 + kind] : kind == 3 ? scale[c] : 32.f * shift[c];
}

// The column's record as the operands of the channel-pair arithmetic.
struct KnnCol {
    f32x2_t d0, d1, d2;                  // the de-centred coordinates, each in both halves of a pair
    bool valid, ok;                      // not a padding column (src != -2); the neighbour exists (src >= 0: its z is gathered)
};
__device__ __forceinline__ KnnCol knn_col(const int4 r) {
    KnnCol k;
    k.d0 = f32x2_t{__int_as_float(r.y), __int_as_float(r.y)};
    k.d1 = f32x2_t{__int_as_float(r.z), __int_as_float(r.z)};
    k.d2 = f32x2_t{__int_as_float(r.w), __int_as_float(r.w)};
    k.valid = r.x != -2;
    k.ok = r.x >= 0;
    return k;
}

// The pre-activation at 32 x its size, on a channel pair (V = f32x2_t: v_pk_fma_f32, what a kernel bound by its vector arithmetic wants)
// or on one channel (V = float: what a kernel wants whose vector instructions ride in the shadow of MFMAs, where a packed f32
// instruction costs more than the two plain ones it replaces).  z32 = 32 z = hi + residual (exact: two fp16 values whose exponents are
// at most 11 apart); then the reference's order: z, the three coordinate channels, the affine.
template <typename V>
__device__ __forceinline__ V knn_h1_preact(V z32, V w0, V w1, V w2, V sc, V sh, V d0, V d1, V d2) {
    V a = __builtin_elementwise_fma(w0, d0, z32);
    a = __builtin_elementwise_fma(w1, d1, a);
    a = __builtin_elementwise_fma(w2, d2, a);
    return __builtin_elementwise_fma(a, sc, sh);
}

// One channel PAIR (elements 2 q, 2 q + 1 of a (chunk, half): two consecutive channels) of one column: the pair's dword of each of the
// two 16-byte gathers of z (hi, residual; zeros for a neighbour that does not exist) -> the pair's dword of h1's hi and residual vectors.
// cf[kind] points at the pair's two coefficients (8-byte aligned: one 8-byte read per kind).  lo: 0 with ReLU, -65504 without -- ReLU
// and the lower clamp of the split are one v_med3_f32 (a NaN leaves it as the lower bound, as in split_act; the range accumulator has
// seen it).  PACKED: the arithmetic on the pair or channel by channel (knn_h1_preact): the same bits.
template <bool PACKED>
__device__ __forceinline__ void knn_h1_pair(unsigned zh, unsigned zm, const float *const (&cf)[5], const KnnCol &k, float lo, RangeAcc &xr,
                                            unsigned &hv, unsigned &mv) {
    const f32x2_t w0 = *reinterpret_cast<const f32x2_t *>(cf[0]), w1 = *reinterpret_cast<const f32x2_t *>(cf[1]),
                w2 = *reinterpret_cast<const f32x2_t *>(cf[2]), sc = *reinterpret_cast<const f32x2_t *>(cf[3]),
                sh = *reinterpret_cast<const f32x2_t *>(cf[4]);
    const f16x2_t zh2 = __builtin_bit_cast(f16x2_t, zh), zm2 = __builtin_bit_cast(f16x2_t, zm);
    f32x2_t a;
    if constexpr (PACKED) {
        a = knn_h1_preact<f32x2_t>(__builtin_convertvector(zh2, f32x2_t) + __builtin_convertvector(zm2, f32x2_t), w0, w1, w2, sc, sh, k.d0, k.d1, k.d2);
    } else {
#pragma unroll
        for (int e = 0; e < 2; ++e)
            a[e] = knn_h1_preact<float>((float)zh2[e] + (float)zm2[e], w0[e], w1[e], w2[e], sc[e], sh[e], k.d0[e], k.d1[e], k.d2[e]);
    }
    if (!k.valid) a = f32x2_t{0.f, 0.f};
    range_track(xr, a[0], a[1]);
    p16_split2(__builtin_amdgcn_fmed3f(a[0], lo, 65504.f), __builtin_amdgcn_fmed3f(a[1], lo, 65504.f), hv, mv);
}

// One (chunk, half) of one column = its four pairs: two 16-byte gathers in, two 16-byte vectors out, the same P16 element order;
// cf[kind] points at the 8 coefficients of this (chunk, half).
__device__ __forceinline__ void knn_h1_half(const uint4 zhq, const uint4 zmq, const float *const (&cf)[5], const KnnCol &k, float lo,
                                            RangeAcc &xr, uint4 &hq, uint4 &mq) {
    const unsigned zh[4] = {zhq.x, zhq.y, zhq.z, zhq.w}, zm[4] = {zmq.x, zmq.y, zmq.z, zmq.w};
    unsigned hv[4], mv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float *const cq[5] = {cf[0] + 2 * q, cf[1] + 2 * q, cf[2] + 2 * q, cf[3] + 2 * q, cf[4] + 2 * q};
        knn_h1_pair<true>(zh[q], zm[q], cq, k, lo, xr, hv[q], mv[q]);
    }
    hq = make_uint4(hv[0], hv[1], hv[2], hv[3]);
    mq = make_uint4(mv[0], mv[1], mv[2], mv[3]);
}

// What a lane reports of values it tracked at 32 x their size before an activation's clamp: after a ReLU only the positive side -- and
// a NaN of either sign -- can leave the range; the factor 32 leaves through the exponent.  (Take wave_umax of the result BEFORE
// range_x32_out: the subtraction is monotone, the order does not matter, and the callers have always reduced first.)
__device__ __forceinline__ unsigned range_act_bits(const RangeAcc &r, int relu) {
    if (!relu) return range_amax_bits(r);
    const unsigned pos = r.mp > 0 ? (unsigned)r.mp : 0u, nan_neg = r.mn > 0xFF800000u ? (r.mn & 0x7FFFFFFFu) : 0u;
    return pos > nan_neg ? pos : nan_neg;
}
__device__ __forceinline__ unsigned range_x32_out(unsigned bits) { return bits > (5u << 23) ? bits - (5u << 23) : 0u; }
