// device.hpp -- the device-side building blocks shared by the kernels of libsonet_hip.so (gfx950 only): one copy of each.
// Included through common.hpp.  Everything here is __device__ __forceinline__ in the global namespace; a kernel file keeps only
// what is its own (its pipeline, its tile constants, helpers whose arithmetic differs from the ones here as written).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// ---- vector types (register shapes of the MFMA operands, packed pairs, buffer descriptors) ------------------------
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// compile-time values handed to generic lambdas (dispatch of a runtime choice to a template instantiation)
template <int V> using int_c = std::integral_constant<int, V>;
template <bool B> using bool_c = std::integral_constant<bool, B>;

// ---- conversions and keys -----------------------------------------------------------------------------------------
// Two f32 -> one dword of two bf16 (lo | hi << 16), round to nearest even, NaN stays NaN: one v_cvt_pk_bf16_f32.  As an asm
// statement so that it IS this one instruction, whatever the compiler's own f32 -> __bf16 lowering does: the split and epilogue
// instruction counts of the layer kernels are budgeted for it.  Not volatile: it is pure and may be scheduled or removed.
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// Two f32 -> one dword of two fp16, round to nearest even: the vector conversion is selected as one v_cvt_pk_f16_f32.
__device__ __forceinline__ unsigned cvt_pk_f16(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
}
// Orderable key of a float's bits: unsigned compare == float compare (a total order), so an integer atomicMax finds a maximum
// deterministically.  -0 counts as +0 (the reference's torch.max does not tell them apart); a NaN maps to 0, the smallest key: it
// never wins (a NaN must not beat the reference's initial running maximum of -1000).
__device__ __forceinline__ unsigned ord_f32(unsigned bits) {
    if (bits == 0x80000000u) bits = 0u;
    const unsigned o = bits ^ ((unsigned)((int)bits >> 31) | 0x80000000u);
    return (bits & 0x7FFFFFFFu) > 0x7F800000u ? 0u : o;
}

// ---- raw buffer descriptors ------------------------------------------------------------------------------------
// `bytes` of memory at `ptr` as a raw buffer (stride 0, offsets in bytes): a load past `bytes` returns 0 and a store past it is
// dropped, which is how the layer kernels handle their edges.  Word 3 is DATA_FORMAT 32 (bits 12..18) with every other field
// zero: no swizzle, no index/offset striding, OOB_SELECT 0 (raw: the byte offset is checked against NUM_RECORDS) -- the value the
// compiler's own raw buffer accesses use on gfx9.  raw_buffer is for the __builtin_amdgcn_raw_buffer_* builtins (the descriptor
// type they take, so hipcc sees the accesses as memory operations and counts them); raw_buffer_sgpr is the same four words made
// wave-uniform by hand, for the "s" operand of a buffer instruction written as inline asm.
constexpr int RAW_BUFFER_WORD3 = 0x00020000;
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_buffer(const T *ptr, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(ptr), 0, bytes, RAW_BUFFER_WORD3);
}
__device__ __forceinline__ i32x4_t raw_buffer_sgpr(const void *base, unsigned bytes) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    i32x4_t r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)((a >> 32) & 0xFFFFu));      // stride 0: raw buffer
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = RAW_BUFFER_WORD3;
    return r;
}

// ---- f32 / bf16 storage by overload (uint16_t = bfloat16 bits): values widened on the load, arithmetic in f32 ----------------------
__device__ __forceinline__ float ld_f32(const float *p, long long i) { return p[i]; }
__device__ __forceinline__ float ld_f32(const uint16_t *p, long long i) { return __uint_as_float((unsigned)p[i] << 16); }
// the two bf16 halves of a dword (two consecutive elements, the lower address in the low half)
__device__ __forceinline__ float bf_lo(unsigned d) { return __uint_as_float(d << 16); }
__device__ __forceinline__ float bf_hi(unsigned d) { return __uint_as_float(d & 0xFFFF0000u); }
// ... and ONE rounding on the store: round to nearest even
__device__ __forceinline__ void st_rne(float *p, long long i, float v) { p[i] = v; }
__device__ __forceinline__ void st_rne(uint16_t *p, long long i, float v) { p[i] = (uint16_t)(cvt_pk_bf16(v, v) & 0xFFFFu); }
// four consecutive values (o 16 / 8 byte aligned)
__device__ __forceinline__ void st4_rne(float *o, const float (&v)[4]) { *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void st4_rne(uint16_t *o, const float (&v)[4]) {
    *reinterpret_cast<uint2 *>(o) = make_uint2(cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]));
}

// ---- BatchNorm / ReLU per element: the ONE copy of the arithmetic of the training step's element-wise passes -----------------------
// (bn_passes.hip, and wherever a layer kernel applies the same pass on its operand load or in its epilogue).  The forward's ReLU and
// the backward's mask must agree at the edge: both hang on the SAME fma, `v < 0 ? 0 : v` keeps -0.0 and NaN, `!(v > 0)` masks +0, -0.0
// and NaN (tests/test_gpu_bn_passes.py: test_relu_mask_agrees_between_forward_and_backward_at_its_edge).
// y = act(x * sc + sh): one fma, then ReLU as a compare-and-select (not fmaxf: that would turn a NaN into 0)
__device__ __forceinline__ float affine_act(float x, float sc, float sh, int relu) {
    float v = __fmaf_rn(x, sc, sh);
    if (relu) v = (v < 0.f) ? 0.f : v;
    return v;
}
// gy * mask, mask = the forward's pre-activation is > 0 (recomputed from raw with the forward's own fma; without ReLU: 1).  g is
// overwritten by value and returned, as every site spelled it before there was one copy: a `relu && ... ? 0.f : g` select compiles
// to other code in some of the kernels.
__device__ __forceinline__ float relu_masked(float g, float r, float sc, float sh, int relu) {
    if (relu && !(__fmaf_rn(r, sc, sh) > 0.f)) g = 0.f;
    return g;
}
// g_raw = a * (gy * mask) + b * raw + c0: two fmas, the inner one first (tests/bn_passes_ref.py emulates exactly these two roundings)
__device__ __forceinline__ float bn_bwd_apply(float g, float r, float sc, float sh, int relu, float a, float b, float c0) {
    return __fmaf_rn(a, relu_masked(g, r, sc, sh, relu), __fmaf_rn(b, r, c0));
}

// ---- bf16 normalise-on-load: a packed bf16 pair through act(raw * s + h) ---------------------------------------------
// f32 fma, one round-to-nearest-even back to bf16, ReLU -- sonet_channel_affine_act_out_bf16's arithmetic per element (there: ReLU in
// f32 in front of the rounding; rounding is monotone and keeps the sign, so the order does not matter.  A -0.0 comes out as +0.0
// here: as an operand of the product that is the same number).  Five vector instructions: two unpacks, v_pk_fma_f32,
// v_cvt_pk_bf16_f32, v_pk_max_i16 against `floor2` (0 with ReLU, the most negative i16 in both halves -- the identity -- without).
// NaN: the integer maximum after the rounding turns a NaN with the sign bit set into 0 and keeps one with the sign bit clear, where
// the f32 `v < 0 ? 0 : v` keeps both: "bit for bit" holds for non-NaN data.
__device__ __forceinline__ unsigned bf16_pair_affine_act(unsigned pk, f32x2_t sc, f32x2_t sh, unsigned floor2) {
    const f32x2_t x = {__uint_as_float(pk << 16), __uint_as_float(pk & 0xFFFF0000u)};
    f32x2_t v;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(v) : "v"(x), "v"(sc), "v"(sh));
    unsigned r = cvt_pk_bf16(v[0], v[1]);
    asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(r), "v"(floor2));
    return r;
}

// sum over the 32 lanes of a half wave, result in every lane (all lanes must be active): xor-1, xor-2 inside a quad, mirror inside
// 8 and 16 lanes (DPP modifiers of the add), then the other row of 16 through ds_swizzle (no LDS memory is touched)
__device__ __forceinline__ float row32_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));                     // lane ^ 16
    return v;
}

// Bijective XCD-aware remap of a 1-D block id: consecutive *virtual* ids land on the same XCD
// (and so share its L2).  Pure speed choice -- correctness never depends on placement.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg / sonet::NUM_XCD, r = nwg % sonet::NUM_XCD;
    const int xcd = bid % sonet::NUM_XCD, local = bid / sonet::NUM_XCD;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + local;
}

// ---- operand-range tracking of the fp16-split kernels (two integer max per value pair) ---------------------------
// |x| as ordered bits over everything a lane has seen: positive floats order as signed ints (mp), negative ones --
// sign bit set -- order by magnitude as unsigned ints (mn); a NaN of either sign lands above +-inf in one of the two.
struct RangeAcc { int mp; unsigned mn; };
__device__ __forceinline__ void range_track(RangeAcc &r, float x0, float x1) {
    const int a = __float_as_int(x0), b = __float_as_int(x1);
    r.mp = max(max(r.mp, a), b);                                           // v_max3_i32
    r.mn = max(max(r.mn, (unsigned)a), (unsigned)b);                       // v_max3_u32
}
__device__ __forceinline__ unsigned range_amax_bits(const RangeAcc &r) {   // bits of max |x| (NaN > inf > finite)
    const unsigned neg = (r.mn & 0x80000000u) ? (r.mn & 0x7FFFFFFFu) : 0u;
    const unsigned pos = (unsigned)r.mp;
    return pos > neg ? pos : neg;
}
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)v, o, 64); v = t > v ? t : v; }
    return v;
}
// one atomic per wave at most, and only while the wave's value still raises the word
__device__ __forceinline__ void range_publish(unsigned *word, unsigned wave_max_bits, int lane) {
    if (lane == 0 && wave_max_bits > __atomic_load_n(word, __ATOMIC_RELAXED)) atomicMax(word, wave_max_bits);
}

// ---- P16 planes (include/sonet_hip.h): a value pair clamped to the fp16-split range, scaled by 32, as packed fp16 hi + packed fp16 residual
// p16_split2: (X0, X1) already scaled by 32 and inside +-65504 -> packed hi, packed residual (exact in f32 before it is rounded)
__device__ __forceinline__ void p16_split2(float X0, float X1, unsigned &h, unsigned &m) {
    h = cvt_pk_f16(X0, X1);
    const f16x2_t hv = __builtin_bit_cast(f16x2_t, h);
    m = cvt_pk_f16(X0 - (float)hv[0], X1 - (float)hv[1]);
}
// the clamp is one v_med3_f32: a NaN leaves as the lower bound, the minimum of the three
__device__ __forceinline__ void p16_split_pair(float x0, float x1, unsigned &h, unsigned &m) {
    p16_split2(32.f * __builtin_amdgcn_fmed3f(x0, -2047.f, 2047.f), 32.f * __builtin_amdgcn_fmed3f(x1, -2047.f, 2047.f), h, m);
}
// the WEIGHT side's clamp (the pack kernels): fmin(fmax()) and v_med3_f32 turn a NaN into the lower bound -- a finite weight nobody asked
// for; two compares keep it, so that the packed pieces of a NaN weight are NaN as its trailer word says.  Every other value: the same bits.
__device__ __forceinline__ float clamp_keep_nan(float w, float lim) { return w < -lim ? -lim : (w > lim ? lim : w); }
// channel of element e (0..7) of half h in a 16-channel chunk of a P16 plane
__device__ __forceinline__ int p16_channel(int h, int e) { return 4 * h + (e & 3) + 8 * (e >> 2); }

// ---- group-max epilogues of the node-level stage (pointmlp_h3p.hip EPI 4 / 5, knn_layer.hip): a tile's 32 x 128 post-activation values
// pass through LDS, rows GM_STRIDE floats apart; the max over a group's columns is taken left to right, NaN wins like torch.max.
constexpr int GM_STRIDE = 136;                                 // floats per staged row: 128 columns + 8 (rows 4 apart land 32 banks apart)
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }
// P16 out: the maxima (m0, m1) of element pair p (rows 2 (p & 1) + 8 (p >> 1) + {0, 1} of half h2 of 16-channel chunk `chunk` of the
// output) of output column n_out -> range log, clamp (the values are 32 x already: split_lo is the unscaled lower bound, 0 with ReLU),
// split, one dword into each form's plane of yp (Lout columns per plane)
__device__ __forceinline__ void gmax_p16_store(float m0, float m1, float split_lo, RangeAcc &yr, void *yp, int chunk, int h2, int p,
                                               size_t Lout, size_t n_out) {
    range_track(yr, m0, m1);
    unsigned hv, mv;
    p16_split2(__builtin_amdgcn_fmed3f(m0, split_lo * 32.f, 65504.f), __builtin_amdgcn_fmed3f(m1, split_lo * 32.f, 65504.f), hv, mv);
    unsigned *dst = reinterpret_cast<unsigned *>(static_cast<char *>(yp) + ((((size_t)chunk * 2) * 2 + h2) * Lout + n_out) * 16) + p;
    dst[0] = hv;
    dst[Lout * 8] = mv;                                        // form 1: two half planes (2 x Lout x 16 bytes) further
}

// ---- three-way bf16 split of an f32 pair (the "x3" arithmetic: pointmlp_x3.hip, upconv_bwd.hip, upconv_wgrad.hip) ------------------------------------
// (x0, x1) -> three packed bf16 pairs (hi, mid, lo), round-to-nearest at each level, residuals exact in f32
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned &h, unsigned &m, unsigned &l) {
    h = cvt_pk_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xFFFF0000u);
    m = cvt_pk_bf16(r0, r1);
    const float q0 = r0 - __uint_as_float(m << 16), q1 = r1 - __uint_as_float(m & 0xFFFF0000u);
    l = cvt_pk_bf16(q0, q1);
}

// The WEIGHT side of the split (the pack kernels: not on a hot path).  split3_pair turns a value whose bf16 rounding is inf -- +-inf, and
// the finite |w| >= 0x7F7F8000 (3.3895e38) -- into h = inf, m = l = NaN (inf - inf), and a NaN piece makes the whole output row NaN where
// the f32 product holds +-inf or even a finite value.  Here instead:
//   finite:  h = the largest finite bf16 of that sign (round towards zero); the residual then fits m and l exactly;
//   +-inf:   h = m = 0, l = +-inf.  The l piece meets ONLY xh (the product Wl.xh), which has x's sign and is zero only where x is: the row
//            comes out as inf * x does in f32 -- +-inf, NaN against a zero -- and no 0 * inf arises from the x pieces that happen to be zero.
// Every other value goes through split3_pair unchanged (bit-identical packs).
__device__ __forceinline__ void split3_fix_w(float w, unsigned &h, unsigned &m, unsigned &l) {       // one value's pieces in the low 16 bits
    if ((h & 0x7FFFu) != 0x7F80u) return;
    if (__builtin_isinf(w)) { l = h; h = 0u; m = 0u; return; }
    h -= 1u;                                                                 // 0x7F80 -> 0x7F7F, sign kept
    const float r = w - __uint_as_float(h << 16);
    m = cvt_pk_bf16(r, 0.f) & 0xFFFFu;
    l = cvt_pk_bf16(r - __uint_as_float(m << 16), 0.f) & 0xFFFFu;
}
__device__ __forceinline__ void split3_pair_w(float w0, float w1, unsigned &h, unsigned &m, unsigned &l) {
    split3_pair(w0, w1, h, m, l);
    unsigned h0 = h & 0xFFFFu, m0 = m & 0xFFFFu, l0 = l & 0xFFFFu, h1 = h >> 16, m1 = m >> 16, l1 = l >> 16;
    split3_fix_w(w0, h0, m0, l0);
    split3_fix_w(w1, h1, m1, l1);
    h = h0 | (h1 << 16); m = m0 | (m1 << 16); l = l0 | (l1 << 16);
}

// The product of two split operands on v_mfma_f32_32x32x16_bf16: six of the nine piece products (Al.Bl, Al.Bm, Am.Bl are below f32's
// last bit), the smallest first, added to acc in this order (pointmlp_x3.hip, upconv_bwd.hip, upconv_wgrad.hip)
__device__ __forceinline__ void x3_chain(f32x16 &acc, bf16x8 Ah, bf16x8 Am, bf16x8 Al, bf16x8 Bh, bf16x8 Bm, bf16x8 Bl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh, acc, 0, 0, 0);
}

// cluster mean of the SOM stage (models/networks.py:142): sum / (count + 1e-5), every step rounded to f32 (no reciprocal, no FMA)
__device__ __forceinline__ float cluster_mean(float sum, float count) { return __fdiv_rn(sum, __fadd_rn(count, 1e-5f)); }
