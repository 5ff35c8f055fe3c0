// common.hpp -- shared host-side helpers of libsonet_hip.so (gfx950 only); the device-side ones are in device.hpp, included at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>

#include "../../include/sonet_hip.h"

namespace sonet {

constexpr int WAVE = 64;            // CDNA4 wavefront
constexpr int NUM_XCD = 8;          // MI355X: 8 XCDs, block b is dispatched to XCD b % 8 (speed only)

// thread-local last-error text behind sonet_last_error()
char *err_buf();
int fail(int code, const char *fmt, ...);

static inline hipStream_t as_stream(sonet_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// post-launch check: launch-configuration errors surface here; no synchronisation.
static inline int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SONET_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return SONET_OK;
}

#define SONET_REQUIRE(cond, ...)                                      \
    do {                                                              \
        if (!(cond)) return ::sonet::fail(SONET_ERR_INVALID_ARG, __VA_ARGS__); \
    } while (0)

// Range log of the fp16-split ("h3") kernels: thread-local pointer to the 8-word slot the NEXT h3 launch of this thread
// reports its operand magnitudes into (sonet_range_log_set; NULL = no report).  See include/sonet_hip.h.
uint32_t *range_log();

// Tuning / ablation knobs (SONET_* environment variables of the experiment tools): they exist only in the VARIANTS build
// (make -C so-net_amd/csrc variants -> lib/libsonet_hip_variants.so, -DSONET_VARIANTS).  The product library reads no
// environment variable: every knob is the constant "unset" there and the code behind it is compiled out.
#ifdef SONET_VARIANTS
static inline const char *knob(const char *name) { return getenv(name); }
#else
static inline const char *knob(const char *) { return nullptr; }
#endif

// integer knob: *out = atoi of the variable and true when it is set; never in the product build, where the caller's branch folds away
static inline bool knob_int(const char *name, int *out) {
    const char *e = knob(name);
    if (e) *out = atoi(e);
    return e != nullptr;
}

// Compute units of the current device, for the launchers that size a persistent grid or count rounds of workgroups: the attribute,
// or 256 (an MI355X) when the query fails or reports fewer than `least`.  The launchers of the streaming bf16 kernels spread
// cus / 8 column streams over the XCDs (least = 8); the others take any positive count (least = 1).  Asked per call, not cached.
// Defined in api.hip.
int cu_count(int least = 8);

// What the layer launchers check first about their shapes, in this order (the first failing check is the message): positive sizes
// (`also` = one more size that must be positive), x2 given exactly when C2 > 0, and C1 a multiple of the K chunk (`chunk` channels)
// when a second panel follows it.  SONET_OK or the error.  Defined in api.hip.
int check_layer_shape(const char *what, bool has_x2, int B, int C1, int C2, int Cout, int L, int also = 1, int chunk = 16);

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline long long ceil_div64(long long a, long long b) { return (a + b - 1) / b; }

// Zero `bytes` (a multiple of 4, 4-byte aligned) of device memory with a KERNEL instead of hipMemsetAsync.  The forward of a batch is
// captured into a HIP graph and several such graphs are replayed concurrently on different streams (bench.py --in-flight); with
// memset NODES in the graphs that combination faulted intermittently ("write access to a read-only page") on this runtime.
// Defined in api.hip.
int zero_words(void *p, size_t bytes, hipStream_t st);

// statistics epilogue of the layer kernels: mean / biased variance from per-workgroup (sum, sum of squares) partials
// [nwg][C][2] (f64), fixed order.  Defined in pointmlp_x3.hip.
int launch_stats_finalize(const double *partial, int nwg, int C, double inv_n, float *mean, float *var, hipStream_t st);

// "BatchNorm rider" of the training forward (sonet_bn_rider_set, include/sonet_hip.h): what the NEXT statistics finalize of this thread
// also computes per channel -- the normalisation coefficients (sonet_bn_fwd_coeffs_f32) and F.batch_norm's running-statistics update
// (sonet_bn_running_update_f32), same arithmetic in the same order -- instead of two more C-element launches per BatchNorm layer and step.
// take_bn_rider() hands it out once and clears it.  Defined in api.hip.
struct BnRider {
    const float *gamma, *beta;            // NULL gamma: no rider
    float eps, momentum, unbias;
    float *rmean, *rvar;                  // running statistics, updated in place (may be NULL)
    float *invstd, *sc, *sh;              // outputs [C]
};
BnRider take_bn_rider();

// Launch of a kernel whose dynamic LDS exceeds the 64 KB a kernel gets unasked: the limit is raised to MAX_LDS bytes ONCE per
// kernel instantiation and process -- the initialiser of a function-local static, so concurrent first calls (autograd's worker
// threads) are serialised by the language -- and never on a later launch: a runtime call per launch is not free on a host-bound step.
template <auto KERNEL, int MAX_LDS, typename... Args>
static inline int launch_lds_once(const char *what, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    static const bool allowed =
        hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS) == hipSuccess;
    if (!allowed) return fail(SONET_ERR_UNSUPPORTED, "%s: cannot reserve the LDS", what);
    hipLaunchKernelGGL(KERNEL, grid, block, lds, st, args...);
    return SONET_OK;
}

}  // namespace sonet

// groups (nodes) per 128-column block of the K-level tensor of the flat node-level stage (node_stage.hip): as many as fit, at most 16
static inline int knn_stage_groups(int K) { const int g = 128 / K; return g > 16 ? 16 : g; }

#include "device.hpp"                   // the device-side building blocks of the kernels

// A runtime tile count as a compile-time constant: f(int_c<V>{}) for the V of the list that equals v, for the last one otherwise --
// the `switch (MT)` of a launcher over its kernel instantiations, which are exactly the counts of the list.
template <int V, int... Vs, typename F>
static inline void with_int_c(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) f(int_c<V>{});
    else if (v == V) f(int_c<V>{});
    else with_int_c<Vs...>(v, f);
}
