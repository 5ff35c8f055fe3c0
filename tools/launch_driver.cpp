// launch_driver.cpp -- the sweep of tools/launch_log.py: calls the C ABI of the layer launchers with fake non-null pointers (nothing is
// dereferenced on the host) against tools/launch_stub.cpp and prints one line per case:
//   group \t case \t return code \t sonet_last_error() when refused \t the launches the stub recorded
// group = entry point, optional features and channel pair; case = B x L and whatever else varies inside the group.
// argv[1..]: group prefixes to run (none: all); "@bn": the family of the BatchNorm / ReLU passes (run_bn_* below) instead of the layer
// launchers; "@upconv": the decoder's up-convolution family (run_upconv below) instead.  Built with -DSONET_VARIANTS for the variants
// library's extra entry points.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "include/sonet_hip.h"                 // (of the tree under test: -I TREE)

extern "C" const char *launch_log_take(void);
#ifdef SONET_VARIANTS
extern "C" int sonet_pointmlp_h3_kmax_f32(const float *x1, int C1, const float *x2, int C2, const void *Wp3, const float *scale,
                                          const float *shift, int relu, float *out, void *keys_ws, int B, int Cout, int L, int M,
                                          sonet_stream_t stream);
#endif

namespace {

int g_argc;
char **g_argv;

// fake device pointers: distinct, 4 KiB apart, never dereferenced
template <typename T = float> T *P(int n, int misalign = 0) { return reinterpret_cast<T *>((uintptr_t)0x100000000ull + (uintptr_t)n * 4096u + misalign); }

std::string fmt(const char *f, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

bool wanted(const std::string &group)
{
    bool any = false;
    for (int i = 1; i < g_argc; ++i) any = any || g_argv[i][0] != '@';
    if (!any) return true;
    for (int i = 1; i < g_argc; ++i)
        if (group.compare(0, strlen(g_argv[i]), g_argv[i]) == 0) return true;
    return false;
}

void report(const std::string &group, const std::string &cs, int rc)
{
    printf("%s\t%s\t%d\t%s\t%s\n", group.c_str(), cs.c_str(), rc, rc ? sonet_last_error() : "", launch_log_take());
}

struct Pair { int C1, C2, Cout; };
// the channel pairs of models/networks.py and models/layers.py, one with Cout % 32 != 0, two with a second input panel, one with a
// second panel behind C1 % 16 != 0 (refused)
const Pair PAIRS[] = {{3, 0, 64}, {64, 0, 128}, {128, 0, 256}, {320, 0, 384}, {384, 0, 512}, {512, 0, 512}, {515, 0, 768}, {640, 0, 768},
                      {768, 0, 640}, {1024, 0, 512}, {393, 0, 1024}, {3356, 0, 1024}, {64, 0, 100}, {256, 64, 384}, {128, 256, 1024}, {3, 64, 128}};
const int BS[] = {1, 2, 8, 64};
const int LS[] = {1, 31, 32, 33, 63, 64, 65, 300, 512, 1024, 3072, 5000, 15000, 1023, 15001};   // (the last two: bf16 entry points only, odd beside even)

const sonet_stream_t ST = nullptr;

// one group per (entry, pair): f(pair, B, L) is called over every size
template <typename F> void sweep(const char *entry, F f)
{
    const int nl = strstr(entry, "bf16") ? 15 : 13;
    for (const Pair &p : PAIRS) {
        const std::string group = fmt("%s %d+%d>%d", entry, p.C1, p.C2, p.Cout);
        if (!wanted(group)) continue;
        for (int B : BS)
            for (int i = 0; i < nl; ++i) report(group, fmt("%dx%d", B, LS[i]), f(p, B, LS[i]));
    }
}
template <typename F> void sweep_bl(const char *entry, F f)
{
    if (!wanted(entry)) return;
    const int nl = strstr(entry, "bf16") ? 15 : 13;
    for (int B : BS)
        for (int i = 0; i < nl; ++i) report(entry, fmt("%dx%d", B, LS[i]), f(B, LS[i]));
}
template <typename F> void one(const char *entry, const char *cs, F f)
{
    if (wanted(entry)) report(entry, cs, f());
}

const float *X2(const Pair &p) { return p.C2 ? P(2) : nullptr; }
template <typename T> const T *X2t(const Pair &p, int mis = 0) { return p.C2 ? P<T>(2, mis) : nullptr; }

void run_pointmlp()
{
    sweep("sonet_pointmlp_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P(6), B, p.Cout, L, ST); });
    sweep("sonet_channel_stats_f32", [](const Pair &p, int B, int L) {
        return sonet_channel_stats_f32(P(1), B, p.Cout, L, P<double>(2), P(3), P(4), ST); });
    sweep("sonet_channel_affine_act_f32", [](const Pair &p, int B, int L) {
        return sonet_channel_affine_act_f32(P(1), P(2), P(3), 1, B, p.Cout, L, ST); });
    for (const Pair &p : PAIRS)
        one("sonet_pointmlp_pack_f32", fmt("%d>%d", p.C1 + p.C2, p.Cout).c_str(), [&] { return sonet_pointmlp_pack_f32(P(1), P(2), p.C1 + p.C2, p.Cout, ST); });
    one("sonet_pointmlp_f32 refused", "null x1", [] { return sonet_pointmlp_f32(nullptr, 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 2, 64, 64, ST); });
    one("sonet_pointmlp_f32 refused", "B=0", [] { return sonet_pointmlp_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 0, 64, 64, ST); });
    one("sonet_pointmlp_f32 refused", "x2 without C2", [] { return sonet_pointmlp_f32(P(1), 64, P(2), 0, P(3), P(4), P(5), 1, P(6), 2, 64, 64, ST); });
    one("sonet_pointmlp_f32 refused", "C1 % 8", [] { return sonet_pointmlp_f32(P(1), 3, P(2), 64, P(3), P(4), P(5), 1, P(6), 2, 64, 64, ST); });
    one("sonet_pointmlp_f32 refused", "Cout 2048 odd tiles", [] { return sonet_pointmlp_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 2, 2080, 64, ST); });
}

void run_x3()
{
    sweep("sonet_pointmlp_x3_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_x3_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P(6), B, p.Cout, L, ST); });
    sweep("sonet_pointmlp_h3_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P(6), B, p.Cout, L, ST); });
    sweep("sonet_pointmlp_h3_gather_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3_gather_f32(P(1), p.C1, 2048, P<int32_t>(7), X2(p), p.C2, P(3), P(4), P(5), 1, P(6), B, p.Cout, L, ST); });
    sweep("sonet_pointmlp_h3_nodeadd_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3_nodeadd_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P(6), B, p.Cout, L, P(8), P<int32_t>(9), 64, ST); });
    sweep("sonet_pointmlp_h3_segpool_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3_segpool_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), 64, P(10),
                                             P<int32_t>(11), P(12), B, p.Cout, L, nullptr, nullptr, nullptr, nullptr, 0, ST); });
    sweep("sonet_pointmlp_h3_segpool_f32 xaff", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3_segpool_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P<int32_t>(7), P<int32_t>(8), nullptr, 64, P(10),
                                             P<int32_t>(11), P(12), B, p.Cout, L, P(13), P(14), p.C2 ? P(15) : nullptr, p.C2 ? P(16) : nullptr, 3, ST); });
    sweep("sonet_pointmlp_h3_stats_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3_stats_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P(6), B, p.Cout, L, P(10), P(11), P(12), ST); });
    sweep("sonet_pointmlp_x3_stats_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_x3_stats_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P(6), B, p.Cout, L, P(10), P(11), P(12), ST); });
    sweep("sonet_pointmlp_h3_stats_xaff_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3_stats_xaff_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P(6), B, p.Cout, L, P(10), P(11), P(12),
                                                P(13), P(14), p.C2 ? P(15) : nullptr, p.C2 ? P(16) : nullptr, 1, ST); });
    sweep("sonet_pointmlp_x3_bnb_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_x3_bnb_f32(P(1), P(2), p.C1 + p.C2, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, P(18), P(6), B, p.Cout, L,
                                         nullptr, nullptr, nullptr, 0, nullptr, nullptr, ST); });
    sweep("sonet_pointmlp_x3_bnb_f32 psums", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_x3_bnb_f32(P(1), P(2), p.C1 + p.C2, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, nullptr, P(6), B, p.Cout, L,
                                         P(19), P(20), P(21), 1, P(22), P<double>(23), ST); });
    sweep("sonet_pointmlp_x3_bnb_acc_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_x3_bnb_acc_f32(P(1), P(2), p.C1 + p.C2, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 0, P(18), P(6), P(6), B, p.Cout, L, ST); });
#ifdef SONET_VARIANTS
    sweep("sonet_pointmlp_h3_kmax_f32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3_kmax_f32(P(1), p.C1, X2(p), p.C2, P(3), P(4), P(5), 1, P(6), P(10), B, p.Cout, L, L % 8 == 0 ? L / 8 : 1, ST); });
#endif
    for (const Pair &p : PAIRS) {
        const std::string cs = fmt("%d>%d", p.C1 + p.C2, p.Cout);
        one("sonet_pointmlp_x3_pack", cs.c_str(), [&] { return sonet_pointmlp_x3_pack(P(1), P(2), p.C1 + p.C2, p.Cout, ST); });
        one("sonet_pointmlp_h3_pack", cs.c_str(), [&] { return sonet_pointmlp_h3_pack(P(1), P(2), p.C1 + p.C2, p.Cout, ST); });
        one("sonet_pointmlp_x3_pack_strided", cs.c_str(), [&] { return sonet_pointmlp_x3_pack_strided(P(1), 1, p.Cout, P(2), p.C1 + p.C2, p.Cout, p.Cout - 1, ST); });
        one("sonet_pointmlp_h3_pack_strided", cs.c_str(), [&] { return sonet_pointmlp_h3_pack_strided(P(1), 1, p.Cout, P(2), p.C1 + p.C2, p.Cout, p.Cout - 1, ST); });
    }
    one("sonet_pack_multi", "7 entries, 1000 blocks", [] { return sonet_pack_multi(P(1), 7, 1000, ST); });
    const char *R = "sonet_pointmlp_h3 refused";
    one(R, "h3 null x1", [] { return sonet_pointmlp_h3_f32(nullptr, 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 2, 64, 64, ST); });
    one(R, "h3 null y", [] { return sonet_pointmlp_h3_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, nullptr, 2, 64, 64, ST); });
    one(R, "h3 L=0", [] { return sonet_pointmlp_h3_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 2, 64, 0, ST); });
    one(R, "h3 B=0", [] { return sonet_pointmlp_h3_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 0, 64, 64, ST); });
    one(R, "h3 x2 without C2", [] { return sonet_pointmlp_h3_f32(P(1), 64, P(2), 0, P(3), P(4), P(5), 1, P(6), 2, 64, 64, ST); });
    one(R, "h3 C2 without x2", [] { return sonet_pointmlp_h3_f32(P(1), 64, nullptr, 64, P(3), P(4), P(5), 1, P(6), 2, 64, 64, ST); });
    one(R, "h3 panel too large", [] { return sonet_pointmlp_h3_f32(P(1), 4096, nullptr, 0, P(3), P(4), P(5), 1, P(6), 1, 64, 300000, ST); });
    one(R, "h3 Cout too large", [] { return sonet_pointmlp_h3_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 1, 32 * 37, 64, ST); });
    one(R, "gather null gidx", [] { return sonet_pointmlp_h3_gather_f32(P(1), 64, 100, nullptr, nullptr, 0, P(3), P(4), P(5), 1, P(6), 2, 64, 64, ST); });
    one(R, "gather L1=0", [] { return sonet_pointmlp_h3_gather_f32(P(1), 64, 0, P<int32_t>(7), nullptr, 0, P(3), P(4), P(5), 1, P(6), 2, 64, 64, ST); });
    one(R, "nodeadd null zidx", [] { return sonet_pointmlp_h3_nodeadd_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 2, 64, 64, P(8), nullptr, 64, ST); });
    one(R, "stats null mean", [] { return sonet_pointmlp_h3_stats_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P(6), 2, 64, 64, P(10), nullptr, P(12), ST); });
    one(R, "stats_xaff null xs2", [] { return sonet_pointmlp_h3_stats_xaff_f32(P(1), 64, P(2), 64, P(3), P(4), P(5), 1, P(6), 2, 128, 64, P(10), P(11), P(12), P(13), P(14), nullptr, nullptr, 1, ST); });
    one(R, "segpool null ws", [] { return sonet_pointmlp_h3_segpool_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<int32_t>(7), P<int32_t>(8), nullptr, 64, nullptr,
                                                                       P<int32_t>(11), P(12), 2, 64, 64, nullptr, nullptr, nullptr, nullptr, 0, ST); });
    one(R, "segpool M=0", [] { return sonet_pointmlp_h3_segpool_f32(P(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<int32_t>(7), P<int32_t>(8), nullptr, 0, P(10),
                                                                   P<int32_t>(11), P(12), 2, 64, 64, nullptr, nullptr, nullptr, nullptr, 0, ST); });
    one(R, "bnb null raw", [] { return sonet_pointmlp_x3_bnb_f32(P(1), nullptr, 64, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, P(18), P(6), 2, 64, 64,
                                                                nullptr, nullptr, nullptr, 0, nullptr, nullptr, ST); });
    one(R, "bnb praw without psums", [] { return sonet_pointmlp_x3_bnb_f32(P(1), P(2), 64, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, P(18), P(6), 2, 64, 64,
                                                                          P(19), P(20), P(21), 1, P(22), nullptr, ST); });
    one(R, "bnb praw without psc", [] { return sonet_pointmlp_x3_bnb_f32(P(1), P(2), 64, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, P(18), P(6), 2, 64, 64,
                                                                        P(19), nullptr, P(21), 1, P(22), P<double>(23), ST); });
    one(R, "bnb C=1024", [] { return sonet_pointmlp_x3_bnb_f32(P(1), P(2), 1024, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, P(18), P(6), 2, 64, 64,
                                                              nullptr, nullptr, nullptr, 0, nullptr, nullptr, ST); });
    one(R, "bnb_acc null yadd", [] { return sonet_pointmlp_x3_bnb_acc_f32(P(1), P(2), 64, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 0, P(18), nullptr, P(6), 2, 64, 64, ST); });
}

void run_bf16()
{
    typedef uint16_t h;
    for (int mis = 0; mis <= 2; mis += 2) {                     // (2-byte-misaligned x1 / y: the unpaired kernels)
        const std::string m = mis ? " misaligned" : "";
        sweep(("sonet_pointmlp_bf16" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16(P<h>(1, mis), p.C1, X2t<h>(p), p.C2, P(3), P(4), P(5), 1, P<h>(6, mis), B, p.Cout, L, ST); });
        sweep(("sonet_pointmlp_bf16_stats" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16_stats(P<h>(1, mis), p.C1, X2t<h>(p), p.C2, P(3), P(4), P(5), 1, P<h>(6, mis), B, p.Cout, L, P(10), P(11), P(12), ST); });
        sweep(("sonet_pointmlp_bf16_stats_xaff" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16_stats_xaff(P<h>(1, mis), p.C1, X2t<h>(p), p.C2, P(3), P(4), P(5), 1, P<h>(6, mis), B, p.Cout, L, P(10), P(11), P(12),
                                                  P(13), P(14), p.C2 ? P(15) : nullptr, p.C2 ? P(16) : nullptr, 3, ST); });
        sweep(("sonet_pointmlp_bf16_pool" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16_pool(P<h>(1, mis), p.C1, X2t<h>(p), p.C2, P(3), P(4), P(5), 1, P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), P(10),
                                            B, p.Cout, L, 64, ST); });
        sweep(("sonet_pointmlp_bf16_pool_xaff" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16_pool_xaff(P<h>(1, mis), p.C1, X2t<h>(p), p.C2, P(3), P(4), P(5), 1, P<int32_t>(7), nullptr, P<int32_t>(9), P(10),
                                                 B, p.Cout, L, 64, P(13), P(14), p.C2 ? P(15) : nullptr, p.C2 ? P(16) : nullptr, 3, ST); });
        sweep(("sonet_pointmlp_bf16_acc" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16_acc(P<h>(1, mis), p.C1, X2t<h>(p), p.C2, P(3), P(4), P(5), 1, P<h>(6), P<h>(6, mis), B, p.Cout, L, ST); });
        sweep(("sonet_pointmlp_bf16_bnb" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16_bnb(P<h>(1, mis), P<h>(2), p.C1 + p.C2, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, P<h>(18), nullptr,
                                           P<h>(6, mis), B, p.Cout, L, ST); });
        sweep(("sonet_pointmlp_bf16_bnb yadd" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16_bnb(P<h>(1), P<h>(2, mis), p.C1 + p.C2, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 0, nullptr, P<h>(6),
                                           P<h>(6), B, p.Cout, L, ST); });
        sweep(("sonet_pointmlp_bf16_gather" + m).c_str(), [mis](const Pair &p, int B, int L) {
            return sonet_pointmlp_bf16_gather(P<h>(1, mis), p.C1, 2048, P<int32_t>(7), X2t<h>(p), p.C2, P(3), P(4), P(5), 1, P<h>(6, mis), B, p.Cout, L, ST); });
    }
    for (const Pair &p : PAIRS) {
        const std::string cs = fmt("%d>%d", p.C1 + p.C2, p.Cout);
        one("sonet_pointmlp_bf16_pack", cs.c_str(), [&] { return sonet_pointmlp_bf16_pack(P(1), P(2), p.C1 + p.C2, p.Cout, ST); });
        one("sonet_pointmlp_bf16_pack_strided", cs.c_str(), [&] { return sonet_pointmlp_bf16_pack_strided(P(1), 1, p.Cout, P(2), p.C1 + p.C2, p.Cout, p.Cout - 1, ST); });
    }
    const char *R = "sonet_pointmlp_bf16 refused";
    one(R, "null x1", [] { return sonet_pointmlp_bf16(nullptr, 64, nullptr, 0, P(3), P(4), P(5), 1, P<h>(6), 2, 64, 64, ST); });
    one(R, "L=0", [] { return sonet_pointmlp_bf16(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<h>(6), 2, 64, 0, ST); });
    one(R, "Cout=0", [] { return sonet_pointmlp_bf16(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<h>(6), 2, 0, 64, ST); });
    one(R, "x2 without C2", [] { return sonet_pointmlp_bf16(P<h>(1), 64, P<h>(2), 0, P(3), P(4), P(5), 1, P<h>(6), 2, 64, 64, ST); });
    one(R, "panel too large", [] { return sonet_pointmlp_bf16(P<h>(1), 4096, nullptr, 0, P(3), P(4), P(5), 1, P<h>(6), 1, 64, 300000, ST); });
    one(R, "Cout too large", [] { return sonet_pointmlp_bf16(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<h>(6), 1, 32 * 37, 64, ST); });
    one(R, "gather L1=0", [] { return sonet_pointmlp_bf16_gather(P<h>(1), 64, 0, P<int32_t>(7), nullptr, 0, P(3), P(4), P(5), 1, P<h>(6), 2, 64, 64, ST); });
    one(R, "gather null gidx", [] { return sonet_pointmlp_bf16_gather(P<h>(1), 64, 64, nullptr, nullptr, 0, P(3), P(4), P(5), 1, P<h>(6), 2, 64, 64, ST); });
    one(R, "stats null var", [] { return sonet_pointmlp_bf16_stats(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<h>(6), 2, 64, 64, P(10), P(11), nullptr, ST); });
    one(R, "stats_xaff null xs2", [] { return sonet_pointmlp_bf16_stats_xaff(P<h>(1), 64, P<h>(2), 64, P(3), P(4), P(5), 1, P<h>(6), 64, 128, 15000, P(10), P(11), P(12),
                                                                            P(13), P(14), nullptr, nullptr, 3, ST); });
    one(R, "acc null yadd", [] { return sonet_pointmlp_bf16_acc(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, nullptr, P<h>(6), 2, 64, 64, ST); });
    one(R, "acc misaligned yadd", [] { return sonet_pointmlp_bf16_acc(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<h>(6, 2), P<h>(6), 2, 64, 64, ST); });
    one(R, "bnb C=16", [] { return sonet_pointmlp_bf16_bnb(P<h>(1), P<h>(2), 16, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, nullptr, nullptr, P<h>(6), 2, 64, 64, ST); });
    one(R, "bnb misaligned g_raw_out", [] { return sonet_pointmlp_bf16_bnb(P<h>(1), P<h>(2), 64, P(3), P(4), P(5), P(13), P(14), P(15), P(16), P(17), 1, P<h>(18, 2), nullptr, P<h>(6), 2, 64, 64, ST); });
    one(R, "pool null ids", [] { return sonet_pointmlp_bf16_pool(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, nullptr, nullptr, P<int32_t>(9), P(10), 2, 64, 64, 64, ST); });
    one(R, "pool M=0", [] { return sonet_pointmlp_bf16_pool(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<int32_t>(7), nullptr, P<int32_t>(9), P(10), 2, 64, 64, 0, ST); });
    one(R, "pool M=300", [] { return sonet_pointmlp_bf16_pool(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<int32_t>(7), nullptr, P<int32_t>(9), P(10), 2, 64, 64, 300, ST); });
    one(R, "pool M=255 no slab fits", [] { return sonet_pointmlp_bf16_pool(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<int32_t>(7), nullptr, P<int32_t>(9), P(10), 2, 96, 64, 255, ST); });
    one(R, "pool_xaff null xh1", [] { return sonet_pointmlp_bf16_pool_xaff(P<h>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, P<int32_t>(7), nullptr, P<int32_t>(9), P(10), 2, 64, 64, 64,
                                                                          P(13), nullptr, nullptr, nullptr, 0, ST); });
}

void run_h3p()
{
    sweep("sonet_pointmlp_h3p y", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3p(P<void>(1), p.C1, 0, nullptr, p.C2 ? P<void>(2) : nullptr, p.C2, P(3), P(4), P(5), 1, P(6), nullptr, B, p.Cout, L,
                                  nullptr, nullptr, 0, nullptr, nullptr, nullptr, ST); });
    sweep("sonet_pointmlp_h3p yp", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3p(P<void>(1), p.C1, 0, nullptr, p.C2 ? P<void>(2) : nullptr, p.C2, P(3), P(4), P(5), 1, nullptr, P<void>(7), B, p.Cout, L,
                                  nullptr, nullptr, 0, nullptr, nullptr, nullptr, ST); });
    sweep("sonet_pointmlp_h3p y+yp gather", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3p(P<void>(1), p.C1, 2048, P<int32_t>(8), p.C2 ? P<void>(2) : nullptr, p.C2, P(3), P(4), P(5), 0, P(6), P<void>(7), B, p.Cout, L,
                                  nullptr, nullptr, 0, nullptr, nullptr, nullptr, ST); });
    sweep("sonet_pointmlp_h3p y zadd64", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3p(P<void>(1), p.C1, 0, nullptr, p.C2 ? P<void>(2) : nullptr, p.C2, P(3), P(4), P(5), 1, P(6), nullptr, B, p.Cout, L,
                                  P(9), P<int32_t>(10), 64, nullptr, nullptr, nullptr, ST); });
    sweep("sonet_pointmlp_h3p yp zadd32", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3p(P<void>(1), p.C1, 0, nullptr, p.C2 ? P<void>(2) : nullptr, p.C2, P(3), P(4), P(5), 1, nullptr, P<void>(7), B, p.Cout, L,
                                  P(9), P<int32_t>(10), 32, nullptr, nullptr, nullptr, ST); });
    sweep("sonet_pointmlp_h3p stats", [](const Pair &p, int B, int L) {
        return sonet_pointmlp_h3p(P<void>(1), p.C1, 0, nullptr, p.C2 ? P<void>(2) : nullptr, p.C2, P(3), P(4), P(5), 1, P(6), nullptr, B, p.Cout, L,
                                  nullptr, nullptr, 0, P<void>(11), P(12), P(13), ST); });
    for (const Pair &p : PAIRS) {
        const std::string gy = fmt("sonet_pointmlp_h3p_gmax y %d+%d>%d", p.C1, p.C2, p.Cout), gp = fmt("sonet_pointmlp_h3p_gmax yp %d+%d>%d", p.C1, p.C2, p.Cout);
        for (int L : {128, 1024, 8192, 100}) {
            for (int G : {1, 2, 3})
                one(gy.c_str(), fmt("L=%d GK=%d G=%d", L, 64 / G / 4 * 4, G).c_str(), [&] {
                    return sonet_pointmlp_h3p_gmax(P<void>(1), p.C1, p.C2 ? P<void>(2) : nullptr, p.C2, P(3), P(4), P(5), 1, p.Cout, L, 64 / G / 4 * 4, G,
                                                   L / 128 * G, 0, P(6), nullptr, ST); });
            for (int K : {3, 9, 16, 64})
                one(gp.c_str(), fmt("L=%d GK=%d", L, K).c_str(), [&] {
                    const int G = 128 / K > 16 ? 16 : 128 / K;
                    return sonet_pointmlp_h3p_gmax(P<void>(1), p.C1, p.C2 ? P<void>(2) : nullptr, p.C2, P(3), P(4), P(5), 1, p.Cout, L, K, G,
                                                   L / 128 * G, L / 128 * G + 5, nullptr, P<void>(7), ST); });
        }
        const std::string cs = fmt("%d>%d", p.C1 + p.C2, p.Cout);
        one("sonet_pointmlp_h3p_pack", cs.c_str(), [&] { return sonet_pointmlp_h3p_pack(P(1), P<void>(2), p.C1 + p.C2, p.Cout, ST); });
    }
    sweep("sonet_p16_from_f32", [](const Pair &p, int B, int L) { return sonet_p16_from_f32(P(1), P<void>(2), B, p.C1, L, nullptr, nullptr, 0, ST); });
    sweep("sonet_p16_from_f32 affine", [](const Pair &p, int B, int L) { return sonet_p16_from_f32(P(1), P<void>(2), B, p.C1, L, P(3), P(4), 1, ST); });
    sweep("sonet_p16_to_f32", [](const Pair &p, int B, int L) { return sonet_p16_to_f32(P<void>(1), P(2), B, p.C1, L, ST); });
    const char *R = "sonet_pointmlp_h3p refused";
#define H3P_CALL(x1, C1, L1, gidx, x2, C2, y, yp, B, Cout, L, zadd, zidx, ZM, ws, mean, var) \
    [] { return sonet_pointmlp_h3p(x1, C1, L1, gidx, x2, C2, P(3), P(4), P(5), 1, y, yp, B, Cout, L, zadd, zidx, ZM, ws, mean, var, ST); }
    one(R, "null x1", H3P_CALL(nullptr, 64, 0, nullptr, nullptr, 0, P(6), nullptr, 2, 64, 64, nullptr, nullptr, 0, nullptr, nullptr, nullptr));
    one(R, "no output", H3P_CALL(P<void>(1), 64, 0, nullptr, nullptr, 0, nullptr, nullptr, 2, 64, 64, nullptr, nullptr, 0, nullptr, nullptr, nullptr));
    one(R, "L=0", H3P_CALL(P<void>(1), 64, 0, nullptr, nullptr, 0, P(6), nullptr, 2, 64, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr));
    one(R, "gather L1=0", H3P_CALL(P<void>(1), 64, 0, P<int32_t>(8), nullptr, 0, P(6), nullptr, 2, 64, 64, nullptr, nullptr, 0, nullptr, nullptr, nullptr));
    one(R, "x2 without C2", H3P_CALL(P<void>(1), 64, 0, nullptr, P<void>(2), 0, P(6), nullptr, 2, 64, 64, nullptr, nullptr, 0, nullptr, nullptr, nullptr));
    one(R, "zadd without zidx", H3P_CALL(P<void>(1), 64, 0, nullptr, nullptr, 0, P(6), nullptr, 2, 64, 64, P(9), nullptr, 64, nullptr, nullptr, nullptr));
    one(R, "zadd ZM=0", H3P_CALL(P<void>(1), 64, 0, nullptr, nullptr, 0, P(6), nullptr, 2, 64, 64, P(9), P<int32_t>(10), 0, nullptr, nullptr, nullptr));
    one(R, "stats with yp", H3P_CALL(P<void>(1), 64, 0, nullptr, nullptr, 0, P(6), P<void>(7), 2, 64, 64, nullptr, nullptr, 0, P<void>(11), P(12), P(13)));
    one(R, "stats with zadd", H3P_CALL(P<void>(1), 64, 0, nullptr, nullptr, 0, P(6), nullptr, 2, 64, 64, P(9), P<int32_t>(10), 64, P<void>(11), P(12), P(13)));
    one(R, "stats null var", H3P_CALL(P<void>(1), 64, 0, nullptr, nullptr, 0, P(6), nullptr, 2, 64, 64, nullptr, nullptr, 0, P<void>(11), P(12), nullptr));
    one(R, "y+yp zadd64", H3P_CALL(P<void>(1), 64, 0, nullptr, nullptr, 0, P(6), P<void>(7), 8, 128, 1024, P(9), P<int32_t>(10), 64, nullptr, nullptr, nullptr));
    one(R, "panel too large", H3P_CALL(P<void>(1), 4096, 0, nullptr, nullptr, 0, P(6), nullptr, 1, 64, 300000, nullptr, nullptr, 0, nullptr, nullptr, nullptr));
#undef H3P_CALL
    one(R, "gmax both outputs", [] { return sonet_pointmlp_h3p_gmax(P<void>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, 64, 128, 8, 16, 16, 16, P(6), P<void>(7), ST); });
    one(R, "gmax G GK > 128", [] { return sonet_pointmlp_h3p_gmax(P<void>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, 64, 128, 16, 16, 16, 16, nullptr, P<void>(7), ST); });
    one(R, "gmax Lout < ngout", [] { return sonet_pointmlp_h3p_gmax(P<void>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, 64, 128, 8, 16, 16, 8, nullptr, P<void>(7), ST); });
    one(R, "gmax G=32 planes", [] { return sonet_pointmlp_h3p_gmax(P<void>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, 64, 128, 4, 32, 32, 32, nullptr, P<void>(7), ST); });
    one(R, "gmax f32 GK=6", [] { return sonet_pointmlp_h3p_gmax(P<void>(1), 64, nullptr, 0, P(3), P(4), P(5), 1, 64, 128, 6, 2, 2, 0, P(6), nullptr, ST); });
}

void run_pointresnet()
{
    for (int Cin0 : {3, 6}) {
        const std::string c = fmt(" Cin0=%d", Cin0);
        sweep_bl(("sonet_pointresnet_fused_f32" + c).c_str(), [=](int B, int L) { return sonet_pointresnet_fused_f32(P(1), Cin0, P(2), P(3), P(4), B, L, ST); });
        sweep_bl(("sonet_pointresnet_fused_p16_f32 y+yp" + c).c_str(), [=](int B, int L) { return sonet_pointresnet_fused_p16_f32(P(1), Cin0, P(2), P(3), P(4), P<void>(5), B, L, ST); });
        sweep_bl(("sonet_pointresnet_fused_p16_f32 yp" + c).c_str(), [=](int B, int L) { return sonet_pointresnet_fused_p16_f32(P(1), Cin0, P(2), P(3), nullptr, P<void>(5), B, L, ST); });
        for (int M : {16, 64, 100}) {
            const std::string m = fmt("%s M=%d", c.c_str(), M);
            sweep_bl(("sonet_pointresnet_fused_pool_f32" + m).c_str(), [=](int B, int L) {
                return sonet_pointresnet_fused_pool_f32(P(1), Cin0, P(2), P(3), P<int32_t>(6), P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), P<void>(10), P(11), B, L, M, ST); });
            sweep_bl(("sonet_pointresnet_fused_pool_p16_f32" + m).c_str(), [=](int B, int L) {
                return sonet_pointresnet_fused_pool_p16_f32(P(1), Cin0, P(2), P(3), P<int32_t>(6), P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), P<void>(10), P(11), P<void>(12), B, L, M, ST); });
            sweep_bl(("sonet_pointresnet_bf16_pool" + m).c_str(), [=](int B, int L) {
                return sonet_pointresnet_bf16_pool(P(1), Cin0, P(2), P(3), P<int32_t>(6), P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), P<void>(10), P(11), B, L, M, ST); });
        }
        sweep_bl(("sonet_pointresnet_bf16" + c).c_str(), [=](int B, int L) { return sonet_pointresnet_bf16(P(1), Cin0, P(2), P(3), P<uint16_t>(4), B, L, ST); });
        one("sonet_pointresnet_pack", c.c_str(), [=] { return sonet_pointresnet_pack(P(1), P(2), P(3), P(4), Cin0, P<void>(5), ST); });
        one("sonet_pointresnet_bf16_pack", c.c_str(), [=] { return sonet_pointresnet_bf16_pack(P(1), P(2), P(3), P(4), Cin0, P<void>(5), ST); });
    }
    const char *R = "sonet_pointresnet refused";
    one(R, "fused null y", [] { return sonet_pointresnet_fused_f32(P(1), 3, P(2), P(3), nullptr, 2, 64, ST); });
    one(R, "fused Cin0=17", [] { return sonet_pointresnet_fused_f32(P(1), 17, P(2), P(3), P(4), 2, 64, ST); });
    one(R, "fused_p16 null yp", [] { return sonet_pointresnet_fused_p16_f32(P(1), 3, P(2), P(3), P(4), nullptr, 2, 64, ST); });
    one(R, "fused_pool M=0", [] { return sonet_pointresnet_fused_pool_f32(P(1), 3, P(2), P(3), P<int32_t>(6), P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), P<void>(10), P(11), 2, 64, 0, ST); });
    one(R, "fused_pool B=70000", [] { return sonet_pointresnet_fused_pool_f32(P(1), 3, P(2), P(3), P<int32_t>(6), P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), P<void>(10), P(11), 70000, 64, 8, ST); });
    one(R, "fused_pool_p16 null planes", [] { return sonet_pointresnet_fused_pool_p16_f32(P(1), 3, P(2), P(3), P<int32_t>(6), P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), P<void>(10), P(11), nullptr, 2, 64, 8, ST); });
    one(R, "bf16 B=0", [] { return sonet_pointresnet_bf16(P(1), 3, P(2), P(3), P<uint16_t>(4), 0, 64, ST); });
    one(R, "bf16_pool null ws", [] { return sonet_pointresnet_bf16_pool(P(1), 3, P(2), P(3), P<int32_t>(6), P<int32_t>(7), P<int32_t>(8), P<int32_t>(9), nullptr, P(11), 2, 64, 8, ST); });
}

void run_wgrad()
{
    typedef uint16_t h;
    sweep("sonet_wgrad_x3_f32", [](const Pair &p, int B, int L) { return sonet_wgrad_x3_f32(P(1), P(2), P(3), P<void>(4), B, p.Cout, p.C1 + p.C2, L, ST); });
    sweep("sonet_wgrad_x3_xaff_f32", [](const Pair &p, int B, int L) { return sonet_wgrad_x3_xaff_f32(P(1), P(2), P(3), P<void>(4), B, p.Cout, p.C1 + p.C2, L, P(5), P(6), 1, ST); });
    sweep("sonet_wgrad_bf16", [](const Pair &p, int B, int L) { return sonet_wgrad_bf16(P<h>(1), P<h>(2), P(3), P<void>(4), B, p.Cout, p.C1 + p.C2, L, ST); });
    sweep("sonet_wgrad_bf16_xaff", [](const Pair &p, int B, int L) { return sonet_wgrad_bf16_xaff(P<h>(1), P<h>(2), P(3), P<void>(4), B, p.Cout, p.C1 + p.C2, L, P(5), P(6), 1, ST); });
    const char *R = "sonet_wgrad refused";
    one(R, "x3 null ws", [] { return sonet_wgrad_x3_f32(P(1), P(2), P(3), nullptr, 2, 64, 64, 64, ST); });
    one(R, "x3 L=0", [] { return sonet_wgrad_x3_f32(P(1), P(2), P(3), P<void>(4), 2, 64, 64, 0, ST); });
    one(R, "x3_xaff null xh", [] { return sonet_wgrad_x3_xaff_f32(P(1), P(2), P(3), P<void>(4), 2, 64, 64, 64, P(5), nullptr, 1, ST); });
    one(R, "bf16 misaligned g", [] { return sonet_wgrad_bf16(P<h>(1, 2), P<h>(2), P(3), P<void>(4), 2, 64, 64, 64, ST); });
    one(R, "bf16 Cin=0", [] { return sonet_wgrad_bf16(P<h>(1), P<h>(2), P(3), P<void>(4), 2, 64, 0, 64, ST); });
    one(R, "bf16_xaff null xs", [] { return sonet_wgrad_bf16_xaff(P<h>(1), P<h>(2), P(3), P<void>(4), 2, 64, 64, 64, nullptr, P(6), 1, ST); });
}

// ---- the BatchNorm / ReLU passes, their node-broadcast forms, the coefficient kernels, the eval-mode head kernels and the pooled sparse
// gradient ("@bn" in argv: this family INSTEAD of the layer launchers above, so that either half of the recording stands on its own) ----
struct Args {
    int B = 3, C = 5, L = 8, M = 64, NL = 3;
    int null = -1;                              // number of the pointer passed as NULL
    int off[3] = {0, 0, 0};                     // element offsets of the [B][C][L] operands
    template <typename T> T *t(int i, int slot) const { return null == i ? nullptr : P<T>(i + 1, off[slot] * (int)sizeof(T)); }
    template <typename T = float> T *v(int i) const { return null == i ? nullptr : P<T>(i + 1); }
};
typedef uint16_t bh;
struct Entry { const char *name; int (*call)(const Args &); int nptr; std::vector<const char *> tensors; };
const Entry BCL[] = {
    {"sonet_channel_stats_f32", [](const Args &a) { return sonet_channel_stats_f32(a.t<float>(0, 0), a.B, a.C, a.L, a.v<double>(1), a.v(2), a.v(3), ST); }, 4, {"y"}},
    {"sonet_channel_stats_bf16", [](const Args &a) { return sonet_channel_stats_bf16(a.t<bh>(0, 0), a.B, a.C, a.L, a.v<double>(1), a.v(2), a.v(3), ST); }, 4, {"y"}},
    {"sonet_channel_affine_act_f32", [](const Args &a) { return sonet_channel_affine_act_f32(a.t<float>(0, 0), a.v(1), a.v(2), 1, a.B, a.C, a.L, ST); }, 3, {"y"}},
    {"sonet_channel_affine_act_out_f32", [](const Args &a) { return sonet_channel_affine_act_out_f32(a.t<float>(0, 0), a.v(1), a.v(2), 1, a.t<float>(3, 1), a.B, a.C, a.L, ST); }, 4, {"x", "y"}},
    {"sonet_channel_affine_act_out_bf16", [](const Args &a) { return sonet_channel_affine_act_out_bf16(a.t<bh>(0, 0), a.v(1), a.v(2), 1, a.t<bh>(3, 1), a.B, a.C, a.L, ST); }, 4, {"x", "y"}},
    {"sonet_pointwise_bwd_stats_f32", [](const Args &a) { return sonet_pointwise_bwd_stats_f32(a.t<float>(0, 0), a.t<float>(1, 1), a.v(2), a.v(3), 1, a.B, a.C, a.L, a.v<double>(4), ST); }, 5, {"gy", "raw"}},
    {"sonet_pointwise_bwd_stats_bf16", [](const Args &a) { return sonet_pointwise_bwd_stats_bf16(a.t<bh>(0, 0), a.t<bh>(1, 1), a.v(2), a.v(3), 1, a.B, a.C, a.L, a.v<double>(4), ST); }, 5, {"gy", "raw"}},
    {"sonet_pointwise_bwd_apply_f32", [](const Args &a) { return sonet_pointwise_bwd_apply_f32(a.t<float>(0, 0), a.t<float>(1, 1), a.v(2), a.v(3), 1, a.v(4), a.v(5), a.v(6), a.t<float>(7, 2), a.B, a.C, a.L, ST); }, 8, {"gy", "raw", "g_raw"}},
    {"sonet_pointwise_bwd_apply_bf16", [](const Args &a) { return sonet_pointwise_bwd_apply_bf16(a.t<bh>(0, 0), a.t<bh>(1, 1), a.v(2), a.v(3), 1, a.v(4), a.v(5), a.v(6), a.t<bh>(7, 2), a.B, a.C, a.L, ST); }, 8, {"gy", "raw", "g_raw"}},
    {"sonet_pointwise_bwd_apply_nodesum_f32", [](const Args &a) { return sonet_pointwise_bwd_apply_nodesum_f32(a.t<float>(0, 0), a.t<float>(1, 1), a.v(2), a.v(3), 1, a.v(4), a.v(5), a.v(6), a.v<int32_t>(7), a.M,
                                                                                                         a.t<float>(8, 2), a.v(9), a.v<void>(10), a.B, a.C, a.L, ST); }, 11, {"gy", "raw", "g_raw"}},
    {"sonet_node_add_affine_act_f32", [](const Args &a) { return sonet_node_add_affine_act_f32(a.t<float>(0, 0), a.v(1), a.v<int32_t>(2), a.v(3), a.v(4), 1, a.B, a.C, a.L, a.M, ST); }, 5, {"t"}},
    {"sonet_node_gather_lead_affine_act_f32", [](const Args &a) { return sonet_node_gather_lead_affine_act_f32(a.v(0), a.t<int32_t>(1, 0), a.t<float>(2, 1), a.v(3), a.v(4), a.v(5), 1, a.t<float>(6, 2),
                                                                                                         a.B, a.C, a.L, a.M, a.NL, ST); }, 7, {"gidx", "lead", "out"}},
    {"sonet_node_gather_lead_affine_act_bf16", [](const Args &a) { return sonet_node_gather_lead_affine_act_bf16(a.v<bh>(0), a.t<int32_t>(1, 0), a.t<float>(2, 1), a.v(3), a.v(4), a.v(5), 1, a.t<bh>(6, 2),
                                                                                                           a.B, a.C, a.L, a.M, a.NL, ST); }, 7, {"gidx", "lead", "out"}},
};
const int BN_BS[] = {1, 3, 9, 17, 64}, BN_CS[] = {1, 5, 1024};
const int BN_LS[] = {1, 2, 6, 7, 8, 1023, 1028, 1030, 2049, 2051, 2056, 4100, 5462, 5463, 8200, 8202, 15000, 40000};
// the statistics pass groups 8 clouds per workgroup once segments * C * ceil(B / 8) >= 2048: both sides, at one and at two segments per row
const int BN_GROUPING[][3] = {{9, 1024, 8}, {9, 1023, 8}, {8, 1024, 8}, {16, 1024, 8}, {17, 683, 8}, {17, 682, 8}, {9, 512, 4100}, {9, 511, 4100}, {9, 512, 8200}, {9, 511, 8200}};

void bcl_sizes(const Entry &e, const std::string &group, Args a)
{
    if (!wanted(group)) return;
    for (int B : BN_BS) for (int C : BN_CS) for (int L : BN_LS) {
        a.B = B; a.C = C; a.L = L;
        report(group, fmt("%dx%dx%d", B, C, L), e.call(a));
    }
    for (const auto &g : BN_GROUPING) {
        a.B = g[0]; a.C = g[1]; a.L = g[2];
        report(group, fmt("%dx%dx%d", g[0], g[1], g[2]), e.call(a));
    }
}

void run_bn_bcl()
{
    for (const Entry &e : BCL) {
        const int nt = (int)e.tensors.size();
        for (int k = 0; k <= 2; ++k) {                            // every [B][C][L] operand k elements into its allocation
            Args a;
            for (int i = 0; i < nt; ++i) a.off[i] = k;
            bcl_sizes(e, fmt("%s k=%d", e.name, k), a);
        }
        for (int i = 0; nt > 1 && i < nt; ++i)                    // ... and one operand alone
            for (int k = 1; k <= 2; ++k) {
                Args a;
                a.off[i] = k;
                bcl_sizes(e, fmt("%s %s+%d", e.name, e.tensors[i], k), a);
            }
        const std::string R = fmt("%s refused", e.name);
        if (!wanted(R)) continue;
        for (int L : {8, 7}) {
            for (int i = 0; i < e.nptr; ++i) { Args a; a.L = L; a.null = i; report(R, fmt("L=%d null pointer %d", L, i), e.call(a)); }
            { Args a; a.L = L; a.B = 0; report(R, fmt("L=%d B=0", L), e.call(a)); }
            { Args a; a.L = L; a.C = 0; report(R, fmt("L=%d C=0", L), e.call(a)); }
            { Args a; a.B = 1; a.L = 0; report(R, fmt("L=0 after %d", L), e.call(a)); }
            { Args a; a.L = L; a.M = 0; report(R, fmt("L=%d M=0", L), e.call(a)); }
            { Args a; a.L = L; a.B = 1; a.C = 65535; report(R, fmt("L=%d C=65535", L), e.call(a)); }
            { Args a; a.L = L; a.B = 1; a.C = 65536; report(R, fmt("L=%d C=65536", L), e.call(a)); }
            { Args a; a.L = L; a.B = 65535; a.C = 1; report(R, fmt("L=%d B=65535", L), e.call(a)); }
            { Args a; a.L = L; a.B = 65536; a.C = 1; report(R, fmt("L=%d B=65536", L), e.call(a)); }
            { Args a; a.L = L; a.B = 32768; a.C = 65535; report(R, fmt("L=%d B*C=2^31-32768", L), e.call(a)); }
            { Args a; a.L = L; a.B = 32768; a.C = 65536; report(R, fmt("L=%d B*C=2^31", L), e.call(a)); }
            { Args a; a.L = L; a.B = 65536; a.C = 32768; report(R, fmt("L=%d B*C=2^31 B=65536", L), e.call(a)); }
            for (int M : {1024, 1025, 8192, 8193}) { Args a; a.L = L; a.M = M; report(R, fmt("L=%d M=%d", L, M), e.call(a)); }
            for (int NL : {-1, 0, 4, 5}) { Args a; a.L = L; a.NL = NL; report(R, fmt("L=%d NL=%d", L, NL), e.call(a)); }
            { Args a; a.L = L; a.NL = 0; a.null = 2; report(R, fmt("L=%d NL=0 without lead", L), e.call(a)); }
            { Args a; a.L = L; a.NL = 0; a.null = 2; a.off[1] = 1; report(R, fmt("L=%d NL=0 without lead misaligned", L), e.call(a)); }
        }
    }
}

void run_bn_coeffs()
{
    const int CS[] = {1, 5, 255, 256, 257, 1024, 65535, 65536, 1 << 24};
    for (int C : CS) {
        const std::string cs = fmt("C=%d", C);
        one("sonet_bn_fwd_coeffs_f32", cs.c_str(), [=] { return sonet_bn_fwd_coeffs_f32(P(1), P(2), P(3), P(4), 1e-5f, C, P(5), P(6), P(7), ST); });
        one("sonet_bn_running_update_f32", cs.c_str(), [=] { return sonet_bn_running_update_f32(P(1), P(2), P(3), P(4), 0.1f, 1.5f, C, ST); });
        one("sonet_bn_bwd_coeffs_f32", cs.c_str(), [=] { return sonet_bn_bwd_coeffs_f32(P<double>(1), P(2), P(3), P(4), 24.0, C, P(5), P(6), P(7), P(8), P(9), ST); });
    }
    auto Q = [](int i, int null) { return i == null ? nullptr : P(i + 1); };
    const char *R = "sonet_bn coefficients refused";
    for (int n = 0; n < 7; ++n)
        one(R, fmt("fwd_coeffs null pointer %d", n).c_str(), [=] { return sonet_bn_fwd_coeffs_f32(Q(0, n), Q(1, n), Q(2, n), Q(3, n), 1e-5f, 5, Q(4, n), Q(5, n), Q(6, n), ST); });
    for (int n = 0; n < 4; ++n)
        one(R, fmt("running_update null pointer %d", n).c_str(), [=] { return sonet_bn_running_update_f32(Q(0, n), Q(1, n), Q(2, n), Q(3, n), 0.1f, 1.5f, 5, ST); });
    for (int n = 0; n < 9; ++n)
        one(R, fmt("bwd_coeffs null pointer %d", n).c_str(), [=] { return sonet_bn_bwd_coeffs_f32(n == 0 ? nullptr : P<double>(1), Q(1, n), Q(2, n), Q(3, n), 24.0, 5, Q(4, n), Q(5, n), Q(6, n), Q(7, n), Q(8, n), ST); });
    for (int C : {0, -1}) {
        one(R, fmt("fwd_coeffs C=%d", C).c_str(), [=] { return sonet_bn_fwd_coeffs_f32(P(1), P(2), P(3), P(4), 1e-5f, C, P(5), P(6), P(7), ST); });
        one(R, fmt("running_update C=%d", C).c_str(), [=] { return sonet_bn_running_update_f32(P(1), P(2), P(3), P(4), 0.1f, 1.5f, C, ST); });
        one(R, fmt("bwd_coeffs C=%d", C).c_str(), [=] { return sonet_bn_bwd_coeffs_f32(P<double>(1), P(2), P(3), P(4), 24.0, C, P(5), P(6), P(7), P(8), P(9), ST); });
    }
    one(R, "bwd_coeffs n=0", [] { return sonet_bn_bwd_coeffs_f32(P<double>(1), P(2), P(3), P(4), 0.0, 5, P(5), P(6), P(7), P(8), P(9), ST); });
}

void run_bn_head()
{
    for (long long rows : {1ll, 9ll, 65535ll})
        for (int N : {1, 7, 8, 1024, 1028, 8192, 8196, 9000})
            for (int k : {1, 2, 3})
                one("sonet_chunk_mean_f32", fmt("%lldx%d k=%d", rows, N, k).c_str(), [=] { return sonet_chunk_mean_f32(P(1), P(2), rows, N, k, ST); });
    one("sonet_chunk_mean_f32", "9x8 misaligned h", [] { return sonet_chunk_mean_f32(P(1, 4), P(2), 9, 8, 3, ST); });
    one("sonet_chunk_mean_f32", "9x8 misaligned out", [] { return sonet_chunk_mean_f32(P(1), P(2, 4), 9, 8, 3, ST); });
    const char *R = "sonet_chunk_mean_f32 refused";
    one(R, "null h", [] { return sonet_chunk_mean_f32(nullptr, P(2), 9, 8, 3, ST); });
    one(R, "null out", [] { return sonet_chunk_mean_f32(P(1), nullptr, 9, 8, 3, ST); });
    one(R, "rows=0", [] { return sonet_chunk_mean_f32(P(1), P(2), 0, 8, 3, ST); });
    one(R, "N=0", [] { return sonet_chunk_mean_f32(P(1), P(2), 9, 0, 3, ST); });
    one(R, "k=0", [] { return sonet_chunk_mean_f32(P(1), P(2), 9, 8, 0, ST); });
    one(R, "k=4", [] { return sonet_chunk_mean_f32(P(1), P(2), 9, 8, 4, ST); });
    one(R, "rows=65536", [] { return sonet_chunk_mean_f32(P(1), P(2), 65536, 8, 3, ST); });
    one(R, "rows=65535*32768+1", [] { return sonet_chunk_mean_f32(P(1), P(2), 65535 * 32768ll + 1, 8, 3, ST); });

    for (int B : {1, 3, 16, 17, 64, 128})
        for (int Cin : {1, 5, 256, 1024, 1028, 1792, 1796, 4096})
            for (int Cout : {1, 8, 40, 512})
                one("sonet_linear_act_f32", fmt("%dx%d>%d", B, Cin, Cout).c_str(), [=] { return sonet_linear_act_f32(P(1), P(2), P(3), P(4), 1, P(5), B, Cin, Cout, ST); });
    one("sonet_linear_act_f32", "3x5>8 misaligned x", [] { return sonet_linear_act_f32(P(1, 4), P(2), P(3), P(4), 1, P(5), 3, 5, 8, ST); });
    const char *RL = "sonet_linear_act_f32 refused";
    auto Q = [](int i, int null) { return i == null ? nullptr : P(i + 1); };
    for (int n = 0; n < 5; ++n)
        one(RL, fmt("null pointer %d", n).c_str(), [=] { return sonet_linear_act_f32(Q(0, n), Q(1, n), Q(2, n), Q(3, n), 1, Q(4, n), 3, 8, 8, ST); });
    one(RL, "B=0", [] { return sonet_linear_act_f32(P(1), P(2), P(3), P(4), 1, P(5), 0, 8, 8, ST); });
    one(RL, "Cin=0", [] { return sonet_linear_act_f32(P(1), P(2), P(3), P(4), 1, P(5), 3, 0, 8, ST); });
    one(RL, "Cout=0", [] { return sonet_linear_act_f32(P(1), P(2), P(3), P(4), 1, P(5), 3, 8, 0, ST); });
    one(RL, "misaligned x", [] { return sonet_linear_act_f32(P(1, 4), P(2), P(3), P(4), 1, P(5), 3, 8, 8, ST); });
    one(RL, "misaligned W", [] { return sonet_linear_act_f32(P(1), P(2, 8), P(3), P(4), 1, P(5), 3, 8, 8, ST); });
    one(RL, "Cin=4097", [] { return sonet_linear_act_f32(P(1), P(2), P(3), P(4), 1, P(5), 3, 4097, 8, ST); });
    one(RL, "Cin=4100", [] { return sonet_linear_act_f32(P(1), P(2), P(3), P(4), 1, P(5), 3, 4100, 8, ST); });
    one(RL, "B=16*65535+1", [] { return sonet_linear_act_f32(P(1), P(2), P(3), P(4), 1, P(5), 16 * 65535 + 1, 8, 8, ST); });
}

struct Pooled { int C, M, C1, C2; };
const Pooled POOLED[] = {{384, 64, 64, 256}, {384, 16, 320, 0}, {128, 64, 3, 64}, {384, 64, 128, 256}, {96, 9, 64, 0}, {385, 64, 64, 256}};

void run_bn_pooled()
{
    for (const Pooled &p : POOLED) {
        const std::string sh = fmt(" C=%d M=%d %d+%d", p.C, p.M, p.C1, p.C2);
        const int Ci = p.C1 + p.C2;
        for (int B : {1, 8, 64})
            for (int L : {1, 31, 128, 1023, 1024, 2049, 5000, 15000, 40000}) {
                const std::string cs = fmt("%dx%d", B, L);
                one(("sonet_pooled_wgrad_f32" + sh).c_str(), cs.c_str(), [&] { return sonet_pooled_wgrad_f32(P(1), P<int32_t>(2), P(3), B, p.C, p.M, Ci, L, P(4), ST); });
                one(("sonet_pooled_wgrad_xaff_f32" + sh).c_str(), cs.c_str(), [&] { return sonet_pooled_wgrad_xaff_f32(P(1), P<int32_t>(2), P(3), B, p.C, p.M, Ci, L, P(4), P(5), P(6), 1, ST); });
                one(("sonet_pooled_wgrad_xbf16" + sh).c_str(), cs.c_str(), [&] { return sonet_pooled_wgrad_xbf16(P(1), P<int32_t>(2), P<bh>(3), B, p.C, p.M, Ci, L, P(4), ST); });
                one(("sonet_pooled_wgrad_xaff_xbf16" + sh).c_str(), cs.c_str(), [&] { return sonet_pooled_wgrad_xaff_xbf16(P(1), P<int32_t>(2), P<bh>(3), B, p.C, p.M, Ci, L, P(4), P(5), P(6), 1, ST); });
                one(("sonet_pooled_dgrad_f32" + sh).c_str(), cs.c_str(), [&] { return sonet_pooled_dgrad_f32(P(1), P<int32_t>(2), P(3), B, p.C, p.M, p.C1, p.C2, L, P<void>(4), P(5), p.C2 ? P(6) : nullptr, ST); });
                one(("sonet_pooled_dgrad_obf16" + sh).c_str(), cs.c_str(), [&] { return sonet_pooled_dgrad_obf16(P(1), P<int32_t>(2), P(3), B, p.C, p.M, p.C1, p.C2, L, P<void>(4), P<bh>(5), p.C2 ? P<bh>(6) : nullptr, ST); });
                one(("sonet_pooled_dgrad_mfma_bf16" + sh).c_str(), cs.c_str(), [&] { return sonet_pooled_dgrad_mfma_bf16(P(1), P<int32_t>(2), P<void>(3), B, p.C, p.M, p.C1, p.C2, L, P<void>(4), P<bh>(5), p.C2 ? P<bh>(6) : nullptr, ST); });
#ifdef SONET_VARIANTS
                one(("sonet_pooled_dgrad_tail_f32" + sh).c_str(), cs.c_str(), [&] { return sonet_pooled_dgrad_tail_f32(P(1), P<int32_t>(2), P(3), B, p.C, p.M, p.C1, p.C2, L, P<void>(4), P(5), p.C2 ? P(6) : nullptr,
                                                                                                            P(7), P<int32_t>(8), p.C2 ? P(9) : nullptr, P(10), P(11), 1, p.C2 ? P<void>(12) : nullptr, p.C2 ? P<double>(13) : nullptr, ST); });
#endif
            }
    }
    const char *R = "sonet_pooled refused";
    auto Q = [](int i, int null) { return i == null ? nullptr : P(i + 1); };
    for (int n = 0; n < 6; ++n) {
        one(R, fmt("wgrad_xaff_f32 null pointer %d", n).c_str(), [=] { return sonet_pooled_wgrad_xaff_f32(Q(0, n), (const int32_t *)Q(1, n), Q(2, n), 2, 384, 64, 320, 1024, Q(3, n), Q(4, n), Q(5, n), 1, ST); });
        one(R, fmt("wgrad_xaff_xbf16 null pointer %d", n).c_str(), [=] { return sonet_pooled_wgrad_xaff_xbf16(Q(0, n), (const int32_t *)Q(1, n), (const bh *)Q(2, n), 2, 384, 64, 320, 1024, Q(3, n), Q(4, n), Q(5, n), 1, ST); });
        one(R, fmt("dgrad_f32 null pointer %d", n).c_str(), [=] { return sonet_pooled_dgrad_f32(Q(0, n), (const int32_t *)Q(1, n), Q(2, n), 2, 384, 64, 64, 256, 1024, Q(3, n), Q(4, n), Q(5, n), ST); });
        one(R, fmt("dgrad_mfma_bf16 null pointer %d", n).c_str(), [=] { return sonet_pooled_dgrad_mfma_bf16(Q(0, n), (const int32_t *)Q(1, n), Q(2, n), 2, 384, 64, 64, 256, 1024, Q(3, n), (bh *)Q(4, n), (bh *)Q(5, n), ST); });
    }
    for (int n = 0; n < 4; ++n) {
        one(R, fmt("wgrad_f32 null pointer %d", n).c_str(), [=] { return sonet_pooled_wgrad_f32(Q(0, n), (const int32_t *)Q(1, n), Q(2, n), 2, 384, 64, 320, 1024, Q(3, n), ST); });
        one(R, fmt("wgrad_xbf16 null pointer %d", n).c_str(), [=] { return sonet_pooled_wgrad_xbf16(Q(0, n), (const int32_t *)Q(1, n), (const bh *)Q(2, n), 2, 384, 64, 320, 1024, Q(3, n), ST); });
    }
    struct S { const char *cs; int B, C, M, C1, C2, L; };
    const S sizes[] = {{"B=0", 0, 384, 64, 64, 256, 1024}, {"C=0", 2, 0, 64, 64, 256, 1024}, {"M=0", 2, 384, 0, 64, 256, 1024}, {"C1=0", 2, 384, 64, 0, 256, 1024},
                       {"L=0", 2, 384, 64, 64, 256, 0}, {"B=65536", 65536, 384, 64, 64, 256, 1024}, {"M=65", 2, 384, 65, 64, 256, 1024}, {"C*M=2^20", 2, 16384, 64, 64, 256, 1024},
                       {"L=300000", 2, 384, 64, 64, 256, 300000}, {"L=1023", 2, 384, 64, 64, 256, 1023}, {"C=8", 2, 8, 64, 64, 256, 1024}, {"C=400", 2, 400, 64, 64, 256, 1024},
                       {"odd tiles", 2, 384, 64, 64, 224, 1024}, {"14 tiles", 2, 384, 64, 192, 256, 1024}};
    for (const S &z : sizes) {
        one(R, fmt("wgrad_f32 %s", z.cs).c_str(), [&] { return sonet_pooled_wgrad_f32(P(1), P<int32_t>(2), P(3), z.B, z.C, z.M, z.C1 + z.C2, z.L, P(4), ST); });
        one(R, fmt("wgrad_xbf16 %s", z.cs).c_str(), [&] { return sonet_pooled_wgrad_xbf16(P(1), P<int32_t>(2), P<bh>(3), z.B, z.C, z.M, z.C1 + z.C2, z.L, P(4), ST); });
        one(R, fmt("dgrad_f32 %s", z.cs).c_str(), [&] { return sonet_pooled_dgrad_f32(P(1), P<int32_t>(2), P(3), z.B, z.C, z.M, z.C1, z.C2, z.L, P<void>(4), P(5), P(6), ST); });
        one(R, fmt("dgrad_obf16 %s", z.cs).c_str(), [&] { return sonet_pooled_dgrad_obf16(P(1), P<int32_t>(2), P(3), z.B, z.C, z.M, z.C1, z.C2, z.L, P<void>(4), P<bh>(5), P<bh>(6), ST); });
        one(R, fmt("dgrad_mfma_bf16 %s", z.cs).c_str(), [&] { return sonet_pooled_dgrad_mfma_bf16(P(1), P<int32_t>(2), P<void>(3), z.B, z.C, z.M, z.C1, z.C2, z.L, P<void>(4), P<bh>(5), P<bh>(6), ST); });
    }
    one(R, "dgrad_f32 gx2 without C2", [] { return sonet_pooled_dgrad_f32(P(1), P<int32_t>(2), P(3), 2, 384, 64, 320, 0, 1024, P<void>(4), P(5), P(6), ST); });
    one(R, "dgrad_f32 C2 without gx2", [] { return sonet_pooled_dgrad_f32(P(1), P<int32_t>(2), P(3), 2, 384, 64, 64, 256, 1024, P<void>(4), P(5), nullptr, ST); });
    one(R, "dgrad_mfma_bf16 misaligned gx1", [] { return sonet_pooled_dgrad_mfma_bf16(P(1), P<int32_t>(2), P<void>(3), 2, 384, 64, 64, 256, 1024, P<void>(4), P<bh>(5, 2), P<bh>(6), ST); });
#ifdef SONET_VARIANTS
    one(R, "dgrad_tail col0 without pos0", [] { return sonet_pooled_dgrad_tail_f32(P(1), P<int32_t>(2), P(3), 2, 384, 64, 64, 256, 1024, P<void>(4), P(5), P(6), P(7), nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, ST); });
    one(R, "dgrad_tail sraw without sums", [] { return sonet_pooled_dgrad_tail_f32(P(1), P<int32_t>(2), P(3), 2, 384, 64, 64, 256, 1024, P<void>(4), P(5), P(6), nullptr, nullptr, P(9), P(10), P(11), 1, P<void>(12), nullptr, ST); });
    one(R, "dgrad_tail C1 + C2 = 67", [] { return sonet_pooled_dgrad_tail_f32(P(1), P<int32_t>(2), P(3), 2, 128, 64, 3, 64, 1024, P<void>(4), P(5), P(6), P(7), P<int32_t>(8), nullptr, nullptr, nullptr, 0, nullptr, nullptr, ST); });
#endif
}

// ---- the decoder's up-convolutions ("@upconv" in argv): the two pack sizes and pack kernels, the forward, the input gradient, the weight
// gradient with its workspace size.  A size function's return value stands in the return-code column. ----
void report_value(const std::string &group, const std::string &cs, size_t v)
{
    if (wanted(group)) printf("%s\t%s\t%zu\t\t%s\n", group.c_str(), cs.c_str(), v, launch_log_take());
}

const int UP_CINS[] = {1, 15, 16, 17, 33, 128, 1024}, UP_COUTS[] = {16, 32, 48, 96, 1024};
const int UP_HW[] = {0, 1, 2, 5, 64, 65}, UP_BS[] = {0, 1, 3, 64};
const int UP_B_MOST = 0x7FFF0000 / (64 * 64);   // B H W = 0x7FFF0000 at 64 x 64: the most columns taken; one more cloud is refused

struct UpShape { int B, Cin, Cout, H, W; };
// pointers: number -1 = none, else that one is NULL (mis = 0) or mis bytes off its allocation
struct UpPtr {
    int which = -1, mis = 0;
    template <typename T = float> T *p(int i) const { return which == i ? (mis ? P<T>(i + 1, mis) : nullptr) : P<T>(i + 1); }
};
int up_fwd(const UpShape &s, const UpPtr &q = UpPtr()) {
    return sonet_upconv3x3_f32(q.p(0), q.p<void>(1), q.p(2), q.p(3), 1, q.p(4), s.B, s.Cin, s.Cout, s.H, s.W, nullptr, ST); }
int up_dgrad(const UpShape &s, const UpPtr &q = UpPtr()) {
    return sonet_upconv3x3_dgrad_f32(q.p(0), q.p<void>(1), q.p(2), s.B, s.Cin, s.Cout, s.H, s.W, ST); }
int up_wgrad(const UpShape &s, const UpPtr &q = UpPtr()) {
    return sonet_upconv3x3_wgrad_f32(q.p(0), q.p(1), q.p(2), q.p<void>(3), s.B, s.Cin, s.Cout, s.H, s.W, ST); }
int up_pack(const UpShape &s, const UpPtr &q = UpPtr()) { return sonet_upconv3x3_pack_f32(q.p(0), q.p<void>(1), s.Cin, s.Cout, ST); }
int up_dgrad_pack(const UpShape &s, const UpPtr &q = UpPtr()) { return sonet_upconv3x3_dgrad_pack_f32(q.p(0), q.p<void>(1), s.Cin, s.Cout, ST); }

struct UpEntry { const char *name; int (*call)(const UpShape &, const UpPtr &); int nptr; bool sized; };
const UpEntry UP_ENTRIES[] = {{"sonet_upconv3x3_pack_f32", up_pack, 2, false}, {"sonet_upconv3x3_dgrad_pack_f32", up_dgrad_pack, 2, false},
                              {"sonet_upconv3x3_f32", up_fwd, 5, true}, {"sonet_upconv3x3_dgrad_f32", up_dgrad, 3, true},
                              {"sonet_upconv3x3_wgrad_f32", up_wgrad, 4, true}};

void run_upconv()
{
    // the size functions
    for (int Cin : {0, 1, 15, 16, 17, 33, 128, 1024})
        for (int Cout : {0, 16, 32, 48, 96, 1024}) {
            const std::string cs = fmt("%d>%d", Cin, Cout);
            report_value("sonet_upconv3x3_pack_size", cs, sonet_upconv3x3_pack_size(Cin, Cout));
            report_value("sonet_upconv3x3_dgrad_pack_size", cs, sonet_upconv3x3_dgrad_pack_size(Cin, Cout));
        }
    auto ws = [](const std::string &group, const UpShape &s) {
        report_value(group, fmt("%dx%dx%d", s.B, s.H, s.W), sonet_upconv3x3_wgrad_ws_size(s.B, s.Cin, s.Cout, s.H, s.W));
    };
    for (const UpEntry &e : UP_ENTRIES) {
        // every channel pair at three sizes
        for (int Cin : UP_CINS)
            for (int Cout : UP_COUTS) {
                const std::string group = fmt("%s %d>%d", e.name, Cin, Cout);
                if (!wanted(group)) continue;
                if (!e.sized) { report(group, "pack", e.call({1, Cin, Cout, 1, 1}, UpPtr())); continue; }
                for (const UpShape &s : {UpShape{1, Cin, Cout, 1, 1}, UpShape{3, Cin, Cout, 2, 5}, UpShape{64, Cin, Cout, 64, 64}}) {
                    report(group, fmt("%dx%dx%d", s.B, s.H, s.W), e.call(s, UpPtr()));
                    if (e.call == up_wgrad) ws(fmt("sonet_upconv3x3_wgrad_ws_size %d>%d", Cin, Cout), s);
                }
            }
        const std::string R = fmt("%s refused", e.name);
        for (int i = 0; i < e.nptr; ++i)
            for (int mis : {0, 4, 8}) {
                UpPtr q;
                q.which = i; q.mis = mis;
                // (W = 4 on 16-byte aligned operands is the weight gradient's vector kernel: a pointer 8 bytes off takes the other one)
                if (wanted(R)) report(R, fmt(mis ? "pointer %d + %d" : "null pointer %d", i, mis), e.call({3, 17, 32, 2, 4}, q));
            }
        if (!wanted(R)) continue;
        report(R, "Cin=0", e.call({3, 0, 32, 2, 4}, UpPtr()));
        report(R, "Cout=0", e.call({3, 17, 0, 2, 4}, UpPtr()));
        report(R, "Cin=-1", e.call({3, -1, 32, 2, 4}, UpPtr()));
        if (!e.sized) continue;
        // every B, H, W at three channel pairs
        for (const UpShape &c : {UpShape{0, 17, 32, 0, 0}, UpShape{0, 128, 96, 0, 0}, UpShape{0, 1024, 1024, 0, 0}}) {
            const std::string group = fmt("%s sizes %d>%d", e.name, c.Cin, c.Cout);
            if (!wanted(group)) continue;
            for (int B : UP_BS)
                for (int H : UP_HW)
                    for (int W : UP_HW) {
                        const UpShape s{B, c.Cin, c.Cout, H, W};
                        report(group, fmt("%dx%dx%d", B, H, W), e.call(s, UpPtr()));
                        if (e.call == up_wgrad) ws(fmt("sonet_upconv3x3_wgrad_ws_size sizes %d>%d", c.Cin, c.Cout), s);
                    }
            for (int B : {UP_B_MOST, UP_B_MOST + 1, -1}) {
                const UpShape s{B, c.Cin, c.Cout, 64, 64};
                report(group, fmt("%dx64x64", B), e.call(s, UpPtr()));
                if (e.call == up_wgrad) ws(fmt("sonet_upconv3x3_wgrad_ws_size sizes %d>%d", c.Cin, c.Cout), s);
            }
        }
    }
    // the weight gradient's choices: 16-byte loads (W % 4 == 0, g and x 16-byte aligned) or element-wise; the slice count against the
    // 64 MiB workspace cap (16 x 1024 x 1024 floats = one slice exactly; a padded Cin above it: still one)
    const char *G = "sonet_upconv3x3_wgrad_f32 vec";
    for (int W : {4, 5, 8, 64})
        for (int which : {-1, 0, 1}) {
            UpPtr q;
            q.which = which; q.mis = 8;
            if (wanted(G)) report(G, fmt(which < 0 ? "W=%d aligned" : "W=%d pointer %d + 8", W, which), up_wgrad({3, 16, 32, 4, W}, q));
        }
    const char *C = "sonet_upconv3x3_wgrad_f32 workspace cap";
    for (const UpShape &s : {UpShape{64, 1024, 1024, 64, 64}, UpShape{1, 1024, 1024, 64, 64}, UpShape{64, 1025, 1024, 64, 64}, UpShape{64, 512, 1024, 64, 64},
                             UpShape{64, 1024, 512, 64, 64}, UpShape{64, 33, 32, 64, 64}}) {
        if (wanted(C)) report(C, fmt("%dx%dx%d %d>%d", s.B, s.H, s.W, s.Cin, s.Cout), up_wgrad(s));
        report_value("sonet_upconv3x3_wgrad_ws_size workspace cap", fmt("%dx%dx%d %d>%d", s.B, s.H, s.W, s.Cin, s.Cout),
                     sonet_upconv3x3_wgrad_ws_size(s.B, s.Cin, s.Cout, s.H, s.W));
    }
}

}  // namespace

int main(int argc, char **argv)
{
    g_argc = argc;
    g_argv = argv;
    for (int i = 1; i < argc; ++i)
        if (strcmp(argv[i], "@bn") == 0) {
            run_bn_bcl();
            run_bn_coeffs();
            run_bn_head();
            run_bn_pooled();
            return 0;
        } else if (strcmp(argv[i], "@upconv") == 0) {
            run_upconv();
            return 0;
        }
    run_pointmlp();
    run_x3();
    run_bf16();
    run_h3p();
    run_pointresnet();
    run_wgrad();
    return 0;
}
