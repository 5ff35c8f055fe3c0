// launch_driver.cpp -- the sweep of tools/launch_log.py: calls the C ABI of the layer launchers with fake non-null pointers (nothing is
// dereferenced on the host) against tools/launch_stub.cpp and prints one line per case:
//   group \t case \t return code \t sonet_last_error() when refused \t the launches the stub recorded
// group = entry point, optional features and channel pair; case = B x L and whatever else varies inside the group.
// argv[1..]: group prefixes to run (none: all).  Built with -DSONET_VARIANTS for the variants library's extra entry points.
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
    if (g_argc <= 1) return true;
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

}  // namespace

int main(int argc, char **argv)
{
    g_argc = argc;
    g_argv = argv;
    run_pointmlp();
    run_x3();
    run_bf16();
    run_h3p();
    run_pointresnet();
    run_wgrad();
    return 0;
}
