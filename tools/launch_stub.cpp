// launch_stub.cpp -- stand-in for the HIP runtime behind tools/launch_log.py: the dozen runtime symbols the host halves of
// so-net_amd/csrc/*.hip need, recording every kernel launch (name, grid, block, dynamic LDS) instead of running it.  Plain C++, no GPU.
// The CU count hipDeviceGetAttribute reports comes from LAUNCH_LOG_CUS (default 256; "fail": the query fails).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

namespace {
struct Dim3 { unsigned x, y, z; };
struct Config { Dim3 grid, block; size_t lds; void *stream; };

std::map<const void *, std::string> &names() { static std::map<const void *, std::string> m; return m; }
std::string g_log;
Config g_cfg;
}  // namespace

extern "C" {

// what was launched since the last call, one " name gx,gy,gz block lds" item per launch
const char *launch_log_take(void)
{
    static std::string out;
    out.swap(g_log);
    g_log.clear();
    return out.c_str();
}

void **__hipRegisterFatBinary(const void *) { static void *handle = nullptr; return &handle; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *)
{
    names()[host_fn] = device_name;
}
void __hipRegisterVar(void **, void *, char *, char *, int, size_t, int, int) {}
void __hipRegisterManagedVar(void **, void **, void *, const char *, size_t, unsigned) {}

int __hipPushCallConfiguration(Dim3 grid, Dim3 block, size_t lds, void *stream)
{
    g_cfg = Config{grid, block, lds, stream};
    return 0;
}
int __hipPopCallConfiguration(Dim3 *grid, Dim3 *block, size_t *lds, void **stream)
{
    *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *stream = g_cfg.stream;
    return 0;
}
int hipLaunchKernel(const void *fn, Dim3 grid, Dim3 block, void **, size_t lds, void *)
{
    const auto it = names().find(fn);
    char buf[96];
    snprintf(buf, sizeof buf, " %u,%u,%u %u,%u,%u %zu", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    g_log += ' ';
    g_log += it == names().end() ? "?" : it->second.c_str();
    g_log += buf;
    return 0;
}
int hipGetLastError(void) { return 0; }
const char *hipGetErrorString(int) { return "stub"; }
int hipGetDevice(int *dev) { *dev = 0; return 0; }
int hipDeviceGetAttribute(int *value, int, int)
{
    const char *e = getenv("LAUNCH_LOG_CUS");
    if (e && strcmp(e, "fail") == 0) return 1;
    *value = e ? atoi(e) : 256;
    return 0;
}
int hipMemsetAsync(void *, int, size_t, void *) { g_log += " memset"; return 0; }
int hipFuncSetAttribute(const void *, int, int) { return 0; }
int hipGetDevicePropertiesR0600(void *, int) { return 1; }
int hipMemcpyFromSymbol(void *, const void *, size_t, size_t, int) { return 1; }

}  // extern "C"
