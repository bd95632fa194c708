// hip_recorder.cpp -- a stand-in for the HIP runtime that records what the library's host side asks of it.
//
// Linked (never preloaded) with host-only objects of the launchers and tests/host/launch_record_main.cpp into a CPU
// program: no device, no libamdhip64.  Every runtime call the launchers make lands here and becomes one line on stdout:
//
//   L <kernel> <gx>,<gy>,<gz> <bx> <dynamic LDS bytes> <hash of the explicit arguments>
//   M <base>+<offset> <value> <bytes>          hipMemsetAsync (pointers are made up: base = address >> 40)
//   A <bytes> / F <base>                       hipMallocAsync / hipFreeAsync
//   S <kernel> <attribute> <value> d<device>   hipFuncSetAttribute
//
// The stream of the four stream-ordered calls is kept as well.  Once the driver has named the stream it hands to the entry
// points (rec_expect_stream), a call on any OTHER stream -- a launch or memset that would race on a side stream and be
// missing from a captured graph -- gets one more line in front of its usual one:
//
//   X <L|M|A|F> <kernel, or base+offset, or base> <stream>
//
// and rec_report_unlaunched prints, for every function the objects registered that was never launched,
//
//   U <kernel>
//
// Without an expectation there are no X lines, and U lines come only on request: the L, M, A, F and S lines are the same
// either way.
//
// The bytes of an argument come from the code-object metadata of the device assembly (kernel -> sizes of the explicit
// arguments, a table the build hands over through rec_load_args); hidden arguments are not looked at.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>
#include <map>
#include <string>
#include <vector>

namespace {

struct Dim3 { unsigned x, y, z; };
struct Kernel { std::string name; std::vector<int> sizes; bool known = false, launched = false; };

// (the registration constructors of the objects run before this file's statics would be built: function-local)
std::map<const void*, Kernel>& kernels() { static std::map<const void*, Kernel> m; return m; }
std::map<std::string, std::vector<int>>& arg_sizes() { static std::map<std::string, std::vector<int>> m; return m; }

struct Config { Dim3 grid, block; size_t lds; void* stream; };
std::vector<Config>& configs() { static std::vector<Config> v; return v; }

int g_device = 0, g_cus = 256, g_devices = 1;
uint64_t g_next_alloc = 0x7f0;
bool g_expecting = false;
void* g_expected = nullptr;

std::string short_name(const char* mangled) {
    int status = 0;
    char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
    std::string s = (status == 0 && d) ? d : mangled;
    std::free(d);
    // "void mr::k<true>(mr::P)" -> "k<true>": the argument list and the namespace say nothing the hash does not
    int depth = 0;
    size_t cut = s.size();
    for (size_t i = 0; i < s.size(); i++) {
        if (s[i] == '<') depth++;
        else if (s[i] == '>') depth--;
        else if (s[i] == '(' && depth == 0) { cut = i; break; }
    }
    s.resize(cut);
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    for (size_t at; (at = s.find("mr::")) != std::string::npos;) s.erase(at, 4);
    for (char& c : s) if (c == ' ') c = '_';
    return s;
}

Kernel& kernel_of(const void* f) {
    auto it = kernels().find(f);
    if (it == kernels().end()) {
        std::fprintf(stderr, "hip_recorder: launch of an unregistered function %p\n", f);
        std::abort();
    }
    Kernel& k = it->second;
    if (!k.known) {
        // the table's key is the mangled name; it was kept in `name` until first use
        auto s = arg_sizes().find(k.name);
        if (s == arg_sizes().end()) {
            std::fprintf(stderr, "hip_recorder: no argument sizes for %s\n", k.name.c_str());
            std::abort();
        }
        k.sizes = s->second;
        k.name = short_name(k.name.c_str());
        k.known = true;
    }
    return k;
}

void region(uintptr_t p, char* out, size_t n) {
    std::snprintf(out, n, "%llx+%llu", (unsigned long long)(p >> 40), (unsigned long long)(p & ((1ULL << 40) - 1)));
}

void on_stream(char kind, const char* what, void* stream) {
    if (g_expecting && stream != g_expected) std::printf("X %c %s %p\n", kind, what, stream);
}

}  // namespace

// ---- what the driver sets ------------------------------------------------------------------------------------------
extern "C" void rec_load_args(const char* path) {
    FILE* fh = std::fopen(path, "r");
    if (!fh) { std::fprintf(stderr, "hip_recorder: cannot read %s\n", path); std::abort(); }
    char name[4096];
    int n;
    while (std::fscanf(fh, "%4095s %d", name, &n) == 2) {
        std::vector<int> sizes(n);
        for (int i = 0; i < n; i++)
            if (std::fscanf(fh, "%d", &sizes[i]) != 1) std::abort();
        arg_sizes()[name] = sizes;
    }
    std::fclose(fh);
}
extern "C" void rec_set_device(int device, int devices) { g_device = device; g_devices = devices; }
extern "C" void rec_set_cus(int cus) { g_cus = cus; }
extern "C" void rec_begin(void) { g_next_alloc = 0x7f0; configs().clear(); }
extern "C" void rec_expect_stream(void* stream) { g_expecting = true; g_expected = stream; }
extern "C" void rec_report_unlaunched(void) {
    for (auto& kv : kernels())
        if (!kv.second.launched) std::printf("U %s\n", kv.second.known ? kv.second.name.c_str() : short_name(kv.second.name.c_str()).c_str());
}
// "K <mangled name> <name as the L lines show it>" for every kernel of the argument table: which source a name belongs to
extern "C" void rec_print_kernel_names(void) {
    for (auto& kv : arg_sizes()) std::printf("K %s %s\n", kv.first.c_str(), short_name(kv.first.c_str()).c_str());
}

// ---- the runtime's entry points ------------------------------------------------------------------------------------
extern "C" {

void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_function, char*, const char* device_name, unsigned, void*, void*, void*,
                           void*, int*) {
    kernels()[host_function].name = device_name;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}

int __hipPushCallConfiguration(Dim3 grid, Dim3 block, size_t lds, void* stream) {
    configs().push_back(Config{grid, block, lds, stream});
    return 0;
}
int __hipPopCallConfiguration(Dim3* grid, Dim3* block, size_t* lds, void** stream) {
    if (configs().empty()) std::abort();
    const Config c = configs().back();
    configs().pop_back();
    *grid = c.grid; *block = c.block; *lds = c.lds; *stream = c.stream;
    return 0;
}

int hipLaunchKernel(const void* f, Dim3 grid, Dim3 block, void** args, size_t lds, void* stream) {
    Kernel& k = kernel_of(f);
    k.launched = true;
    on_stream('L', k.name.c_str(), stream);
    uint64_t h = 0xcbf29ce484222325ULL;  // FNV-1a over the explicit arguments, in order
    for (size_t i = 0; i < k.sizes.size(); i++) {
        const unsigned char* b = static_cast<const unsigned char*>(args[i]);
        for (int j = 0; j < k.sizes[i]; j++) h = (h ^ b[j]) * 0x100000001b3ULL;
    }
    std::printf("L %s %u,%u,%u %u %zu %08x\n", k.name.c_str(), grid.x, grid.y, grid.z, block.x, lds, (unsigned)(h ^ (h >> 32)));
    if (block.y != 1 || block.z != 1) std::printf("  block %u,%u,%u\n", block.x, block.y, block.z);
    return 0;
}

int hipMemsetAsync(void* p, int value, size_t bytes, void* stream) {
    char r[64];
    region(reinterpret_cast<uintptr_t>(p), r, sizeof r);
    on_stream('M', r, stream);
    std::printf("M %s %d %zu\n", r, value, bytes);
    return 0;
}

int hipMallocAsync(void** p, size_t bytes, void* stream) {
    char r[32];
    std::snprintf(r, sizeof r, "%llx", (unsigned long long)g_next_alloc);
    on_stream('A', r, stream);
    *p = reinterpret_cast<void*>(static_cast<uintptr_t>(g_next_alloc++) << 40);
    std::printf("A %zu\n", bytes);
    return 0;
}
int hipFreeAsync(void* p, void* stream) {
    char r[32];
    std::snprintf(r, sizeof r, "%llx", (unsigned long long)(reinterpret_cast<uintptr_t>(p) >> 40));
    on_stream('F', r, stream);
    std::printf("F %llx\n", (unsigned long long)(reinterpret_cast<uintptr_t>(p) >> 40));
    return 0;
}

int hipFuncSetAttribute(const void* f, int attribute, int value) {
    std::printf("S %s %d %d d%d\n", kernel_of(f).name.c_str(), attribute, value, g_device);
    return 0;
}

int hipGetDevice(int* device) { *device = g_device; return 0; }
int hipGetDeviceCount(int* n) { *n = g_devices; return 0; }
int hipDeviceGetAttribute(int* value, int, int) { *value = g_cus; return 0; }
int hipGetLastError(void) { return 0; }

// named by the objects, not reached by the recorded entry points
int hipDeviceSynchronize(void) { std::abort(); }
int hipMemcpyFromSymbol(void*, const void*, size_t, size_t, int) { std::abort(); }
int hipMemcpyToSymbol(const void*, const void*, size_t, size_t, int) { std::abort(); }
int hipGetDevicePropertiesR0600(void*, int) { std::abort(); }

}  // extern "C"
