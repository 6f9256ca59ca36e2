// Stand-in for libamdhip64 in the CPU sanitizer build of the library's HOST half (tests/test_sanitizers.py): "device" memory is
// calloc'd host memory (so every hipMemcpy / hipMemset of the launch logic is bounds-checked by AddressSanitizer), streams and events
// are dummy objects, kernel launches do nothing.  Only what csrc/almpc_api.hip links against.  Test infrastructure, never shipped.
// fake_hip_trace_to(path): every launch from then on appends one line to `path`: the launching stream's creation ordinal (0: the null
// stream), the demangled kernel name, grid, block and dynamic LDS bytes.
// The byte size of every hipMalloc and of every hipHostMalloc that succeeded is kept; fake_hip_dump_allocs(path) writes both lists,
// sorted (tests/golden/host_alloc_sizes.txt).  fake_hip_fail_alloc_at(k): the k-th hipMalloc / hipHostMalloc from now on returns
// hipErrorOutOfMemory, once (k = 0: none); returns what was left of the last such count (0: it has fired, or none was set).
// fake_hip_record_uploads(1) (off by default): every host-to-device hipMemcpy(Async) is kept as (bytes, 64-bit FNV-1a of the payload) and
// every hipMemset(Async) as (bytes, value); fake_hip_print_uploads(f) writes what was kept since the last call, sorted (f null:
// writes nothing), and forgets it.
// fake_hip_trace_calls(1) (off by default): the trace also gets one line, in call order and with the stream's ordinal in front, for
// every hipMemsetAsync (bytes, value), hipMemcpyAsync (kind, bytes), hipEventRecord, hipStreamSynchronize and hipEventSynchronize (the
// stream the event was last recorded on): between the launches of a loop their order is part of what the host does.
#include <hip/hip_runtime_api.h>

#include <cxxabi.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace {
struct Cfg { dim3 grid, block; size_t shmem; hipStream_t stream; };
thread_local Cfg g_cfg;
// (function-local: the library's module constructor registers its kernels before this file's globals would be constructed)
struct State {
    std::mutex mu;   // (a group designs its handles on host threads of their own)
    long launches = 0;
    int streams = 0;
    std::map<const void*, int> stream_ord;
    std::map<const void*, std::string> kernel_name;
    FILE* trace = nullptr;
    std::vector<size_t> device_bytes, pinned_bytes;
    int fail_in = 0;
    bool record_uploads = false;
    bool trace_calls = false;
    std::map<const void*, int> event_ord;   // the ordinal of the stream an event was last recorded on
    std::vector<std::pair<size_t, unsigned long long>> copies, sets;
};
State& S() { static State s; return s; }

int ord_of(State& g, hipStream_t st) {
    const auto o = g.stream_ord.find(st);
    return st && o != g.stream_ord.end() ? o->second : 0;
}
// one line of the ordered trace for a call that is no launch (fake_hip_trace_calls)
void trace_call(int ord, const char* what, const char* detail = "") {
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    if (g.trace && g.trace_calls) std::fprintf(g.trace, "%d %s%s\n", ord, what, detail);
}
void trace_call(hipStream_t st, const char* what, const char* detail = "") {
    int ord;
    { State& g = S(); std::lock_guard<std::mutex> l(g.mu); ord = ord_of(g, st); }
    trace_call(ord, what, detail);
}

hipError_t fake_alloc(void** p, size_t n, std::vector<size_t> State::*sizes) {
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    *p = nullptr;
    if (g.fail_in > 0 && --g.fail_in == 0) return hipErrorOutOfMemory;
    *p = std::calloc(n ? n : 1, 1);
    if (!*p) return hipErrorOutOfMemory;
    (g.*sizes).push_back(n);
    return hipSuccess;
}

hipError_t fake_copy(void* d, const void* s, size_t n, hipMemcpyKind kind) {
    std::memmove(d, s, n);
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    if (g.record_uploads && kind == hipMemcpyHostToDevice) {
        unsigned long long hash = 14695981039346656037ull;
        for (size_t i = 0; i < n; ++i) hash = (hash ^ static_cast<const unsigned char*>(s)[i]) * 1099511628211ull;
        g.copies.emplace_back(n, hash);
    }
    return hipSuccess;
}
hipError_t fake_set(void* d, int v, size_t n) {
    std::memset(d, v, n);
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    if (g.record_uploads) g.sets.emplace_back(n, (unsigned long long)(unsigned char)v);
    return hipSuccess;
}
}

extern "C" {
long fake_hip_launch_count() { State& g = S(); std::lock_guard<std::mutex> l(g.mu); return g.launches; }
int fake_hip_trace_to(const char* path) {
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    if (g.trace) std::fclose(g.trace);
    g.trace = std::fopen(path, "w");
    return g.trace ? 0 : 1;
}
void fake_hip_trace_close() {
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    if (g.trace) std::fclose(g.trace);
    g.trace = nullptr;
}
int fake_hip_fail_alloc_at(int k) {
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    const int left = g.fail_in;
    g.fail_in = k;
    return left;
}
int fake_hip_dump_allocs(const char* path) {
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    FILE* f = std::fopen(path, "w");
    if (!f) return 1;
    for (auto* v : {&g.device_bytes, &g.pinned_bytes}) {
        std::sort(v->begin(), v->end());
        std::fprintf(f, "%s %zu\n", v == &g.device_bytes ? "hipMalloc" : "hipHostMalloc", v->size());
        for (size_t n : *v) std::fprintf(f, "%zu\n", n);
    }
    return std::fclose(f) ? 1 : 0;
}

void fake_hip_trace_calls(int on) { State& g = S(); std::lock_guard<std::mutex> l(g.mu); g.trace_calls = on != 0; }
void fake_hip_record_uploads(int on) { State& g = S(); std::lock_guard<std::mutex> l(g.mu); g.record_uploads = on != 0; }
void fake_hip_print_uploads(FILE* f) {
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    std::sort(g.copies.begin(), g.copies.end());
    std::sort(g.sets.begin(), g.sets.end());
    for (const auto& c : g.copies) if (f) std::fprintf(f, "  upload %zu %016llx\n", c.first, c.second);
    for (const auto& c : g.sets) if (f) std::fprintf(f, "  memset %zu %llu\n", c.first, c.second);
    g.copies.clear(); g.sets.clear();
}

hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t a, int) {
    *v = (a == hipDeviceAttributeMultiprocessorCount) ? 256 : 0;
    return hipSuccess;
}
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int) {
    std::memset(p, 0, sizeof(*p));
    p->multiProcessorCount = 256;
    std::strcpy(p->gcnArchName, "gfx950");
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "fake HIP runtime"; }
hipError_t hipGetLastError() { return hipSuccess; }

hipError_t hipMalloc(void** p, size_t n) { return fake_alloc(p, n, &State::device_bytes); }
hipError_t hipFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return fake_alloc(p, n, &State::pinned_bytes); }
hipError_t hipHostFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k) { return fake_copy(d, s, n, k); }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st) {
    char detail[64];
    std::snprintf(detail, sizeof detail, " kind %d bytes %zu", (int)k, n);
    trace_call(st, "hipMemcpyAsync", detail);
    return fake_copy(d, s, n, k);
}
hipError_t hipMemset(void* d, int v, size_t n) { return fake_set(d, v, n); }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) {
    char detail[64];
    std::snprintf(detail, sizeof detail, " bytes %zu value %d", n, v);
    trace_call(st, "hipMemsetAsync", detail);
    return fake_set(d, v, n);
}

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    *s = reinterpret_cast<hipStream_t>(std::malloc(8));
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    g.stream_ord[*s] = ++g.streams;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    { State& g = S(); std::lock_guard<std::mutex> l(g.mu); g.stream_ord.erase(s); }
    std::free(s);
    return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t st) { trace_call(st, "hipStreamSynchronize"); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = reinterpret_cast<hipEvent_t>(std::malloc(8)); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) {
    { State& g = S(); std::lock_guard<std::mutex> l(g.mu); g.event_ord.erase(e); }
    std::free(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) {
    { State& g = S(); std::lock_guard<std::mutex> l(g.mu); g.event_ord[e] = ord_of(g, st); }
    trace_call(st, "hipEventRecord");
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) {
    int ord = 0;
    { State& g = S(); std::lock_guard<std::mutex> l(g.mu); const auto o = g.event_ord.find(e); if (o != g.event_ord.end()) ord = o->second; }
    trace_call(ord, "hipEventSynchronize");
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.01f; return hipSuccess; }

hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t sh, hipStream_t st) {
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    ++g.launches;
    if (g.trace) {
        const auto k = g.kernel_name.find(f);
        std::fprintf(g.trace, "%d %s grid %u %u %u block %u %u %u lds %zu\n", ord_of(g, st),
                     k != g.kernel_name.end() ? k->second.c_str() : "?", grid.x, grid.y, grid.z, block.x, block.y, block.z, sh);
    }
    return hipSuccess;
}

// what hip-clang's host stubs and module constructor call
void** __hipRegisterFatBinary(const void*) { static void* h[1]; return h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    int ok = -1;
    char* d = abi::__cxa_demangle(device_name, nullptr, nullptr, &ok);
    std::string name = ok == 0 && d ? d : device_name;
    std::free(d);
    if (name.compare(0, 5, "void ") == 0) name.erase(0, 5);   // (return type of a template)
    if (!name.empty() && name.back() == ')') {                 // (parameter list)
        int depth = 0;
        for (size_t i = name.size(); i-- > 0;) {
            depth += name[i] == ')' ? 1 : (name[i] == '(' ? -1 : 0);
            if (depth == 0) { name.erase(i); break; }
        }
    }
    State& g = S(); std::lock_guard<std::mutex> l(g.mu);
    g.kernel_name[host_fn] = name;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t st) { g_cfg = {g, b, sh, st}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* st) { *g = g_cfg.grid; *b = g_cfg.block; *sh = g_cfg.shmem; *st = g_cfg.stream; return hipSuccess; }
}
