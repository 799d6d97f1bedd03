// hip_stub.cpp — the HIP runtime on the CPU, for running the library's host code under sanitizers (tests/test_host_sanitizers.py).
// "Device" memory is exactly-sized, zero-filled heap memory, so a sanitizer's red zones sit at the documented extent of every
// buffer; copies and memsets are checked against the registry of live ranges and then executed at once; streams and events
// are small heap objects (use after destroy is visible); launches run nothing and are logged with their configuration.
// A breach counts as a violation and prints one line; it does not trap.
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cxxabi.h>
#include <dlfcn.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "hip_stub.h"

namespace {

struct Range {
  size_t bytes;
  int kind;
  void *backing;   // what free() gets (nullptr: registered memory, the caller's)
  size_t mapped;   // > 0: `backing` is a mapping of this many bytes (large blocks, below), released with munmap
};

struct Stream { unsigned magic; };
struct Event { unsigned magic; long records; };
constexpr unsigned kStreamMagic = 0x5354524du, kEventMagic = 0x45564e54u;
constexpr size_t kMaxLds = 160 * 1024;
constexpr size_t kMapFrom = 1 << 20;

std::mutex g_mu;
std::map<uintptr_t, Range> g_ranges;
// filled by the static constructors of the library's objects, which may run before this file's: built on first use, never destroyed
std::unordered_map<const void *, std::string> &kernels() {
  static auto *m = new std::unordered_map<const void *, std::string>();
  return *m;
}
std::vector<StubLaunch> g_log;
// kernels whose dynamic-LDS limit was raised (hipFuncSetAttribute) and that were not launched since: a launcher raises the limit
// right in front of its launch, so an entry that stays is a launch that never arrived
std::unordered_map<const void *, long> g_raised;
std::unordered_map<void *, long> g_transfers;
std::unordered_map<std::string, long> g_calls;
long g_transfers_total = 0, g_violations = 0, g_streams = 0, g_events = 0;
std::string g_fail_api;
long g_fail_n = 0;
bool g_fail_fired = false;

// ---- the ordering trace (HIP_STUB_TRACE): one line per launch, event record / wait / query and asynchronous copy or memset,
// in issue order.  Streams and events are numbered in order of first appearance since the last stub_trace_take(true), pointers
// into "device" or pinned memory are printed as offset/size of their range: the text is the same from run to run.
bool trace_on() { static const bool on = getenv("HIP_STUB_TRACE") != nullptr; return on; }
std::vector<std::string> g_trace;
std::unordered_map<const void *, int> g_stream_idx, g_event_idx;
std::map<uintptr_t, Range>::iterator owner(const void *p);

std::string obj_name(std::unordered_map<const void *, int> &idx, char tag, const void *p) {   // g_mu held
  if (!p) return std::string(1, tag) + "-";
  auto it = idx.emplace(p, (int)idx.size()).first;
  return tag + std::to_string(it->second);
}
std::string stream_name(hipStream_t s) { return obj_name(g_stream_idx, 's', s); }
std::string event_name(hipEvent_t e) { return obj_name(g_event_idx, 'e', e); }
std::string ptr_name(const void *p) {   // g_mu held
  if (!p) return "0";
  auto it = owner(p);
  if (it == g_ranges.end()) return "?";
  return std::to_string(reinterpret_cast<uintptr_t>(p) - it->first) + "/" + std::to_string(it->second.bytes);
}
// "void ns::kernel<1, 2>(ns::Params)" -> the name with its template arguments, and the parameter list
void split_signature(const std::string &mangled, std::string *name, std::string *params) {
  int status = 1;
  char *d = abi::__cxa_demangle(mangled.c_str(), nullptr, nullptr, &status);
  std::string full = status == 0 && d ? d : mangled;
  free(d);
  *name = full;
  params->clear();
  if (full.empty() || full.back() != ')') return;
  int depth = 0;
  for (size_t i = full.size(); i-- > 0;) {
    if (full[i] == ')') ++depth;
    else if (full[i] == '(' && --depth == 0) { *name = full.substr(0, i); *params = full.substr(i); break; }
  }
  if (name->compare(0, 5, "void ") == 0) name->erase(0, 5);
}
// the library's spfe::ConvParams (csrc/spfe_kernels.h) as the convolution kernels receive it by value: the trace prints the
// fields a launch configuration does not show (a changed layout there shows as a changed trace)
struct ConvParamsView {
  const void *in; int in_stride, in_choff; const void *wpack, *bias; void *out; int out_stride, out_choff, cout_real;
  int B, H, W, tiles_x, tiles_y, nblk, num_cus;
  const void *img, *w1a, *b1a; int *tile_ctr; int item_lo, item_hi;
};

const char *kind_name(int k) { return k == STUB_DEVICE ? "device" : k == STUB_PINNED ? "pinned" : "registered"; }

// (g_mu held) the live range that holds address p, or end()
std::map<uintptr_t, Range>::iterator owner(const void *p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = g_ranges.upper_bound(a);
  if (it == g_ranges.begin()) return g_ranges.end();
  --it;
  return a < it->first + it->second.bytes || (it->second.bytes == 0 && a == it->first) ? it : g_ranges.end();
}

void violation(const char *api, const void *p, size_t n, const char *what) {   // g_mu held
  ++g_violations;
  auto it = owner(p);
  if (it != g_ranges.end())
    fprintf(stderr, "stub violation: %s %p + %zu: %s (in %s range %p + %zu)\n", api, p, n, what, kind_name(it->second.kind),
            reinterpret_cast<void *>(it->first), it->second.bytes);
  else
    fprintf(stderr, "stub violation: %s %p + %zu: %s (in no live range)\n", api, p, n, what);
}

// (g_mu held) counts the call; true when the armed failure falls on it
bool enter(const char *api) {
  ++g_calls[api];
  if (g_fail_n > 0 && g_fail_api == api && --g_fail_n == 0) {
    g_fail_fired = true;
    return true;
  }
  return false;
}

// (g_mu held) [p, p + n) must lie inside one live range of kind STUB_DEVICE
bool check_device(const char *api, const void *p, size_t n) {
  if (n == 0) return true;
  auto it = owner(p);
  if (it == g_ranges.end() || it->second.kind != STUB_DEVICE) {
    violation(api, p, n, "device side is not device memory");
    return false;
  }
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (a + n > it->first + it->second.bytes) {
    violation(api, p, n, "device side leaves its range");
    return false;
  }
  return true;
}

// (g_mu held) a host side inside a pinned or registered range must stay inside it; ordinary host memory is the sanitizer's
bool check_host(const char *api, const void *p, size_t n) {
  if (n == 0) return true;
  auto it = owner(p);
  if (it == g_ranges.end()) return true;
  if (it->second.kind == STUB_DEVICE) {
    violation(api, p, n, "host side is device memory");
    return false;
  }
  if (reinterpret_cast<uintptr_t>(p) + n > it->first + it->second.bytes) {
    violation(api, p, n, "host side leaves its range");
    return false;
  }
  return true;
}

bool check_copy(const char *api, void *dst, const void *src, size_t n, hipMemcpyKind kind) {
  switch (kind) {
    case hipMemcpyHostToDevice: return check_device(api, dst, n) & check_host(api, src, n);
    case hipMemcpyDeviceToHost: return check_host(api, dst, n) & check_device(api, src, n);
    case hipMemcpyDeviceToDevice: return check_device(api, dst, n) & check_device(api, src, n);
    case hipMemcpyHostToHost: return check_host(api, dst, n) & check_host(api, src, n);
    default: {   // hipMemcpyDefault: each side by what the registry says it is
      bool ok = true;
      for (const void *p : {static_cast<const void *>(dst), src}) {
        auto it = owner(p);
        ok &= it != g_ranges.end() && it->second.kind == STUB_DEVICE ? check_device(api, p, n) : check_host(api, p, n);
      }
      return ok;
    }
  }
}

bool stream_ok(const char *api, hipStream_t s) {   // g_mu held; reads the object: a destroyed stream is the sanitizer's
  if (!s) return true;
  if (reinterpret_cast<Stream *>(s)->magic != kStreamMagic) {
    violation(api, s, 0, "not a live stream");
    return false;
  }
  return true;
}
bool event_ok(const char *api, hipEvent_t e) {
  if (!e || reinterpret_cast<Event *>(e)->magic != kEventMagic) {
    violation(api, e, 0, "not a live event");
    return false;
  }
  return true;
}

void transfer(hipStream_t s) {
  ++g_transfers[s];
  ++g_transfers_total;
}

hipError_t alloc(const char *api, void **p, size_t bytes, int kind) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter(api)) { if (p) *p = nullptr; return hipErrorOutOfMemory; }
  if (!p) return hipErrorInvalidValue;
  *p = nullptr;
  if (bytes == 0) return hipSuccess;
  // Small blocks: calloc, exactly `bytes`, so the sanitizer's red zone starts behind them.  Blocks of a megabyte and more: a
  // mapping of their own whose last page is inaccessible, the block ending (to 16 bytes) against it.  Its pages are zero
  // without being touched, which a frame-sized calloc is not: a create of a large frame spends its time there otherwise.
  if (bytes >= kMapFrom) {
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
    void *base = mmap(nullptr, body + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == MAP_FAILED) return hipErrorOutOfMemory;
    mprotect(static_cast<char *>(base) + body, page, PROT_NONE);
    void *q = static_cast<char *>(base) + (body - bytes) / 16 * 16;
    g_ranges[reinterpret_cast<uintptr_t>(q)] = Range{bytes, kind, base, body + page};
    *p = q;
    return hipSuccess;
  }
  void *q = calloc(1, bytes);
  if (!q) return hipErrorOutOfMemory;
  g_ranges[reinterpret_cast<uintptr_t>(q)] = Range{bytes, kind, q, 0};
  *p = q;
  return hipSuccess;
}

hipError_t release(const char *api, void *p, int kind_a, int kind_b) {
  void *backing = nullptr;
  size_t mapped = 0;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (enter(api)) return hipErrorInvalidValue;
    if (!p) return hipSuccess;
    auto it = g_ranges.find(reinterpret_cast<uintptr_t>(p));
    if (it == g_ranges.end() || (it->second.kind != kind_a && it->second.kind != kind_b)) {
      violation(api, p, 0, "unknown or already freed pointer");
      return hipErrorInvalidValue;
    }
    backing = it->second.backing;
    mapped = it->second.mapped;
    g_ranges.erase(it);
  }
  if (mapped) munmap(backing, mapped);
  else free(backing);
  return hipSuccess;
}

hipError_t launch(const char *api, const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, void **args, hipEvent_t start, hipEvent_t stop) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter(api)) return hipErrorInvalidValue;
  bool ok = stream_ok(api, s);
  if (grid.x == 0 || grid.y == 0 || grid.z == 0 || block.x == 0 || block.y == 0 || block.z == 0) {
    violation(api, fn, 0, "zero grid or block dimension");
    ok = false;
  }
  if ((size_t)block.x * block.y * block.z > 1024) { violation(api, fn, (size_t)block.x * block.y * block.z, "block above 1024 threads"); ok = false; }
  if (lds > kMaxLds) { violation(api, fn, lds, "dynamic LDS above 160 KB"); ok = false; }
  g_raised.erase(fn);
  auto it = kernels().find(fn);
  static const bool echo = getenv("HIP_STUB_ECHO_LAUNCHES") != nullptr;   // diagnostic: one line a launch
  if (echo) fprintf(stderr, "stub launch: %s grid %u %u %u block %u lds %zu\n", it == kernels().end() ? "?" : it->second.c_str(), grid.x, grid.y, grid.z, block.x, lds);
  g_log.push_back(StubLaunch{it == kernels().end() ? "?" : it->second, {grid.x, grid.y, grid.z}, {block.x, block.y, block.z}, lds, s});
  const bool probe = it != kernels().end() && it->second.find("queue_probe_spin_kernel") != std::string::npos;
  // HIP_STUB_EMULATE_PROBE: the queue probe's spin (spfe_schedule.hip: ticks, stamp) writes its two device-clock stamps, the same
  // interval on every stream, so that the spins of two streams overlap: "a free hardware queue"
  if (probe && args && getenv("HIP_STUB_EMULATE_PROBE")) {
    const long long ticks = *static_cast<long long *>(args[0]);
    long long *stamp = *static_cast<long long **>(args[1]);
    stamp[0] = 1000;
    stamp[1] = 1000 + ticks;
  }
  if (trace_on()) {
    std::string name = "?", params, line;
    if (it != kernels().end()) split_signature(it->second, &name, &params);
    char buf[160];
    snprintf(buf, sizeof(buf), " grid %u %u %u block %u %u %u lds %zu ", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    line = "launch " + name + buf + stream_name(s);
    if (start) line += " start " + event_name(start);
    if (stop) line += " stop " + event_name(stop);
    if (args && params == "(spfe::ConvParams)") {
      const ConvParamsView &p = *static_cast<const ConvParamsView *>(args[0]);
      snprintf(buf, sizeof(buf), " B %d H %d W %d tiles %d %d nblk %d cus %d items %d %d out_stride %d", p.B, p.H, p.W, p.tiles_x, p.tiles_y,
               p.nblk, p.num_cus, p.item_lo, p.item_hi, p.out_stride);
      line += buf;
      line += " in " + ptr_name(p.in) + " w " + ptr_name(p.wpack) + " out " + ptr_name(p.out) + " img " + ptr_name(p.img) + " ctr " + ptr_name(p.tile_ctr);
    }
    g_trace.push_back(line);
  }
  return ok ? hipSuccess : hipErrorInvalidConfiguration;
}
void trace_call(const char *api, hipStream_t s, hipEvent_t e, const std::string &more = std::string()) {   // g_mu held
  if (!trace_on()) return;
  std::string line = api;
  if (strcmp(api, "hipEventQuery")) line += " " + stream_name(s);   // (the one call here that names no stream)
  if (e) line += " " + event_name(e);
  g_trace.push_back(more.empty() ? line : line + " " + more);
}

struct CallConfig { dim3 grid, block; size_t lds; hipStream_t stream; };
thread_local std::vector<CallConfig> t_cfg;
thread_local int t_device = 0;
thread_local hipError_t t_last_error = hipSuccess;   // what hipGetLastError answers and clears: a failed launch is read there

hipError_t launch_noted(const char *api, const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, void **args = nullptr,
                        hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
  const hipError_t e = launch(api, fn, grid, block, lds, s, args, start, stop);
  if (e != hipSuccess) t_last_error = e;
  return e;
}

}  // namespace

// ---- hooks -------------------------------------------------------------------------------------------------------------
long stub_launch_count() { std::lock_guard<std::mutex> lk(g_mu); return (long)g_log.size(); }
std::vector<StubLaunch> stub_launches() { std::lock_guard<std::mutex> lk(g_mu); return g_log; }
void stub_clear_launches() { std::lock_guard<std::mutex> lk(g_mu); g_log.clear(); }
long stub_live_ranges() { std::lock_guard<std::mutex> lk(g_mu); return (long)g_ranges.size(); }
long stub_live_ranges_of(int kind) {
  std::lock_guard<std::mutex> lk(g_mu);
  long n = 0;
  for (auto &r : g_ranges) n += r.second.kind == kind;
  return n;
}
long stub_raised_not_launched() {
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto &r : g_raised) {
    auto it = kernels().find(r.first);
    fprintf(stderr, "stub: LDS limit raised but never launched: %s\n", it == kernels().end() ? "?" : it->second.c_str());
  }
  return (long)g_raised.size();
}
long stub_live_streams() { std::lock_guard<std::mutex> lk(g_mu); return g_streams; }
long stub_live_events() { std::lock_guard<std::mutex> lk(g_mu); return g_events; }
long stub_violations() { std::lock_guard<std::mutex> lk(g_mu); return g_violations; }
void stub_reset_violations() { std::lock_guard<std::mutex> lk(g_mu); g_violations = 0; }
long stub_transfers_on(void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_transfers.find(stream);
  return it == g_transfers.end() ? 0 : it->second;
}
long stub_transfers_total() { std::lock_guard<std::mutex> lk(g_mu); return g_transfers_total; }
long stub_calls(const char *api) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_calls.find(api);
  return it == g_calls.end() ? 0 : it->second;
}
void stub_fail_after(const char *api, long n) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_fail_api = api ? api : "";
  g_fail_n = n;
  g_fail_fired = false;
}
bool stub_fail_fired() { std::lock_guard<std::mutex> lk(g_mu); return g_fail_fired; }
std::string stub_trace_take(bool restart_numbering) {
  std::lock_guard<std::mutex> lk(g_mu);
  std::string text;
  for (const std::string &l : g_trace) { text += l; text += '\n'; }
  g_trace.clear();
  if (restart_numbering) { g_stream_idx.clear(); g_event_idx.clear(); }
  return text;
}
void *stub_malloc_in_block(size_t bytes, size_t slack) {
  void *q = calloc(1, bytes + slack);
  std::lock_guard<std::mutex> lk(g_mu);
  g_ranges[reinterpret_cast<uintptr_t>(q)] = Range{bytes, STUB_DEVICE, q, 0};
  return q;
}

// RCCL is absent under the stub, whatever the machine has installed: the real library would bring the real HIP runtime into
// the process.  The request is handed on under a name that does not exist, so that dlerror() reads as it would.
extern "C" void *dlopen(const char *name, int flags) {
  using dlopen_fn = void *(*)(const char *, int);
  static const dlopen_fn next = reinterpret_cast<dlopen_fn>(dlsym(RTLD_NEXT, "dlopen"));
  if (!next) return nullptr;
  if (name && strstr(name, "rccl")) return next("librccl-is-absent-under-the-stub.so", flags);
  return next(name, flags);
}

// ---- the runtime -------------------------------------------------------------------------------------------------------
extern "C" {

hipError_t hipMalloc(void **p, size_t bytes) { return alloc("hipMalloc", p, bytes, STUB_DEVICE); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return alloc("hipHostMalloc", p, bytes, STUB_PINNED); }
hipError_t hipFree(void *p) { return release("hipFree", p, STUB_DEVICE, STUB_DEVICE); }
hipError_t hipHostFree(void *p) { return release("hipHostFree", p, STUB_PINNED, STUB_PINNED); }

hipError_t hipHostRegister(void *p, size_t bytes, unsigned) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipHostRegister")) return hipErrorOutOfMemory;
  if (!p || bytes == 0) return hipErrorInvalidValue;
  if (owner(p) != g_ranges.end()) {
    violation("hipHostRegister", p, bytes, "memory is already in a live range");
    return hipErrorHostMemoryAlreadyRegistered;
  }
  // the whole block must be the caller's: touch its two ends (the sanitizer's part of this check)
  volatile unsigned char sink = static_cast<unsigned char *>(p)[0];
  sink = static_cast<unsigned char *>(p)[bytes - 1];
  (void)sink;
  g_ranges[reinterpret_cast<uintptr_t>(p)] = Range{bytes, STUB_REGISTERED, nullptr, 0};
  return hipSuccess;
}
hipError_t hipHostUnregister(void *p) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipHostUnregister")) return hipErrorInvalidValue;
  auto it = g_ranges.find(reinterpret_cast<uintptr_t>(p));
  if (it == g_ranges.end() || it->second.kind != STUB_REGISTERED) {
    violation("hipHostUnregister", p, 0, "not a registered block");
    return hipErrorHostMemoryNotRegistered;
  }
  g_ranges.erase(it);
  return hipSuccess;
}

static hipError_t do_copy(const char *api, void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (enter(api)) return hipErrorInvalidValue;
    if (!stream_ok(api, s)) return hipErrorInvalidHandle;
    transfer(s);
    if (!strcmp(api, "hipMemcpyAsync")) trace_call(api, s, nullptr, std::to_string(n) + " bytes kind " + std::to_string((int)kind));
    if (!check_copy(api, dst, src, n, kind)) return hipErrorInvalidValue;
  }
  if (n) memmove(dst, src, n);
  return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind) { return do_copy("hipMemcpy", dst, src, n, kind, nullptr); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s) {
  return do_copy("hipMemcpyAsync", dst, src, n, kind, s);
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                            hipMemcpyKind kind, hipStream_t s) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (enter("hipMemcpy2DAsync")) return hipErrorInvalidValue;
    if (!stream_ok("hipMemcpy2DAsync", s)) return hipErrorInvalidHandle;
    transfer(s);
    trace_call("hipMemcpy2DAsync", s, nullptr, std::to_string(width) + " x " + std::to_string(height) + " bytes kind " + std::to_string((int)kind));
    if (width > dpitch || width > spitch) {
      violation("hipMemcpy2DAsync", dst, width, "row wider than a pitch");
      return hipErrorInvalidPitchValue;
    }
    for (size_t r = 0; r < height; ++r)
      if (!check_copy("hipMemcpy2DAsync", static_cast<char *>(dst) + r * dpitch, static_cast<const char *>(src) + r * spitch, width, kind))
        return hipErrorInvalidValue;
  }
  for (size_t r = 0; r < height; ++r)
    if (width) memmove(static_cast<char *>(dst) + r * dpitch, static_cast<const char *>(src) + r * spitch, width);
  return hipSuccess;
}
static hipError_t do_memset(const char *api, void *dst, int v, size_t n, hipStream_t s) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (enter(api)) return hipErrorInvalidValue;
    if (!stream_ok(api, s)) return hipErrorInvalidHandle;
    transfer(s);
    if (!strcmp(api, "hipMemsetAsync")) trace_call(api, s, nullptr, std::to_string(n) + " bytes");
    if (!check_device(api, dst, n)) return hipErrorInvalidValue;
  }
  if (n) memset(dst, v, n);
  return hipSuccess;
}
hipError_t hipMemset(void *dst, int v, size_t n) { return do_memset("hipMemset", dst, v, n, nullptr); }
hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t s) { return do_memset("hipMemsetAsync", dst, v, n, s); }

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipStreamCreateWithFlags")) return hipErrorOutOfMemory;
  *s = reinterpret_cast<hipStream_t>(new Stream{kStreamMagic});
  ++g_streams;
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipStreamDestroy")) return hipErrorInvalidValue;
  if (!s || !stream_ok("hipStreamDestroy", s)) return hipErrorInvalidHandle;
  reinterpret_cast<Stream *>(s)->magic = 0;
  delete reinterpret_cast<Stream *>(s);
  g_transfers.erase(s);
  --g_streams;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipStreamSynchronize")) return hipErrorInvalidValue;
  return stream_ok("hipStreamSynchronize", s) ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipStreamWaitEvent")) return hipErrorInvalidValue;
  if (!(stream_ok("hipStreamWaitEvent", s) & event_ok("hipStreamWaitEvent", e))) return hipErrorInvalidHandle;
  trace_call("hipStreamWaitEvent", s, e);
  return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus *st) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!stream_ok("hipStreamIsCapturing", s)) return hipErrorInvalidHandle;
  *st = hipStreamCaptureStatusNone;
  return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipEventCreateWithFlags")) return hipErrorOutOfMemory;
  *e = reinterpret_cast<hipEvent_t>(new Event{kEventMagic, 0});
  ++g_events;
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipEventCreate")) return hipErrorOutOfMemory;
  *e = reinterpret_cast<hipEvent_t>(new Event{kEventMagic, 0});
  ++g_events;
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipEventDestroy")) return hipErrorInvalidValue;
  if (!event_ok("hipEventDestroy", e)) return hipErrorInvalidHandle;
  reinterpret_cast<Event *>(e)->magic = 0;
  delete reinterpret_cast<Event *>(e);
  --g_events;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipEventRecord")) return hipErrorInvalidValue;
  if (!(stream_ok("hipEventRecord", s) & event_ok("hipEventRecord", e))) return hipErrorInvalidHandle;
  ++reinterpret_cast<Event *>(e)->records;
  trace_call("hipEventRecord", s, e);
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (enter("hipEventSynchronize")) return hipErrorInvalidValue;
  return event_ok("hipEventSynchronize", e) ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipEventQuery(hipEvent_t e) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!event_ok("hipEventQuery", e)) return hipErrorInvalidHandle;
  trace_call("hipEventQuery", nullptr, e);
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!(event_ok("hipEventElapsedTime", a) & event_ok("hipEventElapsedTime", b))) return hipErrorInvalidHandle;
  *ms = 0.125f;
  return hipSuccess;
}

hipError_t hipDeviceSynchronize(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return enter("hipDeviceSynchronize") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t hipSetDevice(int d) {
  if (d != 0) return hipErrorInvalidDevice;
  t_device = d;
  return hipSuccess;
}
hipError_t hipGetDevice(int *d) { *d = t_device; return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600 *prop, int d) {
  if (d != 0 || !prop) return hipErrorInvalidDevice;
  memset(prop, 0, sizeof(*prop));
  snprintf(prop->name, sizeof(prop->name), "stub MI355X");
  snprintf(prop->gcnArchName, sizeof(prop->gcnArchName), "gfx950:sramecc+:xnack-");
  prop->multiProcessorCount = 256;
  prop->warpSize = 64;
  prop->maxThreadsPerBlock = 1024;
  prop->maxThreadsDim[0] = prop->maxThreadsDim[1] = prop->maxThreadsDim[2] = 1024;
  prop->maxGridSize[0] = prop->maxGridSize[1] = prop->maxGridSize[2] = 2147483647;
  prop->sharedMemPerBlock = kMaxLds;
  prop->maxSharedMemoryPerMultiProcessor = kMaxLds;
  prop->sharedMemPerBlockOptin = kMaxLds;
  prop->totalGlobalMem = (size_t)288 << 30;
  prop->clockRate = 2400000;
  prop->major = 9;
  prop->minor = 5;
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void *fn, hipFuncAttribute, int value) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (getenv("HIP_STUB_ECHO_LAUNCHES")) {
    auto it = kernels().find(fn);
    fprintf(stderr, "stub attribute: %s value %d\n", it == kernels().end() ? "?" : it->second.c_str(), value);
  }
  if (enter("hipFuncSetAttribute")) return hipErrorInvalidValue;
  ++g_raised[fn];
  return hipSuccess;
}
hipError_t hipGetLastError(void) {
  const hipError_t e = t_last_error;
  t_last_error = hipSuccess;
  return e;
}
const char *hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorOutOfMemory: return "out of memory (stub)";
    case hipErrorInvalidValue: return "invalid argument (stub)";
    default: return "error (stub)";
  }
}

hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t s) {
  return launch_noted("hipLaunchKernel", fn, grid, block, lds, s, args);
}
hipError_t hipExtLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t s, hipEvent_t start,
                              hipEvent_t stop, int) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if ((start && !event_ok("hipExtLaunchKernel", start)) || (stop && !event_ok("hipExtLaunchKernel", stop))) return hipErrorInvalidHandle;
    if (start) ++reinterpret_cast<Event *>(start)->records;
    if (stop) ++reinterpret_cast<Event *>(stop)->records;
  }
  return launch_noted("hipExtLaunchKernel", fn, grid, block, lds, s, args, start, stop);
}

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t s) {
  t_cfg.push_back(CallConfig{grid, block, lds, s});
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *lds, hipStream_t *s) {
  if (t_cfg.empty()) return hipErrorInvalidValue;
  const CallConfig c = t_cfg.back();
  t_cfg.pop_back();
  *grid = c.grid; *block = c.block; *lds = c.lds; *s = c.stream;
  return hipSuccess;
}

// the compiler's registration calls: the fat binary is ignored, the names are kept for the launch log
static void *g_module_token[1];
void **__hipRegisterFatBinary(const void *) { return g_module_token; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *) {
  std::lock_guard<std::mutex> lk(g_mu);
  kernels()[host_fn] = device_name ? device_name : "?";
}
void __hipRegisterVar(void **, void *, char *, char *, int, size_t, int, int) {}
void __hipRegisterManagedVar(void *, void **, void *, const char *, size_t, unsigned) {}

}  // extern "C"
