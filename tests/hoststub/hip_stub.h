// hip_stub.h — what the driver (host_main.cpp) reads from the stub HIP runtime (hip_stub.cpp).
// The stub is the HIP runtime on the CPU: "device" memory is exactly-sized heap memory, copies execute at once after a check
// against the registry of live ranges, streams and events are small heap objects, launches run nothing and are logged.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

struct StubLaunch {
  std::string kernel;          // name given to __hipRegisterFunction ("?" for an unregistered host function)
  unsigned grid[3], block[3];
  size_t lds;                  // dynamic LDS bytes
  void *stream;
};

enum StubKind { STUB_DEVICE = 0, STUB_PINNED = 1, STUB_REGISTERED = 2 };

long stub_launch_count();
std::vector<StubLaunch> stub_launches();         // a copy of the log
void stub_clear_launches();
long stub_live_ranges();                         // device + pinned + registered
long stub_live_ranges_of(int kind);
long stub_live_streams();
long stub_live_events();
// kernels whose dynamic-LDS limit was raised (hipFuncSetAttribute) with no launch behind it (each is printed): a launcher raises
// the limit right in front of its launch, so this is a launch that was dropped on its way to the runtime
long stub_raised_not_launched();
long stub_violations();
void stub_reset_violations();
// copies and memsets issued on `stream` so far (the null stream counts under nullptr)
long stub_transfers_on(void *stream);
long stub_transfers_total();
// calls of `api` ("hipMalloc", ...) so far
long stub_calls(const char *api);
// the n-th later call (n >= 1) of `api` fails: hipErrorOutOfMemory for the allocating calls, hipErrorInvalidValue otherwise.
// n = 0 disarms.  One API at a time is enough for the driver; arming another replaces the first.
void stub_fail_after(const char *api, long n);
bool stub_fail_fired();                          // the armed failure was delivered
// HIP_STUB_TRACE set: the lines logged since the last call — launches (name with template arguments, grid, block, LDS, stream,
// the events of an extended launch, the geometry of a spfe::ConvParams argument), hipEventRecord, hipStreamWaitEvent,
// hipEventQuery and the asynchronous copies and memsets, in issue order; streams and events as indices in order of first
// appearance.  Taking the text empties the log; restart_numbering: the next stream and event are number 0 again (a new handle).
// (HIP_STUB_EMULATE_PROBE set: a launch of the library's queue probe writes its stamps, and the probe finds a free queue.)
std::string stub_trace_take(bool restart_numbering);
// A "device" range of `bytes` carved out of a larger heap block (`slack` bytes behind it are the stub's own): a copy past the
// range stays inside the block, so only the registry can notice it (stub_selfcheck).  Freed with hipFree.
void *stub_malloc_in_block(size_t bytes, size_t slack);
