// Everything _hsgpu.so exports: the ABI towards Python (hsgpu_abi.h) plus
// the hooks only the library's own files call -- the host engines
// (hsdrain.cpp, hsrestore.cpp) do their device work through them, and
// tests/native/engine_stubs.cpp defines them for CPU-only builds.  Every file
// of the library includes this header, so a definition or a stub that drifts
// from its prototype does not compile.

#ifndef HIPSNAPSHOT_HSGPU_HOOKS_H_
#define HIPSNAPSHOT_HSGPU_HOOKS_H_

#include "hsgpu_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

// hsgpu.hip
int hsg_thread_grid_cap();
int hsg_stream_priority(int dev, int slot, int high);

// hshash.hip
int hsg_hash64_into(int dev, void* stream, const void* p, uint64_t n, uint64_t first_word,
                    int max_grid, void* acc);

// hsdma.hip
int hsg_sdma_release(int dev, void* stream);
int hsg_sdma_d2h_submit_released(int dev, void* dst, const void* src, uint64_t n,
                                 uint64_t* handle);
uint32_t hsg_sdma_h2d_engine_mask(int dev);
int hsg_sdma_h2d_submit_on(int dev, void* dst, const void* src, uint64_t n, int engine,
                           uint64_t* handle);

// hshost.hip
int hsg_rt_trace_on();
void hsg_rt_trace(const char* what, const void* p, uint64_t n, int kind);
int hsg_rt_set_device(int dev);
void* hsg_rt_event_record(void* stream);
int hsg_rt_event_sync(void* ev);
void hsg_rt_event_free(void* ev);
int hsg_rt_stream_after(void* waiter, void* producer);
int hsg_rt_stream_sync(void* stream);

// hsrestore.cpp
int hsg_restore_idle_blocks(int dev, uint64_t* ptrs, uint64_t* sizes, int max);

#ifdef __cplusplus
}  // extern "C"
#endif

#endif  // HIPSNAPSHOT_HSGPU_HOOKS_H_
