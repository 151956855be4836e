// C ABI of _hsio.so: every function the library exports and the constants it
// shares with Python (ops/native.py HSIO_ABI, checked by
// tests/test_native_abi.py).  Plain prototypes over scalars and pointers; the
// contract of each entry point is described at its definition.

#ifndef HIPSNAPSHOT_HSIO_ABI_H_
#define HIPSNAPSHOT_HSIO_ABI_H_

#include <stdint.h>

// `flags` of the hsio_submit_* / hsio_*_sync calls
enum {
  HSIO_DIRECT = 1,  // try O_DIRECT for the aligned body
  HSIO_SYNC = 2,    // fdatasync before completing a write
  HSIO_MKDIRS = 4,  // create parent directories
  HSIO_APPEND = 8,  // write at offset without truncating
  // bits 16..23: NUMA node + 1 whose CPUs run the job (0: any).  A blob
  // written straight from host pages (a host-resident UVM table) is copied into
  // the page cache by the worker's CPU: a worker on the pages' node reads them
  // locally.  Unbound, the workers landed on either socket and an 8 GB DLRM
  // UVM save spread 36-69 GB/s; bound to the wrong node it ran 30-43
  // (profiles/r6/dlrm_var/).
  HSIO_NODE_SHIFT = 16
};

#ifdef __cplusplus
extern "C" {
#endif

// hsio.cpp: file I/O engine
void* hsio_create(int nthreads);
void hsio_destroy(void* e);
int hsio_eventfd(void* e);
void hsio_set_read_split(void* e, uint64_t bytes);
int64_t hsio_submit_write(void* e, const char* path, const void* buf, uint64_t n, uint64_t off,
                          int flags);
int64_t hsio_submit_read(void* e, const char* path, void* buf, uint64_t n, uint64_t off,
                         int flags);
int64_t hsio_submit_delete(void* e, const char* path);
int hsio_poll(void* e, int64_t* ids, int64_t* results, int max);
int64_t hsio_write_sync(void* e, const char* path, const void* buf, uint64_t n, uint64_t off,
                        int flags);
int64_t hsio_read_sync(void* e, const char* path, void* buf, uint64_t n, uint64_t off,
                       int flags);
int64_t hsio_file_size(const char* path);
void* hsio_alloc_aligned(uint64_t n);
void hsio_free_aligned(void* p);
void hsio_parallel_memcpy(void* dst, const void* src, uint64_t n, int nthreads);

// hschk.cpp: hs64 checksum
uint64_t hs64_partial(const void* p, uint64_t n, uint64_t first_word, int nthreads);
uint64_t hs64_finish(uint64_t sum, uint64_t n_bytes);

// hsz_cpu.cpp: HSZ1 host codec
uint64_t hsz_max_encoded_bytes(uint64_t logical, uint32_t frame_bytes);
int64_t hsz_encode_cpu(const void* src, uint64_t logical, int w, uint32_t frame_bytes, void* out,
                       int nthreads);
int hsz_decode_cpu(const void* frames, const uint64_t* offsets, uint32_t first, uint32_t count,
                   uint64_t logical, int w, uint32_t frame_bytes, void* out, int nthreads);

#ifdef __cplusplus
}  // extern "C"
#endif

#endif  // HIPSNAPSHOT_HSIO_ABI_H_
