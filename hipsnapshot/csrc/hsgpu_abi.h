// C ABI of _hsgpu.so towards Python: exactly the functions ops/native.py
// declares (HSGPU_ABI) and the constants both sides use; checked against each
// other by tests/test_native_abi.py.  Functions only the library's own files
// call are in hsgpu_hooks.h.  Plain prototypes over scalars and pointers; the
// contract of each entry point is described at its definition.

#ifndef HIPSNAPSHOT_HSGPU_ABI_H_
#define HIPSNAPSHOT_HSGPU_ABI_H_

#include <stdint.h>

// `flags` of hsg_drain_start
enum {
  HSG_DRAIN_SYNC = 1,  // fdatasync every file
  HSG_DRAIN_HASH = 2,  // hs64 hash every blob on the GPU
  // O_DIRECT files: the pinned slots go to the device with no CPU copy and no
  // page cache (buffered where the filesystem refuses it)
  HSG_DRAIN_DIRECT = 4,
  HSG_DRAIN_HASH_LOW_PRIO = 8,  // keep the hash stream at default (not high) priority
  HSG_DRAIN_NICE_SHIFT = 8,     // bits 8..15: nice increment of the drain threads
  HSG_DRAIN_PARKED_SHIFT = 16   // bits 16..23: parked writers (hsg_drain_boost)
};

// sizes of the buffers hsg_drain_wait / hsg_restore_wait fill
enum {
  HSG_DRAIN_NUM_STATS = 9,     // doubles in `stats` (Stat of hsdrain.cpp)
  HSG_DRAIN_MSG_BYTES = 256,   // bytes of `msg`
  HSG_RESTORE_NUM_STATS = 11,  // doubles in `stats` (Stat of hsrestore.cpp)
  HSG_RESTORE_MSG_BYTES = 320  // bytes of `msg`
};

// `codec` of a restore item
enum {
  HSG_CODEC_RAW = 0,  // raw bytes
  HSG_CODEC_HSZ = 1   // a whole HSZ1 blob
};

#ifdef __cplusplus
extern "C" {
#endif

// hsgpu.hip: the message of the calling thread's last failed hsg_* call (the
// library's only error channel: every failing entry point sets it)
const char* hsg_last_error();

// hsgpu.hip: devices, pinned host pool
int hsg_device_count();
int hsg_pci_location(int dev, int* domain, int* bus, int* device);
void* hsg_pinned_acquire(uint64_t nbytes);
int hsg_pinned_release(void* p);
void* hsg_pinned_acquire_on(uint64_t nbytes, int node);
void hsg_pinned_stats(uint64_t* cached, uint64_t* in_use);
uint64_t hsg_pinned_trim();
void hsg_pinned_set_limit(uint64_t bytes);
int hsg_poison_idle_pools(int dev, int byte);

// hsgpu.hip: uncached device blocks
void* hsg_uncached_acquire(int dev, uint64_t nbytes);
int hsg_uncached_release(void* p);
uint64_t hsg_uncached_trim();
uint64_t hsg_uncached_bytes();

// hsgpu.hip: copies and streams
int hsg_memcpy(int dev, int slot, void* dst, const void* src, uint64_t n, int kind, void* producer,
               int has_producer, int sync);
int hsg_stream_join(int dev, int slot, void* consumer);
int hsg_stream_sync(int dev, int slot);
void* hsg_copy_stream(int dev, int slot);
int hsg_sync_stream_handle(void* stream);
int hsg_set_thread_grid_cap(int cap);
int hsg_prewarm_module(int dev);

// hscopy.hip: batched strided copy / cast
uint64_t hsg_desc_size();
uint64_t hsg_copy_workspace_bytes(const void* descs, int n);
int hsg_copy_nd(int dev, const void* descs, int n, void* workspace, uint64_t ws_bytes,
                void* pinned_stage, void* stream, int sync);

// hshash.hip: hs64 checksum
int hsg_hash64(int dev, int slot, int after_slot, const void* p, uint64_t n, uint64_t first_word,
               int max_grid, int* handle);
int hsg_hash64_result(int dev, int slot, int handle, uint64_t* out);
int hsg_hash64_batch(int dev, void* stream, const void* descs, int n, uint64_t* sums_out);

// hsquant.hip: fp8 / MX8 quantization
int hsg_fp8_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out, void* scales,
                     int vpt, void* stream);
int hsg_fp8_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                       int dst_dtype, int vpt, void* stream);
int hsg_fp8_hadamard_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out,
                              void* scales, void* stream);
int hsg_fp8_hadamard_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                                int dst_dtype, void* stream);
int hsg_mx8_quantize(int dev, const void* src, int src_dtype, int64_t n, void* out, void* scales,
                     void* stream);
int hsg_mx8_dequantize(int dev, const void* q, const void* scales, int64_t n, void* dst,
                       int dst_dtype, void* stream);

// hsgpu.hip: managed memory, stream gate
int hsg_is_managed(const void* p);
int hsg_managed_location(const void* p, uint64_t n, int* preferred, int* last_prefetch);
int hsg_managed_place(int dev, const void* p, uint64_t n, int loc, void* stream);
void* hsg_managed_alloc(int dev, uint64_t n);
int hsg_managed_free(void* p);
int hsg_gate_supported(int dev);
int hsg_gate_arm(int dev, void* stream, uint32_t* value);
int hsg_gate_release(int dev, uint32_t value);
uint32_t hsg_gate_value(int dev);

// hsz.hip: HSZ1 GPU codec
uint64_t hsg_hsz_meta_bytes(uint32_t n_frames);
int hsg_hsz_encode(int dev, const void* src, uint64_t logical, int w, uint32_t frame_bytes,
                   void* out, void* meta, void* total, void* stream);
int hsg_hsz_decode(int dev, const void* frames, const void* offsets, uint32_t first,
                   uint32_t count, uint64_t logical, int w, uint32_t frame_bytes, void* out,
                   void* stream, void* err);

// hsdma.hip: SDMA copies
int hsg_sdma_engines(int dev);
int hsg_sdma_d2h(int dev, void* dst, const void* src, uint64_t n, int max_engines, void* stream);
int hsg_sdma_d2h_submit(int dev, void* dst, const void* src, uint64_t n, void* stream,
                        uint64_t* handle);
int hsg_sdma_h2d(int dev, void* dst, const void* src, uint64_t n);
int hsg_sdma_h2d_submit(int dev, void* dst, const void* src, uint64_t n, uint64_t* handle);
int hsg_sdma_wait(uint64_t handle);

// hshost.hip: HIP runtime calls of the host engines
void hsg_rt_set_trace(int on);
void* hsg_rt_dev_alloc(int dev, uint64_t nbytes, int uncached);
void hsg_rt_dev_free(void* p);
void* hsg_rt_vmm_alloc(int dev, uint64_t nbytes, int uncached);
int hsg_rt_vmm_free(void* p);
uint64_t hsg_rt_vmm_retired_bytes();
int hsg_rt_memcpy_d2h(void* dst, const void* src, uint64_t n);

// hsdrain.cpp: device byte ranges -> files
void* hsg_drain_start(int dev, int n, const uint64_t* srcs, const uint64_t* sizes,
                      const char* const* paths, uint64_t slot_bytes, int nslots, int nwriters,
                      int flags, int max_hash_grid, int* err);
int hsg_drain_wait(void* handle, uint64_t* sums, uint64_t* bytes_written, char* msg,
                   double* stats);
int hsg_drain_pending(void* handle);
void hsg_drain_boost(void* handle);

// hsrestore.cpp: file byte ranges -> HBM
void* hsg_restore_start(int dev, int n, const char* const* paths, const uint64_t* file_lo,
                        const uint64_t* nbytes, const int* codec, const uint64_t* logical,
                        const uint64_t* direct, const uint64_t* base_off, const int64_t* desc_off,
                        const int* desc_n, const void* descs, int64_t n_descs,
                        const uint64_t* producers, int n_producers, uint32_t* err_words,
                        uint64_t slot_bytes, uint64_t first_bytes, uint64_t piece_bytes,
                        int nslots, int nreaders, uint64_t budget, int engine,
                        const int* hash_items, int hash_grid, int* err);
int hsg_restore_wait(void* handle, int* err_item, char* msg, double* stats, uint64_t* bytes_read,
                     uint64_t* sums);
int hsg_restore_prewarm(int dev, uint64_t up_bytes, uint64_t sc_bytes, uint64_t slot_bytes,
                        int nslots, uint64_t table_bytes);
uint64_t hsg_restore_trim(int dev, uint64_t keep);
uint64_t hsg_restore_trim_pools(int dev, uint64_t keep_upload, uint64_t keep_scratch);
void hsg_restore_pool_bytes(int dev, uint64_t* out);

#ifdef __cplusplus
}  // extern "C"
#endif

#endif  // HIPSNAPSHOT_HSGPU_ABI_H_
