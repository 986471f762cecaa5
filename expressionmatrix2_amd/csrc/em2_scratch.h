// em2_scratch.h -- device scratch the process keeps between calls (em2_scratch.hip).
//
// The scratch of a findSimilarPairs5 call (tables, candidate ids, lists: 10 GB at a million cells x 2048 bits) and the one
// block of an em2_subset_find_similar_pairs4 call (13 GB at a million cells) come from a cache of device blocks: hipMalloc of
// gigabytes costs anything between 4 and 200 ms per call depending on the state of the box (measured: the same command, two
// leases), and took 1.6-4 s in one call of twelve.  EM2_SCRATCH_CACHE_MB caps what is kept (default: a sixteenth of the
// device's memory; 0 = nothing is kept); em2_dev_release_scratch() frees it.
#ifndef EM2_SCRATCH_H
#define EM2_SCRATCH_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace em2 {

// Frees every block the cache holds.
void releaseScratch();

// A block from the cache when it holds one of a fitting size on the current device, else from hipMalloc -- once more after
// the cache has been emptied when that fails (memory held by the cache may be what is missing).
// A block may go back to the cache only when the device has finished with it; otherwise it is freed (hipFree waits for the
// device).  Who knows that differs, so there are two ways to say it:
//   * the `idle` member, which the destructor reads: the owner sets it once everything that used the block has been waited
//     for (em2_capi.hip);
//   * drop(bool) from a derived destructor, for owners that keep that knowledge elsewhere (em2_fsp5.hip: one thread-local
//     "the call completed" flag for all the buffers of a call).
struct CachedBuffer {
    void* p = nullptr;
    size_t bytes = 0;          // the block's size in the cache (at least what was asked for)
    int device = 0;
    bool idle = false;
    CachedBuffer() = default;
    CachedBuffer(const CachedBuffer&) = delete;
    CachedBuffer& operator=(const CachedBuffer&) = delete;
    ~CachedBuffer() { drop(idle); }
    // (the caller knows the device has finished with the block)
    void release() { drop(true); }
    void drop(bool isIdle);
    // frees (does not cache) a block the buffer still holds.  reportMalloc: with EM2_TIMING set, the duration of a hipMalloc
    // the cache could not spare the call goes to stderr.
    hipError_t allocate(size_t wanted, bool reportMalloc = false);
    template <class T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace em2

#endif
