// em2_hip_util.h -- the host-side plumbing every driver needs: bail out on a HIP error, a device allocation that frees
// itself and copies typed arrays in and out, the 1-D grid of a 256-thread kernel, blocks per items, signature words, the
// stage timer; with em2_arena.h, which it includes, 256-byte alignment and the layout of one allocation that holds several
// arrays.  (The device-side counterpart is em2_wave.h; device scratch that outlives a call is em2_scratch.h; what a C entry
// point reports its errors with is em2_entry.h; the device-wide sorts, scans and reductions are em2_primitives.h; the kernels
// for runs of equal sorted keys are em2_runs.h.)
#ifndef EM2_HIP_UTIL_H
#define EM2_HIP_UTIL_H

#include "em2_arena.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>

// Returns the hipError_t of a failed call from the enclosing function.  (The call's text is not kept: the entry points
// report one with em2_entry.h's EM2_HIP and EM2_HIP_FOR, createClusterGraph with em2_cluster_graph.hip's EM2_TRYC.)
#define EM2_TRY(call)                        \
    do {                                     \
        hipError_t em2Err_ = (call);         \
        if (em2Err_ != hipSuccess) return em2Err_; \
    } while (0)

namespace em2 {

// RAII device allocation.  allocate() frees what the buffer holds; 0 bytes allocate 1, so that p is never null after it.
struct DeviceBuffer {
    void* p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    hipError_t allocate(size_t bytes)
    {
        release();
        return hipMalloc(&p, bytes ? bytes : 1);
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    // Room for count elements of T; upload() also fills it from the host.  The copies are synchronous hipMemcpy calls (callers
    // rely on them to wait for the null stream); count == 0 copies nothing, and host may then be null.
    template <class T> hipError_t allocateFor(size_t count) { return allocate(count * sizeof(T)); }
    template <class T> hipError_t upload(const T* host, size_t count)
    {
        EM2_TRY(allocateFor<T>(count));
        return count ? hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    }
    template <class T> hipError_t download(T* host, size_t count) const
    {
        return count ? hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
    }
};

// Blocks of 256 threads for n items, at least 1 and at most 16384 (the kernels launched with it stride over the grid).
inline uint32_t gridFor(uint64_t n)
{
    const uint64_t blocks = (n + 255) / 256;
    return uint32_t(blocks > 16384 ? 16384 : (blocks ? blocks : 1));
}

// Blocks of perBlock items that hold `items` items.
inline uint32_t blocksOf(uint64_t items, uint32_t perBlock) { return uint32_t((items + perBlock - 1u) / perBlock); }

// 64-bit words of a signature of lshCount > 0 bits.
inline uint32_t wordCountOf(uint32_t lshCount) { return (lshCount - 1u) / 64u + 1u; }

// EM2_TIMING=1: the wall time of the stages of a device call on stderr, "[em2 timing] <what>: <stage> <ms> ms" (measurements
// only).  stage() synchronises the stream when the timing is on, and does nothing else when it is off.
class StageTimer {
public:
    explicit StageTimer(const char* what)
        : what_(what), on_(getenv("EM2_TIMING") && getenv("EM2_TIMING")[0] == '1'), last_(std::chrono::steady_clock::now()) {}
    hipError_t stage(const char* name, hipStream_t stream)
    {
        if (!on_) return hipSuccess;
        EM2_TRY(hipStreamSynchronize(stream));
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[em2 timing] %s: %s %.3f ms\n", what_, name, std::chrono::duration<double, std::milli>(now - last_).count());
        last_ = now;
        return hipSuccess;
    }
private:
    const char* what_;
    bool on_;
    std::chrono::steady_clock::time_point last_;
};

}  // namespace em2

#endif
