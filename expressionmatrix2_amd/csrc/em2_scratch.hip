// em2_scratch.hip -- the cache of device blocks behind em2_scratch.h.  Host code only (a .hip file for the HIP headers).

#include "em2_scratch.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

namespace em2 {
namespace {

class ScratchCache {
public:
    void* take(size_t bytes, int device, size_t* got)
    {
        std::lock_guard<std::mutex> guard(mutex_);
        size_t best = blocks_.size();
        for (size_t i = 0; i < blocks_.size(); ++i) {
            const Block& b = blocks_[i];
            if (b.device != device || b.bytes < bytes || b.bytes > bytes + bytes / 2u + (size_t(1) << 20)) continue;
            if (best == blocks_.size() || b.bytes < blocks_[best].bytes) best = i;
        }
        if (best == blocks_.size()) return nullptr;
        void* p = blocks_[best].p;
        *got = blocks_[best].bytes;
        total_ -= blocks_[best].bytes;
        blocks_.erase(blocks_.begin() + long(best));
        return p;
    }
    void give(void* p, size_t bytes, int device)
    {
        std::vector<Block> evicted;
        bool kept = false;
        {
            std::lock_guard<std::mutex> guard(mutex_);
            const size_t cap = capBytes();
            if (bytes <= cap) {
                // a block that fits the cap by itself makes room for itself: the OLDEST blocks go first (what the cache is for
                // is the few large blocks of the last call -- the scan's workspace, the result -- not whatever arrived first)
                while (!blocks_.empty() && (total_ + bytes > cap || blocks_.size() >= 256u)) {
                    evicted.push_back(blocks_.front());
                    total_ -= blocks_.front().bytes;
                    blocks_.erase(blocks_.begin());
                }
                blocks_.push_back(Block{p, bytes, device});
                total_ += bytes;
                kept = true;
            }
        }
        for (const Block& b : evicted) (void)hipFree(b.p);
        if (!kept) (void)hipFree(p);
    }
    void clear()
    {
        std::vector<Block> freed;
        {
            std::lock_guard<std::mutex> guard(mutex_);
            freed.swap(blocks_);
            total_ = 0;
        }
        for (const Block& b : freed) (void)hipFree(b.p);
    }
    static ScratchCache& instance()
    {
        static ScratchCache* cache = new ScratchCache();          // (never destroyed: the HIP runtime may be gone at exit)
        return *cache;
    }

private:
    struct Block { void* p; size_t bytes; int device; };
    static size_t capBytes()
    {
        // what a host process can live with: a sixteenth of the device's memory (18 GB of an MI355X's 288) unless
        // EM2_SCRATCH_CACHE_MB says otherwise (0: nothing is kept).  One findSimilarPairs5 call's scratch at a million cells x
        // 2048 bits is 10 GB; the scan workspace of em2_subset_find_similar_pairs4 at a million cells is 12 GB (round 5: 27, and an
        // eighth of the memory to hold it), and it is the block that matters: its hipMalloc took 0.4 ms in 22 calls of 24 on one
        // box and 2.7 and 4.0 s in the other two.
        if (const char* v = getenv("EM2_SCRATCH_CACHE_MB")) return size_t(strtoull(v, nullptr, 10)) << 20;
        static size_t share = 0;
        if (!share) {
            size_t freeBytes = 0, totalBytes = 0;
            share = hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess && totalBytes ? totalBytes / 16u : size_t(4) << 30;
        }
        return share;
    }
    std::mutex mutex_;
    std::vector<Block> blocks_;
    size_t total_ = 0;
};

}  // namespace

void releaseScratch() { ScratchCache::instance().clear(); }

void CachedBuffer::drop(bool isIdle)
{
    if (!p) return;
    if (isIdle) ScratchCache::instance().give(p, bytes, device);
    else (void)hipFree(p);
    p = nullptr;
}

hipError_t CachedBuffer::allocate(size_t wanted, bool reportMalloc)
{
    drop(false);
    wanted = wanted ? wanted : 1;
    if (hipGetDevice(&device) != hipSuccess) device = 0;
    p = ScratchCache::instance().take(wanted, device, &bytes);
    if (p) return hipSuccess;
    bytes = wanted;
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipMalloc(&p, wanted);
    if (reportMalloc && getenv("EM2_TIMING")) {
        fprintf(stderr, "[em2 timing] hipMalloc of %zu bytes (not in the scratch cache): %.1f ms, %s\n", wanted,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), e == hipSuccess ? "ok" : "FAILED");
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ScratchCache::instance().clear();          // (memory held by the cache may be what is missing)
        return hipMalloc(&p, wanted);
    }
    return e;
}

}  // namespace em2
