// em2_arena.h -- the layout of one allocation that holds several arrays (host only, no HIP): a driver asks an ArenaPlan for
// every block it needs, allocates plan.bytes once, and reaches a block with arenaAt<T>(base, offset).  Every block starts at a
// multiple of 256 bytes from the base, and a block of 0 bytes still takes 256, so that no two blocks share an address.
// (The scans, the distributed entry and the projection lay their workspaces out in structs of their own.)
#ifndef EM2_ARENA_H
#define EM2_ARENA_H

#include <stddef.h>
#include <stdint.h>

namespace em2 {

inline size_t alignUp(size_t x) { return (x + 255u) & ~size_t(255u); }

struct ArenaPlan {
    size_t bytes = 0;                       // of the blocks taken so far: the offset of the next one, the size to allocate
    // The offset of a new block of n bytes.
    size_t take(size_t n)
    {
        const size_t here = bytes;
        bytes += alignUp(n ? n : 1u);
        return here;
    }
    template <class T> size_t takeFor(size_t count) { return take(count * sizeof(T)); }
};

template <class T> T* arenaAt(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }

}  // namespace em2

#endif
