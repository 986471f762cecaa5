// em2_arena_main.cpp -- a stand-alone program that checks the arena planner of expressionmatrix2_amd/csrc/em2_arena.h on the
// CPU (host only: no HIP header, never loaded into Python, never run on a GPU).  tests/test_arena_cpu.py builds and runs it;
// the same program under the sanitizers:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/em2_arena_main
//       tests/native/em2_arena_main.cpp
//   /tmp/em2_arena_main
//
// It prints one line per block taken ("block <size> at <offset>") and "em2_arena: <n> checks passed", or the first check
// that failed, and then exits with status 1.
#include "../../expressionmatrix2_amd/csrc/em2_arena.h"

#include <cstdio>
#include <cstdlib>

static int checks = 0;

#define CHECK(condition)                                                          \
    do {                                                                          \
        if (!(condition)) {                                                       \
            fprintf(stderr, "em2_arena: line %d: %s is false\n", __LINE__, #condition); \
            exit(1);                                                              \
        }                                                                         \
        checks++;                                                                 \
    } while (0)

int main()
{
    using em2::ArenaPlan;
    using em2::arenaAt;

    // a block of n bytes takes n rounded up to 256, and 256 where n is 0
    const size_t sizes[] = {0u, 1u, 255u, 256u, 257u, (size_t(1) << 32) + 1u};
    const size_t taken[] = {256u, 256u, 256u, 256u, 512u, (size_t(1) << 32) + 256u};
    ArenaPlan plan;
    CHECK(plan.bytes == 0u);
    size_t sum = 0, last = 0;
    for (int i = 0; i < 6; i++) {
        const size_t at = plan.take(sizes[i]);
        printf("block %zu at %zu\n", sizes[i], at);
        CHECK(at % 256u == 0u);                     // every offset is a multiple of 256
        CHECK(i == 0 ? at == 0u : at > last);       // offsets strictly increase
        CHECK(at == sum);                           // a block begins where the blocks before it end
        CHECK(plan.bytes - at == taken[i]);
        CHECK(plan.bytes % 256u == 0u);
        last = at;
        sum += taken[i];
    }
    CHECK(plan.bytes == sum);                       // the sum of the aligned sizes
    CHECK(plan.bytes == (size_t(1) << 32) + 7u * 256u);

    // a block of 0 bytes between two others shares its address with neither
    ArenaPlan gaps;
    const size_t before = gaps.take(8), empty = gaps.take(0), after = gaps.take(8);
    CHECK(before == 0u && empty == 256u && after == 512u && gaps.bytes == 768u);

    // takeFor<T>(n) is take(n * sizeof(T))
    const size_t counts[] = {0u, 1u, 31u, 32u, 33u, (size_t(1) << 29) + 1u};
    ArenaPlan typed, plain;
    for (const size_t n : counts) {
        CHECK(typed.takeFor<uint64_t>(n) == plain.take(8u * n));
        CHECK(typed.bytes == plain.bytes);
    }
    ArenaPlan words, bytes;
    CHECK(words.takeFor<uint32_t>(65u) == bytes.take(260u) && words.bytes == bytes.bytes && words.bytes == 512u);

    // arenaAt<T>(base, offset) is base + offset, as a T*
    alignas(256) static unsigned char memory[1024];
    ArenaPlan real;
    const size_t offA = real.takeFor<uint32_t>(3), offB = real.takeFor<double>(2), offC = real.take(0);
    CHECK(real.bytes <= sizeof(memory));
    uint32_t* a = arenaAt<uint32_t>(memory, offA);
    double* b = arenaAt<double>(memory, offB);
    CHECK(static_cast<void*>(a) == memory + offA);
    CHECK(static_cast<void*>(b) == memory + offB);
    CHECK(static_cast<void*>(arenaAt<char>(memory, offC)) == memory + offC);
    a[0] = 1u, a[1] = 2u, a[2] = 3u;
    b[0] = 0.5, b[1] = 0.25;
    CHECK(a[0] + a[1] + a[2] == 6u && b[0] + b[1] == 0.75);
    CHECK(memory[offA] + memory[offA + 1] + memory[offA + 2] + memory[offA + 3] == 1);      // (the bytes of a[0], either endianness)

    CHECK(em2::alignUp(0) == 0u && em2::alignUp(1) == 256u && em2::alignUp(256) == 256u && em2::alignUp(257) == 512u);
    printf("em2_arena: %d checks passed\n", checks);
    return 0;
}
