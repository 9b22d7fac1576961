// buf_test.cpp — the owning buffers of the host code (csrc/kan_buf.hpp) on a malloc-backed policy that can be
// told to fail its k-th allocation.  A stand-alone host program: built with -fsanitize=address,undefined by
// tests/test_host_buf.py, so a leak, a double free or a use after free fails the run as well as an assert.
#define KAN_BUF_NO_HIP
#include "kan_buf.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

namespace {

struct Heap {
    int allocs = 0, frees = 0, cleared = 0;
    int fail_at = 0;   // the fail_at-th allocation from now fails (0: none)
    std::set<void*> live;
} heap;

struct MallocPolicy {
    using error = int;
    static constexpr int ok = 0;
    int tag = 0;   // state that travels with the allocation (as MappedPolicy's device address does)
    int alloc(void** p, size_t bytes) {
        if (heap.fail_at > 0 && --heap.fail_at == 0) return 2;
        *p = std::malloc(bytes);
        heap.live.insert(*p);
        ++heap.allocs;
        tag = heap.allocs;
        return 0;
    }
    void release(void* p) {
        if (heap.live.erase(p) != 1) {
            std::fprintf(stderr, "release of a pointer that is not live\n");
            std::abort();
        }
        std::free(p);
        ++heap.frees;
    }
    static void clear_error() { ++heap.cleared; }
};
using B = kan::Buf<MallocPolicy>;

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

void test_reserve() {
    B b;
    CHECK(b.ptr() == nullptr && b.bytes() == 0);
    CHECK(b.reserve(0) == 0 && b.ptr() == nullptr);   // nothing asked, nothing allocated
    CHECK(b.reserve(100) == 0 && b.ptr() && b.bytes() == 100);
    std::memset(b.ptr(), 1, 100);
    void* p = b.ptr();
    CHECK(b.reserve(40) == 0 && b.ptr() == p && b.bytes() == 100);    // smaller: the pointer is kept
    CHECK(b.reserve(100) == 0 && b.ptr() == p);
    CHECK(b.reserve(300) == 0 && b.bytes() == 300 && heap.frees == 1);   // grown: the old one freed
    std::memset(b.as<char>(), 2, 300);
    // a failed reserve leaves the buffer empty with size 0 and clears the sticky error; the next one succeeds
    heap.fail_at = 1;
    const int cleared = heap.cleared;
    CHECK(b.reserve(1000) == 2 && b.ptr() == nullptr && b.bytes() == 0 && b.policy().tag == 0);
    CHECK(heap.cleared == cleared + 1 && heap.live.empty());
    CHECK(b.reserve(8) == 0 && b.ptr() && b.bytes() == 8);
    b.reset();
    CHECK(b.ptr() == nullptr && b.bytes() == 0 && heap.live.empty());
    b.reset();   // (idempotent)
}

void test_move() {
    B a;
    CHECK(a.reserve(64) == 0);
    void* p = a.ptr();
    const int tag = a.policy().tag;
    B b(std::move(a));
    CHECK(a.ptr() == nullptr && a.bytes() == 0 && a.policy().tag == 0);   // the source is empty
    CHECK(b.ptr() == p && b.bytes() == 64 && b.policy().tag == tag);
    B c;
    CHECK(c.reserve(16) == 0);
    const int frees = heap.frees;
    c = std::move(b);   // the target's own allocation is freed
    CHECK(heap.frees == frees + 1 && c.ptr() == p && c.bytes() == 64 && b.ptr() == nullptr && b.bytes() == 0);
    CHECK(a.reserve(8) == 0 && a.ptr() != p);   // a moved-from buffer is usable
}

// grow_keep failed at each of its allocations in turn, and at the copy: the old buffers, sizes and contents
// stay, every new allocation is freed; then it succeeds
void test_grow_keep() {
    B x, y, z;
    CHECK(x.reserve(8) == 0 && y.reserve(16) == 0 && z.reserve(24) == 0);
    std::memset(x.ptr(), 'x', 8);
    std::memset(y.ptr(), 'y', 16);
    std::memset(z.ptr(), 'z', 24);
    void *px = x.ptr(), *py = y.ptr(), *pz = z.ptr();
    int copies = 0, copy_result = 0;
    auto copy = [&](B& nx, B& ny, B& nz) {
        ++copies;
        if (copy_result != 0) return copy_result;
        CHECK(nx.bytes() == 80 && ny.bytes() == 160 && nz.bytes() == 240);
        std::memcpy(nx.ptr(), x.ptr(), x.bytes());
        std::memcpy(ny.ptr(), y.ptr(), y.bytes());
        std::memcpy(nz.ptr(), z.ptr(), z.bytes());
        return 0;
    };
    for (int k = 1; k <= 4; ++k) {
        const size_t live = heap.live.size();
        heap.fail_at = k <= 3 ? k : 0;
        copy_result = k == 4 ? 7 : 0;
        int failed = -1;
        CHECK(kan::grow_keep({80, 160, 240}, &failed, copy, x, y, z) == (k <= 3 ? 2 : 7));
        CHECK(failed == k - 1 && copies == (k == 4 ? 1 : 0));
        CHECK(x.ptr() == px && y.ptr() == py && z.ptr() == pz);
        CHECK(x.bytes() == 8 && y.bytes() == 16 && z.bytes() == 24);
        CHECK(x.as<char>()[7] == 'x' && y.as<char>()[15] == 'y' && z.as<char>()[23] == 'z');
        CHECK(heap.live.size() == live && heap.fail_at == 0);   // every new allocation freed again
    }
    copy_result = 0;
    int failed = -1;
    const int frees = heap.frees;
    CHECK(kan::grow_keep({80, 160, 240}, &failed, copy, x, y, z) == 0 && failed == -1);
    CHECK(x.bytes() == 80 && y.bytes() == 160 && z.bytes() == 240 && heap.frees == frees + 3);
    CHECK(x.as<char>()[7] == 'x' && y.as<char>()[15] == 'y' && z.as<char>()[23] == 'z');
}

}  // namespace

int main() {
    test_reserve();
    test_move();
    test_grow_keep();
    // destruction frees exactly once: every allocation made above has been released, none twice (release aborts)
    CHECK(heap.live.empty() && heap.allocs == heap.frees && heap.allocs > 0);
    std::puts("buf_test ok");
    return 0;
}
