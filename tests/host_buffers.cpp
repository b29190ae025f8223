// host_buffers.cpp - Buf (flow-pipeline_amd/csrc/buffers.h) over a malloc-backed allocator that counts its calls and its
// live blocks and can be told to fail its N-th call.  Built with -fsanitize=address,undefined and run on its own by
// tests/test_host_buffers.py: a double free, a use after free or a leak ends the run through the sanitizers, a wrong count
// through CHECK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../flow-pipeline_amd/csrc/buffers.h"

struct CountingAlloc {
    static int calls, frees, live, fail_at;  // fail_at: the alloc call (counted from 1) that fails; 0 = none
    static bool alloc(void** p, size_t bytes) {
        if (++calls == fail_at) return false;
        *p = malloc(bytes ? bytes : 1);
        if (!*p) return false;
        memset(*p, 0xA5, bytes);
        live++;
        return true;
    }
    static void free(void* p) {
        ::free(p);
        frees++;
        live--;
    }
};
int CountingAlloc::calls = 0, CountingAlloc::frees = 0, CountingAlloc::live = 0, CountingAlloc::fail_at = 0;
using A = CountingAlloc;
using B = Buf<A, unsigned char>;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// stands in for fa_ctx::WChunk: two buffers and some plain fields, moved between vectors and never copied
struct Chunk {
    Buf<A, unsigned> seg, counts;
    unsigned n = 0;
};
static Chunk make_chunk(unsigned n) {
    Chunk k;
    k.n = n;
    if (!k.seg.grow(64 * n) || !k.counts.grow(16 * n)) abort();
    return k;
}

static int run() {
    {  // grow from empty; a sufficient capacity makes no allocator call and keeps the pointer
        B b;
        CHECK(b.get() == nullptr && b.bytes() == 0 && !b);
        CHECK(b.grow(100, 150));
        CHECK(b.get() && b.bytes() == 150 && A::calls == 1 && A::live == 1);
        unsigned char* p = b;
        p[149] = 1;  // (the whole capacity is the buffer's)
        CHECK(b.grow(150, 4000) && b.grow(1, 1) && b.grow(0));
        CHECK(b.get() == p && b.bytes() == 150 && A::calls == 1 && A::frees == 0);
        // a larger grow frees the old block exactly once
        CHECK(b.grow(151, 300));
        CHECK(b.bytes() == 300 && A::calls == 2 && A::frees == 1 && A::live == 1);
        b.get()[299] = 2;
        CHECK(static_cast<void*>(b.get()) == static_cast<void*>((unsigned*)b));  // the cast written out views the same block
        // a failed grow leaves {nullptr, 0} ...
        A::fail_at = A::calls + 1;
        CHECK(!b.grow(301, 600));
        CHECK(b.get() == nullptr && b.bytes() == 0 && A::frees == 2 && A::live == 0);
        // ... and the next grow with the same need asks the allocator again (the stale-capacity defect: it must not pass as "large enough")
        const int before = A::calls;
        CHECK(b.grow(301, 600));
        CHECK(A::calls == before + 1 && b.get() && b.bytes() == 600 && A::live == 1);
        A::fail_at = 0;
        b.reset();
        CHECK(b.get() == nullptr && b.bytes() == 0 && A::live == 0);
        b.reset();  // (twice is nothing)
        CHECK(A::live == 0);
        CHECK(b.grow(8));
        CHECK(A::live == 1);
    }  // the destructor releases
    CHECK(A::live == 0);
    {  // move construction and move assignment empty the source and free the destination's previous block
        B a, d;
        CHECK(a.grow(10) && d.grow(20));
        unsigned char* pa = a;
        B m(std::move(a));
        CHECK(a.get() == nullptr && a.bytes() == 0 && m.get() == pa && m.bytes() == 10 && A::live == 2);
        const int frees = A::frees;
        d = std::move(m);
        CHECK(m.get() == nullptr && m.bytes() == 0 && d.get() == pa && d.bytes() == 10);
        CHECK(A::frees == frees + 1 && A::live == 1);
        B& self = d;
        d = std::move(self);  // (self-assignment keeps the block)
        CHECK(d.get() == pa && A::live == 1);
        // a table swap: the new block moves in, the old one dies with its local
        {
            B nt;
            CHECK(nt.grow(40));
            B old = std::move(d);
            d = std::move(nt);
            CHECK(A::live == 2 && old.get() == pa && d.bytes() == 40);
        }
        CHECK(A::live == 1);
    }
    CHECK(A::live == 0);
    {  // chunks between two vectors, as wlog / wlog_free / the ctx's current pair
        std::vector<Chunk> log, free_list;
        for (unsigned i = 1; i <= 5; i++) log.push_back(make_chunk(i));  // (the vector reallocates on the way: elements move)
        CHECK(A::live == 10 && log.size() == 5);
        // the oldest leaves the log and goes to the free list (wlog_flush_oldest -> wlog_fold)
        Chunk k = std::move(log.front());
        log.erase(log.begin());
        CHECK(A::live == 10 && log.size() == 4 && log.front().n == 2 && k.n == 1);
        free_list.push_back(std::move(k));
        CHECK(A::live == 10 && k.seg.get() == nullptr && k.counts.get() == nullptr);
        // one from the middle is dropped whole (wlog_drop)
        free_list.push_back(std::move(log[1]));
        log.erase(log.begin() + 1);
        CHECK(A::live == 10 && log.size() == 3 && log[0].n == 2 && log[1].n == 4 && log[2].n == 5 && free_list.back().n == 3);
        for (const Chunk& c : log) CHECK(c.seg.bytes() == 64 * c.n && c.counts.bytes() == 16 * c.n && c.seg.get()[0] == 0xA5A5A5A5u);
        // a recycled pair becomes the current pair and is too small: both go, a new pair comes (ensure_wsegments)
        Buf<A, unsigned> cur_seg = std::move(free_list.back().seg), cur_counts = std::move(free_list.back().counts);
        free_list.pop_back();
        CHECK(A::live == 10 && free_list.size() == 1);
        cur_seg.reset();
        cur_counts.reset();
        CHECK(A::live == 8);
        CHECK(cur_seg.grow(1000) && cur_counts.grow(100));
        CHECK(A::live == 10);
        // ... and is recorded as the newest chunk (wlog_record)
        Chunk rec;
        rec.seg = std::move(cur_seg);
        rec.counts = std::move(cur_counts);
        rec.n = 6;
        log.push_back(std::move(rec));
        CHECK(A::live == 10 && cur_seg.get() == nullptr && log.back().seg.bytes() == 1000);
        // a chunk that nobody takes over is released at the end of its scope (wlog_fold on an error path)
        {
            Chunk lost = std::move(log.front());
            log.erase(log.begin());
        }
        CHECK(A::live == 8 && log.size() == 3);
        free_list.clear();
        CHECK(A::live == 6);
    }
    CHECK(A::live == 0 && A::calls == A::frees + 1);  // (every block was freed once; one call was told to fail)
    return 0;
}

int main() {
    const int rc = run();
    if (rc) return rc;
    if (A::live != 0) {
        printf("FAIL: %d blocks alive at exit\n", A::live);
        return 1;
    }
    printf("allocator calls %d, frees %d, live %d\nOK\n", A::calls, A::frees, A::live);
    return 0;
}
