// tests/test_owned.py: the owners of facedeform_amd/csrc/fd_owned.h, as shipped, over the fake runtime of
// tests/tools/owned_fake/hip/hip_runtime.h.  Exit status 0 and nothing on stderr when every check holds; built and run under
// the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <string>
#include <vector>

#include "fd_owned.h"

using namespace fd;
using Calls = std::vector<std::string>;

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// the calls logged since `from`
static Calls since(size_t from) { return Calls(fake::log.begin() + (long)from, fake::log.end()); }

template <typename T>
static void devbuf_checks(size_t elem)
{
    DevBuf<T> b;
    CHECK(b.p == nullptr && b.cap == 0);
    // What the grow sequence of the owners' predecessor issued (fd_capi.hip's dev_grow over dev_alloc): nothing within the capacity;
    // else hipFree of a held block, then hipMalloc; no hipGetLastError on either outcome.
    size_t at = fake::log.size();
    CHECK(b.grow(10) == hipSuccess);
    CHECK(since(at) == Calls({"hipMalloc"}));
    CHECK(b.p != nullptr && b.cap == 10 && fake::bytes[b.p] == 10 * elem);
    T *first = b.p;
    at = fake::log.size();
    CHECK(b.grow(10) == hipSuccess && b.grow(3) == hipSuccess && b.grow(0) == hipSuccess);
    CHECK(since(at).empty());                                   // within capacity: no runtime call
    CHECK(b.p == first && b.cap == 10);
    at = fake::log.size();
    CHECK(b.grow(11) == hipSuccess);
    CHECK(since(at) == Calls({"hipFree", "hipMalloc"}));
    CHECK(b.cap == 11 && fake::bytes[b.p] == 11 * elem && fake::released[first] == 1);
    // a failed growth: null, capacity 0, the old block released once; the smaller request that follows allocates afresh
    T *second = b.p;
    fake::fail_in = 1;
    at = fake::log.size();
    CHECK(b.grow(100) == hipErrorOutOfMemory);
    CHECK(since(at) == Calls({"hipFree", "hipMalloc"}));
    CHECK(b.p == nullptr && b.cap == 0 && fake::released[second] == 1);
    at = fake::log.size();
    CHECK(b.grow(5) == hipSuccess);
    CHECK(since(at) == Calls({"hipMalloc"}));
    CHECK(b.p != nullptr && b.cap == 5 && fake::bytes[b.p] == 5 * elem);
    // the unconditional form: a new block even within the capacity; alloc(0) is one element
    T *third = b.p;
    at = fake::log.size();
    CHECK(b.alloc(2) == hipSuccess);
    CHECK(since(at) == Calls({"hipFree", "hipMalloc"}));
    CHECK(b.cap == 2 && fake::released[third] == 1);
    CHECK(b.alloc(0) == hipSuccess);
    CHECK(b.p != nullptr && b.cap == 1 && fake::bytes[b.p] == elem);
    fake::fail_in = 1;
    CHECK(b.alloc(7) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0);
    T *raw = b;                                                 // converts to its pointer
    CHECK(raw == nullptr);
    CHECK(b.alloc(7) == hipSuccess);
    raw = b;
    CHECK(raw == b.p);
    b.reset();
    CHECK(b.p == nullptr && b.cap == 0);
    at = fake::log.size();
    b.reset();                                                  // nothing held: no call
    CHECK(since(at).empty());
    CHECK(b.grow(4) == hipSuccess);                             // and the destructor releases this one
}

static void event_checks()
{
    Event e;
    size_t at = fake::log.size();
    CHECK(e.make() && e.ev != nullptr);
    hipEvent_t first = e.ev;
    CHECK(e.make() && e.make() && e.ev == first);               // created once and only once
    CHECK(since(at) == Calls({"hipEventCreateWithFlags"}));
    Event f;
    fake::fail_in = 1;
    at = fake::log.size();
    CHECK(!f.make() && f.ev == nullptr);                        // a failed creation: null, false, the error drained
    CHECK(since(at) == Calls({"hipEventCreateWithFlags", "hipGetLastError"}));
    CHECK(fake::last_error == hipSuccess);
    CHECK(f.make() && f.ev != nullptr);                         // and the next use tries again
    Event g;
    fake::fail_in = 1;
    at = fake::log.size();
    CHECK(g.create(hipEventDefault) == hipErrorOutOfMemory && g.ev == nullptr);
    CHECK(since(at) == Calls({"hipEventCreateWithFlags"}));    // the up-front form leaves the error to the caller
    CHECK(hipGetLastError() == hipErrorOutOfMemory);
    hipEvent_t raw = e;
    CHECK(raw == first);
}

static void others_fail_clean()
{
    Stream s;
    fake::fail_in = 1;
    CHECK(s.create() == hipErrorOutOfMemory && s.s == nullptr);
    Pinned<int> h;
    fake::fail_in = 1;
    CHECK(h.alloc(1, hipHostMallocDefault) == hipErrorOutOfMemory && h.p == nullptr);
    CHECK(h.alloc(0, hipHostMallocDefault) == hipSuccess && fake::bytes[h.p] == sizeof(int));
    int *old = h.p;
    CHECK(h.alloc(3, hipHostMallocDefault) == hipSuccess && fake::released[old] == 1 && fake::bytes[h.p] == 3 * sizeof(int));
    *h = 5;
    CHECK(h.p[0] == 5);
    // a block that leaves through release() is the caller's; adopt() takes it back
    Pinned<void> out;
    CHECK(out.alloc(16, hipHostMallocDefault) == hipSuccess);
    void *p = out.release();
    CHECK(out.p == nullptr && fake::released[p] == 0);
    {
        Pinned<void> in;
        in.adopt(p);
    }
    CHECK(fake::released[p] == 1);
    (void)hipGetLastError();
}

int main()
{
    devbuf_checks<float>(sizeof(float));
    devbuf_checks<double>(sizeof(double));
    devbuf_checks<void>(1);                                     // the byte-sized flavour
    event_checks();
    others_fail_clean();
    CHECK(fake::live() == 0 && fake::all_released_once());

    // one of each owner in a scope: everything handed out is released exactly once when it ends, the stream -- declared first --
    // after everything else
    fake::released.clear();
    const size_t at = fake::log.size();
    {
        Stream s;
        DevBuf<float> b;
        DevBuf<void> bytes;
        Pinned<int> h;
        Event lazy, upfront, never;
        GraphExec g, empty;
        CHECK(s.create() == hipSuccess && b.grow(8) == hipSuccess && b.grow(9) == hipSuccess && bytes.grow(100) == hipSuccess);
        CHECK(h.alloc(1, hipHostMallocDefault) == hipSuccess && lazy.make() && upfront.create(hipEventDisableTiming) == hipSuccess);
        g.exec = fake::graph_exec();
        hipGraphExec_t first = g.exec;
        g.reset();                                              // a graph captured again for another key
        CHECK(g.exec == nullptr && fake::released[first] == 1);
        g.exec = fake::graph_exec();
        CHECK(fake::live() == 7);
    }
    CHECK(fake::released.size() == 9);                          // 7 and the two replaced on the way
    CHECK(fake::live() == 0 && fake::all_released_once());
    CHECK(since(at).back() == "hipStreamDestroy");
    for (const std::string &c : since(at)) CHECK(c != "hipGetLastError");
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
