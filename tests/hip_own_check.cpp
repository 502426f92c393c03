// hip_own_check.cpp -- csrc/hip_own.hpp on the CPU, under the host sanitizers (tests/test_hip_own.py compiles and runs it; no HIP runtime
// is linked).  The handful of HIP calls the header makes are counting, malloc-backed stand-ins here; one of them can be told to fail once.
// The program walks the owners through what the library does with them and ends with the live counter at 0 and every stand-in
// allocation freed; anything else is exit status 1 (or the sanitizer's report).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_own.hpp"

namespace {
long n_dev = 0, n_pinned = 0, n_event = 0, n_stream = 0;      // stand-in objects alive
long n_acquired = 0;                                           // ... and ever handed out
const char *fail_next = nullptr;                               // the call of this name fails once

bool failing(const char *name)
{
    if (!fail_next || strcmp(fail_next, name) != 0) return false;
    fail_next = nullptr;
    return true;
}
hipError_t take(const char *name, void **out, size_t bytes, long &alive)
{
    if (failing(name)) return hipErrorOutOfMemory;        // (*out is left as it was, like the runtime's)
    *out = malloc(bytes ? bytes : 1);
    if (!*out) return hipErrorOutOfMemory;
    ++alive;
    ++n_acquired;
    return hipSuccess;
}
hipError_t give(void *p, long &alive)
{
    if (!p) return hipSuccess;
    free(p);
    --alive;
    return hipSuccess;
}

int failures = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

long live() { return ndp::live_resources.load(); }
long standins() { return n_dev + n_pinned + n_event + n_stream; }
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return take("hipMalloc", p, n, n_dev); }
hipError_t hipFree(void *p) { return give(p, n_dev); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return take("hipHostMalloc", p, n, n_pinned); }
hipError_t hipHostFree(void *p) { return give(p, n_pinned); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return take("hipEventCreateWithFlags", (void **)e, 8, n_event); }
hipError_t hipEventDestroy(hipEvent_t e) { return give(e, n_event); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return take("hipStreamCreateWithFlags", (void **)s, 8, n_stream); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return take("hipStreamCreateWithPriority", (void **)s, 8, n_stream); }
hipError_t hipStreamDestroy(hipStream_t s) { return give(s, n_stream); }
}

using ndp::DevBuf;
using ndp::Event;
using ndp::PinnedBuf;
using ndp::Stream;

// a handle in small: streams first (destroyed last), buffers, a page-locked block, events, an array of each
struct Owners {
    Stream stream, aux;
    DevBuf<double> a, b;
    DevBuf<float> ab[2];
    PinnedBuf<unsigned char> mirror;
    Event ev, done[4];
};

// the formation config: built into a local buffer, committed into the owner only behind a successful "copy"
static hipError_t config(DevBuf<int> &owner, size_t n, bool copy_ok)
{
    owner.reset();
    DevBuf<int> blk;
    hipError_t e = blk.alloc(n * sizeof(int));
    if (e != hipSuccess) return e;
    for (size_t i = 0; i < n; ++i) blk[i] = (int)i;
    if (!copy_ok) return hipErrorInvalidValue;         // blk goes out of scope: nothing stays configured
    owner = std::move(blk);
    return hipSuccess;
}

int main()
{
    {   // alloc over a live buffer: the old block goes first, one object stays
        DevBuf<double> d;
        CHECK(!d && d.get() == nullptr && live() == 0);
        CHECK(d.alloc(64) == hipSuccess && d && live() == 1 && n_dev == 1);
        double *first = d;
        first[7] = 1.0;
        CHECK(d.alloc(128) == hipSuccess && live() == 1 && n_dev == 1 && n_acquired == 2);
        d[15] = 2.0;
        // ensure twice: neither allocates
        double *p = d;
        CHECK(d.ensure(4096) == hipSuccess && d.ensure(8) == hipSuccess && p == d.get() && n_acquired == 2);
        // a failed alloc: the buffer is null, the old block is gone, the counter counts nothing
        fail_next = "hipMalloc";
        CHECK(d.alloc(32) == hipErrorOutOfMemory && !d && live() == 0 && n_dev == 0);
        // ... and ensure on the null buffer allocates again
        CHECK(d.ensure(32) == hipSuccess && d && live() == 1);
        // a failed first ensure leaves null and the counter unchanged
        DevBuf<int> never;
        fail_next = "hipMalloc";
        CHECK(never.ensure(16) == hipErrorOutOfMemory && !never && live() == 1);
        // reset on null, twice
        never.reset();
        never.reset();
        CHECK(live() == 1);
    }
    CHECK(live() == 0 && standins() == 0);
    {   // move construction and move assignment into a live target
        DevBuf<float> a, b;
        CHECK(a.alloc(16) == hipSuccess && b.alloc(16) == hipSuccess && live() == 2);
        float *pa = a;
        DevBuf<float> c(std::move(a));
        CHECK(!a && c.get() == pa && live() == 2);
        b = std::move(c);                               // b's own block is released
        CHECK(!c && b.get() == pa && live() == 1 && n_dev == 1);
        DevBuf<float> &same = b;
        b = std::move(same);                            // self-assignment keeps it
        CHECK(b.get() == pa && live() == 1);
        PinnedBuf<unsigned char> h1, h2;
        CHECK(h1.alloc(256) == hipSuccess && live() == 2 && n_pinned == 1);
        h1[255] = 9;
        h2 = std::move(h1);
        CHECK(!h1 && h2 && h2[255] == 9 && live() == 2);
        fail_next = "hipHostMalloc";
        CHECK(h2.alloc(64) == hipErrorOutOfMemory && !h2 && n_pinned == 0 && live() == 1);
    }
    CHECK(live() == 0 && standins() == 0);
    {   // events and streams: ensure creates once, a failed create leaves null, moves carry the object
        Event e;
        CHECK(!e && e.ensure(hipEventDisableTiming) == hipSuccess && e && live() == 1);
        hipEvent_t raw = e;
        CHECK(e.ensure(hipEventDefault) == hipSuccess && raw == (hipEvent_t)e && n_event == 1);
        Event f(std::move(e));
        CHECK(!e && (hipEvent_t)f == raw && live() == 1);
        Event g;
        fail_next = "hipEventCreateWithFlags";
        CHECK(g.ensure(hipEventDefault) != hipSuccess && !g && live() == 1);
        g = std::move(f);
        CHECK((hipEvent_t)g == raw && live() == 1);
        g.reset();
        g.reset();
        CHECK(live() == 0 && n_event == 0);
        Stream s, p;
        CHECK(s.ensure(hipStreamNonBlocking) == hipSuccess && p.ensure(hipStreamNonBlocking, -1) == hipSuccess && live() == 2 && n_stream == 2);
        hipStream_t rs = s;
        CHECK(s.ensure(hipStreamNonBlocking, -1) == hipSuccess && (hipStream_t)s == rs && n_stream == 2);
        p = std::move(s);
        CHECK(!s && (hipStream_t)p == rs && live() == 1 && n_stream == 1);
        Stream q;
        fail_next = "hipStreamCreateWithPriority";
        CHECK(q.ensure(hipStreamNonBlocking, 0) != hipSuccess && !q && live() == 1);
    }
    CHECK(live() == 0 && standins() == 0);
    {   // a struct of several owners, partly filled (a create that failed half-way), going out of scope
        Owners o;
        CHECK(o.stream.ensure(hipStreamNonBlocking) == hipSuccess && o.a.alloc(80) == hipSuccess && o.ab[1].alloc(12) == hipSuccess);
        CHECK(o.mirror.alloc(512) == hipSuccess && o.ev.ensure(hipEventDisableTiming) == hipSuccess);
        for (Event &e : o.done) CHECK(e.ensure(hipEventDisableTiming) == hipSuccess);
        fail_next = "hipMalloc";
        CHECK(o.b.alloc(80) != hipSuccess);
        CHECK(live() == 9 && standins() == 9);
    }
    CHECK(live() == 0 && standins() == 0);
    {   // build locally, commit on success
        DevBuf<int> index;
        CHECK(config(index, 10, true) == hipSuccess && index && index[9] == 9 && live() == 1);
        CHECK(config(index, 20, false) != hipSuccess && !index && live() == 0 && n_dev == 0);      // the failed copy: not configured, nothing held
        fail_next = "hipMalloc";
        CHECK(config(index, 20, true) != hipSuccess && !index && live() == 0);
        CHECK(config(index, 20, true) == hipSuccess && index[19] == 19 && live() == 1 && n_dev == 1);
        CHECK(config(index, 5, true) == hipSuccess && live() == 1 && n_dev == 1);                   // a second configuration replaces the first
    }
    CHECK(live() == 0 && standins() == 0 && n_acquired > 0);
    if (failures) return 1;
    printf("hip_own_check: %ld stand-in objects acquired and released, live counter 0\n", n_acquired);
    return 0;
}
