// buffers_selftest.cpp — TEST-ONLY: the owners of mapad_amd/csrc/lib_buffers.hpp (DevBuf, DevEvent, and CoherentBuf beside them) compiled against
// counting stand-ins for the runtime calls the header makes: every allocation is a malloc, every event a one-byte block, and each stand-in counts what it gave
// out and what it got back.  Checks the growth rule, what a failed allocation leaves, moves, and that everything given out has come back when the owners are gone.
// lib_buffers.hpp is the one piece of the library source that stands alone (mapad_amd.hip includes it in front of the context).
// Built with the address and undefined-behaviour sanitizers by tests/test_buffers_host.py; never loaded by the product.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/mapad_amd.h"

// ---- the runtime, as far as lib_buffers.hpp asks for it ----
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct StandInEvent* hipEvent_t;
enum : unsigned { hipHostMallocPortable = 1, hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000u, hipEventDisableTiming = 2 };

static struct Counts { long dev_alloc, dev_free, host_alloc, host_free, ev_create, ev_destroy, errors_read; } N;
static int fail_next = 0;            // the next device allocations that fail
static hipError_t sticky = hipSuccess;  // what hipGetLastError hands out next
static size_t last_bytes = 0;
static unsigned last_flags = 0;

static const char* hipGetErrorString(hipError_t) { return "stand-in error"; }
static hipError_t hipGetLastError() { const hipError_t e = sticky; sticky = hipSuccess; ++N.errors_read; return e; }
static hipError_t hipMalloc(void** p, size_t bytes) {
    if (fail_next) { --fail_next; sticky = hipErrorOutOfMemory; return hipErrorOutOfMemory; }
    *p = std::malloc(std::max<size_t>(bytes, 1)); last_bytes = bytes; ++N.dev_alloc;
    return hipSuccess;
}
static hipError_t hipFree(void* p) { std::free(p); ++N.dev_free; return hipSuccess; }
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { *p = std::malloc(bytes); ++N.host_alloc; return hipSuccess; }
static hipError_t hipHostFree(void* p) { std::free(p); ++N.host_free; return hipSuccess; }
static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { *e = (hipEvent_t)std::malloc(1); last_flags = flags; ++N.ev_create; return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t e) { std::free(e); ++N.ev_destroy; return hipSuccess; }

#include "../../mapad_amd/csrc/lib_buffers.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("buffers selftest FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int event_twice(DevEvent& e) {  // (ensure() returns through HIP_TRY: it needs a caller that returns an int)
    if (e.ensure()) return 1;
    return e.ensure();
}

int main() {
    {   // growth: the rounding rule, the old block freed exactly once, no-ops below the capacity
        DevBuf<uint32_t> b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.ensure(100) == MAPAD_OK && b.p && b.cap == 176 && last_bytes == 176 * 4 && N.dev_alloc == 1 && N.dev_free == 0);
        uint32_t* const first = b.p;
        CHECK(b.ensure(50) == MAPAD_OK && b.p == first && b.cap == 176 && N.dev_alloc == 1);
        CHECK(b.ensure(176) == MAPAD_OK && b.p == first && N.dev_alloc == 1);
        CHECK(b.ensure(177) == MAPAD_OK && b.cap == 177 + 22 + 64 && N.dev_alloc == 2 && N.dev_free == 1);
        DevBuf<uint8_t> e;
        CHECK(e.ensure(100, true) == MAPAD_OK && e.cap == 100 && last_bytes == 100);
        CHECK(e.ensure(50) == MAPAD_OK && e.cap == 100 && e.ensure(50, true) == MAPAD_OK && e.cap == 100 && N.dev_alloc == 3);
        CHECK(e.ensure(0) == MAPAD_OK && N.dev_alloc == 3);
        // release() twice
        e.release();
        CHECK(e.p == nullptr && e.cap == 0 && N.dev_free == 2);
        e.release();
        CHECK(N.dev_free == 2);
    }
    CHECK(N.dev_alloc == 3 && N.dev_free == 3);
    {   // a failed allocation: MAPAD_ERR_NOMEM, empty, nothing sticky left behind; the old block is gone (as it is when the allocation succeeds); a later ensure works
        DevBuf<uint64_t> b;
        CHECK(b.ensure(10) == MAPAD_OK);
        fail_next = 1;
        CHECK(b.ensure(1000) == MAPAD_ERR_NOMEM && b.p == nullptr && b.cap == 0 && N.dev_free == 4);
        CHECK(sticky == hipSuccess && hipGetLastError() == hipSuccess);
        CHECK(b.ensure(1000, true) == MAPAD_OK && b.p && b.cap == 1000);
        fail_next = 1;
        DevBuf<uint64_t> never;
        CHECK(never.ensure(1) == MAPAD_ERR_NOMEM && never.p == nullptr && never.cap == 0);
    }
    CHECK(N.dev_alloc == 5 && N.dev_free == 5);
    {   // moves: the source ends empty, a buffer moved onto frees what it held once; swap
        DevBuf<int32_t> a, b;
        CHECK(a.ensure(10, true) == MAPAD_OK && b.ensure(20, true) == MAPAD_OK);
        int32_t* const pa = a.p;
        int32_t* const pb = b.p;
        DevBuf<int32_t> c(std::move(a));
        CHECK(c.p == pa && c.cap == 10 && a.p == nullptr && a.cap == 0 && N.dev_free == 5);
        b = std::move(c);  // (the duplicate table's growth: a fresh table over the old one)
        CHECK(b.p == pa && b.cap == 10 && c.p == nullptr && c.cap == 0 && N.dev_free == 6);
        DevBuf<int32_t>& self = b;
        b = std::move(self);
        CHECK(b.p == pa && b.cap == 10 && N.dev_free == 6);
        CHECK(a.ensure(30, true) == MAPAD_OK);
        int32_t* const pa2 = a.p;
        a.swap(b);
        CHECK(a.p == pa && a.cap == 10 && b.p == pa2 && b.cap == 30 && N.dev_free == 6);
        CHECK(a.ensure(10) == MAPAD_OK && a.p == pa && b.ensure(31) == MAPAD_OK && b.cap == 31 + 3 + 64 && N.dev_free == 7);
        (void)pb;
    }
    CHECK(N.dev_alloc == 9 && N.dev_free == 9);
    {   // events: created once, again after reset(), the flags passed on, moves
        DevEvent e;
        CHECK(!e && N.ev_create == 0);
        CHECK(event_twice(e) == MAPAD_OK && e && N.ev_create == 1 && last_flags == 0);
        const hipEvent_t raw = e;
        CHECK(raw == e.e);
        e.reset();
        CHECK(!e && N.ev_destroy == 1);
        e.reset();
        CHECK(N.ev_destroy == 1);
        CHECK(e.ensure(hipEventDisableTiming) == MAPAD_OK && e && N.ev_create == 2 && last_flags == hipEventDisableTiming);
        DevEvent f(std::move(e)), g;
        CHECK(!e && f && g.ensure() == MAPAD_OK && N.ev_create == 3);
        g = std::move(f);
        CHECK(!f && g && N.ev_destroy == 2);
    }
    CHECK(N.ev_create == 3 && N.ev_destroy == 3);
    {   // arrays of owners going out of scope, some of them never filled
        struct Slot { DevBuf<uint8_t> buf[5]; DevEvent ev[4]; DevBuf<float> one; };
        Slot s[3];
        for (auto& x : s) {
            for (int i = 0; i < 4; ++i) CHECK(x.buf[i].ensure(7 + i) == MAPAD_OK);
            for (int i = 0; i < 2; ++i) CHECK(x.ev[i].ensure() == MAPAD_OK);
        }
        CHECK(N.dev_alloc == 9 + 12 && N.ev_create == 3 + 6);
    }
    CHECK(N.dev_alloc == 21 && N.dev_free == 21 && N.ev_create == 9 && N.ev_destroy == 9);
    {   // the coherent block beside them is freed when it grows and with its owner
        CoherentBuf c;
        CHECK(c.ensure(100) && c.cap == 65536 && c.ensure(65537) && c.cap == 131072 && N.host_alloc == 2 && N.host_free == 1);
    }
    CHECK(N.host_alloc == 2 && N.host_free == 2);
    std::printf("buffers selftest ok\n");
    return 0;
}
