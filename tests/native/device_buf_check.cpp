// Runs host/device_buf.h over a counting fake backend for tests/test_device_buf.py: one scripted
// sequence of reserves, moves, releases and scope exits, once without a failure and once for every
// N with the N-th allocation failing.  One line per run:
//   run <N> allocs <allocations> hit <failures injected> checks <checks made> ok|FAIL
// (N = 0: no failure), preceded by one "FAIL <line>: <what>" line per check that did not hold.
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "../../nart_amd/csrc/host/device_buf.h"

namespace {

struct Block {
    int device;
    const void* owner;
};
struct Fake {
    int current = 0;               // the current device
    uintptr_t next = 0x1000;       // addresses are never handed out twice: a stale pointer stays stale
    std::map<void*, Block> live;
    std::map<void*, int> events;   // live events and the device they were created on
    long calls = 0, allocs = 0, fail_at = 0, hit = 0, checks = 0, failed = 0;
    const void* owner = nullptr;   // the buffer the script is reserving
} F;

#define CHECK(cond)                                        \
    do {                                                   \
        ++F.checks;                                        \
        if (!(cond)) {                                     \
            ++F.failed;                                    \
            std::printf("FAIL %d: %s\n", __LINE__, #cond); \
        }                                                  \
    } while (0)

struct FakeBackend {
    using event_t = void*;
    static int malloc(void** p, size_t bytes) {
        ++F.calls;
        CHECK(bytes > 0);
        for (const auto& b : F.live) CHECK(b.second.owner != F.owner);  // old and new never live together
        if (++F.allocs == F.fail_at) {
            ++F.hit;
            *p = reinterpret_cast<void*>(uintptr_t(0xBAD));  // a failed call's output is not to be trusted
            return 2;
        }
        *p = reinterpret_cast<void*>(F.next += 0x1000);
        F.live[*p] = Block{F.current, F.owner};
        return 0;
    }
    static int free(void* p) {
        ++F.calls;
        const auto it = F.live.find(p);
        CHECK(it != F.live.end());  // neither freed twice nor never allocated
        if (it == F.live.end()) return 1;
        CHECK(it->second.device == F.current);  // freed with the owning device current
        F.live.erase(it);
        return 0;
    }
    static int get_device(int* d) {
        ++F.calls;
        *d = F.current;
        return 0;
    }
    static int set_device(int d) {
        ++F.calls;
        F.current = d;
        return 0;
    }
    static int event_create(event_t* e) {
        ++F.calls;
        *e = reinterpret_cast<void*>(F.next += 0x1000);
        F.events[*e] = F.current;
        return 0;
    }
    static int event_destroy(event_t e) {
        ++F.calls;
        const auto it = F.events.find(e);
        CHECK(it != F.events.end());
        if (it == F.events.end()) return 1;
        CHECK(it->second == F.current);
        F.events.erase(it);
        return 0;
    }
};
using Buf = nd::DevBuf<FakeBackend>;
using Event = nd::DevEvent<FakeBackend>;

// What holds of a buffer whenever the script looks at it: empty, or its block live (not used after free).
void look(const Buf& b) {
    if (!b) {
        CHECK(b.bytes() == 0);
        return;
    }
    CHECK(b.bytes() > 0);
    const auto it = F.live.find(b.as<void>());
    CHECK(it != F.live.end());
    if (it != F.live.end()) CHECK(it->second.device == b.device());
}

// One reserve and everything the issue asks of it; a failed one is followed at once by the same reserve.
void reserve(Buf& b, int device, size_t bytes) {
    const int caller = F.current;
    const long calls = F.calls, allocs = F.allocs;
    const size_t had = b.bytes();
    void* const ptr = b.as<void>();
    F.owner = &b;
    int rc = b.reserve(device, bytes);
    CHECK(F.current == caller);
    if (bytes <= had) {  // smaller, equal or zero: no backend call, nothing moves
        CHECK(rc == 0 && F.calls == calls && b.as<void>() == ptr && b.bytes() == had);
        look(b);
        return;
    }
    CHECK(F.allocs == allocs + 1);
    CHECK(F.live.count(ptr) == 0);  // the old block is gone whether or not the new one came
    if (rc) {
        CHECK(!b && b.bytes() == 0 && b.as<void>() == nullptr);
        const long before = F.allocs;
        rc = b.reserve(device, bytes);
        CHECK(rc == 0 && F.allocs == before + 1);
        CHECK(F.current == caller);
    }
    CHECK(rc == 0 && b && b.bytes() == bytes && b.device() == device);
    look(b);
}

// A group of three buffers of one capacity, as render.hip's ensure() keeps them.
struct Group {
    Buf b[3];
    size_t cap = 0;
    int reserve(int device, size_t count) {
        return nd::reserve_group<FakeBackend>(
            cap, count, {{&b[0], count * 4, "a"}, {&b[1], count * 16, "b"}, {&b[2], count * 4, "c"}},
            [&](Buf& one, size_t bytes, const char*) {
                // all of the group's buffers were freed before the first of them is allocated
                for (Buf* later = &one; later < b + 3; ++later) CHECK(!*later);
                F.owner = &one;
                return one.reserve(device, bytes);
            });
    }
};
void reserve(Group& g, int device, size_t count) {
    const int caller = F.current;
    const long calls = F.calls;
    const size_t had = g.cap;
    int rc = g.reserve(device, count);
    CHECK(F.current == caller);
    if (count <= had) {
        CHECK(rc == 0 && F.calls == calls && g.cap == had);
    } else {
        if (rc) {
            CHECK(g.cap == 0);  // never a stale capacity over a null buffer
            bool empty = false;
            for (const Buf& b : g.b) empty = empty || !b;
            CHECK(empty);
            rc = g.reserve(device, count);
            CHECK(F.current == caller);
        }
        CHECK(rc == 0 && g.cap == count);
        for (int i = 0; i < 3; ++i) CHECK(g.b[i].bytes() == count * (i == 1 ? 16 : 4) && g.b[i].device() == device);
    }
    for (const Buf& b : g.b) look(b);
}

// After a move: the block is b's now.
void own(const Buf& b) {
    const auto it = F.live.find(b.as<void>());
    if (it != F.live.end()) it->second.owner = &b;
}

void script() {
    FakeBackend::set_device(0);
    {
        Buf a, b, c;
        Group g;
        reserve(a, 0, 100);   // growing from empty
        reserve(a, 0, 100);   // equal
        reserve(a, 0, 40);    // smaller
        reserve(a, 0, 0);     // zero
        reserve(c, 0, 0);     // zero on an empty buffer: stays empty
        CHECK(!c);
        reserve(b, 1, 64);    // another ordinal than the caller's
        reserve(a, 0, 1000);  // growing: the old block goes first
        FakeBackend::set_device(1);
        reserve(a, 0, 5000);  // growing from the other device
        reserve(b, 1, 10);
        reserve(b, 1, 65);
        reserve(g, 0, 10);
        reserve(g, 0, 10);
        reserve(g, 0, 5);
        reserve(g, 0, 0);
        reserve(g, 0, 30);
        FakeBackend::set_device(0);
        reserve(g, 0, 31);
        look(a), look(b);

        // a move: the block changes hands without a backend call; the source is empty
        long calls = F.calls;
        void* const pa = a.as<void>();
        Buf m(std::move(a));
        own(m);
        CHECK(F.calls == calls && !a && a.bytes() == 0 && m.as<void>() == pa && m.bytes() == 5000 && m.device() == 0);
        reserve(a, 1, 7);  // the moved-from buffer is an empty buffer like any other
        // a move onto a buffer that holds a block: that block is freed on its device, the caller's stays
        const size_t live = F.live.size();
        b = std::move(m);
        own(b);
        CHECK(F.current == 0 && F.live.size() == live - 1 && b.as<void>() == pa && b.device() == 0 && !m);
        look(b);
        std::vector<Buf> v;  // as nart_ctx::env_bufs grows
        for (int i = 0; i < 5; ++i) {
            calls = F.calls;
            v.emplace_back();  // (a reallocation moves the others)
            CHECK(F.calls == calls);
            for (const Buf& e : v) own(e);
            reserve(v.back(), i & 1, 8 + i);
            for (const Buf& e : v) look(e);
        }

        // a release: empty afterwards, a second one calls nothing, the next reserve allocates
        FakeBackend::set_device(1);
        b.release();
        CHECK(F.current == 1 && !b && b.bytes() == 0 && F.live.count(pa) == 0);
        calls = F.calls;
        b.release();
        CHECK(F.calls == calls);
        reserve(b, 0, 5);
        reserve(b, 0, 6);

        // a scope exit: the block and the events go with their owners, the caller's device stays
        {
            Buf s;
            reserve(s, 0, 77);
            Event used[2], unused;
            void *e0 = nullptr, *e1 = nullptr, *again = nullptr;
            FakeBackend::set_device(0);
            CHECK(used[0].handle() == nullptr);
            CHECK(used[0].get(&e0) == 0 && e0 && F.events.size() == 1);
            calls = F.calls;
            CHECK(used[0].get(&again) == 0 && again == e0 && F.calls == calls && used[0].handle() == e0);
            FakeBackend::set_device(1);
            CHECK(used[1].get(&e1) == 0 && e1 != e0 && F.events.size() == 2);
        }
        CHECK(F.current == 1 && F.events.empty());
        FakeBackend::set_device(0);
    }
    CHECK(F.current == 0);
    CHECK(F.live.empty());
    CHECK(F.events.empty());
}

long run(long fail_at) {
    F = Fake();
    F.fail_at = fail_at;
    script();
    const bool ok = F.failed == 0 && F.hit == (fail_at ? 1 : 0);
    std::printf("run %ld allocs %ld hit %ld checks %ld %s\n", fail_at, F.allocs, F.hit, F.checks, ok ? "ok" : "FAIL");
    return ok ? F.allocs : -1;
}

}  // namespace

int main() {
    const long length = run(0);  // the sequence's allocations
    bool ok = length > 0;
    for (long n = 1; n <= length; ++n) ok = run(n) > length && ok;  // (a retry allocates again)
    return ok ? 0 : 1;
}
