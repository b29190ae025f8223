// host_events.cpp - EventPool (flow-pipeline_amd/csrc/events.h) over a fake event API: an event is a malloc'ed record, the API
// counts creates and destroys, can be told to fail its N-th create and answers elapsed_ms with a time the test sets.  Built with
// -fsanitize=address,undefined and run on its own by tests/test_host_events.py: an event destroyed twice or never ends the run
// through the sanitizers, a wrong count through CHECK.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "../flow-pipeline_amd/csrc/events.h"

struct FakeApi {
    struct Rec {
        int id;
        bool timing;
    };
    typedef Rec* Event;
    static int creates, destroys, calls, fail_at;  // fail_at: the create call (counted from 1) that fails; 0 = none
    static float ms;                               // what elapsed_ms answers
    static bool elapsed_ok;
    static bool create(Event* e, bool timing) {
        if (++calls == fail_at) return false;
        *e = (Rec*)malloc(sizeof(Rec));
        if (!*e) return false;
        (*e)->id = creates++;
        (*e)->timing = timing;
        return true;
    }
    static void destroy(Event e) {
        free(e);
        destroys++;
    }
    static bool elapsed_ms(float* out, Event e0, Event e1) {
        if (!elapsed_ok || !e0->timing || !e1->timing) return false;
        *out = ms;
        return true;
    }
};
int FakeApi::creates = 0, FakeApi::destroys = 0, FakeApi::calls = 0, FakeApi::fail_at = 0;
float FakeApi::ms = 0;
bool FakeApi::elapsed_ok = true;
using A = FakeApi;
using Pool = EventPool<A>;

// Copying does not compile (two owners would destroy every event twice), and neither does moving: a pool lives where its state does.
static_assert(!std::is_copy_constructible<Pool>::value && !std::is_copy_assignable<Pool>::value, "EventPool is never copied");
static_assert(!std::is_move_constructible<Pool>::value && !std::is_move_assignable<Pool>::value, "EventPool is never moved");

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int run() {
    {  // a fixed set: ensure creates only what is missing; indexed as an array
        Pool p;
        CHECK(p.size() == 0 && p.used() == 0 && A::creates == 0);
        CHECK(p.ensure(4) && p.size() == 4 && p.used() == 0 && A::creates == 4);
        CHECK(p.ensure(4) && p.ensure(2) && p.ensure(0) && A::creates == 4 && A::calls == 4);
        for (int i = 0; i < 4; i++) CHECK(p[i]->id == i && p[i]->timing);
        CHECK(p.ensure(6) && p.size() == 6 && A::creates == 6 && p[5]->id == 5);
    }  // the destructor destroys each once
    CHECK(A::destroys == 6);
    {  // take: k consecutive events, the cursor moves, only the missing ones are created
        const int c0 = A::creates;
        Pool p;
        CHECK(p.ensure(2));  // (the load pool: two events bracket the decode)
        p.rewind(2);
        A::Event* e = p.take(3);
        CHECK(e && p.used() == 5 && p.size() == 5 && A::creates == c0 + 5);
        CHECK(e[0] == p[2] && e[1] == p[3] && e[2] == p[4] && e[0]->id == c0 + 2 && e[2]->id == c0 + 4);
        e = p.take(3);
        CHECK(e && e[0] == p[5] && e[2] == p[7] && p.used() == 8 && A::creates == c0 + 8);
        // rewind(2), take(3): events 2..4 again, nothing created
        p.rewind(2);
        CHECK(p.used() == 2 && p.size() == 8);
        e = p.take(3);
        CHECK(e && e[0] == p[2] && e[1] == p[3] && e[2] == p[4] && p.used() == 5 && A::creates == c0 + 8);
        // the owner's limit: it asks before the take, reads and rewinds; the pool itself never drains
        const size_t limit = 2 + 3 * 2;
        CHECK(p.used() + 3 <= limit);
        CHECK(p.take(3) && p.used() == 8 && !(p.used() + 3 <= limit));
        p.rewind(2);
        CHECK(p.take(3) && p.used() == 5 && A::creates == c0 + 8);
    }
    CHECK(A::destroys == A::creates);
    {  // a create that fails in the middle of take(3): nothing unowned, the cursor where it was; a later take reuses what was created
        const int c0 = A::creates;
        Pool p;
        CHECK(p.take(3) && p.used() == 3);
        A::fail_at = A::calls + 2;  // the second of the next three
        CHECK(p.take(3) == nullptr);
        CHECK(p.used() == 3 && p.size() == 4 && A::creates == c0 + 4);  // (the first of them stays owned)
        A::fail_at = 0;
        A::Event* e = p.take(3);
        CHECK(e && p.used() == 6 && p.size() == 6 && A::creates == c0 + 6);  // (two more, not three)
        CHECK(e[0]->id == c0 + 3 && e[1]->id == c0 + 4 && e[2]->id == c0 + 5);
        // ... and a failed ensure likewise
        A::fail_at = A::calls + 1;
        CHECK(!p.ensure(7) && p.size() == 6 && p.used() == 6);
        A::fail_at = 0;
    }
    CHECK(A::destroys == A::creates);
    {  // the timing flag reaches create; untimed events are no stopwatch
        Pool sync(false), timed(true);
        CHECK(sync.ensure(2) && timed.ensure(2));
        CHECK(!sync[0]->timing && !sync[1]->timing && timed[0]->timing && timed[1]->timing);
        uint64_t ns = 7;
        CHECK(!Pool::elapsed_ns(sync[0], sync[1], &ns) && ns == 7);
    }
    {  // elapsed_ns adds (uint64_t)((double)ms * 1e6); a failed query adds nothing
        Pool p;
        CHECK(p.ensure(2));
        const float cases[3] = {0.0f, 0.5f, 1234.5f};
        uint64_t sum = 0, want = 0;
        for (float ms : cases) {
            A::ms = ms;
            CHECK(Pool::elapsed_ns(p[0], p[1], &sum));
            want += (uint64_t)((double)ms * 1e6);
            CHECK(sum == want);
        }
        CHECK(sum == 500000ull + 1234500000ull);
        A::elapsed_ok = false;
        A::ms = 99.0f;
        CHECK(!Pool::elapsed_ns(p[0], p[1], &sum) && sum == want);
        A::elapsed_ok = true;
    }
    CHECK(A::destroys == A::creates);
    return 0;
}

int main() {
    const int rc = run();
    if (rc) return rc;
    if (A::creates != A::destroys) {
        printf("FAIL: %d events created, %d destroyed\n", A::creates, A::destroys);
        return 1;
    }
    printf("creates %d, destroys %d, failed creates %d\nOK\n", A::creates, A::destroys, A::calls - A::creates);
    return 0;
}
