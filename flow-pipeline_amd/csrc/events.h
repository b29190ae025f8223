// events.h - the one owner of a HIP event (plain C++17, no HIP include: the tests compile it alone).
//
// EventPool<Api> owns a vector of events and a cursor; its destructor destroys every event once.  Api supplies
//   typedef ... Event;   static bool create(Event* e, bool timing);   static void destroy(Event e);
//   static bool elapsed_ms(float* ms, Event e0, Event e1);
// Never copied, never moved.  A fixed set is ensure(n) and pool[i]; a growing one hands out take(k) and starts over with
// rewind().  The pool knows no limit and drains nothing: its owner asks used() / size() before the next take and reads what is
// pending first.  A pointer take() returned is good until the next take or ensure.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

template <class Api>
class EventPool {
    using Event = typename Api::Event;
    std::vector<Event> ev_;
    size_t used_ = 0;
    bool timing_;

public:
    explicit EventPool(bool timing = true) : timing_(timing) {}
    EventPool(const EventPool&) = delete;
    EventPool& operator=(const EventPool&) = delete;
    ~EventPool() {
        for (Event e : ev_) Api::destroy(e);
    }

    // Events [0, n) exist afterwards.  false: a creation failed; what was created before it stays owned.
    bool ensure(size_t n) {
        if (n > ev_.capacity()) ev_.reserve(n > 2 * ev_.capacity() ? n : 2 * ev_.capacity());  // (no push_back below can throw with an event in hand)
        while (ev_.size() < n) {
            Event e;
            if (!Api::create(&e, timing_)) return false;
            ev_.push_back(e);
        }
        return true;
    }
    // The next k events, consecutive.  nullptr: a creation failed and the cursor has not moved.
    Event* take(size_t k) {
        if (!ensure(used_ + k)) return nullptr;
        Event* e = ev_.data() + used_;
        used_ += k;
        return e;
    }
    size_t used() const { return used_; }
    size_t size() const { return ev_.size(); }
    void rewind(size_t to = 0) { used_ = to; }
    Event operator[](size_t i) const { return ev_[i]; }

    // The time from e0 to e1 (both reached), added to *add in nanoseconds.  false: the query failed, nothing was added.
    static bool elapsed_ns(Event e0, Event e1, uint64_t* add) {
        float ms = 0;
        if (!Api::elapsed_ms(&ms, e0, e1)) return false;
        *add += (uint64_t)((double)ms * 1e6);
        return true;
    }
};
