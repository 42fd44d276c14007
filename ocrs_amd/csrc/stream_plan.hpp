// The stream plan of one device: which lane a call's work goes to, and the accounting behind that choice.  No HIP in here:
// DeviceContext (common.hpp) owns the streams and asks this header which of them a call gets; ocrs_stream_plan_selftest
// drives the same code from a host-only test.
//
// A device with a stream budget of N >= 3 owns exactly N streams, created together and in this order: the conv lane (all
// recognition conv stacks), the recurrence lane (all persistent GRU recurrences), then N - 2 LIGHT lanes that every other
// launch of every call shares.  The runtime multiplexes streams onto a handful of hardware queues (four by default), and
// a packet waiting in a queue holds back every packet behind it whatever stream that came from: a budget no larger than
// the queue count gives every lane a queue of its own, where a stream per call in flight (budget 0, the earlier plan)
// leaves which calls share a queue with the conv lane to the runtime's bookkeeping.
//
// What keeps shared lanes live:
//   * everything queued on a light lane is runnable when it is queued.  A light lane is never made to wait for work on
//     the conv or recurrence lane; the call's host thread waits for that event and enqueues the dependants when it wakes
//     (a call that finds the device otherwise idle may park the wait on its lane: there is nobody to hold up, and a later
//     call is dealt another lane while there is one).  The two dedicated lanes may wait for light-lane work, which by the
//     rule is already runnable;
//   * an event is recorded before anything, host or stream, waits for it;
//   * no host wait happens while heavy_phase, rec_phase, stream_mu or a coalescer lock is held;
//   * a call never waits for a whole lane, only for an event recorded after its own last enqueue, and its scratch goes
//     back to the pool after that event.
#pragma once
#include <mutex>
#include <vector>

namespace ocrs {

class LanePlan {
  public:
    enum { kMinBudget = 3, kMaxBudget = 16, kDefaultBudget = 4, kPrivate = -1 };
    static bool valid_budget(long b) { return b == 0 || (b >= kMinBudget && b <= kMaxBudget); }

    explicit LanePlan(int budget = kDefaultBudget) { (void)set_budget(budget); }

    // 0 = a private stream per call (no lanes).  Refused (false) while a call holds a lease, unless nothing changes.
    bool set_budget(int budget) {
        std::lock_guard<std::mutex> g(mu_);
        if (!valid_budget(budget)) return false;
        if (budget == budget_) return true;
        if (outstanding_ > 0) return false;
        budget_ = budget;
        load_.assign(budget ? budget - 2 : 0, 0);
        next_ = 0;
        return true;
    }
    int budget() const { std::lock_guard<std::mutex> g(mu_); return budget_; }
    int light_lanes() const { std::lock_guard<std::mutex> g(mu_); return (int)load_.size(); }
    int outstanding() const { std::lock_guard<std::mutex> g(mu_); return outstanding_; }
    int load(int lane) const { std::lock_guard<std::mutex> g(mu_); return lane >= 0 && lane < (int)load_.size() ? load_[lane] : 0; }

    // A call starts: the light lane with the fewest calls on it, ties broken round-robin (the search starts behind the lane
    // dealt last); `avoid` (a lane this caller already uses) is passed over while there is another.  kPrivate at budget 0.
    int acquire(int avoid = kPrivate) {
        std::lock_guard<std::mutex> g(mu_);
        outstanding_++;
        const int n = (int)load_.size();
        if (n == 0) return kPrivate;
        int best = -1;
        for (int i = 0; i < n; i++) {
            const int lane = (next_ + i) % n;
            if (lane == avoid && n > 1) continue;
            if (best < 0 || load_[lane] < load_[best]) best = lane;
        }
        load_[best]++;
        next_ = (best + 1) % n;
        return best;
    }
    // The call is over; calls may end in any order.
    void release(int lane) {
        std::lock_guard<std::mutex> g(mu_);
        outstanding_--;
        if (lane >= 0 && lane < (int)load_.size()) load_[lane]--;
    }

  private:
    mutable std::mutex mu_;
    int budget_ = -1, outstanding_ = 0, next_ = 0;
    std::vector<int> load_;
};

}  // namespace ocrs
