// job_slots.hpp — how a library thread is handed work, free of device calls: the polling condition wait of the line front-end's
// threads (wait_polling, spin_budget_us) and the line worker's protocol (JobSlots): a few slots, one thread that serves them in the
// order of their numbers.  A slot is a state word and the time of its post; what a job does and the data it works on stay with the
// caller (line_api.hip: LineTracker).  tests/host_sanitize/job_slots_check.cpp drives this header alone under -fsanitize=thread / address.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <mutex>

namespace plv {
namespace linehost {

// Condition wait that polls first: the library's threads hand each other work several times per frame and a thread that blocked
// pays tens of microseconds (sometimes a millisecond) to be woken.  Polls for up to spin_us (the lock is released between probes),
// then blocks as usual — at camera rates the threads sleep between frames, back to back frames keep them awake.
// How long a waiting library thread polls before it blocks: process-wide, PLV_LINE_SPIN_US (default 300: the hand-overs inside one
// frame follow each other within that time, between frames the threads sleep; 0 = block at once, measured +10..25 us per frame) or
// plv_line_worker_config.
inline std::atomic<int> &spin_budget_us() {
  static std::atomic<int> v{getenv("PLV_LINE_SPIN_US") ? atoi(getenv("PLV_LINE_SPIN_US")) : 300};
  return v;
}
template <class Pred>
inline void wait_polling(std::unique_lock<std::mutex> &lk, std::condition_variable &cv, Pred pred, int spin_us = -1) {
  // `pred` reads atomics only (they are written under the mutex): the polling phase runs WITHOUT the mutex — round 5: eight threads
  // polling by locking and unlocking it kept the thread that wanted to post a job out of it for tens of microseconds
  if (pred()) return;
  if (spin_us < 0) spin_us = spin_budget_us().load(std::memory_order_relaxed);
  if (spin_us > 0) {
    lk.unlock();
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      for (int i = 0; i < 16; ++i) __builtin_ia32_pause();
      if (pred()) break;
      if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) break;
    }
    lk.lock();
    if (pred()) return;
  }
  cv.wait(lk, pred);
}

// kSlots slots served by one thread.  The poster side (one thread at a time per slot) posts a slot, may probe it, and joins it; the worker
// loops over take() and reports with done().  A state is written under the mutex and polled without it (wait_polling); what the
// poster wrote before post() the worker sees after take(), what the worker wrote before done() the joiner sees after join().
struct JobSlots {
  static const int kSlots = 3;
  typedef std::chrono::steady_clock Clock;
  enum { kQuit = -1 };
  // post: stores "posted" and the time, wakes the worker
  void post(int s) {
    std::unique_lock<std::mutex> lk(m);
    state[s] = POSTED, posted[s] = Clock::now();
    lk.unlock();
    cv.notify_all();
  }
  // posted and not done yet (never blocks, takes no lock)
  bool busy(int s) const { return state[s] == POSTED; }
  // false at once for an idle slot; else waits until the slot is done, leaves it idle and returns true
  bool join(int s) {
    if (state[s] == IDLE) return false;  // (only the poster's side makes an idle slot anything else)
    std::unique_lock<std::mutex> lk(m);
    wait_polling(lk, cv, [&] { return state[s] == DONE; });
    state[s] = IDLE;
    return true;
  }
  // the worker: waits for a posted slot and returns the lowest posted one, or kQuit
  int take() {
    int s = kSlots;
    std::unique_lock<std::mutex> lk(m);
    wait_polling(lk, cv, [&] { return (s = quit ? (int)kQuit : first_posted()) != kSlots; });  // (its last evaluation is under the mutex)
    return s;
  }
  // the worker: the job taken from slot s is over (a state that is no longer "posted" is left alone)
  void done(int s) {
    std::unique_lock<std::mutex> lk(m);
    if (state[s] == POSTED) state[s] = DONE;
    lk.unlock();
    cv.notify_all();
  }
  // lets every posted job finish, then makes take() return kQuit; the caller joins the thread
  void drain_and_quit() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return first_posted() == kSlots; });
    quit = true;
    lk.unlock();
    cv.notify_all();
  }
  // time from the slot's last post to `at`
  Clock::duration since_post(int s, Clock::time_point at = Clock::now()) const { return at - posted[s]; }
 private:
  enum { IDLE = 0, POSTED = 1, DONE = 2 };
  int first_posted() const {
    for (int s = 0; s < kSlots; ++s)
      if (state[s] == POSTED) return s;
    return kSlots;
  }
  std::mutex m;
  std::condition_variable cv;
  std::atomic<int> state[kSlots] = {};
  std::atomic<bool> quit{false};
  Clock::time_point posted[kSlots];
};

}  // namespace linehost
}  // namespace plv
