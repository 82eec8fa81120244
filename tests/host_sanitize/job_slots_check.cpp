// job_slots_check.cpp — pl-viwo_amd/csrc/job_slots.hpp on its own (plain g++, no HIP header on the include path), under ThreadSanitizer
// and AddressSanitizer + UBSan: the line worker's protocol driven by three bodies that read and write plain words.  Two rigs, each with
// its own worker and poster thread and nothing in common, run the whole sequence at once, first with spin budget 0 (every wait blocks)
// and then with the default budget (the waits poll): idle join and probe, the joiner reading the body's result, the order of service,
// a few thousand post / join rounds with naps on either side, and drain_and_quit on a loaded and on an idle worker.
// usage: job_slots_check [rounds]
#include <unistd.h>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../pl-viwo_amd/csrc/job_slots.hpp"

using plv::linehost::JobSlots;
using plv::linehost::spin_budget_us;
typedef std::chrono::steady_clock Clock;

enum { HAND_BACK = 0, DETECT = 1, FEED = 2 };  // line_api.hip's slots, in the order the worker serves them

static std::atomic<int> fails{0};
#define CHECK(c)                                                                      \
  do {                                                                                \
    if (!(c) && fails++ < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
  } while (0)

struct Rig {
  JobSlots slots;
  // plain words: `in` is the poster's until post(), `out`, `woke_ns` and `order` are the worker's until done()
  long in[3] = {0, 0, 0}, out[3] = {0, 0, 0}, woke_ns[3] = {0, 0, 0};
  std::vector<int> order;  // the slots in the order they were served
  int nap_us = 0;          // the bodies nap for up to this long
  unsigned rng;
  std::atomic<bool> gate_closed{false}, at_gate{false};  // (the test's own: holds the worker at the end of a body)
  std::thread worker;

  explicit Rig(unsigned seed) : rng(seed) { worker = std::thread([this] { serve(); }); }
  static long f(int s, long v) { return 3 * v + s + 1; }
  static void nap(unsigned &r, int max_us) {
    r = r * 1664525u + 1013904223u;
    const int us = max_us > 0 ? (int)((r >> 8) % (unsigned)(max_us + 1)) : 0;
    if (us >= 10) std::this_thread::sleep_for(std::chrono::microseconds(us));  // (shorter ones: none at all)
  }
  // a body as line_api.hip's: reads what was posted, writes its result, reports — and is then held at the gate, still inside
  void body(int s, unsigned &r) {
    woke_ns[s] = (long)std::chrono::duration_cast<std::chrono::nanoseconds>(slots.since_post(s)).count();
    nap(r, nap_us);
    out[s] = f(s, in[s]);
    order.push_back(s);
    slots.done(s);
    if (gate_closed) {
      at_gate = true;
      while (gate_closed) std::this_thread::yield();
      at_gate = false;
    }
  }
  void serve() {
    unsigned r = rng ^ 0x9e3779b9u;
    for (;;) {
      const int s = slots.take();
      if (s == JobSlots::kQuit) return;
      body(s, r);
    }
  }
};

static long sequence(unsigned seed, int rounds) {
  long done_rounds = 0;
  {
    Rig R(seed);
    // ---- idle: join returns false at once, nothing is busy
    for (int s = 0; s < 3; ++s) {
      const auto t0 = Clock::now();
      CHECK(!R.slots.join(s) && !R.slots.busy(s));
      CHECK(Clock::now() - t0 < std::chrono::milliseconds(100));
    }
    // ---- one job; the worker stays at the gate behind it.  busy from post to done, the result is the joiner's after join
    R.gate_closed = true;
    R.in[FEED] = 7;
    R.slots.post(FEED);
    CHECK(R.slots.join(FEED));
    CHECK(!R.slots.busy(FEED) && R.out[FEED] == Rig::f(FEED, 7) && R.woke_ns[FEED] >= 0);
    CHECK(!R.slots.join(FEED));
    while (!R.at_gate) std::this_thread::yield();
    // ---- all three posted behind the worker's back, lowest priority first: served hand-back, detect, feed
    const int rev[3] = {FEED, DETECT, HAND_BACK};
    for (int s : rev) R.in[s] = 100 + s, R.slots.post(s);
    for (int s = 0; s < 3; ++s) CHECK(R.slots.busy(s));
    std::this_thread::sleep_for(std::chrono::microseconds(200));
    CHECK(R.slots.since_post(FEED) >= std::chrono::microseconds(200));
    R.gate_closed = false;
    for (int s : rev) CHECK(R.slots.join(s) && !R.slots.busy(s) && R.out[s] == Rig::f(s, 100 + s));
    CHECK(R.order.size() == 4 && R.order[0] == FEED && R.order[1] == HAND_BACK && R.order[2] == DETECT && R.order[3] == FEED);
    // ---- rounds: a random set of slots posted and joined, naps of 0-50 us on either side
    R.nap_us = 50;
    unsigned r = seed * 2654435761u + 12345u;
    for (int i = 0; i < rounds; ++i) {
      r = r * 1664525u + 1013904223u;
      const unsigned set = ((r >> 20) % 7u) + 1u;
      const int first = (int)(r >> 28);  // (joined in a rotated order)
      for (int s = 0; s < 3; ++s)
        if (set >> s & 1u) {
          Rig::nap(r, 50);
          R.in[s] = 1000L * i + s;
          R.slots.post(s);
        }
      for (int q = 0; q < 3; ++q) {
        const int s = (q + first) % 3;
        if (!(set >> s & 1u)) {
          CHECK(!R.slots.join(s));
          continue;
        }
        Rig::nap(r, 50);
        CHECK(R.slots.join(s));
        CHECK(R.out[s] == Rig::f(s, 1000L * i + s) && !R.slots.busy(s));
        ++done_rounds;
      }
    }
    // ---- drain with all three posted: every body has run when it returns, and the thread ends
    R.nap_us = 200;
    for (int s = 0; s < 3; ++s) R.in[s] = -5 - s, R.slots.post(s);
    R.slots.drain_and_quit();
    for (int s = 0; s < 3; ++s) CHECK(!R.slots.busy(s));
    R.worker.join();
    for (int s = 0; s < 3; ++s) CHECK(R.out[s] == Rig::f(s, -5 - s));
  }
  // ---- drain on an idle worker
  Rig idle(seed + 1);
  idle.slots.drain_and_quit();
  idle.worker.join();
  CHECK(idle.order.empty());
  return done_rounds;
}

int main(int argc, char **argv) {
  alarm(240);  // (a lost wake-up hangs: the run then ends here, with a signal)
  const int rounds = argc > 1 ? atoi(argv[1]) : 3000;
  const int budgets[2] = {0, spin_budget_us().load()};
  long total = 0;
  for (int b : budgets) {
    spin_budget_us().store(b);
    long n[2] = {0, 0};
    std::thread other([&] { n[1] = sequence(77u + (unsigned)b, rounds); });  // two rigs at once, nothing shared
    n[0] = sequence(1234u + (unsigned)b, rounds);
    other.join();
    total += n[0] + n[1];
  }
  if (fails) {
    printf("FAILED: %d checks\n", fails.load());
    return 1;
  }
  printf("ok: job slots, %ld post / join rounds (spin budgets %d and %d us)\n", total, budgets[0], budgets[1]);
  return 0;
}
