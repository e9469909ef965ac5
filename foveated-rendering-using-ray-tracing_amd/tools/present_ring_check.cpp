// present_ring_check — the present ring's bookkeeping (csrc/present_ring.h) under the host sanitizers, with its own
// main and no device: a few thousand random enqueue / acquire / release / re-enable steps per ring size against a
// model. The model: a ticket is live from its enqueue to its release; an enqueue succeeds exactly when fewer than n
// tickets are live and then returns the count of enqueues that succeeded so far; a live ticket names one slot, which
// no other live ticket names. (make ring-check)
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>

#include "../csrc/present_ring.h"

static int fails = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } \
  } while (0)

int main() {
  using fr::PresentRing;
  std::mt19937 rng(20261021u);
  PresentRing r;
  uint64_t issued = 0;  // the model's ticket count: it survives a reset, as the ring's does
  CHECK(r.n == 0 && r.all_free());
  {
    uint64_t t = 77;
    CHECK(r.enqueue(&t) == -1 && t == 77);  // a ring that is off takes nothing
    CHECK(r.find(0) == -1 && r.find(1) == -1);
  }
  for (int n = 1; n <= PresentRing::MAX_SLOTS; n++) {
    r.reset(n);
    std::map<uint64_t, int> live;  // ticket -> slot
    std::map<uint64_t, bool> held;
    CHECK(r.all_free());
    for (int step = 0; step < 4000; step++) {
      const unsigned op = rng() % 8;
      if (op < 3) {  // enqueue
        uint64_t t = 0;
        const int s = r.enqueue(&t);
        if ((int)live.size() < n) {
          CHECK(s >= 0 && s < n && t == ++issued);
          for (const auto& kv : live) CHECK(kv.second != s);
          live[t] = s;
          held[t] = false;
          CHECK(r.state[s] == PresentRing::FLIGHT);
        } else {
          CHECK(s == -1 && t == 0);  // the backpressure: nothing written
        }
      } else if (op < 5 && !live.empty()) {  // acquire a random live ticket (twice is fine)
        auto it = live.begin();
        std::advance(it, rng() % live.size());
        CHECK(r.find(it->first) == it->second);
        r.acquired(it->second);
        held[it->first] = true;
        CHECK(r.state[it->second] == PresentRing::HELD);
      } else if (op < 7 && !live.empty()) {  // release one, acquired or not, in any order
        auto it = live.begin();
        std::advance(it, rng() % live.size());
        const uint64_t t = it->first;
        const int s = r.find(t);
        CHECK(s == it->second);
        r.release(s);
        live.erase(it);
        held.erase(t);
        CHECK(r.find(t) == -1);  // a released ticket names nothing
      } else {  // tickets that were never issued or are long gone
        CHECK(r.find(issued + 1 + rng() % 5) == -1);
        if (issued > 0) {
          const uint64_t t = 1 + rng() % issued;
          CHECK((r.find(t) >= 0) == (live.count(t) == 1));
        }
      }
      // the ring and the model agree on every live ticket and on how many there are
      int taken = 0;
      for (int i = 0; i < n; i++) taken += r.state[i] != PresentRing::FREE;
      CHECK(taken == (int)live.size());
      CHECK(r.all_free() == live.empty());
      for (const auto& kv : live) {
        CHECK(r.find(kv.first) == kv.second);
        CHECK((r.state[kv.second] == PresentRing::HELD) == held[kv.first]);
      }
    }
    // a remade ring forgets the old tickets and keeps counting
    const uint64_t last = issued;
    r.reset(n);
    for (const auto& kv : live) CHECK(r.find(kv.first) == -1);
    uint64_t t = 0;
    CHECK(r.enqueue(&t) >= 0 && t == last + 1);
    issued = t;
  }
  if (fails) return 1;
  printf("present_ring_check ok: %llu tickets\n", (unsigned long long)issued);
  return 0;
}
