// present_ring.h — the bookkeeping of the present ring (fr_present_enqueue / _acquire / _release, ctx_present.cpp):
// which slot a ticket names and whether a slot is free, in flight (enqueued, its copy not yet seen complete) or held
// (acquired by the caller). Plain host state with no HIP call in it, so tools/present_ring_check.cpp drives it alone.
#pragma once
#include <stdint.h>

namespace fr {

struct PresentRing {
  static constexpr int MAX_SLOTS = 8;
  enum State : uint8_t { FREE = 0, FLIGHT = 1, HELD = 2 };
  int n = 0;               // slots in use, 0: the feature is off
  int next = 0;            // where the search for a free slot starts: slots are taken round robin
  uint64_t issued = 0;     // tickets handed out since the context was made; the next one is issued + 1
  State state[MAX_SLOTS] = {};
  uint64_t ticket[MAX_SLOTS] = {};  // the ticket of a slot that is not free

  // A ring of `slots` free slots; tickets keep counting, so a ticket of the old ring names nothing in the new one.
  void reset(int slots) {
    n = slots;
    next = 0;
    for (int i = 0; i < MAX_SLOTS; i++) { state[i] = FREE; ticket[i] = 0; }
  }
  bool all_free() const {
    for (int i = 0; i < n; i++) if (state[i] != FREE) return false;
    return true;
  }
  // The next free slot, now in flight under a new ticket; -1 with nothing changed when every slot is taken.
  int enqueue(uint64_t* t) {
    for (int k = 0; k < n; k++) {
      const int i = (next + k) % n;
      if (state[i] != FREE) continue;
      state[i] = FLIGHT;
      ticket[i] = ++issued;
      next = (i + 1) % n;
      *t = issued;
      return i;
    }
    return -1;
  }
  // The slot a live ticket names; -1 for one never issued or already released.
  int find(uint64_t t) const {
    if (t == 0) return -1;
    for (int i = 0; i < n; i++) if (state[i] != FREE && ticket[i] == t) return i;
    return -1;
  }
  void acquired(int slot) { state[slot] = HELD; }  // the caller has seen the slot's copy complete
  void release(int slot) { state[slot] = FREE; ticket[slot] = 0; }
};

}  // namespace fr
