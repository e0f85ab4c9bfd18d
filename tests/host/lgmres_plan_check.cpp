// The cycle plan and the ring arithmetic of the augmented restarts (csrc/gmres_dense.h, lgm_*) on the host, over every small case.
// Includes only gmres_dense.h.  Prints one line per group of cases and "ok" at the end; any failure exits with 1.
#include "gmres_dense.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

static int fails = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
      ++fails;                      \
    }                               \
  } while (0)

int main() {
  // ---- the plan, over all (stored, augment, left), stored <= 8, augment <= 8, left <= 12, and the slots of one cycle: the ka sources and the slot that is due are distinct, for every handle size >= augment and every head
  long plans = 0, cycles = 0;
  for (int augment = 0; augment <= 8; ++augment)
    for (int stored = 0; stored <= 8; ++stored)
      for (int left = 1; left <= 12; ++left) {
        const int ka = lgm_plan_ka(stored, augment, left), nk = lgm_plan_nk(stored, augment, left);
        CHECK(nk >= 1, "stored %d augment %d left %d: nk %d", stored, augment, left, nk);
        CHECK(ka >= 0 && nk + ka == left, "stored %d augment %d left %d: nk %d ka %d", stored, augment, left, nk, ka);
        CHECK(ka <= stored && ka <= augment, "stored %d augment %d left %d: ka %d", stored, augment, left, ka);
        CHECK(ka == std::max(0, std::min(std::min(stored, augment), left - 1)), "stored %d augment %d left %d: ka %d", stored, augment,
              left, ka);
        ++plans;
        for (int cap = std::max(augment, 1); cap <= 8; ++cap) {   // the handle's augment; the ring has cap + 1 slots
          const int nslots = cap + 1;
          for (int head = 0; head < nslots; ++head) {
            std::vector<int> used{lgm_slot_due(head)};
            for (int i = 0; i < ka; ++i) used.push_back(lgm_slot_newest(head, nslots, i));
            for (int s : used) CHECK(s >= 0 && s < nslots, "slot %d of %d", s, nslots);
            std::sort(used.begin(), used.end());
            CHECK(std::adjacent_find(used.begin(), used.end()) == used.end(), "augment %d stored %d left %d cap %d head %d: a slot twice",
                  augment, stored, left, cap, head);
            ++cycles;
          }
        }
      }
  std::printf("case plans: %ld plans, %ld cycles' slots\n", plans, cycles);

  // ---- after any sequence of pushes the i-th newest is what a plain list says.  The ring's memory is modelled as nslots labels;
  // a push writes the label into the slot that is due, as the combine does, and may be refused (dy = 0), which changes nothing.
  long pushes = 0;
  unsigned rng = 12345u;
  for (int cap = 1; cap <= 8; ++cap)
    for (int augment = 1; augment <= cap; ++augment) {
      const int nslots = cap + 1;
      std::vector<int> slot(nslots, -1);
      std::deque<int> list;   // newest first
      int head = 0, stored = 0;
      for (int label = 0; label < 200; ++label) {
        rng = rng * 1664525u + 1013904223u;
        slot[lgm_slot_due(head)] = label;      // the combine writes dy into the slot that is due
        if ((rng >> 16) % 5 == 0) continue;    // n = 0 or not finite: not stored, head and count stay
        head = lgm_push(head, nslots);
        stored = lgm_stored_after_push(stored, augment);
        list.push_front(label);
        if ((int)list.size() > augment) list.pop_back();
        CHECK(stored == (int)list.size(), "cap %d augment %d label %d: stored %d, list %zu", cap, augment, label, stored, list.size());
        CHECK(head >= 0 && head < nslots, "head %d of %d", head, nslots);
        for (int i = 0; i < stored; ++i)
          CHECK(slot[lgm_slot_newest(head, nslots, i)] == list[i], "cap %d augment %d label %d: %d-th newest is %d, the list says %d", cap,
                augment, label, i, slot[lgm_slot_newest(head, nslots, i)], list[i]);
        ++pushes;
      }
    }
  std::printf("case ring: %ld pushes\n", pushes);
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
