// Host-only check of ccvpe_amd/csrc/dev_cache.h (no HIP, no GPU): built and run by tests/test_dev_cache.py with the host
// compiler, and once more under -fsanitize=thread where the toolchain links that runtime.  Exit status 0 = every check held.
#include <cstdio>
#include <thread>
#include <vector>

#include "dev_cache.h"

using ccvpe::DevCache;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static bool all_zero(const DevCache& c) {
  for (int d = 0; d < DevCache::MAX_DEVICES; ++d)
    if (c.get(d) != 0) return false;
  return true;
}

int main() {
  static_assert(DevCache::MAX_DEVICES == 64, "an MI355X node in CPX mode shows 64 logical devices");
  {  // a value raised for device 0 is not seen by device 1
    DevCache c;
    CHECK(all_zero(c));
    CHECK(!c.covers(0, 1));
    c.raise(0, 96 * 1024);
    CHECK(c.covers(0, 96 * 1024) && c.covers(0, 1));
    CHECK(!c.covers(0, 96 * 1024 + 1));
    CHECK(!c.covers(1, 1) && c.get(1) == 0);
    for (int d = 1; d < DevCache::MAX_DEVICES; ++d) CHECK(c.get(d) == 0);
  }
  {  // grow-only: a smaller later request neither lowers the value nor reports "not covered"
    DevCache c;
    c.raise(3, 160 * 1024);
    c.raise(3, 64 * 1024);
    CHECK(c.get(3) == 160 * 1024);
    CHECK(c.covers(3, 64 * 1024) && c.covers(3, 160 * 1024));
    c.raise(3, 160 * 1024);
    CHECK(c.get(3) == 160 * 1024);
  }
  {  // ordinals outside the table: never covered, never recorded, the neighbouring slots untouched
    DevCache c;
    const int bad[] = {-1, -64, DevCache::MAX_DEVICES, DevCache::MAX_DEVICES + 1, 1 << 20, -2147483647 - 1, 2147483647};
    for (int d : bad) {
      c.raise(d, 1000);
      CHECK(!c.covers(d, 1));
      CHECK(!c.covers(d, 0));
      CHECK(c.get(d) == 0);
    }
    CHECK(all_zero(c));                                  // slots 0 and 63 among them
    c.raise(0, 7);
    c.raise(DevCache::MAX_DEVICES - 1, 9);
    for (int d : bad) c.raise(d, 1000);
    CHECK(c.get(0) == 7 && c.get(DevCache::MAX_DEVICES - 1) == 9 && c.get(1) == 0 && c.get(DevCache::MAX_DEVICES - 2) == 0);
  }
  {  // eight threads raise and read the same four slots: every slot ends at the maximum, and no reader sees a value fall
    DevCache c;
    constexpr int THREADS = 8, ITERS = 20000, SLOTS = 4;
    // each thread walks its own order of values, all distinct across threads
    auto slot_of = [](int t, int i) { return (i + t) % SLOTS; };
    auto value_of = [](int t, int i) { return ((i * 7919 + t * 13) % ITERS) * THREADS + t + 1; };
    int want[SLOTS] = {0, 0, 0, 0};
    for (int t = 0; t < THREADS; ++t)
      for (int i = 0; i < ITERS; ++i)
        if (value_of(t, i) > want[slot_of(t, i)]) want[slot_of(t, i)] = value_of(t, i);
    std::vector<int> fell(THREADS, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; ++t)
      th.emplace_back([&, t] {
        int seen[SLOTS] = {0, 0, 0, 0};
        for (int i = 0; i < ITERS; ++i) {
          const int s = slot_of(t, i), v = value_of(t, i);
          c.raise(s, v);
          if (!c.covers(s, v)) ++fell[t];                // at least what this thread has just raised
          const int now = c.get(s);
          if (now < seen[s]) ++fell[t];
          seen[s] = now;
        }
      });
    for (auto& x : th) x.join();
    for (int t = 0; t < THREADS; ++t) CHECK(fell[t] == 0);
    for (int s = 0; s < SLOTS; ++s) CHECK(want[s] > 0 && c.get(s) == want[s]);
    for (int d = SLOTS; d < DevCache::MAX_DEVICES; ++d) CHECK(c.get(d) == 0);
  }
  if (failures) return 1;
  std::printf("dev_cache ok\n");
  return 0;
}
