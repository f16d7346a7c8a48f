// A per-device, grow-only integer for launch state that the driver keeps per device (a kernel's dynamic-LDS limit, the CU
// count).  Host only, no HIP headers: tests/host/dev_cache_main.cpp compiles it with a plain host compiler.
// Relaxed atomics: a racing second writer repeats a driver call that is idempotent for the same or a larger value.
#pragma once
#include <atomic>

namespace ccvpe {

class DevCache {
 public:
  static constexpr int MAX_DEVICES = 64;       // an MI355X node in CPX partition mode shows 64 logical devices

  // does device `dev` already hold a value >= v?  An ordinal outside the table never does.
  bool covers(int dev, int v) const { return dev >= 0 && dev < MAX_DEVICES && v_[dev].load(std::memory_order_relaxed) >= v; }
  int get(int dev) const { return dev >= 0 && dev < MAX_DEVICES ? v_[dev].load(std::memory_order_relaxed) : 0; }

  // raise device `dev` to at least v; never lowers, never records an ordinal outside the table
  void raise(int dev, int v) {
    if (dev < 0 || dev >= MAX_DEVICES) return;
    int cur = v_[dev].load(std::memory_order_relaxed);
    while (cur < v && !v_[dev].compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
  }

 private:
  std::atomic<int> v_[MAX_DEVICES] = {};
};

}  // namespace ccvpe
