// Per-device once-table: which dynamic-LDS limit has a kernel been granted on each device?  Plain C++17, no HIP in here, so that
// tests/test_per_device_once.py can compile and race it on a machine without a GPU.  common.hpp's allow_lds<Kernel>() owns one per kernel.
#pragma once
#include <atomic>

namespace rc {

constexpr int kMaxDevices = 64;

struct PerDeviceLimit {
    std::atomic<int> granted[kMaxDevices] = {};         // bytes; 0 = nothing granted yet

    // Make device `dev`'s limit at least `bytes`.  `set(bytes) -> bool` (hipFuncSetAttribute) runs only if the recorded limit is lower, and
    // its limit is recorded only if it succeeded: a failure is reported by every call until one succeeds, never once and then forgotten.
    // Two threads racing on a fresh slot may both call `set` -- it is idempotent, so no mutex.  (A kernel launched with several sizes asks
    // for its largest first, at every site: `set` never lowers a limit another thread relies on.)
    template <class Set>
    bool ensure(int dev, int bytes, Set&& set) {
        std::atomic<int>& slot = granted[dev];
        int seen = slot.load(std::memory_order_acquire);
        if (seen >= bytes) return true;
        if (!set(bytes)) return false;
        while (seen < bytes && !slot.compare_exchange_weak(seen, bytes, std::memory_order_release, std::memory_order_acquire)) {}
        return true;
    }
    int limit(int dev) const { return granted[dev].load(std::memory_order_acquire); }
};

}  // namespace rc
