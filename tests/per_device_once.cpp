// Stand-alone exercise of csrc/per_device.hpp (no HIP, no GPU): counting stubs stand in for hipFuncSetAttribute.
// Prints one "name=value" line per figure; tests/test_per_device_once.py asserts on them.
#include <cstdio>
#include <thread>

#include "../realcamnet_amd/csrc/per_device.hpp"

int main() {
    constexpr int KB = 1024, N = rc::kMaxDevices;
    std::printf("slots=%d\n", N);

    {   // (a) 8 threads x 64 devices on a fresh table, then a second pass of smaller requests
        rc::PerDeviceLimit t;
        std::atomic<int> calls[N] = {};
        std::atomic<int> failed{0};
        std::thread th[8];
        for (auto& x : th)
            x = std::thread([&] {
                for (int d = 0; d < N; ++d)
                    if (!t.ensure(d, 100 * KB, [&](int) { calls[d].fetch_add(1); return true; })) failed.fetch_add(1);
            });
        for (auto& x : th) x.join();
        int granted = 0, min_calls = 1 << 30, max_calls = 0;
        for (int d = 0; d < N; ++d) {
            granted += t.limit(d) == 100 * KB;
            const int c = calls[d].load();
            min_calls = c < min_calls ? c : min_calls;
            max_calls = c > max_calls ? c : max_calls;
        }
        int second = 0, second_ok = 0;
        for (int d = 0; d < N; ++d) {
            second_ok += t.ensure(d, 100 * KB, [&](int) { ++second; return true; });
            second_ok += t.ensure(d, 64 * KB, [&](int) { ++second; return true; });
        }
        std::printf("a_failed=%d\na_granted=%d\na_min_calls=%d\na_max_calls=%d\na_second_calls=%d\na_second_ok=%d\n", failed.load(), granted, min_calls, max_calls,
                    second, second_ok);
    }
    {   // (b) a failing `set` leaves the slot unmarked; the next request tries again and is recorded
        rc::PerDeviceLimit t;
        int calls = 0;
        const bool r1 = t.ensure(5, 100 * KB, [&](int) { ++calls; return false; });
        const int after_fail = t.limit(5);
        const bool r2 = t.ensure(5, 100 * KB, [&](int) { ++calls; return false; });
        const bool r3 = t.ensure(5, 100 * KB, [&](int) { ++calls; return true; });
        const bool r4 = t.ensure(5, 100 * KB, [&](int) { ++calls; return true; });
        std::printf("b_results=%d%d%d%d\nb_limit_after_fail=%d\nb_calls=%d\nb_limit=%d\n", r1, r2, r3, r4, after_fail, calls, t.limit(5));
    }
    {   // (c) a larger request after a grant calls `set` once more, with the larger size; a smaller one after it does not
        rc::PerDeviceLimit t;
        int calls = 0, last = 0;
        auto set = [&](int bytes) { ++calls; last = bytes; return true; };
        t.ensure(0, 100 * KB, set);
        const int c1 = calls;
        t.ensure(0, 160 * KB, set);
        const int c2 = calls, asked = last;
        t.ensure(0, 120 * KB, set);
        std::printf("c_calls=%d,%d,%d\nc_asked=%d\nc_limit=%d\n", c1, c2, calls, asked, t.limit(0));
    }
    {   // (d) the last index works; slots do not alias
        rc::PerDeviceLimit t;
        int calls = 0;
        auto set = [&](int) { ++calls; return true; };
        t.ensure(0, 100 * KB, set);
        const int l1 = t.limit(1);
        t.ensure(N - 1, 100 * KB, set);
        t.ensure(N - 1, 100 * KB, set);
        int others = 0;
        for (int d = 1; d < N - 1; ++d) others += t.limit(d) != 0;
        std::printf("d_limit0=%d\nd_limit1=%d\nd_limit_last=%d\nd_calls=%d\nd_others=%d\n", t.limit(0), l1, t.limit(N - 1), calls, others);
    }
    return 0;
}
