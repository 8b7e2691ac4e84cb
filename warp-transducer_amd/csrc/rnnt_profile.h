// rnnt_profile.h -- the stage timers (rnnt_profile_*: HIP events on the caller's stream) and the roctx stage ranges of the main
// library: what run_gpu (rnnt_gpu_impl.h) and run_gpu_joint (rnnt_joint_impl.h) bracket their stages with.  Only those two
// drivers include it; the state is defined once, in rnnt_gpu.hip.  The side libraries (pruned, TDT, HAT) have no profiling.
#pragma once

#include <atomic>
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdlib>
#include <mutex>

namespace rnnt {

// ----------------------------------------------------------------------------- profiling
// Stage boundaries as HIP events on the caller's stream: 0 start, 1 after the statistics, 2 after the lattice, 3 after
// the coefficients (end of a forward phase), 4 start and 5 end of the gradient stage.  A one-call entry records all six;
// the two-phase entries record 0-3 (compute_rnnt_loss_fwd) and 4-5 (compute_rnnt_loss_bwd), and whatever the caller
// enqueues between the two calls is in neither stage.  One rnnt_profile_collect() reads what has been recorded since
// the last one as ONE step.
struct Profile {
    std::atomic<bool> on{false};   // read without the mutex to decide whether to take it; everything else below is guarded by g_prof_mu
    bool ready = false;
    hipEvent_t ev[6];
    double ms[5] = {0, 0, 0, 0, 0};   // statistics, lattice, coefficients, gradient, first event to last
    int calls = 0;
    bool pending = false;   // events of an asynchronous call recorded, not yet read
    bool has_fwd = false, has_bwd = false;
    // A call in the two-half schedule (rnnt_set_aux_stream, run_gpu) records these instead of ev[1..4]: on the caller's stream
    // h0 / h1 = {before the half's statistics, after them, before its coefficients, after them, after its gradient kernel};
    // on the auxiliary stream the start and end of each half's lattice kernel.
    bool split = false;
    hipEvent_t hev[2][5], lev[2][2];
};
extern Profile g_prof;     // one instance for the library (defined in rnnt_gpu.hip)
extern std::mutex g_prof_mu;   // held by a profiled call from its first event record to its last, and by the
                               // rnnt_profile_* entries: concurrent callers cannot tear the shared event set (their
                               // calls are serialised while the timers are on; off -- the default -- nobody takes it)

// `locked`: the caller holds g_prof_mu (it took it because it saw `on`); without the lock nothing of the shared event set is touched
static inline bool prof_prepare(bool locked) {
    if (!locked || !g_prof.on.load(std::memory_order_relaxed)) return false;   // (switched off between the caller's test and its lock: a plain, unprofiled call)
    if (!g_prof.ready) {
        for (auto& e : g_prof.ev)
            if (hipEventCreate(&e) != hipSuccess) return false;
        for (auto& h : g_prof.hev) for (auto& e : h) if (hipEventCreate(&e) != hipSuccess) return false;
        for (auto& h : g_prof.lev) for (auto& e : h) if (hipEventCreate(&e) != hipSuccess) return false;
        g_prof.ready = true;
    }
    return true;
}

// mark(i) of the run_* functions: i = 0..4 are the boundaries of the four stages of one call
static inline void prof_mark(int i, bool do_fwd, bool do_bwd, hipStream_t stream) {
    if (i < 3) { if (do_fwd) (void)hipEventRecord(g_prof.ev[i], stream); return; }
    if (i == 3) {
        if (do_fwd) { (void)hipEventRecord(g_prof.ev[3], stream); g_prof.has_fwd = true; }
        if (do_bwd) (void)hipEventRecord(g_prof.ev[4], stream);
        return;
    }
    if (do_bwd) { (void)hipEventRecord(g_prof.ev[5], stream); g_prof.has_bwd = true; }
}

static inline void prof_accumulate() {
    float ms = 0.f;
    if (g_prof.split) {
        // two-half schedule: statistics, coefficients and gradient = the sums over the halves (they run back to back on the
        // caller's stream); lattice = what the auxiliary stream spent on it, CONCURRENTLY with the other half's streaming
        // kernels -- it is not part of the critical path, ms[4] (first event to last) is
        auto add = [&](double& acc, hipEvent_t a, hipEvent_t b) { if (hipEventElapsedTime(&ms, a, b) == hipSuccess) acc += ms; };
        for (int h = 0; h < 2; ++h) {
            add(g_prof.ms[0], g_prof.hev[h][0], g_prof.hev[h][1]);
            add(g_prof.ms[1], g_prof.lev[h][0], g_prof.lev[h][1]);
            if (g_prof.has_fwd && g_prof.has_bwd) {
                add(g_prof.ms[2], g_prof.hev[h][2], g_prof.hev[h][3]);
                add(g_prof.ms[3], g_prof.hev[h][3], g_prof.hev[h][4]);
            } else if (g_prof.has_fwd) {
                add(g_prof.ms[2], g_prof.hev[h][2], g_prof.hev[h][3]);
            }
        }
        add(g_prof.ms[4], g_prof.hev[0][0], g_prof.hev[1][g_prof.has_bwd ? 4 : 3]);
        g_prof.calls++;
        g_prof.pending = g_prof.has_fwd = g_prof.has_bwd = g_prof.split = false;
        return;
    }
    if (g_prof.has_fwd)
        for (int i = 0; i < 3; ++i)
            if (hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]) == hipSuccess) g_prof.ms[i] += ms;
    if (g_prof.has_bwd && hipEventElapsedTime(&ms, g_prof.ev[4], g_prof.ev[5]) == hipSuccess) g_prof.ms[3] += ms;
    if ((g_prof.has_fwd || g_prof.has_bwd) &&
        hipEventElapsedTime(&ms, g_prof.ev[g_prof.has_fwd ? 0 : 4], g_prof.ev[g_prof.has_bwd ? 5 : 3]) == hipSuccess)
        g_prof.ms[4] += ms;
    g_prof.calls++;
    g_prof.pending = g_prof.has_fwd = g_prof.has_bwd = false;
}

// ----------------------------------------------------------------------------- stage ranges for external profilers
// rocprofv3 --kernel-trace shows kernel names only; with ranges on (rnnt_profile_enable bit 1, or WARPRNNT_ROCTX=1 in the
// environment) every call brackets the ENQUEUE of its four stages with roctx ranges -- the counterpart of the reference's
// DEBUG_TIME stage timers (include/detail/gpu_rnnt.h:112-122) -- which `rocprofv3 --marker-trace` puts on the same
// timeline as the kernels.  The marker library is looked up at run time (librocprofiler-sdk-roctx, else libroctx64):
// the library does not link against a profiler, and without one the switch does nothing.
struct Ranges {
    std::atomic<int> mode{-1};     // -1: not decided (environment), 0 off, 1 on
    std::once_flag resolved;       // the two entry points below are written once, inside call_once, and only read afterwards
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
extern Ranges g_ranges;            // one instance for the library (defined in rnnt_gpu.hip)

static inline bool ranges_prepare() {
    int mode = g_ranges.mode.load(std::memory_order_relaxed);
    if (mode < 0) {
        const char* e = getenv("WARPRNNT_ROCTX");
        int expected = -1;
        mode = (e != nullptr && atoi(e) > 0) ? 1 : 0;
        if (!g_ranges.mode.compare_exchange_strong(expected, mode, std::memory_order_relaxed)) mode = expected;   // (rnnt_profile_enable got there first)
    }
    if (mode != 1) return false;
    std::call_once(g_ranges.resolved, [] {          // concurrent first calls: one resolves, the others wait; both pointers or neither
        for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h == nullptr) continue;
            auto push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
            auto pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (push != nullptr && pop != nullptr) { g_ranges.push = push; g_ranges.pop = pop; break; }
        }
    });
    return g_ranges.push != nullptr;
}

// boundary i of a call (the same five as prof_mark): closes stage i-1, opens stage i
static inline void ranges_mark(int i, bool do_fwd, bool do_bwd, const char* const names[4]) {
    auto active = [&](int stage) { return stage >= 0 && stage < 4 && (stage < 3 ? do_fwd : do_bwd); };
    if (active(i - 1)) (void)g_ranges.pop();
    if (active(i)) (void)g_ranges.push(names[i]);
}

}  // namespace rnnt
