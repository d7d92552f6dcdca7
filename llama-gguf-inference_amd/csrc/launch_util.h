// launch_util.h — host-side launch helper shared by the kernel translation units
// (kernels.hip, attn.hip, attn86.hip, the per-type matvec units mv_*.hip, prefill.hip).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <type_traits>

namespace llmi {

// Launch-event hook (llmi_profile_kernels, kernels.hip): while armed, the timed launches
// record `start` when the first kernel of the op begins and `stop` when the last one ends
// (hipExtLaunchKernelGGL), i.e. kernel execution time without dependent-launch gaps.
hipEvent_t launch_event(bool stop);

// CUs of the current device, cached per device (in-process replicas run one scheduler
// thread per GPU; a benign race writes the same value twice)
static inline int cu_count() {
    static int cache[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    int n = __atomic_load_n(&cache[dev], __ATOMIC_RELAXED);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 0) n = 0;
        __atomic_store_n(&cache[dev], n, __ATOMIC_RELAXED);
    }
    return n;
}

template <typename K, typename... Args>
static void launch_k(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, bool first, bool last, Args... args) {
    hipEvent_t e0 = first ? launch_event(false) : nullptr, e1 = last ? launch_event(true) : nullptr;
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, s, e0, e1, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

// Run-time values -> template arguments.  Of<As...>{v} is a value and the constants it may
// equal; pick(f, of...) calls f(std::integral_constant<int, A>{}...) with the constant each
// value equals and returns true, or returns false when a value is in no list.  The lists at
// the call sites are therefore the whole set of instantiated kernels.
template <int... As>
struct Of { int v; };
template <class F>
static bool pick(F&& f) { return f(), true; }
template <class F, int... As, class... Rest>
static bool pick(F&& f, Of<As...> a, Rest... rest) {
    return ((a.v == As && pick([&](auto... r) { f(std::integral_constant<int, As>{}, r...); }, rest...)) || ...);
}
using OfD = Of<128, 64>;     // head dims
using OfG = Of<1, 2, 4, 8>;  // GQA groups of the kernels that take the group as a template argument

}  // namespace llmi

