// launch_dispatch.h -- host-side helpers of the kernel launchers: the error check behind a launch, and run-time flag -> template argument.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#define BU_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

namespace bu {

// f(std::true_type{}) or f(std::false_type{}): a launcher writes its launch once, in a generic lambda, and names the kernel k<decltype(p)::value>
template <class F>
inline void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}

} // namespace bu
