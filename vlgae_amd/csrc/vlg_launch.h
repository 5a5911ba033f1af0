// vlg_launch.h -- the one way a kernel of this library is launched: raise the dynamic-LDS limit if the launch needs it,
// launch, ask the runtime whether it accepted the launch.  Kept out of vlg_common.h, which plain C++ units include too.
#pragma once
#include <stddef.h>

#include "vlg_common.h"

namespace vlg {

// Dynamic LDS a launch may ask for without raising the kernel's hipFuncAttributeMaxDynamicSharedMemorySize (the HIP default).
constexpr size_t kDefaultDynamicLds = 64 * 1024;

// Every argument is converted to the kernel's own parameter type, as a direct call would.  The limit is raised on every
// launch that needs it and never remembered: it belongs to a (function, device) pair, and a later launch may need more.
template <typename... P, typename... A>
int launch(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... args) {
    static_assert(sizeof...(P) == sizeof...(A), "launch: argument count differs from the kernel's parameter count");
    if (lds > kDefaultDynamicLds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return set_error((int)e, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu): %s", name, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, s, static_cast<P>(args)...);
    return check_launch(name);
}

}  // namespace vlg
