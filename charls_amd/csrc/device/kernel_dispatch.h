// kernel_dispatch.h -- the one place a launch turns runtime values into a template instantiation, and the one way a kernel
// with dynamic LDS is launched.  Host side only; compiled by hipcc with the launch units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "runtime.h"

namespace jls::dev {

constexpr size_t kMaxDynamicLds = 64 * 1024; // what a kernel may ask for without hipFuncSetAttribute

// f(std::integral_constant<int, V>{}) for the listed V that equals `value`; the LAST listed value is the catch-all.
template <int V0, int... Vs, typename F>
void dispatch_int(int value, F&& f)
{
    if constexpr (sizeof...(Vs) == 0)
        f(std::integral_constant<int, V0>{});
    else if (value == V0)
        f(std::integral_constant<int, V0>{});
    else
        dispatch_int<Vs...>(value, f);
}

// f(std::true_type{}) or f(std::false_type{}).
template <typename F>
void dispatch_bool(bool value, F&& f)
{
    if (value)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// f(sample_tag<uint16_t>{}) for samples of more than 8 bits, f(sample_tag<uint8_t>{}) otherwise.
template <typename S>
struct sample_tag
{
    using type = S;
};
template <typename F>
void dispatch_sample(int bits_per_sample, F&& f)
{
    if (bits_per_sample > 8)
        f(sample_tag<uint16_t>{});
    else
        f(sample_tag<uint8_t>{});
}

// Launches `kernel` with `lds` bytes of dynamic LDS (beyond kMaxDynamicLds the kernel's limit is raised first) and raises
// what the launch reports.
template <typename... Params, typename... Args>
void launch_kernel(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args)
{
    if (lds > kMaxDynamicLds)
        hip_check(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      static_cast<int>(lds)));
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, static_cast<Params>(args)...);
    hip_check(hipGetLastError());
}

} // namespace jls::dev
