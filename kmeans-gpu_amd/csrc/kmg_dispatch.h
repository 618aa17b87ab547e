// kmg_dispatch.h -- a runtime value to a template argument, once per launcher.  Device-free C++17: nothing of HIP or of the
// library (tests/native/check_dispatch.cpp builds it alone).
//
// Each helper calls the generic lambda `f` exactly once with a tag that carries the value in its type and returns true; for a
// value it does not list it calls nothing and returns false (the launcher then returns hipErrorInvalidValue).  In the lambda
//     [&](auto A) { ... k_x<A()> ... }                     a bool or an integer: a std::integral_constant
//     [&](auto t) { using OutT = typename decltype(t)::type; ... }
// A launcher nests them, the kernel launch in the innermost lambda, so every instantiation is named once and an argument cannot
// land on another axis than its own.
#pragma once

#include <stdint.h>
#include <type_traits>

namespace kmg {

template <typename T>
struct TypeTag { using type = T; };

template <typename F>
inline bool with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{}); else f(std::false_type{});
    return true;
}

// one of a small set of integers: PPT 1 / 2 / 4 / 8, list halves 1 / 2, skew 2 / 3, routes, the error forms and `what` masks
template <int... Vs, typename F>
inline bool with_value(int v, F &&f)
{
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// kmg_output_format (include/kmeans_hip.h: RGBA8 = 0, INDEX8 = 1, INDEX16 = 2) -> the type of an output pixel
template <typename F>
inline bool with_out_type(int format, F &&f)
{
    switch (format) {
    case 0: f(TypeTag<uint32_t>{}); return true;
    case 1: f(TypeTag<uint8_t>{}); return true;
    case 2: f(TypeTag<uint16_t>{}); return true;
    default: return false;
    }
}

// the index formats only: by format (INDEX8 / INDEX16; RGBA8 is not listed) ...
template <typename F>
inline bool with_index_type(int format, F &&f)
{
    switch (format) {
    case 1: f(TypeTag<uint8_t>{}); return true;
    case 2: f(TypeTag<uint16_t>{}); return true;
    default: return false;
    }
}

// ... or by `wide` (u16, else u8)
template <typename F>
inline bool with_index_type(bool wide, F &&f)
{
    if (wide) f(TypeTag<uint16_t>{}); else f(TypeTag<uint8_t>{});
    return true;
}

}  // namespace kmg
