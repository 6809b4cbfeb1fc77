// rollout_dispatch.h - host only: the run-time arguments that pick a rollout kernel's instantiation, turned into compile-time
// ones.  Each rollout unit is its kernel launch inside one nest of these; the instantiation set is the product of the branches.
#pragma once
#include <cstdint>
#include <type_traits>

namespace hjb {

template <typename T>
struct LabelType {
    using type = T;
};

// f(LabelType<TL>{}): TL = uint8_t / uint16_t / int32_t for idx_bytes 1 / 2 / anything else (hjb_rollout_create admits 1, 2, 4)
template <typename F>
void with_label_type(int idx_bytes, F &&f) {
    switch (idx_bytes) {
        case 1: f(LabelType<uint8_t>{}); break;
        case 2: f(LabelType<uint16_t>{}); break;
        default: f(LabelType<int32_t>{}); break;
    }
}

// f(std::true_type{}) or f(std::false_type{})
template <typename F>
void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// f(std::integral_constant<int, A>{}) when v == A, else f(std::integral_constant<int, B>{})
template <int A, int B, typename F>
void with_int(int v, F &&f) {
    if (v == A) f(std::integral_constant<int, A>{});
    else f(std::integral_constant<int, B>{});
}

// f(std::integral_constant<int, D>{}) for D = 1..6 (HJB_MAX_D; anything else goes to 6: hjb_rollout_create admits 1..6)
template <typename F>
void with_dim(int D, F &&f) {
    switch (D) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        default: f(std::integral_constant<int, 6>{}); break;
    }
}

}  // namespace hjb
