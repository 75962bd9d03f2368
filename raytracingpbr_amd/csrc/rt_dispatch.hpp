// rt_dispatch.hpp — from run-time values to a kernel instance, once: the launchers hand their booleans, radius or scene kind to one of
// the with_* functions below and launch `kernel<...>` from the constants the callback receives.  Which combinations of a kernel
// family's booleans have an instance is one constexpr rule per family: the kernel asserts it, the launcher asks it (a combination
// without an instance is reported to the caller, never replaced by a neighbour), and the count beside it pins the set.
// Plain C++17 without a HIP include, so that a host compiler takes it as it is (tests/dispatch).
#pragma once
#include <type_traits>
#include <utility>

namespace rt {

// scene specialisations: GENERIC = analytic primitives (no neural SDF code), BOXES = all boxes
// (Cornell), BUNNY = all objects are the neural bunny, MIXED = bunny next to analytic primitives
enum { KIND_GENERIC = 0, KIND_BOXES = 1, KIND_BUNNY = 2, KIND_MIXED = 3 };

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...), in the order given; returns what f returns (the same type for every tuple)
template <class F, class... Bs>
decltype(auto) with_bools(F&& f, bool b0, Bs... bs) {
    if constexpr (sizeof...(bs) == 0) return b0 ? f(std::true_type{}) : f(std::false_type{});
    else if (b0) return with_bools([&](auto... cs) -> decltype(auto) { return f(std::true_type{}, cs...); }, bs...);
    else return with_bools([&](auto... cs) -> decltype(auto) { return f(std::false_type{}, cs...); }, bs...);
}

// f(std::integral_constant<int, R>{}) for the window kernels' R = radius (rt_capi.hip admits radius 1..3 only)
template <class F>
decltype(auto) with_radius(int radius, F&& f) {
    if (radius == 1) return f(std::integral_constant<int, 1>{});
    if (radius == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 3>{});
}

// f(std::integral_constant<int, KIND_*>{}); a value that names no kind takes the general instance
template <class F>
decltype(auto) with_kind(int kind, F&& f) {
    if (kind == KIND_BOXES) return f(std::integral_constant<int, KIND_BOXES>{});
    if (kind == KIND_BUNNY) return f(std::integral_constant<int, KIND_BUNNY>{});
    if (kind == KIND_MIXED) return f(std::integral_constant<int, KIND_MIXED>{});
    return f(std::integral_constant<int, KIND_GENERIC>{});
}

// how many of the 2^N tuples of N booleans a rule admits
template <class Rule, std::size_t... I>
constexpr int forms_admitted(Rule ok, std::index_sequence<I...>) {
    int n = 0;
    for (unsigned m = 0; m < (1u << sizeof...(I)); m++) n += ok((((m >> I) & 1u) != 0u)...) ? 1 : 0;
    return n;
}

// atrous_level (rt_features.hip).  LINEAR is a last level's; COVER is the plain filter, linear exactly at its last level; FILL is the
// plain filter, linear only as COVER's last level; GUIDED is never LINEAR.  FIRST is free.
constexpr bool atrous_form_ok(bool /*FIRST*/, bool LAST, bool GUIDED, bool LINEAR, bool COVER, bool FILL) {
    return (LAST || !LINEAR) && (!COVER || (!GUIDED && LAST == LINEAR)) && (!FILL || !GUIDED) && (!FILL || !LINEAR || COVER) &&
           !(GUIDED && LINEAR);
}
static_assert(forms_admitted(atrous_form_ok, std::make_index_sequence<6>{}) == 22, "the instances of atrous_level");

// level_blend (rt_half.hip), per radius and ERR: the linear exit and the filled pixels are a last level's.  FIRST is free.
constexpr bool level_blend_form_ok(bool /*FIRST*/, bool LAST, bool LIN, bool FILL) { return (LAST || !LIN) && (LAST || !FILL); }
static_assert(forms_admitted(level_blend_form_ok, std::make_index_sequence<4>{}) == 10, "the instances of level_blend per (R, ERR)");

}  // namespace rt
