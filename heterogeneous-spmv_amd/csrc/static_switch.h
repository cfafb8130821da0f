// static_switch.h -- turns a run-time plan value into a compile-time constant
// for the kernel launchers (host code).
#pragma once
#include <type_traits>

namespace hspmv {

// Calls f(std::integral_constant<int, V>{}) for the V among Vs equal to v and
// returns true; false (f not called) when v is none of them.  Inside f the
// argument converts to a constant expression: a template argument of the
// kernel, or the condition of an `if constexpr`.
template <int... Vs, typename F>
bool static_switch(int v, F &&f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// The same for a flag that only some instantiations offer: f(true_type) when
// `on` and OFFERED, f(false_type) otherwise -- so a variant that is not OFFERED
// is never instantiated, and a plan that asks for it runs the plain one.
template <bool OFFERED = true, typename F>
void static_flag(bool on, F &&f) {
  if constexpr (OFFERED) {
    if (on) return f(std::true_type{});
  }
  f(std::false_type{});
}

}  // namespace hspmv
