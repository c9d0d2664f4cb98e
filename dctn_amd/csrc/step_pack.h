// The trailing parameter pack of the flat optimizers' step kernel (flat_step_k in flat_step.h, which
// Adam, SGD and RMSprop share).  Every optional block of a step - guard, step state, schedule, group table - is one pointer type; a
// kernel finds a block in its pack by that type, and the launchers build the pack from the blocks a step has.  The three
// block headers include this file.
#pragma once

#include <type_traits>

// Members of a kernel's trailing parameter pack by type: whether one is there, and its value
template <typename T, typename... G> constexpr bool pack_has_v = (std::is_same_v<T, G> || ...);

#if defined(__HIPCC__)
template <typename T, typename First, typename... Rest>
__device__ __forceinline__ T pack_get(First first, Rest... rest) {
  if constexpr (std::is_same_v<T, First>) return first; else return pack_get<T>(rest...);
}
#endif

// Host: launch(p...) with the pointers of `blocks` that are not null, in the order given.  Each block is there or not on
// its own, so n optional blocks reach 2^n instantiations of `launch` from one line per block and no ladder.
template <typename F> void with_blocks(F&& launch) { launch(); }
template <typename F, typename T, typename... Rest> void with_blocks(F&& launch, T* block, Rest*... rest) {
  if (block) with_blocks([&](auto... tail) { launch(block, tail...); }, rest...);
  else with_blocks(launch, rest...);
}
