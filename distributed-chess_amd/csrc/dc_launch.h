// dc_launch.h -- host-only launch helpers of the perft kernels (dc_perft.hip,
// dc_perft_stats.hip): the occupancy cache behind every resident grid, the one
// launch through it, and the dispatch of a runtime side to move, rule set or
// flag to the template arguments of a kernel.
//
// The dispatchers call a generic lambda with a tag per choice:
//   with_stm(stm, [&](auto S) { launch_resident(k_level_moves<S(), W>, ...); });
// Only the choices a call site nests are instantiated, so a kernel variant that
// exists in one build alone stays behind that call site's #ifdef.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <type_traits>

#include "dc_kernels.h"

namespace dc {

// Grid-stride kernels get at most one resident wave of blocks (occupancy x CUs):
// a second, partial round of statically assigned blocks is pure tail.
template <class K>
static u32 resident_grid(K kernel, u32 block, u32 want) {
  static std::mutex mu;
  static std::map<const void*, u32> cache;
  const void* key = reinterpret_cast<const void*>(kernel);
  u32 cap;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(key);
    if (it == cache.end()) {
      int per_cu = 0, dev = 0, cus = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)block, 0) != hipSuccess || per_cu < 1)
        per_cu = 1;
      (void)hipGetDevice(&dev);
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
      it = cache.emplace(key, (u32)(per_cu * cus)).first;
    }
    cap = it->second;
  }
  return std::max<u32>(1, std::min(want, cap));
}

// `want` blocks of `block` threads, at most the resident grid.
template <class K, class... A>
static void launch_resident(K kernel, u32 block, u32 want, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kernel, dim3(resident_grid(kernel, block, want)), dim3(block), 0, st, args...);
}

template <class T>
struct type_tag {
  using type = T;
};
template <class Tag>
using tagged = typename Tag::type;  // tagged<decltype(R)>: the type a lambda's tag argument R stands for

// f(std::integral_constant<int, stm>)
template <class F>
static void with_stm(int stm, F&& f) {
  if (stm) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 0>{});
}

// f(type_tag<Ref>) under RULES_REF (0), f(type_tag<Fide>) under RULES_FIDE
template <class Ref, class Fide, class F>
static void with_rules(u32 rules, F&& f) {
  if (rules == 0) f(type_tag<Ref>{});
  else f(type_tag<Fide>{});
}

// f(std::true_type) or f(std::false_type)
template <class F>
static void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace dc
