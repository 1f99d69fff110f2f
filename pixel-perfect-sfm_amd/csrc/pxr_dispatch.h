// pxr_dispatch.h -- runtime (dtype, channel count, flag) -> template arguments, host side.
//
// An entry point names the storage types and channel counts ITS kernels exist for as the template arguments of these helpers,
// next to the launch they guard; a generic lambda receives the match as a tag type and holds the one hipLaunchKernelGGL:
//
//   bool ok = false;
//   for_storage<_Float16, float>(arena->dtype, [&](auto st) {
//     using ST = typename decltype(st)::type;
//     ok = for_channels<128, 64>(arena->C, [&](auto c) {
//       constexpr int C = decltype(c)::value;
//       for_flag(cfg->use_float_simd, [&](auto fs) { hipLaunchKernelGGL((kernel<ST, C, decltype(fs)::value>), ...); });
//     });
//   });
//   if (!ok) return set_error(PXR_EUNSUPPORTED, ...);
//
// Only the listed combinations are instantiated: each site lists its own sets (the arenas accept combinations some kernels lack).
#pragma once
#include <type_traits>

#include "pxr_internal.h"

namespace pxr {

template <typename T> struct type_tag { using type = T; };

// the pxr_dtype of a storage type (the one place that pairs them)
template <typename ST> inline constexpr int dtype_of = -1;
template <> inline constexpr int dtype_of<_Float16> = PXR_F16;
template <> inline constexpr int dtype_of<float> = PXR_F32;
template <> inline constexpr int dtype_of<double> = PXR_F64;
template <> inline constexpr int dtype_of<unsigned char> = PXR_U8;

// f(type_tag<ST>{}) for the ST among STs whose pxr_dtype is `dtype`; false: none is
template <typename... STs, typename F>
bool for_storage(int dtype, F&& f) {
  return ((dtype == dtype_of<STs> ? (f(type_tag<STs>{}), true) : false) || ...);
}

// f(std::integral_constant<int, C>{}) for the one of Cs that equals C; false: none does
template <int... Cs, typename F>
bool for_channels(int C, F&& f) {
  return ((C == Cs ? (f(std::integral_constant<int, Cs>{}), true) : false) || ...);
}

template <typename F>
void for_flag(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// the arena part of a kernel argument struct (InnerArgs, BaEvalArgs, GramArgs, KaArgs: the same five field names)
template <typename Args>
void set_arena(Args& a, const pxr_arena* arena) {
  a.arena = arena->d_data; a.corners = arena->d_corners; a.scales = arena->d_scales;
  a.H = arena->H; a.W = arena->W;
}

}  // namespace pxr
