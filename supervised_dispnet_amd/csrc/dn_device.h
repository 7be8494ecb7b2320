// Device helpers shared by the kernels of libdispnet_hip.so: vector types, activations, the three-piece bf16 split, wave / row sums,
// raw buffer loads and index helpers.  Each is defined here once.  Device code only; not part of the ABI.
#pragma once
#include <type_traits>
#include <utility>

#include "dn_internal.h"

namespace dn {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// compile-time loop: the body is instantiated once per index, so register arrays indexed by it never become dynamic
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ float apply_act(float v, int act, float p0, float p1) {
  switch (act) {
    case DN_ACT_RELU: return v > 0.f ? v : 0.f;
    case DN_ACT_LEAKY: return v > 0.f ? v : v * p0;
    case DN_ACT_ELU: return v > 0.f ? v : (expf(v) - 1.f);
    case DN_ACT_SIGMOID_AFFINE: return p0 / (1.f + expf(-v)) + p1;
    default: return v;
  }
}

// four values at once: ONE (wave-uniform) branch on the activation instead of one per element
__device__ __forceinline__ f32x4 apply_act4(f32x4 v, int act, float p0, float p1) {
  f32x4 r = v;
  switch (act) {
    case DN_ACT_RELU:
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = v[e] > 0.f ? v[e] : 0.f;
      break;
    case DN_ACT_LEAKY:
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = v[e] > 0.f ? v[e] : v[e] * p0;
      break;
    case DN_ACT_ELU:
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = v[e] > 0.f ? v[e] : (expf(v[e]) - 1.f);
      break;
    case DN_ACT_SIGMOID_AFFINE:
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = p0 / (1.f + expf(-v[e])) + p1;
      break;
    default: break;
  }
  return r;
}

// x = h + m + l exactly (round to bf16, subtract, round, subtract: the last residual has <= 8 significant bits)
__device__ __forceinline__ void split3(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    const f32x2 x = f32x2{v[e], v[e + 1]};
    const bf16x2 h2 = __builtin_convertvector(x, bf16x2);
    const f32x2 r = x - __builtin_convertvector(h2, f32x2);
    const bf16x2 m2 = __builtin_convertvector(r, bf16x2);
    const f32x2 q = r - __builtin_convertvector(m2, f32x2);
    const bf16x2 l2 = __builtin_convertvector(q, bf16x2);
    h[e] = h2[0]; h[e + 1] = h2[1];
    m[e] = m2[0]; m[e + 1] = m2[1];
    l[e] = l2[0]; l[e + 1] = l2[1];
  }
}

// one value through scalar casts: the same three pieces as split3 yields
__device__ __forceinline__ void wino_split3(float x, __bf16* pc) {
  pc[0] = (__bf16)x;
  const float r1 = x - (float)pc[0];        // exact (Sterbenz), at most 16 significant bits
  pc[1] = (__bf16)r1;
  pc[2] = (__bf16)(r1 - (float)pc[1]);      // exact, at most 8 significant bits: the conversion does not round
}

__device__ __forceinline__ float wave_sum(float v) {       // sum over the 64 lanes of a wave, in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int ROT>
__device__ __forceinline__ float dpp_row_ror(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + ROT, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float v) {      // sum over the 16 lanes of a DPP row, in every lane
  v += dpp_row_ror<8>(v);
  v += dpp_row_ror<4>(v);
  v += dpp_row_ror<2>(v);
  v += dpp_row_ror<1>(v);
  return v;
}

template <int VW> struct VecOf;
template <> struct VecOf<4> { typedef f32x4 type; };
template <> struct VecOf<2> { typedef f32x2 type; };

template <int VW>
__device__ __forceinline__ typename VecOf<VW>::type buffer_load_vec(__amdgpu_buffer_rsrc_t r, int voffset) {
  if constexpr (VW == 4) {
    const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voffset, 0, 0);
    return __builtin_bit_cast(f32x4, v);
  } else {
    const i32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voffset, 0, 0);
    return __builtin_bit_cast(f32x2, v);
  }
}

// floor(n/d) on the device with the plan's magic (estimate is exact or one low; branch-free fix-up); *rem = n - q*d
__device__ __forceinline__ unsigned fastdiv_dev(unsigned n, unsigned d, unsigned M, unsigned* rem) {
  unsigned q = __umulhi(n, M);
  unsigned r = n - q * d;
  const bool fix = r >= d;
  q += fix ? 1u : 0u;
  r -= fix ? d : 0u;
  *rem = r;
  return q;
}

// ReflectionPad2d index map for v in [-(n-1), 2(n-1)]
__device__ __forceinline__ int reflect_idx(int v, int n) {
  const int m = n - 1;
  int a = v < 0 ? -v : v;
  a = m - a;
  a = a < 0 ? -a : a;
  return m - a;
}

// Which operand piece does K-chunk `kc` of a phase with `ntaps` taps fall in?  Uniform across the block.
__device__ __forceinline__ int select_operand(const IgemmParams& p, int ntaps, int kc, int* kc_local) {
  int s = 0;
#pragma unroll
  for (int i = 0; i < DN_MAX_OPERANDS - 1; ++i) {
    if (s == i && i < p.n_in - 1) {
      int nch = (ntaps * p.in[i].C + kChunk - 1) / kChunk;
      if (kc >= nch) {
        kc -= nch;
        s = i + 1;
      }
    }
  }
  *kc_local = kc;
  return s;
}

}  // namespace dn
