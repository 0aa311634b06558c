// plane_unit.h — the device helpers every kernel file shares: vector types, the MFMA wrappers, the hi / lo split of a value and the
// load / store of one 16-byte plane unit (8 channels of a pixel).  A leaf header: it includes nothing of the project but the C header.
// A helper belongs here when its body is the same in every file that needs it and it knows nothing about one kernel: no tile shape, no LDS
// layout, no kernel-specific constant.  Those stay in the <arch>.hip that owns them, with that file's prefix.  Host-side helpers (argument
// checks, launch status, format dispatch) live in common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "resselt_amd.h"

namespace rsa {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;  // also the 128-bit container of an fp16 fragment (bit-cast at the MFMA)
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(8))) uint16_t u16x8;  // eight 16-bit patterns of either plane format (split_elem's results)

// D[16][16] += A[16][32] * B[32][16] on 16-bit fragments of plane format FMT (enum rsa_plane_fmt: 0 = bf16, 1 = fp16); same fragment
// layout, same cycles
template <int FMT>
__device__ __forceinline__ f32x4 mfma16(const bf16x8 a, const bf16x8 b, const f32x4 c) {
  if constexpr (FMT == RSA_PF_F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// D[32][32] += A[32][16] * B[16][32], the same way
template <int FMT>
__device__ __forceinline__ f32x16 mfma32(const bf16x8 a, const bf16x8 b, const f32x16 c) {
  if constexpr (FMT == RSA_PF_F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// eight values -> one 16-bit fragment of plane format FMT (RNE, no residual)
template <int FMT>
__device__ __forceinline__ bf16x8 pack16(const float (&v)[8]) {
  if constexpr (FMT == RSA_PF_F16) {
    f16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (_Float16)v[j];
    return __builtin_bit_cast(bf16x8, h);
  } else {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (__bf16)v[j];
    return r;
  }
}

// (a, b) -> packed 16-bit pair (RNE) of plane format FMT and the pair's rounding residuals, also packed
template <int FMT = 0>
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  if constexpr (FMT == RSA_PF_F16) {
    // The values are made opaque first: with a = x * y still visible, the compiler fuses the conversion of the residual into
    // v_fma_mix*_f16 (x * y - hi rounded once from the exact product) while hi itself is v_cvt_pk_f16_f32 of the f32 product -- the two
    // roundings of x * y can differ by an fp16 ulp, and hi + lo is then off by that ulp instead of being a 22-bit value (seen on the
    // Mish / SiLU / gate epilogues: 2.4e-4 on single elements).
    asm("" : "+v"(a), "+v"(b));
    const f16x2 h = {(_Float16)a, (_Float16)b};
    hi = __builtin_bit_cast(uint32_t, h);
    const f16x2 l = {(_Float16)(a - (float)h[0]), (_Float16)(b - (float)h[1])};
    lo = __builtin_bit_cast(uint32_t, l);
  } else {
    const bf16x2 h = {(__bf16)a, (__bf16)b};
    hi = __builtin_bit_cast(uint32_t, h);
    const float ra = a - __builtin_bit_cast(float, hi << 16);
    const float rb = b - __builtin_bit_cast(float, hi & 0xffff0000u);
    const bf16x2 l = {(__bf16)ra, (__bf16)rb};
    lo = __builtin_bit_cast(uint32_t, l);
  }
}
// runtime format (wave-uniform): the generic epilogue
__device__ __forceinline__ void split2_rt(bool f16, float a, float b, uint32_t& hi, uint32_t& lo) {
  if (f16)
    split2<RSA_PF_F16>(a, b, hi, lo);
  else
    split2<RSA_PF_BF16>(a, b, hi, lo);
}
// four channels of a unit half: hi (+ lo) -> f32
template <int FMT>
__device__ __forceinline__ f32x4 widen4(uint2 h, uint2 l) {
  if constexpr (FMT == RSA_PF_F16) {
    const f16x2 h0 = __builtin_bit_cast(f16x2, h.x), h1 = __builtin_bit_cast(f16x2, h.y);
    const f16x2 l0 = __builtin_bit_cast(f16x2, l.x), l1 = __builtin_bit_cast(f16x2, l.y);
    return (f32x4){(float)h0[0] + (float)l0[0], (float)h0[1] + (float)l0[1], (float)h1[0] + (float)l1[0], (float)h1[1] + (float)l1[1]};
  } else {
    return (f32x4){__builtin_bit_cast(float, h.x << 16) + __builtin_bit_cast(float, l.x << 16),
                   __builtin_bit_cast(float, h.x & 0xffff0000u) + __builtin_bit_cast(float, l.x & 0xffff0000u),
                   __builtin_bit_cast(float, h.y << 16) + __builtin_bit_cast(float, l.y << 16),
                   __builtin_bit_cast(float, h.y & 0xffff0000u) + __builtin_bit_cast(float, l.y & 0xffff0000u)};
  }
}

// four output values -> the 8-byte half of a plane unit (hi, and the rounding residual for a lo plane)
template <int FMT>
__device__ __forceinline__ void round4(const float (&v)[4], bf16x4& h, bf16x4& lo4) {
  if constexpr (FMT == RSA_PF_F16) {
    f16x4 hh, ll;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float ve = v[e];
      asm("" : "+v"(ve));  // opaque: see split2
      hh[e] = (_Float16)ve;
      ll[e] = (_Float16)(ve - (float)hh[e]);
    }
    h = __builtin_bit_cast(bf16x4, hh);
    lo4 = __builtin_bit_cast(bf16x4, ll);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const __bf16 hb = (__bf16)v[e];
      h[e] = hb;
      lo4[e] = (__bf16)(v[e] - (float)hb);
    }
  }
}

// One 16-byte unit of planes in the compile-time format FMT at a byte offset: hi (+ lo where the buffer has it) <-> f32
template <int FMT>
__device__ __forceinline__ void load_unit(const char* hi, const char* lo, int64_t byte_off, float (&v)[8]) {
  const uint4 h = *(const uint4*)(hi + byte_off);
  const uint4 l = lo ? *(const uint4*)(lo + byte_off) : make_uint4(0u, 0u, 0u, 0u);
  const f32x4 a = widen4<FMT>(make_uint2(h.x, h.y), make_uint2(l.x, l.y));
  const f32x4 b = widen4<FMT>(make_uint2(h.z, h.w), make_uint2(l.z, l.w));
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = a[j], v[4 + j] = b[j];
}
template <int FMT>
__device__ __forceinline__ void store_unit(char* hi, char* lo, int64_t byte_off, const float (&v)[8]) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) split2<FMT>(v[2 * j], v[2 * j + 1], h[j], l[j]);
  *(uint4*)(hi + byte_off) = make_uint4(h[0], h[1], h[2], h[3]);
  if (lo) *(uint4*)(lo + byte_off) = make_uint4(l[0], l[1], l[2], l[3]);
}

// A unit already in registers (an MFMA fragment loaded straight from planes): hi + lo -> f32
template <int FMT>
__device__ __forceinline__ void widen_unit(const bf16x8 h, const bf16x8 l, float (&v)[8]) {
  if constexpr (FMT == RSA_PF_F16) {
    const f16x8 hf = __builtin_bit_cast(f16x8, h), lf = __builtin_bit_cast(f16x8, l);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)hf[j] + (float)lf[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j] + (float)l[j];
  }
}

// The same for a run-time format fmt (enum rsa_plane_fmt, wave-uniform) and unit index u
__device__ __forceinline__ void get_unit(const bf16x8* hi, const bf16x8* lo, int64_t u, float (&v)[8], int fmt) {
  const bf16x8 h = hi[u];
  bf16x8 l = {};
  if (lo != nullptr) l = lo[u];
  if (fmt == RSA_PF_F16) {
    const f16x8 hf = __builtin_bit_cast(f16x8, h), lf = __builtin_bit_cast(f16x8, l);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)hf[j] + (lo != nullptr ? (float)lf[j] : 0.f);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j] + (lo != nullptr ? (float)l[j] : 0.f);
  }
}
__device__ __forceinline__ void put_unit(bf16x8* hi, bf16x8* lo, int64_t u, const float (&v)[8], int fmt) {
  if (fmt == RSA_PF_F16) {
    f16x8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float vj = v[j];
      asm("" : "+v"(vj));  // opaque: the lo half is the rounding error of THIS hi (see split2)
      const _Float16 hb = (_Float16)vj;
      h[j] = hb;
      l[j] = (_Float16)(vj - (float)hb);
    }
    hi[u] = __builtin_bit_cast(bf16x8, h);
    if (lo != nullptr) lo[u] = __builtin_bit_cast(bf16x8, l);
    return;
  }
  bf16x8 h, l;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 hb = (__bf16)v[j];
    h[j] = hb;
    l[j] = (__bf16)(v[j] - (float)hb);
  }
  hi[u] = h;
  if (lo != nullptr) lo[u] = l;
}

// one value -> its (hi, lo) halves of the run-time plane format fmt, as 16-bit patterns
__device__ __forceinline__ void split_elem(float v, int fmt, uint16_t& hi, uint16_t& lo) {
  if (fmt == RSA_PF_F16) {
    asm("" : "+v"(v));  // opaque: see split2
    const _Float16 h = (_Float16)v;
    hi = __builtin_bit_cast(uint16_t, h);
    lo = __builtin_bit_cast(uint16_t, (_Float16)(v - (float)h));
  } else {
    const __bf16 h = (__bf16)v;
    hi = __builtin_bit_cast(uint16_t, h);
    lo = __builtin_bit_cast(uint16_t, (__bf16)(v - (float)h));
  }
}

// The activations as torch computes them, on the device library's erff / expf.  NOT conv_common.h's gelu_fast / exp_fast forms, which
// round differently: the two families are not interchangeable.
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float sigmoid_exact(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float mish_exact(float v) {  // x * tanh(softplus(x)), softplus' threshold 20
  if (v > 20.f) return v;
  const float e = expf(v);
  const float t = e * (e + 2.f);
  return v * (t / (t + 2.f));
}

}  // namespace rsa
