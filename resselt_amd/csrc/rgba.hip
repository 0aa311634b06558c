// rgba.hip — the still-image formats of upscale_rgba(): interleaved gray / gray + alpha / RGB / RGBA images of 8 or 16 bits <-> float NCHW
// (resselt_amd/tiling.py).
//
// rsa_image_to_nchw_alpha turns such an image into the [N][Cm][H][W] colour tensor in [0, 1] a model reads, the alpha tensor beside it, and one
// flag per image that says whether any alpha code is below the maximum; the colour it writes under fully transparent pixels is bled in from
// the visible edge.  rsa_nchw_to_image_alpha turns a model's output (and an optional alpha source) back into the interleaved image.
//
// Definition.  C = 1: gray, 2: gray + alpha, 3: RGB, 4: RGBA; alpha is straight (not premultiplied) and is the last channel.  M = 255 for
// bits = 8 (uint8 samples), 65535 for bits = 16 (uint16 samples, the full range).
//   read: value = code / M (a true f32 division: what torch's img.float() / M gives).  Gray is written to all Cm channels of the colour tensor.
//   edge bleed (C = 2, 4; `bleed` passes): K_0 = {alpha code > 0}.  Pass p = 1 .. bleed: every pixel outside K_(p-1) whose 3 x 3 neighbours
//     (centre and positions outside the image excluded) hold a set S of pixels of K_(p-1), S not empty, takes the colour
//     sum_S w c_(p-1) / sum_S w, w = 2 for the four edge neighbours and 1 for the four diagonal ones, and joins K_p.  Every other pixel keeps
//     its colour; alpha is never changed.  Both sums are f32, taken in row-major order over the 3 x 3, and divided by a true division.
//   write: gray = the f32 mean of the Cm colour channels in channel order ((c0 + c1) + c2) / 3 (Cm = 1: the channel itself), alpha = the f32
//     mean of the Ca channels of the alpha source in the same way (no alpha source: the maximum code); each value is clamped to [0, 1]
//     (NaN -> 0, the rule of rsa_nchw_to_image_u8), multiplied by M and rounded half to even.
//
// Layout of rsa_image_to_nchw_alpha: a thread owns 4 consecutive pixels of a row, a workgroup is 256 threads = a 64 x 16 pixel tile
// (kRgbaTileW x kRgbaTileH); grid = (tiles across, tiles down, batch).  A pixel is filled in exactly one pass (the pass equal to its Chebyshev
// distance from K_0), from pixels that were filled in earlier passes, so a tile can run the passes in place on a copy of its surroundings: a
// tile that holds an alpha = 0 pixel stages itself and a halo of `bleed` pixels in LDS (f32 colour and one byte per pixel: the pass in which it
// became known, 255 = not yet, 254 = outside the image), runs the passes there (pass p on the staged region shrunk by p pixels: what the
// tile's own pixels can still depend on) and writes its own pixels.  Everything a pixel within `bleed` of K_0 depends on lies within `bleed`
// of it, so the result does not depend on the tiling.  A tile without an alpha = 0 pixel needs none of this and stages nothing (an opaque image
// costs what bleed = 0 costs); a tile whose staged region holds no known pixel skips the passes.  LDS: (64 + 2 bleed) x (16 + 2 bleed) pixels of
// 13 bytes (5 for gray), dynamic: 33,280 bytes at bleed 8, 59,904 at bleed 16 (two workgroups per CU at the largest).
// Layout of rsa_nchw_to_image_alpha: a thread owns 4 consecutive pixels, a workgroup 64 x 4 threads = 256 x 4 pixels, no LDS.
// When W is a multiple of 4 and every base, pitch and batch stride is a multiple of the thread's vector (4 pixels: 4 C bytes of an 8-bit, 8 C
// of a 16-bit image, moved as 4-, 8- or 16-byte accesses; 8 or 16 bytes of the float side) each access is a vector; any other frame takes the
// element-wise instantiation of the same arithmetic.  No atomics anywhere: two runs are bit-identical.
//
// Byte model: every operand once.  Measurements: profiles/rgba_measure.txt.
//
// No header under include/ declares these entry points (helpers of the engine's tiler, registered in engine/lib.py INTERNAL):
//
//   int rsa_image_to_nchw_alpha(const void* img, int64_t pitch, int64_t batch_stride, int32_t bits, int32_t batch, int32_t H, int32_t W, int32_t C,
//                               int32_t Cm, int32_t bleed, void* color, int32_t color_dtype, void* alpha, int32_t alpha_mode, void* flags,
//                               void* stream);
//   int rsa_nchw_to_image_alpha(const void* color, int32_t color_dtype, int32_t Cm, const void* alpha, int32_t alpha_dtype, int32_t Ca,
//                               int32_t batch, int32_t H, int32_t W, int32_t C, int32_t bits, void* img, int64_t pitch, int64_t batch_stride,
//                               void* stream);
//
//   img         [batch][H] rows of W pixels of C samples; a row starts `pitch` BYTES after the one before, an image `batch_stride` bytes after
//               the one before.  Bytes of a pitch past the row are never read or written.
//   bits        8 (uint8 samples) or 16 (uint16 samples)
//   C           1 .. 4 (see above);  Cm  the channels of the model, 1 or 3 (C >= 3 needs 3)
//   bleed       0 .. 16 passes; ignored for C = 1, 3
//   color       dense [batch][Cm][H][W] of RSA_F32 / RSA_F16 / RSA_BF16 (color_dtype)
//   alpha       read side, by alpha_mode: 0 = not written (may be NULL); 1 = dense [batch][Cm][H][W] of color_dtype, alpha replicated (further
//               batch entries for the model); 2 = dense [batch][1][H][W] of f32.  Ignored for C = 1, 3.
//               write side: NULL (alpha = the maximum code) or dense [batch][Ca][H][W] of alpha_dtype, Ca = 1 or Cm.  Ignored for C = 1, 3.
//   flags       int32 [batch], ZERO on entry; flags[n] becomes 1 when an alpha code of image n is below the maximum (a plain store of the
//               same value by every thread that sees one).  Needed for C = 2, 4, ignored otherwise.
//
// RSA_E_ARG before any launch for a null operand, C outside 1..4, Cm not 1 or 3 (or 1 with C >= 3), Ca not 1 or Cm, bits other than 8 / 16,
// bleed outside 0..16, alpha_mode outside 0..2, batch, H or W < 1, a dtype that is not RSA_F32 / RSA_F16 / RSA_BF16, a pitch smaller than a
// row, a batch stride (batch > 1) smaller than an image, or a grid that does not fit (more than 65535 images or tile rows).  RSA_E_ALIGN for an
// image base, pitch or stride that is no multiple of the sample size, a float tensor not aligned to its element, or flags not aligned to 4.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "common.h"

namespace rsa {
namespace {

constexpr int kRgbaPix = 4;                              // pixels of a thread
constexpr int kRgbaTileW = 64, kRgbaTileH = 16;          // read kernel: 16 x 16 threads
constexpr int kRgbaThreads = 256;
constexpr int kRgbaMaxBleed = 16;
constexpr int kRgbaWriteTx = 64, kRgbaWriteTy = 4;       // write kernel: 256 x 4 pixels
constexpr unsigned char kUnknown = 255, kOutside = 254;  // pass marks of a staged pixel beyond 0 .. 16

constexpr int rgba_vec_align(int bytes) { return (bytes & -bytes) > 16 ? 16 : (bytes & -bytes); }

template <typename Code, int C>
struct alignas(rgba_vec_align(kRgbaPix * C * (int)sizeof(Code))) PixVec {  // a thread's 4 pixels
  Code v[kRgbaPix * C];
};
template <typename Code, int C>
struct alignas((C == 2 || C == 4) ? C * sizeof(Code) : sizeof(Code)) OnePix {
  Code v[C];
};
template <typename F>
struct alignas(kRgbaPix * sizeof(F)) Vec4 {
  F v[kRgbaPix];
};

__device__ __forceinline__ float clamp01_(float v) { return fminf(fmaxf(v, 0.f), 1.f); }  // NaN -> 0

// 4 values of a row of F starting at `row + x0` (element-wise: columns at or past W read as 0)
template <typename F, bool kVec>
__device__ __forceinline__ void load4(const F* row, int x0, int W, float out[kRgbaPix]) {
  if constexpr (kVec) {
    const Vec4<F> t = *(const Vec4<F>*)(row + x0);
#pragma unroll
    for (int p = 0; p < kRgbaPix; ++p) out[p] = (float)t.v[p];
  } else {
#pragma unroll
    for (int p = 0; p < kRgbaPix; ++p) out[p] = x0 + p < W ? (float)row[x0 + p] : 0.f;
  }
}

template <typename F, bool kVec>
__device__ __forceinline__ void store4(F* row, int x0, int W, const float v[kRgbaPix]) {
  if constexpr (kVec) {
    Vec4<F> t;
#pragma unroll
    for (int p = 0; p < kRgbaPix; ++p) t.v[p] = (F)v[p];
    *(Vec4<F>*)(row + x0) = t;
  } else {
#pragma unroll
    for (int p = 0; p < kRgbaPix; ++p)
      if (x0 + p < W) row[x0 + p] = (F)v[p];
  }
}

// grid: x = tiles of 64 columns, y = tiles of 16 rows, z = batch; block 256; dynamic LDS: rgba_lds_bytes (0 when nothing can bleed)
template <typename Code, typename F, int C, bool kVec>
__global__ __launch_bounds__(kRgbaThreads) void image_to_nchw_alpha_kernel(const uint8_t* __restrict__ img, int64_t pitch, int64_t batch_stride, int H, int W,
                                                                             int Cm, int bleed, F* __restrict__ color, void* __restrict__ alpha,
                                                                             int alpha_mode, int32_t* __restrict__ flags) {
  constexpr int kCs = C <= 2 ? 1 : 3;  // colour channels of the image
  constexpr bool kHasA = C == 2 || C == 4;
  constexpr float kM = sizeof(Code) == 1 ? 255.f : 65535.f;
  constexpr unsigned kMax = sizeof(Code) == 1 ? 255u : 65535u;
  extern __shared__ __align__(16) unsigned char rgba_smem[];
  const int t = threadIdx.x, n = blockIdx.z;
  const int tx0 = blockIdx.x * kRgbaTileW, ty0 = blockIdx.y * kRgbaTileH;
  const int x0 = tx0 + (t & 15) * kRgbaPix, y = ty0 + (t >> 4);
  const bool live = x0 < W && y < H;  // no thread leaves before the last barrier
  const uint8_t* base = img + (int64_t)n * batch_stride;

  float col[kCs][kRgbaPix];
  unsigned a[kRgbaPix];
  {
    PixVec<Code, C> pv;
#pragma unroll
    for (int i = 0; i < kRgbaPix * C; ++i) pv.v[i] = (i % C == C - 1 && kHasA) ? (Code)kMax : (Code)0;  // what a pixel past the frame counts as
    if (live) {
      const Code* row = (const Code*)(base + (int64_t)y * pitch);
      if constexpr (kVec) {
        pv = *(const PixVec<Code, C>*)(row + (int64_t)x0 * C);
      } else {
#pragma unroll
        for (int p = 0; p < kRgbaPix; ++p)
          if (x0 + p < W) {
#pragma unroll
            for (int c = 0; c < C; ++c) pv.v[p * C + c] = row[(int64_t)(x0 + p) * C + c];
          }
      }
    }
#pragma unroll
    for (int p = 0; p < kRgbaPix; ++p) {
#pragma unroll
      for (int c = 0; c < kCs; ++c) col[c][p] = (float)pv.v[p * C + c] / kM;
      a[p] = kHasA ? (unsigned)pv.v[p * C + C - 1] : kMax;
    }
  }

  if constexpr (kHasA) {
    bool below = false, zero = false;
#pragma unroll
    for (int p = 0; p < kRgbaPix; ++p) below |= a[p] < kMax, zero |= a[p] == 0;
    if (below) flags[n] = 1;
    if (bleed > 0 && __syncthreads_or(zero)) {  // `bleed` is uniform: every thread of the block takes the barrier, or none
      const int RW = kRgbaTileW + 2 * bleed, RH = kRgbaTileH + 2 * bleed, R = RW * RH;
      float* lc = (float*)rgba_smem;                           // [kCs][R] colour
      unsigned char* ld = rgba_smem + (size_t)kCs * R * 4;     // [R] pass in which the pixel became known
      bool known = false;
      for (int ly = t >> 6; ly < RH; ly += kRgbaThreads / 64)
        for (int lx = t & 63; lx < RW; lx += 64) {
          const int gx = tx0 - bleed + lx, gy = ty0 - bleed + ly, i = ly * RW + lx;
          unsigned char d = kOutside;
          if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const Code* px = (const Code*)(base + (int64_t)gy * pitch) + (int64_t)gx * C;
            OnePix<Code, C> q;
            if constexpr (kVec) {
              q = *(const OnePix<Code, C>*)px;
            } else {
#pragma unroll
              for (int c = 0; c < C; ++c) q.v[c] = px[c];
            }
#pragma unroll
            for (int c = 0; c < kCs; ++c) lc[c * R + i] = (float)q.v[c] / kM;
            d = q.v[C - 1] > 0 ? 0 : kUnknown;
            known |= q.v[C - 1] > 0;
          }
          ld[i] = d;
        }
      if (__syncthreads_or(known)) {
        for (int p = 1; p <= bleed; ++p) {
          // a pixel q rings outside the tile matters to the tile up to pass bleed - q only
          for (int ly = p + (t >> 6); ly < RH - p; ly += kRgbaThreads / 64)
            for (int lx = p + (t & 63); lx < RW - p; lx += 64) {
              const int i = ly * RW + lx;
              if (ld[i] != kUnknown) continue;
              float num[kCs], den = 0.f;
#pragma unroll
              for (int c = 0; c < kCs; ++c) num[c] = 0.f;
#pragma unroll
              for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                  if (dy == 0 && dx == 0) continue;
                  const int j = i + dy * RW + dx;  // 1 <= p <= lx, ly and lx < RW - p, ly < RH - p: inside the staged region
                  // a neighbour that is being filled in this very pass reads as 255 or as p: neither is below p
                  if (ld[j] < p) {
                    const float w = (dy == 0 || dx == 0) ? 2.f : 1.f;
#pragma unroll
                    for (int c = 0; c < kCs; ++c) num[c] += w * lc[c * R + j];
                    den += w;
                  }
                }
              if (den > 0.f) {
#pragma unroll
                for (int c = 0; c < kCs; ++c) lc[c * R + i] = num[c] / den;
                ld[i] = (unsigned char)p;
              }
            }
          __syncthreads();
        }
        const int li = ((t >> 4) + bleed) * RW + (t & 15) * kRgbaPix + bleed;
#pragma unroll
        for (int p = 0; p < kRgbaPix; ++p)
          if (a[p] == 0) {
#pragma unroll
            for (int c = 0; c < kCs; ++c) col[c][p] = lc[c * R + li + p];
          }
      }
    }
  }
  if (!live) return;

#pragma unroll
  for (int cm = 0; cm < 3; ++cm)
    if (cm < Cm) store4<F, kVec>(color + (((int64_t)n * Cm + cm) * H + y) * W, x0, W, col[kCs == 1 ? 0 : cm]);
  if constexpr (kHasA) {
    float av[kRgbaPix];
#pragma unroll
    for (int p = 0; p < kRgbaPix; ++p) av[p] = (float)a[p] / kM;
    if (alpha_mode == 1) {
#pragma unroll
      for (int cm = 0; cm < 3; ++cm)
        if (cm < Cm) store4<F, kVec>((F*)alpha + (((int64_t)n * Cm + cm) * H + y) * W, x0, W, av);
    } else if (alpha_mode == 2) {
      store4<float, kVec>((float*)alpha + ((int64_t)n * H + y) * W, x0, W, av);
    }
  }
}

// the f32 mean of `channels` (1 or 3) rows of a float tensor, 4 pixels; `dtype` is uniform
template <bool kVec>
__device__ __forceinline__ void mean4(const void* src, int dtype, int64_t first, int64_t plane, int channels, int x0, int W, float out[kRgbaPix]) {
  float v[3][kRgbaPix];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (c < channels) {
      const int64_t o = first + c * plane;
      if (dtype == RSA_F32)
        load4<float, kVec>((const float*)src + o, x0, W, v[c]);
      else if (dtype == RSA_F16)
        load4<_Float16, kVec>((const _Float16*)src + o, x0, W, v[c]);
      else
        load4<__bf16, kVec>((const __bf16*)src + o, x0, W, v[c]);
    }
#pragma unroll
  for (int p = 0; p < kRgbaPix; ++p) out[p] = channels == 3 ? ((v[0][p] + v[1][p]) + v[2][p]) / 3.f : v[0][p];
}

// grid: x = tiles of 256 columns, y = tiles of 4 rows, z = batch; block (64, 4)
template <typename F, typename Code, int C, bool kVec>
__global__ __launch_bounds__(kRgbaThreads) void nchw_to_image_alpha_kernel(const F* __restrict__ color, int Cm, const void* __restrict__ alpha, int alpha_dtype,
                                                                             int Ca, int H, int W, uint8_t* __restrict__ img, int64_t pitch,
                                                                             int64_t batch_stride) {
  constexpr int kCs = C <= 2 ? 1 : 3;
  constexpr bool kHasA = C == 2 || C == 4;
  constexpr float kM = sizeof(Code) == 1 ? 255.f : 65535.f;
  constexpr int kDtype = std::is_same<F, float>::value ? RSA_F32 : std::is_same<F, _Float16>::value ? RSA_F16 : RSA_BF16;
  const int n = blockIdx.z;
  const int x0 = (blockIdx.x * kRgbaWriteTx + threadIdx.x) * kRgbaPix, y = blockIdx.y * kRgbaWriteTy + threadIdx.y;
  if (x0 >= W || y >= H) return;
  const int64_t plane = (int64_t)H * W, at = (int64_t)y * W;

  float val[C][kRgbaPix];
  if constexpr (kCs == 1) {
    mean4<kVec>(color, kDtype, (int64_t)n * Cm * plane + at, plane, Cm, x0, W, val[0]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) load4<F, kVec>(color + ((int64_t)n * 3 + c) * plane + at, x0, W, val[c]);
  }
  if constexpr (kHasA) {
    if (alpha != nullptr) {
      mean4<kVec>(alpha, alpha_dtype, (int64_t)n * Ca * plane + at, plane, Ca, x0, W, val[C - 1]);
    } else {
#pragma unroll
      for (int p = 0; p < kRgbaPix; ++p) val[C - 1][p] = 1.f;
    }
  }
  PixVec<Code, C> pv;
#pragma unroll
  for (int p = 0; p < kRgbaPix; ++p)
#pragma unroll
    for (int c = 0; c < C; ++c) pv.v[p * C + c] = (Code)rintf(clamp01_(val[c][p]) * kM);  // rintf: half to even
  Code* row = (Code*)(img + (int64_t)n * batch_stride + (int64_t)y * pitch);
  if constexpr (kVec) {
    *(PixVec<Code, C>*)(row + (int64_t)x0 * C) = pv;
  } else {
#pragma unroll
    for (int p = 0; p < kRgbaPix; ++p)
      if (x0 + p < W) {
#pragma unroll
        for (int c = 0; c < C; ++c) row[(int64_t)(x0 + p) * C + c] = pv.v[p * C + c];
      }
  }
}

// Run-time (bits, float dtype, C, vector path) -> the kernel's template arguments, spelled once per entry point
template <class Fn>
void with_rgba_types(int bits, int dtype, int C, bool vec, Fn&& f) {
  auto with_vec = [&](auto code, auto flt, auto c) {
    if (vec)
      f(code, flt, c, std::true_type{});
    else
      f(code, flt, c, std::false_type{});
  };
  auto with_c = [&](auto code, auto flt) {
    if (C == 1)
      with_vec(code, flt, std::integral_constant<int, 1>{});
    else if (C == 2)
      with_vec(code, flt, std::integral_constant<int, 2>{});
    else if (C == 3)
      with_vec(code, flt, std::integral_constant<int, 3>{});
    else
      with_vec(code, flt, std::integral_constant<int, 4>{});
  };
  auto with_float = [&](auto code) {
    if (dtype == RSA_F32)
      with_c(code, float{});
    else if (dtype == RSA_F16)
      with_c(code, _Float16{});
    else
      with_c(code, __bf16{});
  };
  if (bits == 8)
    with_float(uint8_t{});
  else
    with_float(uint16_t{});
}

inline uintptr_t elem_mask(int dtype) { return dtype == RSA_F32 ? 3 : 1; }

// The argument checks both entry points share; `who` names the entry point in the message.  RSA_OK, or the status to return.
int rgba_check(const char* who, const void* img, int64_t pitch, int64_t batch_stride, int bits, int batch, int H, int W, int C, int Cm, const void* color,
               int color_dtype, int64_t tile_h) {
  char msg[160];  // set_error copies it
  auto fail = [&](int code, const char* what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return set_error(code, msg);
  };
  if (img == nullptr || color == nullptr) return fail(RSA_E_ARG, "null pointer");
  if (C < 1 || C > 4) return fail(RSA_E_ARG, "C must be 1 (gray), 2 (gray + alpha), 3 (RGB) or 4 (RGBA)");
  if (bits != 8 && bits != 16) return fail(RSA_E_ARG, "bits must be 8 or 16");
  if (batch < 1 || H < 1 || W < 1) return fail(RSA_E_ARG, "batch, H and W must be >= 1");
  if ((Cm != 1 && Cm != 3) || (C >= 3 && Cm != 3)) return fail(RSA_E_ARG, "Cm must be 1 or 3, and 3 for a colour image");
  if (color_dtype < RSA_F32 || color_dtype > RSA_BF16) return fail(RSA_E_ARG, "the float tensor must be RSA_F32, RSA_F16 or RSA_BF16");
  const int64_t sample = bits / 8, row = (int64_t)W * C * sample;
  if (pitch < row) return fail(RSA_E_ARG, "the pitch is smaller than a row");
  if (batch > 1 && batch_stride < pitch * H) return fail(RSA_E_ARG, "the batch stride is smaller than an image");
  if (batch > 65535 || ((int64_t)H + tile_h - 1) / tile_h > 65535) return fail(RSA_E_ARG, "more than 65535 images or tile rows: the grid does not fit");
  if (((uintptr_t)img | (uintptr_t)pitch | (uintptr_t)batch_stride) & (sample - 1)) return fail(RSA_E_ALIGN, "image base, pitch or batch stride is no multiple of the sample size");
  if ((uintptr_t)color & elem_mask(color_dtype)) return fail(RSA_E_ALIGN, "the float tensor is not aligned to its element size");
  return RSA_OK;
}

// One vector per lane and access: W a multiple of 4, the image's base, pitch and stride multiples of the 4-pixel vector, the float tensors of
// 4 elements (their rows then are too)
bool rgba_vector_path(const void* img, int64_t pitch, int64_t batch_stride, int bits, int W, int C, const void* color, int color_dtype, const void* alpha,
                      int alpha_dtype) {
  const uintptr_t vec = (uintptr_t)rgba_vec_align(kRgbaPix * C * bits / 8);
  const uintptr_t cvec = kRgbaPix * (elem_mask(color_dtype) + 1), avec = kRgbaPix * (elem_mask(alpha_dtype) + 1);
  return W % kRgbaPix == 0 && (((uintptr_t)img | (uintptr_t)pitch | (uintptr_t)batch_stride) & (vec - 1)) == 0 && ((uintptr_t)color & (cvec - 1)) == 0 &&
         ((uintptr_t)alpha & (avec - 1)) == 0;
}

}  // namespace
}  // namespace rsa

extern "C" int rsa_image_to_nchw_alpha(const void* img, int64_t pitch, int64_t batch_stride, int32_t bits, int32_t batch, int32_t H, int32_t W, int32_t C,
                                       int32_t Cm, int32_t bleed, void* color, int32_t color_dtype, void* alpha, int32_t alpha_mode, void* flags,
                                       void* stream) {
  using namespace rsa;
  const char* who = "rsa_image_to_nchw_alpha";
  const int rc = rgba_check(who, img, pitch, batch_stride, bits, batch, H, W, C, Cm, color, color_dtype, kRgbaTileH);
  if (rc != RSA_OK) return rc;
  if (bleed < 0 || bleed > kRgbaMaxBleed) return set_error(RSA_E_ARG, "rsa_image_to_nchw_alpha: bleed must be 0 .. 16");
  if (alpha_mode < 0 || alpha_mode > 2) return set_error(RSA_E_ARG, "rsa_image_to_nchw_alpha: alpha_mode must be 0 (none), 1 (model) or 2 (resample)");
  const bool has_alpha = C == 2 || C == 4;
  if (!has_alpha) alpha = nullptr, alpha_mode = 0, bleed = 0;
  if (has_alpha && (flags == nullptr || (alpha_mode != 0 && alpha == nullptr))) return set_error(RSA_E_ARG, "rsa_image_to_nchw_alpha: null pointer (alpha or flags)");
  if (alpha_mode == 0) alpha = nullptr;
  if (has_alpha && ((uintptr_t)flags & 3)) return set_error(RSA_E_ALIGN, "rsa_image_to_nchw_alpha: flags are not aligned to 4 bytes");
  if ((uintptr_t)alpha & (alpha_mode == 2 ? 3 : elem_mask(color_dtype))) return set_error(RSA_E_ALIGN, "rsa_image_to_nchw_alpha: the alpha tensor is not aligned to its element size");
  const bool vec = rgba_vector_path(img, pitch, batch_stride, bits, W, C, color, color_dtype, alpha, alpha_mode == 2 ? RSA_F32 : color_dtype);
  const size_t lds = bleed > 0 ? (size_t)(kRgbaTileW + 2 * bleed) * (kRgbaTileH + 2 * bleed) * ((C <= 2 ? 1 : 3) * 4 + 1) : 0;  // at most 59,904 bytes
  const dim3 grid((unsigned)((W + kRgbaTileW - 1) / kRgbaTileW), (unsigned)((H + kRgbaTileH - 1) / kRgbaTileH), (unsigned)batch);
  with_rgba_types(bits, color_dtype, C, vec, [&](auto code, auto flt, auto c, auto v) {
    using Code = decltype(code);
    using F = decltype(flt);
    hipLaunchKernelGGL((image_to_nchw_alpha_kernel<Code, F, decltype(c)::value, decltype(v)::value>), grid, dim3(kRgbaThreads), lds, (hipStream_t)stream,
                       (const uint8_t*)img, pitch, batch_stride, H, W, Cm, bleed, (F*)color, alpha, alpha_mode, (int32_t*)flags);
  });
  return launch_status("rsa_image_to_nchw_alpha: launch failed");
}

extern "C" int rsa_nchw_to_image_alpha(const void* color, int32_t color_dtype, int32_t Cm, const void* alpha, int32_t alpha_dtype, int32_t Ca, int32_t batch,
                                       int32_t H, int32_t W, int32_t C, int32_t bits, void* img, int64_t pitch, int64_t batch_stride, void* stream) {
  using namespace rsa;
  const char* who = "rsa_nchw_to_image_alpha";
  const int rc = rgba_check(who, img, pitch, batch_stride, bits, batch, H, W, C, Cm, color, color_dtype, kRgbaWriteTy);
  if (rc != RSA_OK) return rc;
  if (!(C == 2 || C == 4)) alpha = nullptr;
  if (alpha != nullptr) {
    if (Ca != 1 && Ca != Cm) return set_error(RSA_E_ARG, "rsa_nchw_to_image_alpha: Ca must be 1 or Cm");
    if (alpha_dtype < RSA_F32 || alpha_dtype > RSA_BF16) return set_error(RSA_E_ARG, "rsa_nchw_to_image_alpha: the alpha source must be RSA_F32, RSA_F16 or RSA_BF16");
    if ((uintptr_t)alpha & elem_mask(alpha_dtype)) return set_error(RSA_E_ALIGN, "rsa_nchw_to_image_alpha: the alpha source is not aligned to its element size");
  }
  const bool vec = rgba_vector_path(img, pitch, batch_stride, bits, W, C, color, color_dtype, alpha, alpha != nullptr ? alpha_dtype : RSA_F32);
  const dim3 grid((unsigned)((W + kRgbaWriteTx * kRgbaPix - 1) / (kRgbaWriteTx * kRgbaPix)), (unsigned)((H + kRgbaWriteTy - 1) / kRgbaWriteTy), (unsigned)batch);
  with_rgba_types(bits, color_dtype, C, vec, [&](auto code, auto flt, auto c, auto v) {
    using Code = decltype(code);
    using F = decltype(flt);
    hipLaunchKernelGGL((nchw_to_image_alpha_kernel<F, Code, decltype(c)::value, decltype(v)::value>), grid, dim3(kRgbaWriteTx, kRgbaWriteTy), 0,
                       (hipStream_t)stream, (const F*)color, Cm, alpha, alpha_dtype, Ca, H, W, (uint8_t*)img, pitch, batch_stride);
  });
  return launch_status("rsa_nchw_to_image_alpha: launch failed");
}
