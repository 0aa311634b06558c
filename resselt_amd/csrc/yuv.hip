// yuv.hip — the pixel formats of video for upscale_yuv(): two-plane Y'CbCr 4:2:0 (NV12, P010) <-> float R'G'B' NCHW (resselt_amd/tiling.py,
// DESIGN.md §31).
//
// A video decoder delivers, and an encoder accepts, a luma plane and a plane of interleaved (Cb, Cr) pairs at half the resolution of both axes.
// rsa_yuv420_to_nchw turns such a frame into the [N][3][H][W] tensor in [0, 1] a model reads, rsa_nchw_to_yuv420 turns a model's output back.
//
// Definition (bits = 8: NV12, uint8 samples; bits = 10: P010, uint16 words that hold the code in their top 10 bits: code = word >> 6 on read,
// the low 6 bits ignored; word = code << 6 on write).  With m = 2^(bits - 8):
//   limited range  Y' = (code - 16 m) / (219 m)        Cb, Cr = (code - 128 m) / (224 m)
//   full range     Y' = code / (2^bits - 1)            Cb, Cr = (code - 2^(bits - 1)) / (2^bits - 1)
//   matrix (non-constant luminance), (Kr, Kb) = BT.601 (0.299, 0.114), BT.709 (0.2126, 0.0722), BT.2020 (0.2627, 0.0593), Kg = 1 - Kr - Kb:
//     R = Y' + 2 (1 - Kr) Cr,  B = Y' + 2 (1 - Kb) Cb,  G = (Y' - Kr R - Kb B) / Kg;   Y' = Kr R + Kg G + Kb B,  Cb = (B - Y') / (2 (1 - Kb)),
//     Cr = (R - Y') / (2 (1 - Kr)).  The transfer function is untouched: R'G'B' stays gamma-encoded.
//   siting: chroma sample j of an axis sits at luma coordinate 2 j + o; `left` (H.264 / HEVC default): o = 0 horizontally, 0.5 vertically;
//     `center`: o = 0.5 on both axes.
//   read: luma coordinate x takes chroma position u = (x - o) / 2 linearly from the samples floor(u), floor(u) + 1 (indices clamped to the
//     plane; every weight is 0, 1/4, 1/2, 3/4 or 1, so the interpolation of the CODES is exact in f32); R, G, B are clamped to [0, 1].
//   write: the source is clamped to [0, 1] first (NaN -> 0, the rule of rsa_nchw_to_image_u8); Cb, Cr are formed per luma pixel and each axis
//     filters by its siting: o = 0.5: the mean of luma positions 2 j, 2 j + 1; o = 0: [1 2 1] / 4 over 2 j - 1, 2 j, 2 j + 1 (indices clamped);
//     codes are rounded half to even and clamped to [0, 2^bits - 1].
//
// Layout of both kernels: a thread owns 8 luma columns x 2 luma rows = 4 chroma pairs of one chroma row; a workgroup is 32 x 8 threads = a
// 256 x 16 luma tile (kYuvTileW x kYuvTileH); grid = (tiles across, tiles down, batch).  When W is a multiple of 8 and every base, pitch and
// batch stride is a multiple of a thread's vector (8 samples, 16 bytes of the float side) each access of the block is one 8- to 32-byte vector
// per lane; any other frame takes the element-wise variant of the same kernel (same arithmetic, same results).
//   rsa_yuv420_to_nchw: per thread 2 luma vectors, the chroma vector of rows i - 1, i, i + 1 and the neighbouring pair on either side (the
//     vertical neighbours and the side pairs are re-reads, served by the vector cache / L2), 6 stores.
//   rsa_nchw_to_yuv420: per thread 6 source vectors; Y and UV are written by the same launch from the same registers.  The vertical filter
//     (always o = 0.5) runs first in the thread; `left` siting then needs the column to the left of the block: it is the neighbouring lane's
//     last column and comes by a lane shift, only the first thread of a tile row reads it from memory (the one-pixel halo).
// Every sum has a fixed order and there are no atomics: two runs are bit-identical.
//
// Byte model: every operand once (the source planes once, the destination once); measurements: profiles/yuv_measure.txt.
//
// No header under include/ declares these entry points (helpers of the engine's tiler, registered in engine/lib.py INTERNAL):
//
//   int rsa_yuv420_to_nchw(const void* y, int64_t y_pitch, int64_t y_batch_stride, const void* uv, int64_t uv_pitch, int64_t uv_batch_stride,
//                          int32_t bits, int32_t batch, int32_t H, int32_t W, int32_t matrix, int32_t full_range, int32_t chroma_loc,
//                          void* dst, int32_t dst_dtype, void* stream);
//   int rsa_nchw_to_yuv420(const void* src, int32_t src_dtype, int32_t batch, int32_t H, int32_t W, int32_t matrix, int32_t full_range,
//                          int32_t chroma_loc, int32_t bits, void* y, int64_t y_pitch, int64_t y_batch_stride, void* uv, int64_t uv_pitch,
//                          int64_t uv_batch_stride, void* stream);
//
//   y, uv       the planes: y is [batch][H] rows of W samples, uv [batch][H / 2] rows of W / 2 (Cb, Cr) pairs; a row starts y_pitch / uv_pitch
//               BYTES after the one before, an image y_batch_stride / uv_batch_stride bytes after the one before (decoder surfaces are pitched).
//               Bytes of a pitch past the row are never read or written.
//   bits        8 (uint8 samples) or 10 (uint16 words, see above)
//   H, W        luma size, both even
//   matrix      0 = BT.601, 1 = BT.709, 2 = BT.2020;  full_range  0 = limited, 1 = full;  chroma_loc  0 = left, 1 = center
//   dst / src   dense [batch][3][H][W] of RSA_F32 / RSA_F16 / RSA_BF16 (dst_dtype / src_dtype) in R, G, B order
//
// RSA_E_ARG before any launch for a null pointer, bits other than 8 or 10, batch < 1, an odd or non-positive H or W, an enum out of range, a
// dtype that is not RSA_F32 / RSA_F16 / RSA_BF16, a pitch smaller than its row, a batch stride (batch > 1) smaller than its image, or a grid
// that does not fit (more than 65535 images or tile rows).  RSA_E_ALIGN for a y base, pitch or stride that is no multiple of the sample size,
// a uv base, pitch or stride that is no multiple of one (Cb, Cr) pair, or a float tensor not aligned to its element.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "common.h"

namespace rsa {
namespace {

constexpr int kYuvCols = 8;                        // luma columns of a thread
constexpr int kYuvThreadsX = 32, kYuvThreadsY = 8;
constexpr int kYuvTileW = kYuvThreadsX * kYuvCols;  // 256 luma columns of a workgroup
constexpr int kYuvTileH = kYuvThreadsY * 2;         // 16 luma rows

struct YuvRead {
  float y_off, y_mul, c_off, c_mul;  // Y' = (code - y_off) * y_mul, Cb = (code - c_off) * c_mul
  float rv, gu, gv, bu;              // R = Y' + rv Cr, G = Y' - gu Cb - gv Cr, B = Y' + bu Cb
};

struct YuvWrite {
  float kr, kg, kb;
  float y_mul, y_add;           // luma code = Y' * y_mul + y_add
  float cb_mul, cr_mul, c_add;  // chroma code = (filter sum of B - Y' / R - Y') * c?_mul + c_add: the filter's 1/4 or 1/8 is folded in
  float code_max;
};

template <typename T>
struct alignas(8 * sizeof(T) < 16 ? 8 * sizeof(T) : 16) Vec8 {  // 8 samples or pixels: one 8- or 16-byte access, two for f32
  T v[8];
};
template <typename T>
struct alignas(2 * sizeof(T)) Pair {
  T cb, cr;
};

template <typename Code>
constexpr int code_shift() {
  return sizeof(Code) == 2 ? 6 : 0;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }  // NaN -> 0

// grid: x = tiles of 256 luma columns, y = tiles of 16 luma rows, z = batch; block (32, 8)
template <typename Code, typename F, bool kVec, bool kCenter>
__global__ __launch_bounds__(kYuvThreadsX* kYuvThreadsY) void yuv420_to_nchw_kernel(const uint8_t* __restrict__ y, int64_t y_pitch, int64_t y_batch_stride,
                                                                                      const uint8_t* __restrict__ uv, int64_t uv_pitch,
                                                                                      int64_t uv_batch_stride, int H, int W, YuvRead k,
                                                                                      F* __restrict__ dst) {
  constexpr int kShift = code_shift<Code>();
  const int n = blockIdx.z;
  const int x0 = (blockIdx.x * kYuvThreadsX + threadIdx.x) * kYuvCols;
  const int ci = blockIdx.y * kYuvThreadsY + threadIdx.y;  // chroma row: luma rows 2 ci, 2 ci + 1
  const int CH = H / 2, CW = W / 2;
  if (x0 >= W || ci >= CH) return;
  const int j0 = x0 / 2 - 1;  // chroma column of slot 0; slots 1 .. 4 are the block's own pairs

  // chroma codes of rows ci - 1, ci, ci + 1 (clamped), slots 0 .. 5
  float cb[3][6], cr[3][6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int row = min(max(ci - 1 + r, 0), CH - 1);
    const Pair<Code>* p = (const Pair<Code>*)(uv + (int64_t)n * uv_batch_stride + (int64_t)row * uv_pitch);
    if constexpr (kVec) {
      const Vec8<Code> v = *(const Vec8<Code>*)(p + j0 + 1);
#pragma unroll
      for (int s = 0; s < 4; ++s) cb[r][s + 1] = (float)(v.v[2 * s] >> kShift), cr[r][s + 1] = (float)(v.v[2 * s + 1] >> kShift);
      const Pair<Code> hi = p[min(j0 + 5, CW - 1)];
      cb[r][5] = (float)(hi.cb >> kShift), cr[r][5] = (float)(hi.cr >> kShift);
      if constexpr (kCenter) {
        const Pair<Code> lo = p[max(j0, 0)];
        cb[r][0] = (float)(lo.cb >> kShift), cr[r][0] = (float)(lo.cr >> kShift);
      } else {
        cb[r][0] = cr[r][0] = 0.f;  // `left` siting never reads the pair to the left
      }
    } else {
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const Pair<Code> q = p[min(max(j0 + s, 0), CW - 1)];
        cb[r][s] = (float)(q.cb >> kShift), cr[r][s] = (float)(q.cr >> kShift);
      }
    }
  }

#pragma unroll
  for (int lr = 0; lr < 2; ++lr) {
    const int row = 2 * ci + lr;
    // vertical (o = 0.5): row 2 i = 1/4 c[i - 1] + 3/4 c[i], row 2 i + 1 = 3/4 c[i] + 1/4 c[i + 1]; exact: codes have at most 10 bits
    float vb[6], vr[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      vb[s] = lr == 0 ? 0.25f * cb[0][s] + 0.75f * cb[1][s] : 0.75f * cb[1][s] + 0.25f * cb[2][s];
      vr[s] = lr == 0 ? 0.25f * cr[0][s] + 0.75f * cr[1][s] : 0.75f * cr[1][s] + 0.25f * cr[2][s];
    }
    float yc[8];
    const Code* yrow = (const Code*)(y + (int64_t)n * y_batch_stride + (int64_t)row * y_pitch);
    if constexpr (kVec) {
      const Vec8<Code> v = *(const Vec8<Code>*)(yrow + x0);
#pragma unroll
      for (int p = 0; p < 8; ++p) yc[p] = (float)(v.v[p] >> kShift);
    } else {
#pragma unroll
      for (int p = 0; p < 8; ++p) yc[p] = (float)(yrow[min(x0 + p, W - 1)] >> kShift);
    }
    Vec8<F> out[3];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int s = p / 2 + 1;  // slot of chroma column (x0 + p) / 2
      float b, r;
      if constexpr (kCenter) {  // o = 0.5: even x = 1/4 c[j - 1] + 3/4 c[j], odd x = 3/4 c[j] + 1/4 c[j + 1]
        b = p % 2 == 0 ? 0.25f * vb[s - 1] + 0.75f * vb[s] : 0.75f * vb[s] + 0.25f * vb[s + 1];
        r = p % 2 == 0 ? 0.25f * vr[s - 1] + 0.75f * vr[s] : 0.75f * vr[s] + 0.25f * vr[s + 1];
      } else {  // o = 0: even x = c[j], odd x = 1/2 c[j] + 1/2 c[j + 1]
        b = p % 2 == 0 ? vb[s] : 0.5f * vb[s] + 0.5f * vb[s + 1];
        r = p % 2 == 0 ? vr[s] : 0.5f * vr[s] + 0.5f * vr[s + 1];
      }
      const float Y = (yc[p] - k.y_off) * k.y_mul, Cb = (b - k.c_off) * k.c_mul, Cr = (r - k.c_off) * k.c_mul;
      out[0].v[p] = (F)clamp01(fmaf(k.rv, Cr, Y));
      out[1].v[p] = (F)clamp01(fmaf(-k.gv, Cr, fmaf(-k.gu, Cb, Y)));
      out[2].v[p] = (F)clamp01(fmaf(k.bu, Cb, Y));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      F* drow = dst + (((int64_t)n * 3 + c) * H + row) * W;
      if constexpr (kVec) {
        *(Vec8<F>*)(drow + x0) = out[c];
      } else {
#pragma unroll
        for (int p = 0; p < 8; ++p)
          if (x0 + p < W) drow[x0 + p] = out[c].v[p];
      }
    }
  }
}

// One luma pixel of the write path: its code-valued Y' (before rounding) and the two colour differences.
__device__ __forceinline__ void yuv_pixel(float r, float g, float b, const YuvWrite& k, float& ycode, float& db, float& dr) {
  const float Y = fmaf(k.kr, r, fmaf(k.kg, g, k.kb * b));
  ycode = fmaf(Y, k.y_mul, k.y_add);
  db = b - Y, dr = r - Y;
}

__device__ __forceinline__ float to_code(float v, float code_max) { return fminf(fmaxf(rintf(v), 0.f), code_max); }  // rintf: half to even

// grid and block as above
template <typename F, typename Code, bool kVec, bool kCenter>
__global__ __launch_bounds__(kYuvThreadsX* kYuvThreadsY) void nchw_to_yuv420_kernel(const F* __restrict__ src, int H, int W, YuvWrite k,
                                                                                      uint8_t* __restrict__ y, int64_t y_pitch, int64_t y_batch_stride,
                                                                                      uint8_t* __restrict__ uv, int64_t uv_pitch, int64_t uv_batch_stride) {
  constexpr int kShift = code_shift<Code>();
  const int n = blockIdx.z;
  const int x0 = (blockIdx.x * kYuvThreadsX + threadIdx.x) * kYuvCols;
  const int ci = blockIdx.y * kYuvThreadsY + threadIdx.y;
  const bool live = x0 < W && ci < H / 2;
  // a thread past the frame computes on clamped coordinates and stores nothing: every lane takes part in the lane shift below
  const int cic = min(ci, H / 2 - 1);
  const int xv = kVec ? min(x0, W - kYuvCols) : x0;

  float sb[8], sr[8];  // B - Y' and R - Y' summed over the two rows (the vertical filter: o = 0.5 in both sitings)
  Vec8<Code> ycodes[2];
#pragma unroll
  for (int lr = 0; lr < 2; ++lr) {
    const int row = 2 * cic + lr;
    float v[3][8];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const F* srow = src + (((int64_t)n * 3 + c) * H + row) * W;
      if constexpr (kVec) {
        const Vec8<F> t = *(const Vec8<F>*)(srow + xv);
#pragma unroll
        for (int p = 0; p < 8; ++p) v[c][p] = clamp01((float)t.v[p]);
      } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) v[c][p] = clamp01((float)srow[min(xv + p, W - 1)]);
      }
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      float yc, db, dr;
      yuv_pixel(v[0][p], v[1][p], v[2][p], k, yc, db, dr);
      ycodes[lr].v[p] = (Code)((unsigned)to_code(yc, k.code_max) << kShift);
      sb[p] = lr == 0 ? db : sb[p] + db;
      sr[p] = lr == 0 ? dr : sr[p] + dr;
    }
  }

  float hb[4], hr[4];
  if constexpr (kCenter) {  // o = 0.5: luma columns 2 j, 2 j + 1
#pragma unroll
    for (int j = 0; j < 4; ++j) hb[j] = sb[2 * j] + sb[2 * j + 1], hr[j] = sr[2 * j] + sr[2 * j + 1];
  } else {  // o = 0: [1 2 1] over 2 j - 1, 2 j, 2 j + 1; the column left of the block is the last column of the lane before
    float lb = __shfl_up(sb[7], 1), lr_ = __shfl_up(sr[7], 1);
    if (threadIdx.x == 0) {  // first thread of a tile row: the frame's border (clamped to column 0) or the one-pixel halo of the tile
      if (x0 == 0) {
        lb = sb[0], lr_ = sr[0];
      } else {
        const int xl = min(x0, W) - 1;
#pragma unroll
        for (int lr = 0; lr < 2; ++lr) {
          const int64_t o = ((int64_t)n * 3 * H + 2 * cic + lr) * W + xl;
          float yc, db, dr;
          yuv_pixel(clamp01((float)src[o]), clamp01((float)src[o + (int64_t)H * W]), clamp01((float)src[o + 2 * (int64_t)H * W]), k, yc, db, dr);
          lb = lr == 0 ? db : lb + db;
          lr_ = lr == 0 ? dr : lr_ + dr;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hb[j] = ((j == 0 ? lb : sb[2 * j - 1]) + 2.f * sb[2 * j]) + sb[2 * j + 1];
      hr[j] = ((j == 0 ? lr_ : sr[2 * j - 1]) + 2.f * sr[2 * j]) + sr[2 * j + 1];
    }
  }
  if (!live) return;

  Vec8<Code> ccodes;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ccodes.v[2 * j] = (Code)((unsigned)to_code(fmaf(hb[j], k.cb_mul, k.c_add), k.code_max) << kShift);
    ccodes.v[2 * j + 1] = (Code)((unsigned)to_code(fmaf(hr[j], k.cr_mul, k.c_add), k.code_max) << kShift);
  }
  Code* uvrow = (Code*)(uv + (int64_t)n * uv_batch_stride + (int64_t)ci * uv_pitch);
  if constexpr (kVec) {
    *(Vec8<Code>*)(uvrow + x0) = ccodes;
  } else {
#pragma unroll
    for (int p = 0; p < 8; ++p)
      if (x0 + p < W) uvrow[x0 + p] = ccodes.v[p];  // W is even: a pair is stored whole or not at all
  }
#pragma unroll
  for (int lr = 0; lr < 2; ++lr) {
    Code* yrow = (Code*)(y + (int64_t)n * y_batch_stride + (int64_t)(2 * ci + lr) * y_pitch);
    if constexpr (kVec) {
      *(Vec8<Code>*)(yrow + x0) = ycodes[lr];
    } else {
#pragma unroll
      for (int p = 0; p < 8; ++p)
        if (x0 + p < W) yrow[x0 + p] = ycodes[lr].v[p];
    }
  }
}

struct YuvMatrix {
  double kr, kb;
};
constexpr YuvMatrix kYuvMatrices[3] = {{0.299, 0.114}, {0.2126, 0.0722}, {0.2627, 0.0593}};  // BT.601, BT.709, BT.2020

// Run-time (bits, float dtype, vector path, siting) -> the kernel's template arguments, spelled once per entry point
template <class Fn>
void with_yuv_types(int bits, int dtype, bool vec, bool center, Fn&& f) {
  auto with_flags = [&](auto code, auto flt) {
    using Code = decltype(code);
    using F = decltype(flt);
    if (vec && center)
      f(Code{}, F{}, std::true_type{}, std::true_type{});
    else if (vec)
      f(Code{}, F{}, std::true_type{}, std::false_type{});
    else if (center)
      f(Code{}, F{}, std::false_type{}, std::true_type{});
    else
      f(Code{}, F{}, std::false_type{}, std::false_type{});
  };
  auto with_float = [&](auto code) {
    if (dtype == RSA_F32)
      with_flags(code, float{});
    else if (dtype == RSA_F16)
      with_flags(code, _Float16{});
    else
      with_flags(code, __bf16{});
  };
  if (bits == 8)
    with_float(uint8_t{});
  else
    with_float(uint16_t{});
}

// The argument checks both entry points share; `who` names the entry point in the message.  RSA_OK, or the status to return.
int yuv_check(const char* who, const void* flt, int dtype, int batch, int H, int W, int matrix, int full_range, int chroma_loc, int bits, const void* y,
              int64_t y_pitch, int64_t y_batch_stride, const void* uv, int64_t uv_pitch, int64_t uv_batch_stride) {
  char msg[160];  // set_error copies it
  auto fail = [&](int code, const char* what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return set_error(code, msg);
  };
  if (flt == nullptr || y == nullptr || uv == nullptr) return fail(RSA_E_ARG, "null pointer");
  if (bits != 8 && bits != 10) return fail(RSA_E_ARG, "bits must be 8 (NV12) or 10 (P010)");
  if (batch < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(RSA_E_ARG, "batch must be >= 1, H and W positive and even");
  if (matrix < 0 || matrix > 2 || full_range < 0 || full_range > 1 || chroma_loc < 0 || chroma_loc > 1)
    return fail(RSA_E_ARG, "matrix must be 0..2, full_range 0 or 1, chroma_loc 0 (left) or 1 (center)");
  if (dtype < RSA_F32 || dtype > RSA_BF16) return fail(RSA_E_ARG, "the float tensor must be RSA_F32, RSA_F16 or RSA_BF16");
  const int64_t sample = bits == 8 ? 1 : 2, row = (int64_t)W * sample;  // a uv row has W / 2 pairs = W samples too
  if (y_pitch < row || uv_pitch < row) return fail(RSA_E_ARG, "a pitch is smaller than its row");
  if (batch > 1 && (y_batch_stride < y_pitch * H || uv_batch_stride < uv_pitch * (H / 2))) return fail(RSA_E_ARG, "a batch stride is smaller than its image");
  const int64_t tiles_y = ((int64_t)H + kYuvTileH - 1) / kYuvTileH;
  if (batch > 65535 || tiles_y > 65535) return fail(RSA_E_ARG, "more than 65535 images or tile rows: the grid does not fit");
  if (((uintptr_t)y | (uintptr_t)y_pitch | (uintptr_t)y_batch_stride) & (sample - 1)) return fail(RSA_E_ALIGN, "y base, pitch or batch stride is no multiple of the sample size");
  if (((uintptr_t)uv | (uintptr_t)uv_pitch | (uintptr_t)uv_batch_stride) & (2 * sample - 1))
    return fail(RSA_E_ALIGN, "uv base, pitch or batch stride is not aligned to one (Cb, Cr) pair");
  if ((uintptr_t)flt & (dtype == RSA_F32 ? 3 : 1)) return fail(RSA_E_ALIGN, "the float tensor is not aligned to its element size");
  return RSA_OK;
}

// One vector per lane and access: W a multiple of 8, the planes' bases, pitches and strides multiples of 8 samples, the float tensor of 16 bytes
bool yuv_vector_path(const void* flt, int W, int bits, const void* y, int64_t y_pitch, int64_t y_batch_stride, const void* uv, int64_t uv_pitch,
                     int64_t uv_batch_stride) {
  const uintptr_t vec = bits == 8 ? 8 : 16;
  const uintptr_t planes = (uintptr_t)y | (uintptr_t)y_pitch | (uintptr_t)y_batch_stride | (uintptr_t)uv | (uintptr_t)uv_pitch | (uintptr_t)uv_batch_stride;
  return W % kYuvCols == 0 && (planes & (vec - 1)) == 0 && !misaligned16(flt);
}

inline dim3 yuv_grid(int batch, int H, int W) {
  return dim3((unsigned)((W + kYuvTileW - 1) / kYuvTileW), (unsigned)((H + kYuvTileH - 1) / kYuvTileH), (unsigned)batch);
}

}  // namespace
}  // namespace rsa

extern "C" int rsa_yuv420_to_nchw(const void* y, int64_t y_pitch, int64_t y_batch_stride, const void* uv, int64_t uv_pitch, int64_t uv_batch_stride,
                                  int32_t bits, int32_t batch, int32_t H, int32_t W, int32_t matrix, int32_t full_range, int32_t chroma_loc, void* dst,
                                  int32_t dst_dtype, void* stream) {
  using namespace rsa;
  const int rc = yuv_check("rsa_yuv420_to_nchw", dst, dst_dtype, batch, H, W, matrix, full_range, chroma_loc, bits, y, y_pitch, y_batch_stride, uv, uv_pitch,
                           uv_batch_stride);
  if (rc != RSA_OK) return rc;
  const double m = bits == 8 ? 1.0 : 4.0, code_max = bits == 8 ? 255.0 : 1023.0;
  const double kr = kYuvMatrices[matrix].kr, kb = kYuvMatrices[matrix].kb, kg = 1.0 - kr - kb;
  YuvRead k;
  k.y_off = (float)(full_range ? 0.0 : 16.0 * m), k.y_mul = (float)(full_range ? 1.0 / code_max : 1.0 / (219.0 * m));
  k.c_off = (float)(128.0 * m), k.c_mul = (float)(full_range ? 1.0 / code_max : 1.0 / (224.0 * m));
  k.rv = (float)(2.0 * (1.0 - kr)), k.bu = (float)(2.0 * (1.0 - kb));
  k.gu = (float)(kb * 2.0 * (1.0 - kb) / kg), k.gv = (float)(kr * 2.0 * (1.0 - kr) / kg);
  const bool vec = yuv_vector_path(dst, W, bits, y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride);
  with_yuv_types(bits, dst_dtype, vec, chroma_loc == 1, [&](auto code, auto flt, auto v, auto c) {
    using Code = decltype(code);
    using F = decltype(flt);
    hipLaunchKernelGGL((yuv420_to_nchw_kernel<Code, F, decltype(v)::value, decltype(c)::value>), yuv_grid(batch, H, W), dim3(kYuvThreadsX, kYuvThreadsY), 0,
                       (hipStream_t)stream, (const uint8_t*)y, y_pitch, y_batch_stride, (const uint8_t*)uv, uv_pitch, uv_batch_stride, H, W, k, (F*)dst);
  });
  return launch_status("rsa_yuv420_to_nchw: launch failed");
}

extern "C" int rsa_nchw_to_yuv420(const void* src, int32_t src_dtype, int32_t batch, int32_t H, int32_t W, int32_t matrix, int32_t full_range,
                                  int32_t chroma_loc, int32_t bits, void* y, int64_t y_pitch, int64_t y_batch_stride, void* uv, int64_t uv_pitch,
                                  int64_t uv_batch_stride, void* stream) {
  using namespace rsa;
  const int rc = yuv_check("rsa_nchw_to_yuv420", src, src_dtype, batch, H, W, matrix, full_range, chroma_loc, bits, y, y_pitch, y_batch_stride, uv, uv_pitch,
                           uv_batch_stride);
  if (rc != RSA_OK) return rc;
  const double m = bits == 8 ? 1.0 : 4.0, code_max = bits == 8 ? 255.0 : 1023.0;
  const double kr = kYuvMatrices[matrix].kr, kb = kYuvMatrices[matrix].kb, kg = 1.0 - kr - kb;
  const double c_range = full_range ? code_max : 224.0 * m, filter = chroma_loc == 1 ? 0.25 : 0.125;  // 2 x 2 mean, or 2 rows x [1 2 1]
  YuvWrite k;
  k.kr = (float)kr, k.kg = (float)kg, k.kb = (float)kb;
  k.y_mul = (float)(full_range ? code_max : 219.0 * m), k.y_add = (float)(full_range ? 0.0 : 16.0 * m);
  k.cb_mul = (float)(c_range * filter / (2.0 * (1.0 - kb))), k.cr_mul = (float)(c_range * filter / (2.0 * (1.0 - kr)));
  k.c_add = (float)(128.0 * m), k.code_max = (float)code_max;
  const bool vec = yuv_vector_path(src, W, bits, y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride);
  with_yuv_types(bits, src_dtype, vec, chroma_loc == 1, [&](auto code, auto flt, auto v, auto c) {
    using Code = decltype(code);
    using F = decltype(flt);
    hipLaunchKernelGGL((nchw_to_yuv420_kernel<F, Code, decltype(v)::value, decltype(c)::value>), yuv_grid(batch, H, W), dim3(kYuvThreadsX, kYuvThreadsY), 0,
                       (hipStream_t)stream, (const F*)src, H, W, k, (uint8_t*)y, y_pitch, y_batch_stride, (uint8_t*)uv, uv_pitch, uv_batch_stride);
  });
  return launch_status("rsa_nchw_to_yuv420: launch failed");
}
