// tile_blend.hip — feathered-overlap reassembly of tiled inference (resselt_amd/tiling.py, DESIGN.md "Tile seams").
//
// upscale(..., blend = b) lets neighbouring tiles overlap by 2*b input pixels around every interior tile edge and cross-fades them there.
// Each tile contributes a WINDOW of its model output to a full-frame f32 accumulator, weighted by wy(row) * wx(column):
//
//   rising ramp  (top / left,     R output pixels wide, only at an interior edge):  u = (i + 0.5) / R,  i = 0 .. R-1 from the window's edge
//   falling ramp (bottom / right, R output pixels wide, only at an interior edge):  1 - u,  u = (i + 0.5) / R, i counted from the ramp's start
//   elsewhere 1.
//
// The two neighbours at a seam evaluate the same u on the same pixels, so their weights sum to one and nothing is normalised afterwards.
//
// Store / accumulate: tiles arrive in row-major grid order, so a window pixel has had an earlier contributor iff it lies in the window's top
// ramp (tiles of the row above) or its left ramp (the left neighbour).  Such a pixel is load-add-stored, every other pixel is STORED: the
// accumulator needs no zero fill, one launch touches each of its pixels once, there are no atomics and every sum has a fixed order.
//
// No header under include/ declares this entry point (it is a helper of the engine's tiler, registered in engine/lib.py INTERNAL):
//
//   int rsa_tile_blend_accumulate(const void* src, int32_t src_dtype, int32_t batch, int32_t C, int32_t win_h, int32_t win_w,
//                                 int32_t src_h, int32_t src_w, int32_t src_y, int32_t src_x,
//                                 float* acc, int32_t acc_h, int32_t acc_w, int32_t acc_y, int32_t acc_x,
//                                 int32_t ramp_top, int32_t ramp_bottom, int32_t ramp_left, int32_t ramp_right, void* stream);
//
//   src          the model's output for the tile, dense: [batch][C][src_h][src_w] of RSA_F32 / RSA_F16 / RSA_BF16, or for RSA_U8 an 8-bit image
//                [batch][src_h][src_w][C] whose codes enter as code / 255.  (The strides follow from the sizes.)
//   win_h, win_w the window, in output pixels; it starts at (src_y, src_x) in src -- the halo behind the band is skipped -- and at
//                (acc_y, acc_x) in acc.
//   acc          [batch][C][acc_h][acc_w] f32, 16-byte aligned.
//   ramp_*       widths of the four ramps in output pixels, 0 = no ramp on that side (an image border).
//
// RSA_E_ARG before any launch for a null pointer, a size < 1, a negative offset or ramp, a window that leaves src or acc, a ramp wider than the
// window, a dtype that is no rsa_dtype or a grid past the launch limits; RSA_E_ALIGN for a misaligned acc or src.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"

namespace rsa {
namespace {

// One thread: 4 consecutive output pixels of a row (one 16 B accumulator vector); one workgroup: up to 1024 pixels of ONE row.  Workgroups
// that walk several rows (their column weights computed once) were measured slower, monotonically: 35.9 / 32.6 / 29.2 / 26.2 us per launch
// with 8 / 4 / 2 / 1 rows on the 2224 x 3904 x 3 window of a 1080p frame (profiles/tile_blend_measure.txt) -- a thread's rows are a serial
// chain of load -> table look-up -> store, and more, shorter workgroups hide it.  The row weight is the same for the whole workgroup and the
// column weights divide only inside a ramp, so the divisions stay far below one per element.
constexpr int kBlendThreads = 256;

// weight of position i of a window axis of length len with a rising ramp of `rise` pixels at its start and a falling one of `fall` at its end
__device__ __forceinline__ float ramp_weight(int i, int len, int rise, int fall) {
  float w = 1.f;
  if (i < rise) w = ((float)i + 0.5f) / (float)rise;
  if (i >= len - fall) w *= 1.f - ((float)(i - (len - fall)) + 0.5f) / (float)fall;
  return w;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ float bits16_to_float(uint16_t b) {
  if constexpr (std::is_same<T, _Float16>::value) {
    union { uint16_t u; _Float16 h; } c;
    c.u = b;
    return (float)c.h;
  } else {
    return __uint_as_float((uint32_t)b << 16);  // bf16: the upper half of an f32
  }
}

// 4 consecutive elements of a float row: one 16 B / 8 B load where the address allows it
__device__ __forceinline__ void load4(const float* p, float y[4]) {
  if (((uintptr_t)p & 15) == 0) {
    const f32x4 v = *(const f32x4*)p;
    y[0] = v[0], y[1] = v[1], y[2] = v[2], y[3] = v[3];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = p[k];
  }
}
template <typename T>
__device__ __forceinline__ void load4(const T* p, float y[4]) {
  if (((uintptr_t)p & 7) == 0) {
    const u16x4 v = *(const u16x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = bits16_to_float<T>(v[k]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = (float)p[k];
  }
}

// One accumulator row segment [x0, x0 + 4) of the window (clipped to [0, win_w)): `full` segments are 16 B aligned in acc.
// y[k] = source value, w[k] = wy * wx, add = the row lies in the top ramp; columns below ramp_left always add.
__device__ __forceinline__ void blend_store(float* dst, int x0, int win_w, const float y[4], const float wx[4], float wy, bool add, int ramp_left) {
  if (x0 >= 0 && x0 + 4 <= win_w) {
    f32x4 old = {0.f, 0.f, 0.f, 0.f};
    const bool any_add = add || x0 < ramp_left;
    if (any_add) old = *(const f32x4*)(dst + x0);  // lanes of the vector that are stored may read anything: the select drops it
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float w = wy * wx[k];
      v[k] = (add || x0 + k < ramp_left) ? fmaf(w, y[k], old[k]) : w * y[k];
    }
    *(f32x4*)(dst + x0) = v;
  } else {  // ragged head / tail of the row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      if (x < 0 || x >= win_w) continue;
      const float w = wy * wx[k];
      dst[x] = (add || x < ramp_left) ? fmaf(w, y[k], dst[x]) : w * y[k];
    }
  }
}

struct BlendGeom {
  int C, win_h, win_w;
  int src_h, src_w, src_y, src_x;
  int acc_h, acc_w, acc_y, acc_x;
  int ramp_top, ramp_bottom, ramp_left, ramp_right;
};

// the four column weights of a thread's segment (positions outside the window are not used)
__device__ __forceinline__ void column_weights(int x0, const BlendGeom& g, float wx[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) wx[k] = ramp_weight(min(max(x0 + k, 0), g.win_w - 1), g.win_w, g.ramp_left, g.ramp_right);
}

// grid: x = 4-pixel segments of a row / 256, y = window row, z = batch * C
template <typename T>
__global__ __launch_bounds__(kBlendThreads) void tile_blend_nchw_kernel(const T* __restrict__ src, float* __restrict__ acc, BlendGeom g) {
  const int r = blockIdx.y;
  const int64_t plane = blockIdx.z;                                        // n * C + c
  const int64_t d0 = (plane * g.acc_h + g.acc_y + r) * g.acc_w + g.acc_x;  // element index of the window row in acc
  const int x0 = (blockIdx.x * kBlendThreads + threadIdx.x) * 4 - (int)(d0 & 3);  // segments start on 16 B boundaries of acc
  if (x0 >= g.win_w) return;
  float wx[4], y[4];
  column_weights(x0, g, wx);
  const T* s = src + (plane * g.src_h + g.src_y + r) * g.src_w + g.src_x;
  if (x0 >= 0 && x0 + 4 <= g.win_w) {
    load4(s + x0, y);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = (x0 + k >= 0 && x0 + k < g.win_w) ? (float)s[x0 + k] : 0.f;
  }
  blend_store(acc + d0, x0, g.win_w, y, wx, ramp_weight(r, g.win_h, g.ramp_top, g.ramp_bottom), r < g.ramp_top, g.ramp_left);
}

// 8-bit image source [N][src_h][src_w][C]: a thread takes the 4*C bytes of its 4 pixels (whole words where they are word aligned) and writes
// one accumulator vector per channel.  CT = compile-time C (1, 3, 4) or 0 for any other channel count.  code / 255 comes from a table of
// the 256 true quotients, one division per thread.
// grid: x = 4-pixel segments of a row / 256, y = window row, z = batch
template <int CT>
__global__ __launch_bounds__(kBlendThreads) void tile_blend_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ acc, BlendGeom g) {
  __shared__ float s_code[256];
  s_code[threadIdx.x] = (float)threadIdx.x / 255.f;
  __syncthreads();
  const int C = CT ? CT : g.C;
  const int r = blockIdx.y;
  const int64_t n = blockIdx.z;
  // every channel plane of acc has the same row alignment iff acc_h * acc_w is a multiple of 4; otherwise the segments follow channel 0
  // and the planes take the element-wise path below
  const int64_t plane_stride = (int64_t)g.acc_h * g.acc_w;
  const int64_t d0 = (n * C * g.acc_h + g.acc_y + r) * g.acc_w + g.acc_x;
  const int x0 = (blockIdx.x * kBlendThreads + threadIdx.x) * 4 - (int)(d0 & 3);
  if (x0 >= g.win_w) return;
  float wx[4];
  column_weights(x0, g, wx);
  const float wy = ramp_weight(r, g.win_h, g.ramp_top, g.ramp_bottom);
  const bool add = r < g.ramp_top;
  const uint8_t* s = src + ((n * g.src_h + g.src_y + r) * g.src_w + g.src_x) * C;
  const bool full = x0 >= 0 && x0 + 4 <= g.win_w;
  if (CT != 0 && full && (((uintptr_t)(s + (int64_t)x0 * C)) & 3) == 0 && (plane_stride & 3) == 0) {
    uint32_t words[CT ? CT : 1];
#pragma unroll
    for (int j = 0; j < CT; ++j) words[j] = ((const uint32_t*)(s + (int64_t)x0 * C))[j];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      float y[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = k * CT + c;
        y[k] = s_code[(words[b >> 2] >> (8 * (b & 3))) & 255u];
      }
      blend_store(acc + d0 + c * plane_stride, x0, g.win_w, y, wx, wy, add, g.ramp_left);
    }
  } else {
    for (int c = 0; c < C; ++c) {
      float* dst = acc + d0 + c * plane_stride;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        if (x < 0 || x >= g.win_w) continue;
        const float w = wy * wx[k];
        const float yv = s_code[s[(int64_t)x * C + c]];
        dst[x] = (add || x < g.ramp_left) ? fmaf(w, yv, dst[x]) : w * yv;
      }
    }
  }
}

}  // namespace
}  // namespace rsa

extern "C" int rsa_tile_blend_accumulate(const void* src, int32_t src_dtype, int32_t batch, int32_t C, int32_t win_h, int32_t win_w, int32_t src_h,
                                         int32_t src_w, int32_t src_y, int32_t src_x, float* acc, int32_t acc_h, int32_t acc_w, int32_t acc_y,
                                         int32_t acc_x, int32_t ramp_top, int32_t ramp_bottom, int32_t ramp_left, int32_t ramp_right, void* stream) {
  using namespace rsa;
  if (src == nullptr || acc == nullptr) return set_error(RSA_E_ARG, "rsa_tile_blend_accumulate: null src or acc");
  if (src_dtype < RSA_F32 || src_dtype > RSA_U8) return set_error(RSA_E_ARG, "rsa_tile_blend_accumulate: src_dtype must be an rsa_dtype");
  if (batch < 1 || C < 1 || win_h < 1 || win_w < 1 || src_h < 1 || src_w < 1 || acc_h < 1 || acc_w < 1)
    return set_error(RSA_E_ARG, "rsa_tile_blend_accumulate: batch, C and every size must be >= 1");
  if (src_y < 0 || src_x < 0 || (int64_t)src_y + win_h > src_h || (int64_t)src_x + win_w > src_w)
    return set_error(RSA_E_ARG, "rsa_tile_blend_accumulate: the window leaves the source");
  if (acc_y < 0 || acc_x < 0 || (int64_t)acc_y + win_h > acc_h || (int64_t)acc_x + win_w > acc_w)
    return set_error(RSA_E_ARG, "rsa_tile_blend_accumulate: the window leaves the accumulator");
  if (ramp_top < 0 || ramp_bottom < 0 || ramp_left < 0 || ramp_right < 0)
    return set_error(RSA_E_ARG, "rsa_tile_blend_accumulate: a ramp width is negative");
  if (ramp_top > win_h || ramp_bottom > win_h || ramp_left > win_w || ramp_right > win_w)
    return set_error(RSA_E_ARG, "rsa_tile_blend_accumulate: a ramp is wider than the window");
  const int64_t planes = src_dtype == RSA_U8 ? (int64_t)batch : (int64_t)batch * C;
  if (planes > 65535 || win_h > 65535) return set_error(RSA_E_ARG, "rsa_tile_blend_accumulate: more than 65535 planes or window rows");
  if (misaligned16(acc)) return set_error(RSA_E_ALIGN, "rsa_tile_blend_accumulate: acc must be 16-byte aligned");
  const uintptr_t elem = src_dtype == RSA_F32 ? 4 : src_dtype == RSA_U8 ? 1 : 2;
  if ((uintptr_t)src & (elem - 1)) return set_error(RSA_E_ALIGN, "rsa_tile_blend_accumulate: src is not aligned to its element size");

  const BlendGeom g = {C, win_h, win_w, src_h, src_w, src_y, src_x, acc_h, acc_w, acc_y, acc_x, ramp_top, ramp_bottom, ramp_left, ramp_right};
  const int segs = (win_w + 3) / 4 + 1;  // + 1: a row that starts off a 16 B boundary has a head segment
  const dim3 grid((unsigned)((segs + kBlendThreads - 1) / kBlendThreads), (unsigned)win_h, (unsigned)planes), block(kBlendThreads);
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == RSA_F32)
    hipLaunchKernelGGL(tile_blend_nchw_kernel<float>, grid, block, 0, st, (const float*)src, acc, g);
  else if (src_dtype == RSA_F16)
    hipLaunchKernelGGL(tile_blend_nchw_kernel<_Float16>, grid, block, 0, st, (const _Float16*)src, acc, g);
  else if (src_dtype == RSA_BF16)
    hipLaunchKernelGGL(tile_blend_nchw_kernel<__bf16>, grid, block, 0, st, (const __bf16*)src, acc, g);
  else if (C == 1)
    hipLaunchKernelGGL(tile_blend_u8_kernel<1>, grid, block, 0, st, (const uint8_t*)src, acc, g);
  else if (C == 3)
    hipLaunchKernelGGL(tile_blend_u8_kernel<3>, grid, block, 0, st, (const uint8_t*)src, acc, g);
  else if (C == 4)
    hipLaunchKernelGGL(tile_blend_u8_kernel<4>, grid, block, 0, st, (const uint8_t*)src, acc, g);
  else
    hipLaunchKernelGGL(tile_blend_u8_kernel<0>, grid, block, 0, st, (const uint8_t*)src, acc, g);
  return launch_status("rsa_tile_blend_accumulate: launch failed");
}
