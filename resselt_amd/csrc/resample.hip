// resample.hip — any output size for upscale(): separable antialiased resampling of the native frame (resselt_amd/tiling.py).
//
// upscale(..., out_size / out_scale) delivers the model's H*scale x W*scale frame at another size.  Each axis is a table made on the host
// in f64 (tiling.resample_table: torch's antialiased bicubic / bilinear weights): output position i reads the `taps` source positions
// start[i] .. start[i] + taps - 1 with the weights weight[i][0 .. taps - 1]; rows shorter than `taps` are padded with zero weights, and
// start[i] + taps <= n_in holds for every row.
//
// One launch, no full-frame intermediate in HBM.  A workgroup owns a 16 x 64 tile of output pixels of one (n, c) plane:
//   1. the horizontal filter runs from global memory into an f32 BAND in LDS: the source rows start_y[first row] .. start_y[last row] + taps_y - 1
//      that the tile's output rows need, already reduced to the tile's 64 output columns;
//   2. the vertical filter runs out of the band, and the result is stored in the destination format.
// Every sum is an fmaf chain in ascending tap order from zero, so results are identical from run to run.  A padded tap multiplies its source
// pixel by zero: a non-finite source pixel therefore spreads over up to `taps` outputs per axis, also where its true weight is zero.  The
// engine's finite check (rsa_check_finite) runs on the model's side before this kernel, so that is accepted.
//
// Byte model: the source once, the destination once.  What the launch adds to it: neighbouring tiles in y re-read the vertical halo of their
// bands, about (16 r + taps_y) / (16 r) of the source for a ratio r = src_h / dst_h (from L2 where the neighbour ran recently); the taps of a
// row overlap within a workgroup and are served by the vector cache.  Measurements: profiles/resample_measure.txt.
//
// No header under include/ declares this entry point (a helper of the engine's tiler, registered in engine/lib.py INTERNAL):
//
//   int rsa_resample(const void* src, int32_t src_dtype, int32_t batch, int32_t C, int32_t src_h, int32_t src_w,
//                    void* dst, int32_t dst_dtype, int32_t dst_h, int32_t dst_w,
//                    const int32_t* start_y, const float* weight_y, int32_t taps_y,
//                    const int32_t* start_x, const float* weight_x, int32_t taps_x, void* stream);
//
//   src       dense [batch][C][src_h][src_w] of RSA_F32 / RSA_F16 / RSA_BF16, or for RSA_U8 an 8-bit image [batch][src_h][src_w][C] whose codes
//             enter as code / 255.
//   dst       dense [batch][C][dst_h][dst_w] of RSA_F32 / RSA_F16 / RSA_BF16 (one rounding to the format), or for RSA_U8 an 8-bit image
//             [batch][dst_h][dst_w][C] = round-half-even(clamp(v, 0, 1) * 255), the rule of rsa_nchw_to_image_u8 (NaN -> 0).
//   start_y   [dst_h] int32, weight_y [dst_h][taps_y] f32: the table of the rows; start_x [dst_w], weight_x [dst_w][taps_x]: of the columns.
//             Device pointers.  The kernel clamps every source index to the source (and every band index to the band), so a wrong table gives
//             wrong pixels but never reads outside src.
//
// RSA_E_ARG before any launch for a null pointer, batch, C, a size or taps < 1, taps above 33 (kResampleMaxTaps: bicubic at the ratio limit
// of 8), a dtype that is no rsa_dtype, more than 65535 planes or tile rows, or a band that does not fit the 64 KB of LDS of a workgroup
// (ratios far above 8); RSA_E_ALIGN for a src / dst that is not aligned to its element size or a table that is not 4-byte aligned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"

namespace rsa {
namespace {

// Output tile of a workgroup: 64 columns = one wave per output row, so the band and the destination rows are read and written with
// consecutive lanes on consecutive elements (no LDS bank conflicts: lane stride one dword), and the vertical weights are wave-uniform.
// 16 rows: at the ratio limit the band is 15 * 8 + 1 + 33 = 154 source rows x 64 columns x 4 B = 38.5 KB, and with the two weight tables
// (8.25 KB + 2.1 KB) the workgroup stays under 64 KB; at ratio 2 it is 10 KB and the halo re-read is (32 + 9) / 32 of the source.
constexpr int kResampleTileH = 16;
constexpr int kResampleTileW = 64;
constexpr int kResampleThreads = 256;
constexpr int kResampleRowsPerPass = kResampleThreads / kResampleTileW;
constexpr int kResampleMaxTaps = 33;
constexpr int64_t kResampleMaxLds = 64 * 1024;

struct ResampleGeom {
  int C, src_h, src_w, dst_h, dst_w, taps_y, taps_x;
  int band_cap;  // rows of the LDS band
};

template <typename S>
__device__ __forceinline__ float src_value(S v, const float* s_code) {
  if constexpr (std::is_same<S, uint8_t>::value)
    return s_code[v];
  else
    return (float)v;
}

template <typename D>
__device__ __forceinline__ D dst_value(float v) {
  if constexpr (std::is_same<D, uint8_t>::value) {
    v = fminf(fmaxf(v, 0.f), 1.f);  // NaN -> 0, as in rsa_nchw_to_image_u8
    return (uint8_t)rintf(v * 255.f);
  } else {
    return (D)v;
  }
}

// grid: x = tiles of 64 output columns, y = tiles of 16 output rows, z = batch * C; dynamic LDS: band, both weight tiles, both start tiles
template <typename S, typename D>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const S* __restrict__ src, D* __restrict__ dst, const int32_t* __restrict__ start_y,
                                                                    const float* __restrict__ weight_y, const int32_t* __restrict__ start_x,
                                                                    const float* __restrict__ weight_x, ResampleGeom g) {
  extern __shared__ float s_mem[];
  float* s_band = s_mem;                                              // [band_cap][64]
  float* s_wx = s_band + (size_t)g.band_cap * kResampleTileW;         // [taps_x][64]: tap-major, so a wave reads consecutive dwords
  float* s_wy = s_wx + (size_t)g.taps_x * kResampleTileW;             // [16][taps_y]
  int* s_sx = (int*)(s_wy + (size_t)kResampleTileH * g.taps_y);       // [64]
  int* s_sy = s_sx + kResampleTileW;                                  // [16]
  __shared__ float s_code[std::is_same<S, uint8_t>::value ? 256 : 1]; // the 256 true quotients code / 255

  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * kResampleTileW, oy0 = blockIdx.y * kResampleTileH;
  const int n = blockIdx.z / g.C, c = blockIdx.z - n * g.C;
  if constexpr (std::is_same<S, uint8_t>::value) s_code[tid] = (float)tid / 255.f;

  // the tile's slices of the tables; columns / rows past the image repeat the last one (computed, never stored)
  for (int i = tid; i < kResampleTileW * g.taps_x; i += kResampleThreads) {
    const int x = i / g.taps_x, t = i - x * g.taps_x;
    s_wx[t * kResampleTileW + x] = weight_x[(int64_t)min(ox0 + x, g.dst_w - 1) * g.taps_x + t];
  }
  for (int i = tid; i < kResampleTileH * g.taps_y; i += kResampleThreads) {
    const int y = i / g.taps_y, t = i - y * g.taps_y;
    s_wy[i] = weight_y[(int64_t)min(oy0 + y, g.dst_h - 1) * g.taps_y + t];
  }
  if (tid < kResampleTileW) s_sx[tid] = min(max(start_x[min(ox0 + tid, g.dst_w - 1)], 0), g.src_w - 1);
  if (tid >= kResampleTileW && tid < kResampleTileW + kResampleTileH)
    s_sy[tid - kResampleTileW] = min(max(start_y[min(oy0 + tid - kResampleTileW, g.dst_h - 1)], 0), g.src_h - 1);
  __syncthreads();

  const int y_last = min(kResampleTileH, g.dst_h - oy0) - 1;  // last output row of the tile that exists
  const int band0 = s_sy[0];
  const int rows = min(max(s_sy[y_last] + g.taps_y - band0, 1), g.band_cap);
  const int x = tid & (kResampleTileW - 1);

  // 1. horizontal: source rows band0 .. band0 + rows - 1 -> the band, one wave per row
  // A thread walks two band rows at once, four taps at a time: the eight loads of a step are issued before the first fmaf needs one, and
  // each row's chain still adds its taps in ascending order.  (Between device events, x2 / x3 of the f16 frame of
  // profiles/resample_measure.txt: one row and one tap at a time 272 / 452 us; this 288 / 349 us; four rows and eight taps at a time
  // 316 / 369 us.  More loads in flight do not help further: the time follows the number of load instructions, one per tap and wave.)
  const int sx0 = s_sx[x];
  constexpr bool kImage = std::is_same<S, uint8_t>::value;
  const int64_t xstride = kImage ? g.C : 1;
  for (int r = tid / kResampleTileW; r < rows; r += 2 * kResampleRowsPerPass) {
    const int r1 = min(r + kResampleRowsPerPass, rows - 1);  // the last pass may have no second row: it repeats a row and stores nothing
    const int sya = min(band0 + r, g.src_h - 1), syb = min(band0 + r1, g.src_h - 1);
    const S* rowa = kImage ? src + (((int64_t)n * g.src_h + sya) * g.src_w) * g.C + c : src + (((int64_t)n * g.C + c) * g.src_h + sya) * g.src_w;
    const S* rowb = kImage ? src + (((int64_t)n * g.src_h + syb) * g.src_w) * g.C + c : src + (((int64_t)n * g.C + c) * g.src_h + syb) * g.src_w;
    float acca = 0.f, accb = 0.f;
    int t = 0;
    for (; t + 4 <= g.taps_x; t += 4) {
      S va[4], vb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t o = (int64_t)min(sx0 + t + k, g.src_w - 1) * xstride;
        va[k] = rowa[o], vb[k] = rowb[o];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float w = s_wx[(t + k) * kResampleTileW + x];
        acca = fmaf(w, src_value<S>(va[k], s_code), acca);
        accb = fmaf(w, src_value<S>(vb[k], s_code), accb);
      }
    }
    for (; t < g.taps_x; ++t) {
      const int64_t o = (int64_t)min(sx0 + t, g.src_w - 1) * xstride;
      const float w = s_wx[t * kResampleTileW + x];
      acca = fmaf(w, src_value<S>(rowa[o], s_code), acca);
      accb = fmaf(w, src_value<S>(rowb[o], s_code), accb);
    }
    s_band[r * kResampleTileW + x] = acca;
    if (r + kResampleRowsPerPass < rows) s_band[r1 * kResampleTileW + x] = accb;
  }
  __syncthreads();

  // 2. vertical: the band -> the tile, one wave per output row
  const int ox = ox0 + x;
  for (int y = tid / kResampleTileW; y <= y_last; y += kResampleRowsPerPass) {
    const int b0 = s_sy[y] - band0;
    const float* wy = s_wy + y * g.taps_y;
    float acc = 0.f;
#pragma unroll 4
    for (int t = 0; t < g.taps_y; ++t) acc = fmaf(wy[t], s_band[min(max(b0 + t, 0), rows - 1) * kResampleTileW + x], acc);
    if (ox < g.dst_w) {
      const int oy = oy0 + y;
      if constexpr (std::is_same<D, uint8_t>::value)
        dst[(((int64_t)n * g.dst_h + oy) * g.dst_w + ox) * g.C + c] = dst_value<D>(acc);
      else
        dst[(((int64_t)n * g.C + c) * g.dst_h + oy) * g.dst_w + ox] = dst_value<D>(acc);
    }
  }
}

template <typename S>
void launch_resample(int dst_dtype, dim3 grid, size_t lds, hipStream_t st, const void* src, void* dst, const int32_t* start_y, const float* weight_y,
                     const int32_t* start_x, const float* weight_x, const ResampleGeom& g) {
  const dim3 block(kResampleThreads);
  if (dst_dtype == RSA_F32)
    hipLaunchKernelGGL((resample_kernel<S, float>), grid, block, lds, st, (const S*)src, (float*)dst, start_y, weight_y, start_x, weight_x, g);
  else if (dst_dtype == RSA_F16)
    hipLaunchKernelGGL((resample_kernel<S, _Float16>), grid, block, lds, st, (const S*)src, (_Float16*)dst, start_y, weight_y, start_x, weight_x, g);
  else if (dst_dtype == RSA_BF16)
    hipLaunchKernelGGL((resample_kernel<S, __bf16>), grid, block, lds, st, (const S*)src, (__bf16*)dst, start_y, weight_y, start_x, weight_x, g);
  else
    hipLaunchKernelGGL((resample_kernel<S, uint8_t>), grid, block, lds, st, (const S*)src, (uint8_t*)dst, start_y, weight_y, start_x, weight_x, g);
}

inline uintptr_t elem_bytes(int dtype) { return dtype == RSA_F32 ? 4 : dtype == RSA_U8 ? 1 : 2; }

}  // namespace
}  // namespace rsa

extern "C" int rsa_resample(const void* src, int32_t src_dtype, int32_t batch, int32_t C, int32_t src_h, int32_t src_w, void* dst, int32_t dst_dtype,
                            int32_t dst_h, int32_t dst_w, const int32_t* start_y, const float* weight_y, int32_t taps_y, const int32_t* start_x,
                            const float* weight_x, int32_t taps_x, void* stream) {
  using namespace rsa;
  if (src == nullptr || dst == nullptr) return set_error(RSA_E_ARG, "rsa_resample: null src or dst");
  if (start_y == nullptr || weight_y == nullptr || start_x == nullptr || weight_x == nullptr) return set_error(RSA_E_ARG, "rsa_resample: null table");
  if (src_dtype < RSA_F32 || src_dtype > RSA_U8 || dst_dtype < RSA_F32 || dst_dtype > RSA_U8)
    return set_error(RSA_E_ARG, "rsa_resample: src_dtype and dst_dtype must be an rsa_dtype");
  if (batch < 1 || C < 1 || src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1) return set_error(RSA_E_ARG, "rsa_resample: batch, C and every size must be >= 1");
  if (taps_y < 1 || taps_x < 1 || taps_y > kResampleMaxTaps || taps_x > kResampleMaxTaps)
    return set_error(RSA_E_ARG, "rsa_resample: taps must be 1 .. 33");
  const int64_t planes = (int64_t)batch * C;
  const int64_t tiles_y = ((int64_t)dst_h + kResampleTileH - 1) / kResampleTileH, tiles_x = ((int64_t)dst_w + kResampleTileW - 1) / kResampleTileW;
  if (planes > 65535 || tiles_y > 65535) return set_error(RSA_E_ARG, "rsa_resample: more than 65535 planes or tile rows");
  // rows of a tile's band: the starts of its first and last output row are at most ceil(15 * src_h / dst_h) + 1 apart (torch's rule)
  const int64_t span = ((int64_t)(kResampleTileH - 1) * src_h + dst_h - 1) / dst_h + 1 + taps_y;
  const int64_t band_cap = span < src_h ? span : src_h;
  const int64_t lds = 4 * (band_cap * kResampleTileW + (int64_t)taps_x * kResampleTileW + (int64_t)kResampleTileH * taps_y + kResampleTileW + kResampleTileH);
  if (lds + 1024 > kResampleMaxLds) return set_error(RSA_E_ARG, "rsa_resample: the band of a tile does not fit the LDS (src_h / dst_h far above 8)");
  if (((uintptr_t)src & (elem_bytes(src_dtype) - 1)) || ((uintptr_t)dst & (elem_bytes(dst_dtype) - 1)))
    return set_error(RSA_E_ALIGN, "rsa_resample: src or dst is not aligned to its element size");
  if (((uintptr_t)start_y | (uintptr_t)weight_y | (uintptr_t)start_x | (uintptr_t)weight_x) & 3)
    return set_error(RSA_E_ALIGN, "rsa_resample: a table is not 4-byte aligned");

  const ResampleGeom g = {C, src_h, src_w, dst_h, dst_w, taps_y, taps_x, (int)band_cap};
  const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)planes);
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == RSA_F32)
    launch_resample<float>(dst_dtype, grid, (size_t)lds, st, src, dst, start_y, weight_y, start_x, weight_x, g);
  else if (src_dtype == RSA_F16)
    launch_resample<_Float16>(dst_dtype, grid, (size_t)lds, st, src, dst, start_y, weight_y, start_x, weight_x, g);
  else if (src_dtype == RSA_BF16)
    launch_resample<__bf16>(dst_dtype, grid, (size_t)lds, st, src, dst, start_y, weight_y, start_x, weight_x, g);
  else
    launch_resample<uint8_t>(dst_dtype, grid, (size_t)lds, st, src, dst, start_y, weight_y, start_x, weight_x, g);
  return launch_status("rsa_resample: launch failed");
}
