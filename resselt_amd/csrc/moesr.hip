// moesr.hip — the one kernel MoESR (reference resselt/archs/moesr/arch.py) adds to the MoSR / MoSRv2 path:
//   rsa_moesr_stream   the f32 residual stream between the convolutions: block tail (a * gamma + s), the PixelUnshuffle of MSG.down, the
//                      PixelShuffle + residual(s) of MSG.up, each with the next block's LayerNorm (or plain planes) in the same pass
//                      GatedCNNBlock.forward :163-164, MSG :170-177, MoESR.forward :225
// An HBM-bound streaming kernel.  Byte model per output pixel (every operand read once, every output written once), C = dim:
//   reads   4C (a: C f32 values in every mode -- C/4 channels at four source pixels, or four source channels per channel at a quarter
//           of the pixels) + 4C (s_in, modes 0 and 2) + 4C (s2_in, where given); gamma / ln_gamma / ln_beta are 4C bytes per launch
//   writes  4C (s_out, where given) + 2C (hi planes, where given) + 2C (lo planes, where given)
// e.g. the block tail with LayerNorm planes in three products: 4C + 4C + 4C + 2C + 2C = 16C bytes per pixel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd_moesr.h"

namespace rsa {
namespace {

// A lane owns one output pixel and keeps all C channels of it in registers (MAXG groups of 4), so the LayerNorm needs no exchange between
// lanes: no LDS, no barrier, and the four waves of a workgroup are independent.  A wave is a 32 x 2 pixel tile: neighbouring lanes own
// neighbouring pixels, so every load / store of a channel group is 32 consecutive 16-byte units per row, and the 2 x 2 output pixels that
// share a source pixel in mode 2 sit in one wave -- the wave reads each 16-byte unit of `a` once and its four lanes take one component
// each.  In mode 1 a lane reads the 2 x 2 source pixels of its output pixel as four whole units and uses all sixteen values.
constexpr int MS_TW = 32, MS_TH = 8;

__device__ __forceinline__ float pick4(const f32x4 v, int k) { return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3]; }

// grid (tiles, batch), 256 threads
template <int MAXG, int MODE, int FMT>
__global__ __launch_bounds__(256) void moesr_stream_kernel(const rsa_moesr_stream_params p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tiles_x = (p.W + MS_TW - 1) / MS_TW;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int n = blockIdx.y;
  const int y0 = ty * MS_TH + wave * 2;
  if (y0 >= p.H) return;  // wave-uniform
  const int x = tx * MS_TW + (lane & 31), y = y0 + (lane >> 5);
  const bool live = x < p.W && y < p.H;
  const int xc = min(x, p.W - 1), yc = min(y, p.H - 1);  // a lane outside the map reads the nearest pixel inside and stores nothing
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)yc * p.W + xc;
  const int p4 = p.C >> 2;  // C % 8 == 0

  float s[MAXG][4];
  if constexpr (MODE == 0) {
    const f32x4* a = (const f32x4*)p.a + (int64_t)n * p4 * HW + pix;
    const f32x4* si = (const f32x4*)p.s_in + (int64_t)n * p4 * HW + pix;
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
      if (g < p4) {
        const f32x4 av = a[(int64_t)g * HW], sv = si[(int64_t)g * HW];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[g][r] = fmaf(av[r], p.gamma[4 * g + r], sv[r]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[g][r] = 0.f;
      }
    }
  } else if constexpr (MODE == 1) {
    // source channel g = output group g; it is component g % 4 of source group g / 4 at the 2 x 2 source pixels
    const int64_t aW = 2 * (int64_t)p.W, aHW = 4 * HW;
    const int sp4 = (p4 + 3) >> 2;
    const f32x4* a = (const f32x4*)p.a + (int64_t)n * sp4 * aHW + (int64_t)(2 * yc) * aW + 2 * xc;
#pragma unroll
    for (int q = 0; q < MAXG / 4; ++q) {
      f32x4 v00 = {0.f, 0.f, 0.f, 0.f}, v01 = v00, v10 = v00, v11 = v00;
      if (q < sp4) {
        const f32x4* aq = a + (int64_t)q * aHW;
        v00 = aq[0], v01 = aq[1], v10 = aq[aW], v11 = aq[aW + 1];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int g = 4 * q + k;
        const bool in = g < p4;  // (the last source group's tail components are not channels of a)
        s[g][0] = in ? v00[k] : 0.f;
        s[g][1] = in ? v01[k] : 0.f;
        s[g][2] = in ? v10[k] : 0.f;
        s[g][3] = in ? v11[k] : 0.f;
      }
    }
  } else {
    // output channel 4g + r reads source channel 16g + 4r + k = component k of source group 4g + r, k the pixel's place in its 2 x 2 block
    const int64_t aW = p.W >> 1, aHW = HW >> 2;
    const int k = 2 * (yc & 1) + (xc & 1);
    const f32x4* a = (const f32x4*)p.a + (int64_t)n * (4 * p4) * aHW + (int64_t)(yc >> 1) * aW + (xc >> 1);
    const f32x4* si = (const f32x4*)p.s_in + (int64_t)n * p4 * HW + pix;
    const f32x4* s2 = p.s2_in ? (const f32x4*)p.s2_in + (int64_t)n * p4 * HW + pix : nullptr;
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
      if (g < p4) {
        const f32x4 sv = si[(int64_t)g * HW];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[g][r] = pick4(a[(int64_t)(4 * g + r) * aHW], k) + sv[r];
        if (s2 != nullptr) {
          const f32x4 tv = s2[(int64_t)g * HW];
#pragma unroll
          for (int r = 0; r < 4; ++r) s[g][r] += tv[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[g][r] = 0.f;
      }
    }
  }

  if (p.s_out != nullptr && live) {
    f32x4* so = (f32x4*)p.s_out + (int64_t)n * p4 * HW + pix;
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
      if (g < p4) so[(int64_t)g * HW] = (f32x4){s[g][0], s[g][1], s[g][2], s[g][3]};
  }
  if (p.out_hi == nullptr) return;

  const bool ln = p.ln_gamma != nullptr;
  float mean = 0.f, rstd = 1.f;
  if (ln) {  // centred form; channels beyond C are zero in s and left out of both sums
    const float inv_c = 1.f / (float)p.C;
    float sum = 0.f;
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
      if (g < p4) sum += (s[g][0] + s[g][1]) + (s[g][2] + s[g][3]);
    mean = sum * inv_c;
    float var = 0.f;
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
      if (g < p4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = s[g][r] - mean;
          var = fmaf(d, d, var);
        }
      }
    rstd = rsqrtf(var * inv_c + p.eps);
  }
  char* hi = (char*)p.out_hi + ((int64_t)n * p.out_batch_stride + pix) * 16;
  char* lo = p.out_lo ? (char*)p.out_lo + ((int64_t)n * p.out_batch_stride + pix) * 16 : nullptr;
#pragma unroll
  for (int pl = 0; pl < MAXG / 2; ++pl) {
    if (2 * pl < p4) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = s[2 * pl + (j >> 2)][j & 3];
        v[j] = ln ? fmaf((t - mean) * rstd, p.ln_gamma[8 * pl + j], p.ln_beta[8 * pl + j]) : t;
      }
      if (live) store_unit<FMT>(hi, lo, (int64_t)pl * p.out_plane_stride * 16, v);
    }
  }
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_moesr_stream(const rsa_moesr_stream_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "moesr_stream: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->mode < 0 || p->mode > 2 || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "moesr_stream: bad geometry (mode 0, 1 or 2, reserved0 0)");
  if (p->C < 8 || p->C > 128 || (p->C & 7)) return set_error(RSA_E_ARG, "moesr_stream: C must be a multiple of 8 from 8 to 128");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "moesr_stream: bad plane format");
  if (p->mode == 0 && (p->a_H != p->H || p->a_W != p->W)) return set_error(RSA_E_ARG, "moesr_stream: mode 0 reads a at H x W");
  if (p->mode == 1 && ((p->a_H & 1) || (p->a_W & 1) || p->a_H != 2 * p->H || p->a_W != 2 * p->W))
    return set_error(RSA_E_ARG, "moesr_stream: mode 1 reads a at 2H x 2W (an odd source size cannot be unshuffled)");
  if (p->mode == 2 && ((p->H & 1) || (p->W & 1) || 2 * p->a_H != p->H || 2 * p->a_W != p->W))
    return set_error(RSA_E_ARG, "moesr_stream: mode 2 reads a at H/2 x W/2 (an odd stream size is no shuffled map)");
  if (!p->a || (p->mode == 0 && !p->gamma) || (p->mode != 1 && !p->s_in)) return set_error(RSA_E_ARG, "moesr_stream: null operand");
  if (!p->s_out && !p->out_hi) return set_error(RSA_E_ARG, "moesr_stream: no output (s_out and out_hi are both NULL)");
  if (p->out_lo && !p->out_hi) return set_error(RSA_E_ARG, "moesr_stream: out_lo without out_hi");
  if (p->out_hi && p->ln_gamma && (!p->ln_beta || !(p->eps > 0.f))) return set_error(RSA_E_ARG, "moesr_stream: the LayerNorm needs ln_beta and eps > 0");
  if (misaligned16(p->a) || misaligned16(p->gamma) || misaligned16(p->s_in) || misaligned16(p->s2_in) || misaligned16(p->s_out) ||
      misaligned16(p->ln_gamma) || misaligned16(p->ln_beta) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "moesr_stream: maps, planes and channel vectors must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->out_hi && p->out_plane_stride < HW) return set_error(RSA_E_ARG, "moesr_stream: the plane stride is smaller than the map");
  const int64_t tiles = (int64_t)((p->W + MS_TW - 1) / MS_TW) * ((p->H + MS_TH - 1) / MS_TH);
  if (tiles > 0x7fffffff) return set_error(RSA_E_ARG, "moesr_stream: map too large");
  const dim3 grid((unsigned)tiles, (unsigned)p->batch);
  const hipStream_t s = (hipStream_t)stream;
  const int mode = p->mode, C = p->C;
  with_fmt(p->fmt, [&](auto F) {
    constexpr int FMT = decltype(F)::value;
#define MS_GO(MAXG, MODE) hipLaunchKernelGGL((moesr_stream_kernel<MAXG, MODE, FMT>), grid, dim3(256), 0, s, *p)
#define MS_MODE(MAXG) \
  if (mode == 0)      \
    MS_GO(MAXG, 0);   \
  else if (mode == 1) \
    MS_GO(MAXG, 1);   \
  else                \
    MS_GO(MAXG, 2);
    if (C <= 32) {
      MS_MODE(8)
    } else if (C <= 64) {
      MS_MODE(16)
    } else {
      MS_MODE(32)
    }
#undef MS_MODE
#undef MS_GO
  });
  return launch_status("moesr_stream: launch failed");
}
