// gfisr1.hip — what GFISR (v1) adds to the kernels of the GFISR family (reference resselt/archs/gfisr/arch.py:385-471):
//   rsa_gfisr_ln_spectral   FourierUnit's spectral stage in one launch, all f32: ln (channel LayerNorm) + fpe (depthwise 3x3 + bias) with its
//                           residual + fdc (1x1, C -> C) + GELU, f32 map -> f32 map                                  FourierUnit.forward :459-465
//   rsa_plane_window        the reflect pad in front of the transform and the crop behind it, on split planes       pad_to_even / unpad :385-413
// The transforms between them are rsa_gfisr_dft (csrc/gfisr.hip), unchanged.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd_gfisr1.h"

namespace rsa {
namespace {

// ---------------------------------------------------------------------------------------------------------------- ln + fpe + fdc + GELU
constexpr int LS_TW = 32, LS_TH = 8, LS_HW = LS_TW + 2, LS_HH = LS_TH + 2, LS_NPIX = LS_HW * LS_HH;

// grid (tiles, batch), 256 threads: a 32 x 8 tile of the spectral grid, CG = ceil(C / 4) channel groups (CP = 4 CG channel slots, the slots
// past C hold zeros and are never loaded from the map).  The weights go to LDS first (fdc zero-padded to CP x CP: the fma chain of an output
// then ends in exact + 0 * 0 terms).  Phase 1: the LayerNorm values v of the tile's 34 x 10 halo pixels into LDS as [channel][pixel], ZERO
// outside the grid (the depthwise convolution pads the normalised map with zeros, ln_b included).  Phase 2: a lane owns a pixel: the
// depthwise sums of all channels in registers, then the C x C product row by row (the weight reads are wave-uniform LDS broadcasts).
template <int CG>
__global__ __launch_bounds__(256) void gfisr_ln_spectral_kernel(const rsa_gfisr_ln_spectral_params p) {
  constexpr int CP = 4 * CG;
  __shared__ float vs[CP * LS_NPIX];
  __shared__ float wf[CP * CP];
  __shared__ float wd[CP * 9];
  __shared__ float lw[CP], lb[CP], fb[CP], db[CP];
  const int tid = threadIdx.x;
  const int C = p.C;
  for (int i = tid; i < CP * CP; i += 256) {
    const int o = i / CP, c = i - o * CP;
    wf[i] = (o < C && c < C) ? p.fdc_w[o * C + c] : 0.f;
  }
  for (int i = tid; i < CP * 9; i += 256) wd[i] = i < C * 9 ? p.fpe_w[i] : 0.f;
  if (tid < CP) {
    const bool in = tid < C;
    lw[tid] = in ? p.ln_w[tid] : 0.f, lb[tid] = in ? p.ln_b[tid] : 0.f, fb[tid] = in ? p.fpe_b[tid] : 0.f, db[tid] = in ? p.fdc_b[tid] : 0.f;
  }
  __syncthreads();
  const int tiles_x = (p.W + LS_TW - 1) / LS_TW;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int n = blockIdx.y;
  const int x0 = tx * LS_TW, y0 = ty * LS_TH;
  const int64_t HW = (int64_t)p.H * p.W;
  const f32x4* xm = (const f32x4*)p.x + (int64_t)n * CG * HW;
  const float rc = 1.f / (float)C;
  for (int idx = tid; idx < LS_NPIX; idx += 256) {
    const int hy = idx / LS_HW, hx = idx - hy * LS_HW;
    const int gy = y0 + hy - 1, gx = x0 + hx - 1;
    if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
      float xr[CP];
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < CG; ++g) {
        const f32x4 v = xm[(int64_t)g * HW + (int64_t)gy * p.W + gx];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          xr[4 * g + c] = 4 * g + c < C ? v[c] : 0.f;  // (a select, not a product: a NaN in an unused component stays out)
          s += xr[4 * g + c];
        }
      }
      const float mean = s * rc;
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        xr[c] -= mean;
        if (c < C) q = fmaf(xr[c], xr[c], q);
      }
      const float rstd = 1.f / sqrtf(q * rc + p.eps);
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) vs[c * LS_NPIX + idx] = fmaf(xr[c] * rstd, lw[c], lb[c]);
    } else {
#pragma unroll
      for (int c = 0; c < CP; ++c) vs[c * LS_NPIX + idx] = 0.f;
    }
  }
  __syncthreads();
  const int lx = tid & (LS_TW - 1), ly = tid / LS_TW;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= p.W || y >= p.H) return;
  float u[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    u[c] = 0.f;
    if (c < C) {
      const float* vc = vs + c * LS_NPIX + ly * LS_HW + lx;
      float acc = 0.f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) acc = fmaf(wd[c * 9 + dy * 3 + dx], vc[dy * LS_HW + dx], acc);
      u[c] = acc + fb[c] + vc[LS_HW + 1];
    }
  }
  float* om = p.out + (((int64_t)n * CG * HW) + (int64_t)y * p.W + x) * 4;
#pragma unroll
  for (int g = 0; g < CG; ++g) {
    f32x4 z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = 4 * g + k;
      float a = db[o];
#pragma unroll
      for (int c = 0; c < CP; ++c) a = fmaf(wf[o * CP + c], u[c], a);
      z[k] = gelu_erf(a);
    }
    float* dst = om + (int64_t)g * HW * 4;
    if (4 * g + 3 < C) {
      *(f32x4*)dst = z;
    } else {  // the last group of a C that is no multiple of 4: the components past C are not written
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * g + k < C) dst[k] = z[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- reflect window
__device__ __forceinline__ int reflect_once(int t, int S) { return t < 0 ? -t : (t >= S ? 2 * (S - 1) - t : t); }

// grid (ceil(out_H out_W / 256), planes, batch), 256 threads: a lane copies one 16-byte unit of hi (and of lo)
__global__ __launch_bounds__(256) void plane_window_kernel(const rsa_plane_window_params p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.out_H * p.out_W) return;
  const int y = (int)(i / p.out_W), x = (int)(i - (int64_t)y * p.out_W);
  const int sy = reflect_once(y - p.top, p.H), sx = reflect_once(x - p.left, p.W);
  const int64_t src = (int64_t)blockIdx.z * p.in_batch_stride + (int64_t)blockIdx.y * p.in_plane_stride + (int64_t)sy * p.W + sx;
  const int64_t dst = (int64_t)blockIdx.z * p.out_batch_stride + (int64_t)blockIdx.y * p.out_plane_stride + i;
  ((uint4*)p.out_hi)[dst] = ((const uint4*)p.in_hi)[src];
  if (p.out_lo) ((uint4*)p.out_lo)[dst] = ((const uint4*)p.in_lo)[src];
}

// every index of [0, out) - first lands in [0, S) after at most one reflection
bool window_ok(int S, int out, int first) { return first <= S - 1 && (int64_t)out - 1 - first <= 2 * ((int64_t)S - 1); }

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_gfisr_ln_spectral(const rsa_gfisr_ln_spectral_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gfisr_ln_spectral: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->C < 1 || p->reserved0 != 0 || !(p->eps > 0.f))
    return set_error(RSA_E_ARG, "gfisr_ln_spectral: bad geometry (eps > 0, reserved0 0)");
  if (p->C < 2 || p->C > 32 || (p->C & 1)) return set_error(RSA_E_UNSUPPORTED, "gfisr_ln_spectral: C must be even and in 2..32");
  if (!p->x || !p->ln_w || !p->ln_b || !p->fpe_w || !p->fpe_b || !p->fdc_w || !p->fdc_b || !p->out)
    return set_error(RSA_E_ARG, "gfisr_ln_spectral: null pointer");
  if (misaligned16(p->x) || misaligned16(p->ln_w) || misaligned16(p->ln_b) || misaligned16(p->fpe_w) || misaligned16(p->fpe_b) ||
      misaligned16(p->fdc_w) || misaligned16(p->fdc_b) || misaligned16(p->out))
    return set_error(RSA_E_ALIGN, "gfisr_ln_spectral: the maps and the weights must be 16-byte aligned");
  if (p->x == p->out) return set_error(RSA_E_ARG, "gfisr_ln_spectral: x and out must not overlap");
  const int64_t tiles = (int64_t)((p->W + LS_TW - 1) / LS_TW) * ((p->H + LS_TH - 1) / LS_TH);
  if (tiles > 0x7fffffff) return set_error(RSA_E_ARG, "gfisr_ln_spectral: map too large");
  const dim3 grid((unsigned)tiles, (unsigned)p->batch), block(256);
  const hipStream_t s = (hipStream_t)stream;
  switch ((p->C + 3) / 4) {
    case 1: hipLaunchKernelGGL(gfisr_ln_spectral_kernel<1>, grid, block, 0, s, *p); break;
    case 2: hipLaunchKernelGGL(gfisr_ln_spectral_kernel<2>, grid, block, 0, s, *p); break;
    case 3: hipLaunchKernelGGL(gfisr_ln_spectral_kernel<3>, grid, block, 0, s, *p); break;
    case 4: hipLaunchKernelGGL(gfisr_ln_spectral_kernel<4>, grid, block, 0, s, *p); break;
    case 5: hipLaunchKernelGGL(gfisr_ln_spectral_kernel<5>, grid, block, 0, s, *p); break;
    case 6: hipLaunchKernelGGL(gfisr_ln_spectral_kernel<6>, grid, block, 0, s, *p); break;
    case 7: hipLaunchKernelGGL(gfisr_ln_spectral_kernel<7>, grid, block, 0, s, *p); break;
    default: hipLaunchKernelGGL(gfisr_ln_spectral_kernel<8>, grid, block, 0, s, *p); break;
  }
  return launch_status("gfisr_ln_spectral: launch failed");
}

extern "C" int rsa_plane_window(const rsa_plane_window_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "plane_window: null params");
  if (p->batch < 1 || p->batch > 65535 || p->planes < 1 || p->planes > 65535 || p->H < 1 || p->W < 1 || p->out_H < 1 || p->out_W < 1)
    return set_error(RSA_E_ARG, "plane_window: bad geometry");
  if (!p->in_hi || !p->out_hi) return set_error(RSA_E_ARG, "plane_window: null pointer");
  if ((p->in_lo == nullptr) != (p->out_lo == nullptr)) return set_error(RSA_E_ARG, "plane_window: in_lo and out_lo go together");
  if (misaligned16(p->in_hi) || misaligned16(p->in_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "plane_window: the planes must be 16-byte aligned");
  if (p->in_plane_stride < (int64_t)p->H * p->W || p->out_plane_stride < (int64_t)p->out_H * p->out_W)
    return set_error(RSA_E_ARG, "plane_window: a plane stride is smaller than its map");
  if (!window_ok(p->H, p->out_H, p->top) || !window_ok(p->W, p->out_W, p->left))
    return set_error(RSA_E_ARG, "plane_window: an index would need a second reflection (a pad >= the side)");
  const int64_t blocks = ((int64_t)p->out_H * p->out_W + 255) / 256;
  if (blocks > 0x7fffffff) return set_error(RSA_E_ARG, "plane_window: map too large");
  hipLaunchKernelGGL(plane_window_kernel, dim3((unsigned)blocks, (unsigned)p->planes, (unsigned)p->batch), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("plane_window: launch failed");
}
