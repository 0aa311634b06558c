// mosr.hip — the non-convolution kernels of the MoSR / MoSRv2 path (reference resselt/archs/mosr/arch.py, resselt/archs/mosrv2/arch.py):
//   rsa_gated_dwconv   mish(g) * cat(i, segments(c)) on split planes: identity, k x k, 1 x k and k x 1 depthwise    GatedCNNBlock.forward
//   rsa_gfisr_gate     the same kernel with the gate activation as a template argument: silu(g) for GFISRv2 (resselt_amd_gfisr.h)
//   rsa_bilinear_add   out += bilinear x scale of the reflect-padded input (the image shortcut of MoSRv2)              MoSRv2.forward :328-337
// Both are HBM-bound streaming kernels; the fc1 / fc2 convolutions around the first are single launches of the fused convolution.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"
#include "resselt_amd_gfisr.h"

namespace rsa {
namespace {

// A workgroup is a TW x TH pixel tile of one output plane (a 2-D tile, not a row: dat.hip dwconv_kernel, round 4 -- the rows a row-shaped
// workgroup reads were fetched by neighbouring workgroups on other XCDs).  A convolution plane stages its (TH + kh - 1) x (TW + kw - 1) halo
// once in LDS as f32 (hi + lo summed, zero outside the map) in two 4-channel halves, so a tap is two conflict-free 16-byte LDS reads.
constexpr int TW = 32, TH = 8;
constexpr int MAX_K = 11;
constexpr int HALO_UNITS = (TH + MAX_K - 1) * (TW + MAX_K - 1);

struct Operands {
  const bf16x8* g_hi;
  const bf16x8* g_lo;
  const bf16x8* x_hi;
  const bf16x8* x_lo;
  bf16x8* o_hi;
  bf16x8* o_lo;
};

// the gate activation: Mish (MoSR, MoSRv2, MoESR) or SiLU (GFISRv2: x / (1 + exp(-x)), as torch computes it)
template <int ACT>
__device__ __forceinline__ float gate_act(float v) {
  if constexpr (ACT == RSA_ACT_SILU)
    return v / (1.f + expf(-v));
  else
    return mish_exact(v);
}

template <int ACT>
__device__ __forceinline__ void finish(const Operands& o, int64_t pix, const float (&m)[8], int fmt) {
  float g[8], r[8];
  get_unit(o.g_hi, o.g_lo, pix, g, fmt);
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = gate_act<ACT>(g[j]) * m[j];
  put_unit(o.o_hi, o.o_lo, pix, r, fmt);
}

template <int ACT, int KH, int KW>
__device__ __forceinline__ void conv_tile(const Operands& o, const float* __restrict__ w, const float* __restrict__ b, int H, int W, int x0, int y0,
                                          int fmt, f32x4* lds0, f32x4* lds1) {
  constexpr int RH = KH / 2, RW = KW / 2, HH = TH + KH - 1, HWP = TW + KW - 1, KK = KH * KW;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < HH * HWP; idx += 256) {
    const int hy = idx / HWP, hx = idx - hy * HWP;
    const int gy = y0 + hy - RH, gx = x0 + hx - RW;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) get_unit(o.x_hi, o.x_lo, (int64_t)gy * W + gx, v, fmt);
    lds0[idx] = (f32x4){v[0], v[1], v[2], v[3]};
    lds1[idx] = (f32x4){v[4], v[5], v[6], v[7]};
  }
  __syncthreads();
  const int tx = tid & (TW - 1), ty = tid / TW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = b[j];
#pragma unroll 1
  for (int dy = 0; dy < KH; ++dy) {  // (one row of taps at a time: a fully unrolled 11 x 11 keeps 968 weights live)
#pragma unroll
    for (int dx = 0; dx < KW; ++dx) {
      const int q = (ty + dy) * HWP + tx + dx;
      const f32x4 a = lds0[q], c = lds1[q];
      const int t = dy * KW + dx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j] += w[j * KK + t] * a[j];
        acc[j + 4] += w[(j + 4) * KK + t] * c[j];
      }
    }
  }
  finish<ACT>(o, (int64_t)y * W + x, acc, fmt);
}

// shape ids: 0 identity, 1 + (k - 3) / 2 square k x k, 6 + (k - 3) / 2 band 1 x k, 11 + (k - 3) / 2 band k x 1; -1 not compiled
__host__ __device__ inline int shape_id(int kh, int kw) {
  if (kh == 1 && kw == 1) return 0;
  const int k = kh > kw ? kh : kw;
  if (k < 3 || k > MAX_K || !(k & 1)) return -1;
  if (kh == kw) return 1 + (k - 3) / 2;
  if (kh == 1) return 6 + (k - 3) / 2;
  if (kw == 1) return 11 + (k - 3) / 2;
  return -1;
}

// grid (tiles, planes, batch), 256 threads
template <int ACT>
__global__ __launch_bounds__(256) void gated_dwconv_kernel(const rsa_gated_dwconv_params p) {
  __shared__ f32x4 lds[2][HALO_UNITS];
  const int tiles_x = (p.W + TW - 1) / TW;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int x0 = tx * TW, y0 = ty * TH;
  const int pl = blockIdx.y, n = blockIdx.z;
  Operands o;
  o.g_hi = (const bf16x8*)p.g_hi + (int64_t)n * p.g_batch_stride + (int64_t)pl * p.g_plane_stride;
  o.g_lo = p.g_lo ? (const bf16x8*)p.g_lo + (int64_t)n * p.g_batch_stride + (int64_t)pl * p.g_plane_stride : nullptr;
  o.x_hi = (const bf16x8*)p.x_hi + (int64_t)n * p.x_batch_stride + (int64_t)pl * p.x_plane_stride;
  o.x_lo = p.x_lo ? (const bf16x8*)p.x_lo + (int64_t)n * p.x_batch_stride + (int64_t)pl * p.x_plane_stride : nullptr;
  o.o_hi = (bf16x8*)p.out_hi + (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride;
  o.o_lo = p.out_lo ? (bf16x8*)p.out_lo + (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride : nullptr;
  // the segment of this plane (workgroup-uniform)
  int sid = 0, first = p.i_planes;
  const float* w = nullptr;
  const float* b = nullptr;
  if (pl >= p.i_planes) {
    for (int s = 0; s < p.n_segments; ++s) {
      if (pl < first + p.seg[s].planes) {
        sid = shape_id(p.seg[s].kh, p.seg[s].kw);
        w = p.seg[s].weight + (int64_t)(pl - first) * 8 * p.seg[s].kh * p.seg[s].kw;
        b = p.seg[s].bias + (int64_t)(pl - first) * 8;
        break;
      }
      first += p.seg[s].planes;
    }
  }
  const int fmt = p.fmt;
  f32x4* l0 = lds[0];
  f32x4* l1 = lds[1];
  switch (sid) {
    case 0: {  // passthrough: straight vector loads, no halo
      const int x = x0 + (int)(threadIdx.x & (TW - 1)), y = y0 + (int)(threadIdx.x / TW);
      if (x >= p.W || y >= p.H) return;
      const int64_t pix = (int64_t)y * p.W + x;
      float m[8];
      get_unit(o.x_hi, o.x_lo, pix, m, fmt);
      finish<ACT>(o, pix, m, fmt);
      return;
    }
#define RSA_MOSR_CASE(ID, KH, KW) \
  case ID:                        \
    conv_tile<ACT, KH, KW>(o, w, b, p.H, p.W, x0, y0, fmt, l0, l1); \
    return;
    RSA_MOSR_CASE(1, 3, 3)
    RSA_MOSR_CASE(2, 5, 5)
    RSA_MOSR_CASE(3, 7, 7)
    RSA_MOSR_CASE(4, 9, 9)
    RSA_MOSR_CASE(5, 11, 11)
    RSA_MOSR_CASE(6, 1, 3)
    RSA_MOSR_CASE(7, 1, 5)
    RSA_MOSR_CASE(8, 1, 7)
    RSA_MOSR_CASE(9, 1, 9)
    RSA_MOSR_CASE(10, 1, 11)
    RSA_MOSR_CASE(11, 3, 1)
    RSA_MOSR_CASE(12, 5, 1)
    RSA_MOSR_CASE(13, 7, 1)
    RSA_MOSR_CASE(14, 9, 1)
    RSA_MOSR_CASE(15, 11, 1)
#undef RSA_MOSR_CASE
    default:
      return;
  }
}

__device__ __forceinline__ float ld_elem(const void* p, int64_t i, int dtype) {
  if (dtype == RSA_F32) return ((const float*)p)[i];
  if (dtype == RSA_F16) return (float)((const _Float16*)p)[i];
  return (float)((const __bf16*)p)[i];
}

__device__ __forceinline__ void st_elem(void* p, int64_t i, float v, int dtype) {
  if (dtype == RSA_F32)
    ((float*)p)[i] = v;
  else if (dtype == RSA_F16)
    ((_Float16*)p)[i] = (_Float16)v;
  else
    ((__bf16*)p)[i] = (__bf16)v;
}

__device__ __forceinline__ int reflect_hi(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }

// thread = output element of one (image, channel); grid (ceil(out_h * out_w / 256), C, batch).  Source index as torch's
// upsample_bilinear2d with a scale factor: src = (1 / scale) * (dst + 0.5) - 0.5, clamped at 0; the upper neighbour is clamped to pad - 1.
__global__ __launch_bounds__(256) void bilinear_add_kernel(const rsa_bilinear_add_params p, float rscale) {
  const int64_t hw = (int64_t)p.out_h * p.out_w;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= hw) return;
  const int c = blockIdx.y, n = blockIdx.z;
  const int Y = (int)(e / p.out_w), X = (int)(e - (int64_t)Y * p.out_w);
  const float sy = fmaxf(rscale * ((float)Y + 0.5f) - 0.5f, 0.f), sx = fmaxf(rscale * ((float)X + 0.5f) - 0.5f, 0.f);
  const int y0 = min((int)sy, p.pad_h - 1), x0 = min((int)sx, p.pad_w - 1);
  const int y1 = y0 + (y0 < p.pad_h - 1 ? 1 : 0), x1 = x0 + (x0 < p.pad_w - 1 ? 1 : 0);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const int64_t base = ((int64_t)n * p.C + c) * p.h * p.w;
  const int r0 = reflect_hi(y0, p.h), r1 = reflect_hi(y1, p.h), c0 = reflect_hi(x0, p.w), c1 = reflect_hi(x1, p.w);
  const float v00 = ld_elem(p.x, base + (int64_t)r0 * p.w + c0, p.dtype), v01 = ld_elem(p.x, base + (int64_t)r0 * p.w + c1, p.dtype);
  const float v10 = ld_elem(p.x, base + (int64_t)r1 * p.w + c0, p.dtype), v11 = ld_elem(p.x, base + (int64_t)r1 * p.w + c1, p.dtype);
  const float v = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  const int64_t oi = (((int64_t)n * p.C + c) * p.out_H + Y) * p.out_W + X;
  st_elem(p.out, oi, ld_elem(p.out, oi, p.dtype) + v, p.dtype);
}

}  // namespace
}  // namespace rsa

using namespace rsa;

// every argument check of rsa_gated_dwconv / rsa_gfisr_gate, then the launch with the gate activation ACT
template <int ACT>
static int gated_dwconv_launch(const rsa_gated_dwconv_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gated_dwconv: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->i_planes < 0 || p->n_segments < 0 || p->n_segments > 4 ||
      !plane_fmt_ok(p->fmt))
    return set_error(RSA_E_ARG, "gated_dwconv: bad geometry");
  int64_t planes = p->i_planes;
  for (int s = 0; s < p->n_segments; ++s) {
    const rsa_gated_dwconv_segment& g = p->seg[s];
    if (g.planes < 1 || g.reserved0 != 0) return set_error(RSA_E_ARG, "gated_dwconv: a segment needs >= 1 plane and reserved0 = 0");
    const int id = shape_id(g.kh, g.kw);
    if (id < 0) return set_error(RSA_E_UNSUPPORTED, "gated_dwconv: tap shape not compiled (1x1, kxk, 1xk, kx1 with odd k in [3, 11])");
    if (id > 0 && (g.weight == nullptr || g.bias == nullptr)) return set_error(RSA_E_ARG, "gated_dwconv: a convolution segment needs weight and bias");
    planes += g.planes;
  }
  if (planes < 1 || planes > 65535) return set_error(RSA_E_ARG, "gated_dwconv: total planes must be in [1, 65535]");
  if (!p->g_hi || !p->x_hi || !p->out_hi) return set_error(RSA_E_ARG, "gated_dwconv: null pointer");
  if (misaligned16(p->g_hi) || misaligned16(p->g_lo) || misaligned16(p->x_hi) || misaligned16(p->x_lo) || misaligned16(p->out_hi) ||
      misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "gated_dwconv: planes must be 16-byte aligned");
  const int64_t tiles = (int64_t)((p->W + TW - 1) / TW) * ((p->H + TH - 1) / TH);
  if (tiles > 0x7fffffff) return set_error(RSA_E_ARG, "gated_dwconv: map too large");
  hipLaunchKernelGGL(gated_dwconv_kernel<ACT>, dim3((unsigned)tiles, (unsigned)planes, (unsigned)p->batch), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("gated_dwconv: launch failed");
}

extern "C" int rsa_gated_dwconv(const rsa_gated_dwconv_params* p, void* stream) { return gated_dwconv_launch<RSA_ACT_MISH>(p, stream); }

extern "C" int rsa_gfisr_gate(const rsa_gated_dwconv_params* p, int32_t act, void* stream) {
  if (act == RSA_ACT_MISH) return gated_dwconv_launch<RSA_ACT_MISH>(p, stream);
  if (act == RSA_ACT_SILU) return gated_dwconv_launch<RSA_ACT_SILU>(p, stream);
  return set_error(RSA_E_UNSUPPORTED, "gfisr_gate: the gate activation must be RSA_ACT_MISH or RSA_ACT_SILU");
}

extern "C" int rsa_bilinear_add(const rsa_bilinear_add_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "bilinear_add: null params");
  if (p->dtype != RSA_F32 && p->dtype != RSA_F16 && p->dtype != RSA_BF16) return set_error(RSA_E_UNSUPPORTED, "bilinear_add: dtype must be f32, f16 or bf16");
  if (!p->x || !p->out || p->batch < 1 || p->batch > 65535 || p->C < 1 || p->C > 65535 || p->h < 1 || p->w < 1 || p->scale < 1 || p->scale > 8 ||
      p->pad_h < p->h || p->pad_w < p->w || p->pad_h >= 2 * p->h || p->pad_w >= 2 * p->w || p->out_h < 1 || p->out_w < 1 || p->out_h > p->out_H ||
      p->out_w > p->out_W || p->out_H > p->pad_h * p->scale || p->out_W > p->pad_w * p->scale)
    return set_error(RSA_E_ARG, "bilinear_add: bad geometry");
  const int64_t hw = (int64_t)p->out_h * p->out_w;
  const float rscale = (float)(1.0 / p->scale);
  hipLaunchKernelGGL(bilinear_add_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)p->C, (unsigned)p->batch), dim3(256), 0, (hipStream_t)stream, *p,
                     rscale);
  return launch_status("bilinear_add: launch failed");
}
