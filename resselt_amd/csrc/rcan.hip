// rcan.hip — the kernels RCAN needs beside the fused convolution (reference archs/rcan/arch.py):
//   rsa_rcab_tail    the channel attention's gate from the pooled sums of the block's second convolution, and  out = x + gate * y   :148-196
//   rsa_rcan_input   x * rgb_range and the sub_mean 1x1 convolution as one pointwise step                                          :323-324
// The sums come from the convolution's own epilogue (rsa_conv_params.pool_sums; conv_common.h EM 5), so an RCAB is two convolutions, one
// single-workgroup gate kernel per image and ONE pass over the map, where conv + conv + rsa_channel_gate + an apply pass reads the map twice.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

constexpr int RT_GATE_THREADS = 1024;
constexpr int RT_MAX_C = 512, RT_MAX_HIDDEN = 128;

// grid (batch), 1024 threads.  Thread t owns four channels (t % C4) of the slots  t / C4, + NSL, + 2 NSL ...: consecutive threads read
// consecutive 16-byte groups of a slot row (a wave covers 1 KiB), every partial is the f64 sum of its strided slots in ascending order, and
// the NSL partials of a channel are then added in order by one thread.  Not slot order, but a fixed order for a given slot count: the same
// bits on every run.
__global__ __launch_bounds__(RT_GATE_THREADS) void rcab_gate_kernel(const float* __restrict__ sums, int slots, int C, int Cp, int hidden, double inv_hw,
                                                                   const float* __restrict__ w1, const float* __restrict__ b1,
                                                                   const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ gate) {
  __shared__ double s_part[RT_GATE_THREADS * 4];  // [slot lane][Cp]: NSL * Cp <= 4096
  __shared__ double s_mean[RT_MAX_C];
  __shared__ double s_hid[RT_MAX_HIDDEN];
  const int n = blockIdx.x, t = threadIdx.x;
  const int C4 = Cp >> 2;
  const int NSL = RT_GATE_THREADS / C4;
  const int c4 = t % C4, sl = t / C4;
  if (sl < NSL) {
    const f32x4* src = (const f32x4*)(sums + (int64_t)n * slots * Cp) + c4;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t s = sl;  // (slots goes up to 2^30: the look-ahead below must not wrap)
    for (; s + 3 * NSL < slots; s += 4 * NSL) {  // four loads in flight per thread
      const f32x4 v0 = src[s * C4], v1 = src[(s + NSL) * C4], v2 = src[(s + 2 * NSL) * C4], v3 = src[(s + 3 * NSL) * C4];
      a0 = (((a0 + v0[0]) + v1[0]) + v2[0]) + v3[0];
      a1 = (((a1 + v0[1]) + v1[1]) + v2[1]) + v3[1];
      a2 = (((a2 + v0[2]) + v1[2]) + v2[2]) + v3[2];
      a3 = (((a3 + v0[3]) + v1[3]) + v2[3]) + v3[3];
    }
    for (; s < slots; s += NSL) {
      const f32x4 v = src[s * C4];
      a0 += v[0], a1 += v[1], a2 += v[2], a3 += v[3];
    }
    double* dst = s_part + (sl * Cp + c4 * 4);
    dst[0] = a0, dst[1] = a1, dst[2] = a2, dst[3] = a3;
  }
  __syncthreads();
  for (int c = t; c < C; c += RT_GATE_THREADS) {
    double s = 0.0;
    for (int k = 0; k < NSL; ++k) s += s_part[k * Cp + c];
    s_mean[c] = s * inv_hw;
  }
  __syncthreads();
  if (t < hidden) {
    double s = (double)b1[t];
    for (int c = 0; c < C; ++c) s += (double)w1[(int64_t)t * C + c] * s_mean[c];
    s_hid[t] = s > 0.0 ? s : 0.0;
  }
  __syncthreads();
  for (int c = t; c < C; c += RT_GATE_THREADS) {
    double s = (double)b2[c];
    for (int k = 0; k < hidden; ++k) s += (double)w2[(int64_t)c * hidden + k] * s_hid[k];
    gate[(int64_t)n * C + c] = (float)(1.0 / (1.0 + exp(-s)));
  }
}

// grid (ceil(HW / 256), planes, batch), 256 threads: thread = one 16-byte unit (8 channels of one pixel) of y, x and out; a wave reads and
// writes 1 KiB runs of each plane (hi and lo).  out may be x or y (a thread loads its unit of both before it stores): the plane operands are
// not __restrict__
template <int FMT>
__global__ __launch_bounds__(256) void rcab_apply_kernel(const char* yhi, const char* ylo, int64_t y_ps, int64_t y_bs,
                                                         const char* xhi, const char* xlo, int64_t x_ps, int64_t x_bs, char* ohi,
                                                         char* olo, int64_t o_ps, int64_t o_bs, int64_t HW, int C, const float* __restrict__ gate) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pl = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  const f32x4 g0 = *(const f32x4*)(gate + (int64_t)n * C + pl * 8), g1 = *(const f32x4*)(gate + (int64_t)n * C + pl * 8 + 4);
  const int64_t yo = ((int64_t)n * y_bs + (int64_t)pl * y_ps + pix) * 16, xo = ((int64_t)n * x_bs + (int64_t)pl * x_ps + pix) * 16;
  const uint4 yh = *(const uint4*)(yhi + yo), xh = *(const uint4*)(xhi + xo);
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const uint4 yl = ylo ? *(const uint4*)(ylo + yo) : z, xl = xlo ? *(const uint4*)(xlo + xo) : z;
  const f32x4 ya = widen4<FMT>(make_uint2(yh.x, yh.y), make_uint2(yl.x, yl.y)), yb = widen4<FMT>(make_uint2(yh.z, yh.w), make_uint2(yl.z, yl.w));
  const f32x4 xa = widen4<FMT>(make_uint2(xh.x, xh.y), make_uint2(xl.x, xl.y)), xb = widen4<FMT>(make_uint2(xh.z, xh.w), make_uint2(xl.z, xl.w));
  float o[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = fmaf(g0[j], ya[j], xa[j]);
    o[4 + j] = fmaf(g1[j], yb[j], xb[j]);
  }
  uint32_t h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) split2<FMT>(o[2 * j], o[2 * j + 1], h[j], l[j]);
  const int64_t oo = ((int64_t)n * o_bs + (int64_t)pl * o_ps + pix) * 16;
  *(uint4*)(ohi + oo) = make_uint4(h[0], h[1], h[2], h[3]);
  if (olo) *(uint4*)(olo + oo) = make_uint4(l[0], l[1], l[2], l[3]);
}

// thread = pixel; grid (ceil(HW / 256), batch)
__global__ __launch_bounds__(256) void rcan_input_kernel(const void* __restrict__ x, int dtype, int C, int64_t HW, float scale, const float* __restrict__ weight,
                                                         const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (pix >= HW) return;
  float v[4];
  for (int c = 0; c < C; ++c) {
    float a;
    if (dtype == RSA_U8)
      a = (float)((const uint8_t*)x)[((int64_t)n * HW + pix) * C + c] / 255.f;
    else if (dtype == RSA_F32)
      a = ((const float*)x)[((int64_t)n * C + c) * HW + pix];
    else if (dtype == RSA_F16)
      a = (float)((const _Float16*)x)[((int64_t)n * C + c) * HW + pix];
    else
      a = (float)((const __bf16*)x)[((int64_t)n * C + c) * HW + pix];
    v[c] = a * scale;
  }
  for (int o = 0; o < C; ++o) {
    float s = bias[o];
    for (int c = 0; c < C; ++c) s = fmaf(weight[o * C + c], v[c], s);
    out[((int64_t)n * C + o) * HW + pix] = s;
  }
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_rcab_tail(const float* pool_sums, int32_t slots, const float* w1, const float* b1, const float* w2, const float* b2, int32_t hidden,
                             float* gate, const void* y_hi, const void* y_lo, int64_t y_plane_stride, int64_t y_batch_stride, const void* x_hi,
                             const void* x_lo, int64_t x_plane_stride, int64_t x_batch_stride, void* out_hi, void* out_lo, int64_t out_plane_stride,
                             int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t fmt, void* stream) {
  if (!gate || !y_hi || !x_hi || !out_hi) return set_error(RSA_E_ARG, "rcab_tail: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || C < 8 || (C & 7) || C > RT_MAX_C) return set_error(RSA_E_ARG, "rcab_tail: bad geometry (C % 8 == 0, C <= 512)");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "rcab_tail: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  if (y_plane_stride < HW || x_plane_stride < HW || out_plane_stride < HW) return set_error(RSA_E_ARG, "rcab_tail: a plane stride is smaller than the map");
  if (misaligned16(y_hi) || misaligned16(y_lo) || misaligned16(x_hi) || misaligned16(x_lo) || misaligned16(out_hi) || misaligned16(out_lo) || misaligned16(gate))
    return set_error(RSA_E_ALIGN, "rcab_tail: planes and the gate must be 16-byte aligned");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "rcab_tail: map too large");
  hipStream_t s = (hipStream_t)stream;
  if (pool_sums != nullptr) {
    if (!w1 || !b1 || !w2 || !b2) return set_error(RSA_E_ARG, "rcab_tail: null gate weights");
    if (slots < 1 || hidden < 1 || hidden > RT_MAX_HIDDEN) return set_error(RSA_E_ARG, "rcab_tail: bad slots / hidden (1..128)");
    if (misaligned16(pool_sums)) return set_error(RSA_E_ALIGN, "rcab_tail: pool_sums must be 16-byte aligned");
    const int Cp = (C + 15) & ~15;
    hipLaunchKernelGGL(rcab_gate_kernel, dim3((unsigned)batch), dim3(RT_GATE_THREADS), 0, s, pool_sums, (int)slots, (int)C, Cp, (int)hidden, 1.0 / (double)HW, w1, b1,
                       w2, b2, gate);
    const int rc = (int)hipGetLastError();
    if (rc) return set_error(rc, "rcab_tail: gate kernel launch failed");
  }
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(C / 8), (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(rcab_apply_kernel<decltype(F)::value>, grid, dim3(256), 0, s, (const char*)y_hi, (const char*)y_lo, y_plane_stride, y_batch_stride, (const char*)x_hi,
                       (const char*)x_lo, x_plane_stride, x_batch_stride, (char*)out_hi, (char*)out_lo, out_plane_stride, out_batch_stride, HW, (int)C, gate);
  });
  return launch_status("rcab_tail: launch failed");
}

extern "C" int rsa_rcan_input(const void* x, int32_t dtype, int32_t batch, int32_t C, int32_t H, int32_t W, float scale, const float* weight, const float* bias,
                              float* out, void* stream) {
  if (!x || !weight || !bias || !out || batch < 1 || batch > 65535 || H < 1 || W < 1 || C < 1 || C > 4) return set_error(RSA_E_ARG, "rcan_input: bad argument (C <= 4)");
  if (dtype < RSA_F32 || dtype > RSA_U8) return set_error(RSA_E_ARG, "rcan_input: bad dtype");
  const int64_t HW = (int64_t)H * W;
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "rcan_input: map too large");
  hipLaunchKernelGGL(rcan_input_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x, (int)dtype, (int)C, HW, scale, weight,
                     bias, out);
  return launch_status("rcan_input: launch failed");
}
