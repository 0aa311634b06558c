// figsr.hip — what FIGSR (reference resselt/archs/figsr/arch.py) adds to the shared convolution path and to GFISRv2's Fourier kernels:
//   rsa_figsr_mix     silu(g) * cat(pass-through, convhw's output, dense 1 x K band, dense K x 1 band): both bands on the MFMA and the gate
//                     in one launch                                                  InceptionConv2d :563-591, GatedCNNBlock :612-618
//   rsa_figsr_input   NCHW image -> (v - shift) / scale_norm -> reflect pad (4, 4 + w % 2, 4, 4 + h % 2) -> one plane       FIGSR.forward :672-690
//   rsa_figsr_output  a window of the head's f32 result -> v * scale_norm + shift -> the caller's dtype                     FIGSR.forward :701-708
// Byte model of rsa_figsr_mix per pixel, `planes` planes of 16-byte units with h halves each (hi, or hi + lo): g read once (16 h planes),
// x read once except its c_hw planes, which are not read at all (16 h (planes - P)), hw read once (16 h P), out written once
// (16 h planes): 48 h planes bytes, the band halos (K - 1 columns or rows beside a 16 x 32 tile) on top of that.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd_figsr.h"

namespace rsa {
namespace {

// ---- rsa_figsr_mix.  The tile and the fragment layout are rsa_plk_conv's (plksr.hip): a workgroup owns 16 x 32 pixels, its four waves 8
// rows each; D[cout 16][pixel 16] += A[cout][k 32] * B[k][pixel] with k = 4 taps x 8 channels of one input plane, so a B fragment is the
// 16-byte unit of that plane at the pixel shifted by the lane group's tap -- along the row for the 1 x K band, down the column for the
// K x 1 band.  The two bands run one after the other through ONE halo buffer in LDS (16 + K - 1 columns x 32 rows, then 16 columns x
// 32 + K - 1 rows: a halo in one direction only), so the buffer is sized by the wider of the two; zeros outside the image.  The taps past
// K of the last step multiply zero weights; their LDS address is clamped to tap K - 1 so that it stays inside the halo.
// Before the bands every thread gates the tile's pass-through planes and convhw's planes (two pixels per thread, a plane at a time);
// after them a lane holds, per band, 4 output channels of 8 rows at one column: half a unit, gated with the matching half of g's unit.
constexpr int FM_TW = 16, FM_ROWS = 8, FM_TH = 4 * FM_ROWS;

__host__ __device__ constexpr int fm_halo_units(int k) { return FM_TH * (FM_TW + k - 1); }  // >= (FM_TH + k - 1) * FM_TW

__device__ __forceinline__ float silu_exact(float v) { return v / (1.f + expf(-v)); }  // as rsa_gfisr_gate (mosr.hip)

template <int FMT, int PROD, int KMAX>
__global__ __launch_bounds__(256) void figsr_mix_kernel(const rsa_figsr_mix_params p) {
  constexpr int HL = PROD == 3 ? 2 : 1;
  __shared__ uint4 s_in[HL][fm_halo_units(KMAX)];
  const int K = p.ksize, S = (K + 3) >> 2, R = K >> 1, P = p.gc >> 3;
  const int n = blockIdx.z, tx0 = blockIdx.x * FM_TW, ty0 = blockIdx.y * FM_TH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 4, col = lane & 15;
  const char* g_hi = (const char*)p.g_hi + (int64_t)n * p.g_batch_stride * 16;
  const char* g_lo = p.g_lo ? (const char*)p.g_lo + (int64_t)n * p.g_batch_stride * 16 : nullptr;
  const char* x_hi = (const char*)p.x_hi + (int64_t)n * p.x_batch_stride * 16;
  const char* x_lo = p.x_lo ? (const char*)p.x_lo + (int64_t)n * p.x_batch_stride * 16 : nullptr;
  const char* w_hi = (const char*)p.hw_hi + (int64_t)n * p.hw_batch_stride * 16;
  const char* w_lo = p.hw_lo ? (const char*)p.hw_lo + (int64_t)n * p.hw_batch_stride * 16 : nullptr;
  char* o_hi = (char*)p.out_hi + (int64_t)n * p.out_batch_stride * 16;
  char* o_lo = p.out_lo ? (char*)p.out_lo + (int64_t)n * p.out_batch_stride * 16 : nullptr;

  // the planes no convolution touches here: i, the Fourier branch and convhw's output
  const int ew_planes = p.pass_planes + P;
  for (int u = tid; u < FM_TW * FM_TH; u += 256) {
    const int gy = ty0 + (u >> 4), gx = tx0 + (u & 15);
    if (gy >= p.H || gx >= p.W) continue;
    const int64_t pix = (int64_t)gy * p.W + gx;
#pragma unroll 2
    for (int q = 0; q < ew_planes; ++q) {
      float g[8], v[8], r[8];
      load_unit<FMT>(g_hi, g_lo, ((int64_t)q * p.g_plane_stride + pix) * 16, g);
      if (q < p.pass_planes)
        load_unit<FMT>(x_hi, x_lo, ((int64_t)q * p.x_plane_stride + pix) * 16, v);
      else
        load_unit<FMT>(w_hi, w_lo, ((int64_t)(q - p.pass_planes) * p.hw_plane_stride + pix) * 16, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = silu_exact(g[j]) * v[j];
      store_unit<FMT>(o_hi, o_lo, ((int64_t)q * p.out_plane_stride + pix) * 16, r);
    }
  }

  f32x4 acc[2][FM_ROWS];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < FM_ROWS; ++r) acc[b][r] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const uint4* wts = (const uint4*)p.w_packed;
#pragma unroll
  for (int band = 0; band < 2; ++band) {
    const int hw = band == 0 ? FM_TW + K - 1 : FM_TW;  // the halo of this band: width, height, and where the tile sits in it
    const int hh = band == 0 ? FM_TH : FM_TH + K - 1;
    const int ox = band == 0 ? R : 0, oy = band == 0 ? 0 : R;
    const int nunits = hw * hh;
    for (int pl = 0; pl < P; ++pl) {
      const int64_t plane = (int64_t)(p.pass_planes + (1 + band) * P + pl) * p.x_plane_stride;
      __syncthreads();  // the previous halo is no longer read
      for (int u = tid; u < nunits; u += 256) {
        const int yy = u / hw, xx = u - yy * hw;
        const int gy = ty0 + yy - oy, gx = tx0 + xx - ox;
        uint4 h = {0u, 0u, 0u, 0u}, l = {0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
          const int64_t off = (plane + (int64_t)gy * p.W + gx) * 16;
          h = *(const uint4*)(x_hi + off);
          if constexpr (PROD == 3) l = *(const uint4*)(x_lo + off);
        }
        s_in[0][u] = h;
        if constexpr (PROD == 3) s_in[HL - 1][u] = l;
      }
      __syncthreads();
      const uint4* wpl = wts + (int64_t)((band * P + pl) * S) * HL * 64 + lane;
      for (int s = 0; s < S; ++s) {
        int t = 4 * s + grp;
        if (t >= K) t = K - 1;  // zero weights: any address inside the halo
        const bf16x8 ah = __builtin_bit_cast(bf16x8, wpl[(int64_t)s * HL * 64]);
        bf16x8 al = {};
        if constexpr (PROD == 3) al = __builtin_bit_cast(bf16x8, wpl[(int64_t)s * HL * 64 + 64]);
        const int base = band == 0 ? wave * FM_ROWS * hw + col + t : (wave * FM_ROWS + t) * hw + col;
#pragma unroll
        for (int r = 0; r < FM_ROWS; ++r) {
          const bf16x8 bh = __builtin_bit_cast(bf16x8, s_in[0][base + r * hw]);
          acc[band][r] = mfma16<FMT>(ah, bh, acc[band][r]);
          if constexpr (PROD == 3) {
            const bf16x8 bl = __builtin_bit_cast(bf16x8, s_in[HL - 1][base + r * hw]);
            acc[band][r] = mfma16<FMT>(ah, bl, acc[band][r]);
            acc[band][r] = mfma16<FMT>(al, bh, acc[band][r]);
          }
        }
      }
    }
  }

  // epilogue: lane (grp, col) holds pixel column col, output channels 4 grp .. + 3 = half a unit of plane grp / 2 of either band
  const int x = tx0 + col;
  const int c0 = 4 * grp;
  if (x >= p.W || c0 >= p.gc) return;
#pragma unroll
  for (int band = 0; band < 2; ++band) {
    const int plane = p.pass_planes + (1 + band) * P + (c0 >> 3);
    const f32x4 b = *(const f32x4*)((band == 0 ? p.bias_w : p.bias_h) + c0);
#pragma unroll
    for (int r = 0; r < FM_ROWS; ++r) {
      const int y = ty0 + wave * FM_ROWS + r;
      if (y >= p.H) break;
      const int64_t pix = (int64_t)y * p.W + x;
      const int64_t goff = (((int64_t)plane * p.g_plane_stride + pix) << 4) + ((c0 & 4) << 1);
      const uint2 gh = *(const uint2*)(g_hi + goff);
      const uint2 gl = g_lo ? *(const uint2*)(g_lo + goff) : make_uint2(0u, 0u);
      const f32x4 g = widen4<FMT>(gh, gl);
      const f32x4 v = acc[band][r] + b;
      uint32_t h01, l01, h23, l23;
      split2<FMT>(silu_exact(g[0]) * v[0], silu_exact(g[1]) * v[1], h01, l01);
      split2<FMT>(silu_exact(g[2]) * v[2], silu_exact(g[3]) * v[3], h23, l23);
      const int64_t off = (((int64_t)plane * p.out_plane_stride + pix) << 4) + ((c0 & 4) << 1);
      *(uint2*)(o_hi + off) = make_uint2(h01, h23);
      if (o_lo) *(uint2*)(o_lo + off) = make_uint2(l01, l23);
    }
  }
}

template <int FMT, int PROD>
int figsr_mix_launch(const rsa_figsr_mix_params& p, hipStream_t stream) {
  const dim3 grid((p.W + FM_TW - 1) / FM_TW, (p.H + FM_TH - 1) / FM_TH, p.batch);
  if (p.ksize <= 17)
    hipLaunchKernelGGL((figsr_mix_kernel<FMT, PROD, 17>), grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL((figsr_mix_kernel<FMT, PROD, 31>), grid, dim3(256), 0, stream, p);
  return launch_status("figsr_mix: launch failed");
}

// the reflected source index of padded index i (pad before, src pixels, anything behind): the reflection of F.pad(mode='reflect')
__device__ __forceinline__ int figsr_reflect(int i, int pad, int src) {
  int s = i - pad;
  if (s < 0) s = -s;
  if (s >= src) s = 2 * (src - 1) - s;
  return s;
}

// ---- rsa_figsr_input: one thread per (n, y, x) unit of the padded plane, the value path of nchw_to_planes_kernel (capi.hip) behind the
// affine: an f32 subtraction and a true f32 division (nothing here can be contracted, and the build has no fast-math).
__global__ __launch_bounds__(256) void figsr_input_kernel(const rsa_figsr_input_params p) {
  const int H = p.src_h + 2 * p.pad + (p.src_h & 1), W = p.src_w + 2 * p.pad + (p.src_w & 1);
  const int64_t HW = (int64_t)H * W, sHW = (int64_t)p.src_h * p.src_w;
  const int64_t total = (int64_t)p.batch * HW;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pix = idx % HW;
    const int n = (int)(idx / HW);
    const int sy = figsr_reflect((int)(pix / W), p.pad, p.src_h), sx = figsr_reflect((int)(pix % W), p.pad, p.src_w);
    u16x8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = 0.f;
      if (j < p.C) {
        const int64_t src = ((int64_t)n * p.C + j) * sHW + (int64_t)sy * p.src_w + sx;
        if (p.dtype == RSA_F32)
          v = ((const float*)p.x)[src];
        else if (p.dtype == RSA_F16)
          v = (float)((const _Float16*)p.x)[src];
        else
          v = (float)((const __bf16*)p.x)[src];
        v = (v - p.shift[j]) / p.scale_norm[j];
      }
      uint16_t hb, lb;
      split_elem(v, p.fmt, hb, lb);
      h[j] = hb;
      l[j] = lb;
    }
    const int64_t unit = (int64_t)n * p.out_batch_stride + pix;
    ((u16x8*)p.out_hi)[unit] = h;
    if (p.out_lo != nullptr) ((u16x8*)p.out_lo)[unit] = l;
  }
}

// ---- rsa_figsr_output: one thread per output element
__global__ __launch_bounds__(256) void figsr_output_kernel(const rsa_figsr_output_params p) {
  const int64_t total = (int64_t)p.batch * p.C * p.out_h * p.out_w;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(idx % p.out_w);
    const int64_t t = idx / p.out_w;
    const int yo = (int)(t % p.out_h);
    const int64_t nc = t / p.out_h;
    const int c = (int)(nc % p.C);
    float prod = p.y[(nc * p.H + p.y0 + yo) * p.W + p.x0 + xo] * p.scale_norm[c];
    asm("" : "+v"(prod));  // opaque: the product is rounded before the sum, as torch's two operations round (no contraction into an fma)
    const float v = prod + p.shift[c];
    if (p.dtype == RSA_F32)
      ((float*)p.out)[idx] = v;
    else if (p.dtype == RSA_F16)
      ((_Float16*)p.out)[idx] = (_Float16)v;
    else
      ((__bf16*)p.out)[idx] = (__bf16)v;
  }
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_figsr_band_packed_weight_bytes(int32_t ksize, int32_t gc, int32_t products) {
  if (ksize < 3 || ksize > 31 || !(ksize & 1) || (gc != 8 && gc != 16) || (products != 1 && products != 3)) return -1;
  return (int64_t)2 * (gc / 8) * ((ksize + 3) / 4) * (products == 3 ? 2 : 1) * 64 * 16;
}

extern "C" int rsa_figsr_mix(const rsa_figsr_mix_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "figsr_mix: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "figsr_mix: bad geometry (reserved0 0)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "figsr_mix: bad plane format");
  if (p->products != 1 && p->products != 3) return set_error(RSA_E_ARG, "figsr_mix: products must be 1 or 3");
  if (p->ksize < 3 || p->ksize > 31 || !(p->ksize & 1)) return set_error(RSA_E_UNSUPPORTED, "figsr_mix: ksize must be odd, 3..31");
  if (p->gc != 8 && p->gc != 16) return set_error(RSA_E_UNSUPPORTED, "figsr_mix: gc must be 8 or 16");
  if (p->pass_planes < 0 || p->planes != p->pass_planes + 3 * (p->gc / 8)) return set_error(RSA_E_ARG, "figsr_mix: planes must be pass_planes + 3 gc / 8");
  if (!p->w_packed || !p->bias_w || !p->bias_h || !p->g_hi || !p->x_hi || !p->hw_hi || !p->out_hi) return set_error(RSA_E_ARG, "figsr_mix: null operand");
  if (p->products == 3 && !p->x_lo) return set_error(RSA_E_ARG, "figsr_mix: three products need x_lo");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->g_plane_stride < HW || p->x_plane_stride < HW || p->hw_plane_stride < HW || p->out_plane_stride < HW)
    return set_error(RSA_E_ARG, "figsr_mix: a plane stride is smaller than the map");
  if (p->out_hi == p->g_hi || p->out_hi == p->x_hi || p->out_hi == p->hw_hi) return set_error(RSA_E_ARG, "figsr_mix: out must not be g, x or hw (no in-place form)");
  if (misaligned16(p->w_packed) || misaligned16(p->bias_w) || misaligned16(p->bias_h) || misaligned16(p->g_hi) || misaligned16(p->g_lo) || misaligned16(p->x_hi) ||
      misaligned16(p->x_lo) || misaligned16(p->hw_hi) || misaligned16(p->hw_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "figsr_mix: weights, biases and planes must be 16-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  if (p->fmt == RSA_PF_BF16 && p->products == 3) return figsr_mix_launch<RSA_PF_BF16, 3>(*p, s);
  if (p->fmt == RSA_PF_F16 && p->products == 1) return figsr_mix_launch<RSA_PF_F16, 1>(*p, s);
  return set_error(RSA_E_UNSUPPORTED, "figsr_mix: compiled for bf16 planes with three products and fp16 planes with one product");
}

extern "C" int rsa_figsr_input(const rsa_figsr_input_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "figsr_input: null params");
  if (p->batch < 1 || p->C < 1 || p->src_h < 1 || p->src_w < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "figsr_input: bad geometry (reserved0 0)");
  if (p->C > 8) return set_error(RSA_E_UNSUPPORTED, "figsr_input: at most 8 channels (one plane)");
  if (p->pad < 0 || p->pad > (1 << 20) || p->pad + (p->src_h & 1) >= p->src_h || p->pad + (p->src_w & 1) >= p->src_w)
    return set_error(RSA_E_ARG, "figsr_input: the reflection needs 0 <= pad + src % 2 < src in either direction");
  if (p->dtype != RSA_F32 && p->dtype != RSA_F16 && p->dtype != RSA_BF16) return set_error(RSA_E_ARG, "figsr_input: bad dtype (f32, f16 or bf16)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "figsr_input: bad plane format");
  if (!p->x || !p->shift || !p->scale_norm || !p->out_hi) return set_error(RSA_E_ARG, "figsr_input: null operand");
  if (misaligned16(p->out_hi) || misaligned16(p->out_lo)) return set_error(RSA_E_ALIGN, "figsr_input: planes must be 16-byte aligned");
  const int64_t HW = (int64_t)(p->src_h + 2 * p->pad + (p->src_h & 1)) * (p->src_w + 2 * p->pad + (p->src_w & 1));
  if (p->out_plane_stride < HW) return set_error(RSA_E_ARG, "figsr_input: the plane stride is smaller than the padded map");
  const int64_t blocks = ((int64_t)p->batch * HW + 255) / 256;
  hipLaunchKernelGGL(figsr_input_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("figsr_input: launch failed");
}

extern "C" int rsa_figsr_output(const rsa_figsr_output_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "figsr_output: null params");
  if (p->batch < 1 || p->C < 1 || p->H < 1 || p->W < 1 || p->out_h < 1 || p->out_w < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "figsr_output: bad geometry (reserved0 0)");
  if (p->y0 < 0 || p->x0 < 0 || (int64_t)p->y0 + p->out_h > p->H || (int64_t)p->x0 + p->out_w > p->W) return set_error(RSA_E_ARG, "figsr_output: the window leaves the map");
  if (p->dtype != RSA_F32 && p->dtype != RSA_F16 && p->dtype != RSA_BF16) return set_error(RSA_E_ARG, "figsr_output: bad dtype (f32, f16 or bf16)");
  if (!p->y || !p->shift || !p->scale_norm || !p->out) return set_error(RSA_E_ARG, "figsr_output: null operand");
  const int64_t blocks = ((int64_t)p->batch * p->C * p->out_h * p->out_w + 255) / 256;
  hipLaunchKernelGGL(figsr_output_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("figsr_output: launch failed");
}
