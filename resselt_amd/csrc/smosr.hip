// smosr.hip — what SMoSR (reference resselt/archs/smosr/arch.py) adds to the shared convolution path:
//   rsa_smosr_gate   the tail of an SMB: (a[:C] + shortcut) * tanh(a[C:]) (+ trunk) -> the f32 stream and / or the next convolution's planes
//                    SMB.forward :413-415, SMoSR.forward :455
//   rsa_smosr_pad    the front end: NCHW image -> planes with the four-sided reflect pad fused into the read          SMoSR.forward :452
//   rsa_smosr_pa     pixel attention of the pa_up head, y = leaky_relu(x * sigmoid(W x + b)), planes to planes on MFMA   PA :78-84
// All three are HBM-bound streaming kernels over a run of H*W pixels (nothing here looks at a neighbour, so no size is special).
// Byte models per pixel (every operand read once, every output written once), C channels:
//   gate  reads 8C (a: 2C f32) + 4C (s_in) + 4C (s2_in, where given); writes 4C (s_out, where given) + 2C per plane half (hi, lo)
//         e.g. stream + hi + lo planes, no trunk: 8C + 4C + 4C + 2C + 2C = 20C bytes
//   pa    reads 2C per half of x, writes 2C per half of y; the weight fragments (at most 64 KB) are staged once per workgroup
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd_smosr.h"

namespace rsa {
namespace {

// ---- rsa_smosr_gate: a lane owns one pixel and walks its planes; the 8 channels of a plane are in registers between the loads and the
// stores, so s_out may be s_in (or s2_in).  No LDS, no barrier.  64 neighbouring lanes load 64 neighbouring 16-byte units.
// grid (ceil(HW / 256), batch), 256 threads
template <int FMT>
__global__ __launch_bounds__(256) void smosr_gate_kernel(const rsa_smosr_gate_params p) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int n = blockIdx.y;
  const int p4 = p.C >> 2;  // C % 8 == 0
  const f32x4* a = (const f32x4*)p.a + (int64_t)n * 2 * p4 * HW + pix;
  const f32x4* si = (const f32x4*)p.s_in + (int64_t)n * p4 * HW + pix;
  const f32x4* s2 = p.s2_in ? (const f32x4*)p.s2_in + (int64_t)n * p4 * HW + pix : nullptr;
  f32x4* so = p.s_out ? (f32x4*)p.s_out + (int64_t)n * p4 * HW + pix : nullptr;
  char* hi = p.out_hi ? (char*)p.out_hi + ((int64_t)n * p.out_batch_stride + pix) * 16 : nullptr;
  char* lo = p.out_lo ? (char*)p.out_lo + ((int64_t)n * p.out_batch_stride + pix) * 16 : nullptr;
  for (int pl = 0; pl < (p4 >> 1); ++pl) {
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t g = 2 * pl + h;
      const f32x4 av = a[g * HW], gv = a[(p4 + g) * HW], sv = si[g * HW];
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (av[r] + sv[r]) * tanhf(gv[r]);
      if (s2 != nullptr) {
        const f32x4 tv = s2[g * HW];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] += tv[r];
      }
      if (so != nullptr) so[g * HW] = o;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * h + r] = o[r];
    }
    if (hi != nullptr) store_unit<FMT>(hi, lo, (int64_t)pl * p.out_plane_stride * 16, v);
  }
}

// ---- rsa_smosr_pad: one thread per (n, plane, y, x) unit of the padded map, as nchw_to_planes_kernel (capi.hip) with the reflection on
// all four sides; the value path (load, widen, split_elem) is that kernel's, so the planes are bit-identical to its output for F.pad(x).
__global__ __launch_bounds__(256) void smosr_pad_kernel(const rsa_smosr_pad_params p) {
  const int H = p.src_h + 2 * p.pad, W = p.src_w + 2 * p.pad;
  const int planes = (p.C + 7) >> 3;
  const int64_t HW = (int64_t)H * W, sHW = (int64_t)p.src_h * p.src_w;
  const int64_t total = (int64_t)p.batch * planes * HW;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pix = idx % HW;
    const int64_t t = idx / HW;
    const int pl = (int)(t % planes);
    const int n = (int)(t / planes);
    int sy = (int)(pix / W) - p.pad, sx = (int)(pix % W) - p.pad;
    if (sy < 0) sy = -sy;
    if (sy >= p.src_h) sy = 2 * (p.src_h - 1) - sy;
    if (sx < 0) sx = -sx;
    if (sx >= p.src_w) sx = 2 * (p.src_w - 1) - sx;
    u16x8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = pl * 8 + j;
      float v = 0.f;
      if (c < p.C) {
        const int64_t src = ((int64_t)n * p.C + c) * sHW + (int64_t)sy * p.src_w + sx;
        if (p.dtype == RSA_F32)
          v = ((const float*)p.x)[src];
        else if (p.dtype == RSA_F16)
          v = (float)((const _Float16*)p.x)[src];
        else
          v = (float)((const __bf16*)p.x)[src];
      }
      uint16_t hb, lb;
      split_elem(v, p.fmt, hb, lb);
      h[j] = hb;
      l[j] = lb;
    }
    const int64_t unit = (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride + pix;
    ((u16x8*)p.out_hi)[unit] = h;
    if (p.out_lo != nullptr) ((u16x8*)p.out_lo)[unit] = l;
  }
}

// ---- rsa_smosr_pa.  D[16 out][16 pixels] += A[16 out][32 in] * B[32 in][16 pixels] (v_mfma_f32_16x16x32): lane l of a B fragment holds
// channels 8 (l >> 4) .. + 7 of chunk k at pixel l & 15 -- exactly the 16-byte unit of plane 4 k + (l >> 4), loaded straight from memory.
// The rows of the two A tiles of an output chunk are ordered (resselt_amd_smosr.h) so that the lane's two accumulators are channels
// 0..3 and 4..7 of plane 4 mo + (l >> 4) at the same pixel: the unit the lane holds as its B fragment of chunk mo is the x of the gate,
// and the result leaves as one 16-byte store per half.  x is read once, y written once.
// A wave takes 32 pixels per step (two pixel groups share every A fragment read from LDS), a workgroup 128; the workgroups stride over
// the image so that the weights are staged once per workgroup.  grid (min(steps, workgroups the device holds at once), batch), 256
// threads, LDS = the fragments: as many workgroups as the device holds at once (what the runtime says fits a CU, times its CUs).
constexpr int PA_WAVE_PX = 32, PA_WG_PX = 128;

template <int NCH, int FMT, int NP>
__global__ __launch_bounds__(256) void smosr_pa_kernel(const rsa_smosr_pa_params p) {
  extern __shared__ bf16x8 pa_w[];  // [NCH][NCH][2][NHL][64]
  constexpr int NHL = NP == 3 ? 2 : 1;
  constexpr int NFRAG = NCH * NCH * 2 * NHL;
  for (int i = threadIdx.x; i < NFRAG * 64; i += 256) pa_w[i] = ((const bf16x8*)p.w_frag)[i];
  __syncthreads();  // the only barrier: from here on the four waves are independent

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane >> 4, col = lane & 15;
  const int n = blockIdx.y;
  const int planes = p.C >> 3;
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t steps = (HW + PA_WG_PX - 1) / PA_WG_PX;
  const bf16x8 zero = {};
  const char* in_hi = (const char*)p.in_hi + (int64_t)n * p.in_batch_stride * 16;
  const char* in_lo = p.in_lo ? (const char*)p.in_lo + (int64_t)n * p.in_batch_stride * 16 : nullptr;
  char* out_hi = (char*)p.out_hi + (int64_t)n * p.out_batch_stride * 16;
  char* out_lo = p.out_lo ? (char*)p.out_lo + (int64_t)n * p.out_batch_stride * 16 : nullptr;

  for (int64_t step = blockIdx.x; step < steps; step += gridDim.x) {
    const int64_t base = step * PA_WG_PX + wave * PA_WAVE_PX;
    if (base >= HW) continue;  // wave-uniform
    int64_t pix[2];
    bool live[2];
    bf16x8 bh[NCH][2], bl[NCH][2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      pix[g] = base + 16 * g + col;
      live[g] = pix[g] < HW;
      const int64_t pc = live[g] ? pix[g] : HW - 1;  // a lane past the image reads its last pixel and stores nothing
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int pl = 4 * k + q;
        bh[k][g] = zero, bl[k][g] = zero;
        if (pl < planes) {
          const int64_t off = ((int64_t)pl * p.in_plane_stride + pc) * 16;
          bh[k][g] = *(const bf16x8*)(in_hi + off);
          if (in_lo != nullptr) bl[k][g] = *(const bf16x8*)(in_lo + off);
        }
      }
    }
#pragma unroll
    for (int mo = 0; mo < NCH; ++mo) {
      f32x4 acc[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 2; ++g) acc[t][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8* f = pa_w + (((mo * NCH + k) * 2 + t) * NHL) * 64 + lane;
          const bf16x8 ah = f[0];
          if constexpr (NP == 3) {
            const bf16x8 al = f[64];
#pragma unroll
            for (int g = 0; g < 2; ++g) {  // the small terms first
              acc[t][g] = mfma16<FMT>(al, bh[k][g], acc[t][g]);
              acc[t][g] = mfma16<FMT>(ah, bl[k][g], acc[t][g]);
            }
          }
#pragma unroll
          for (int g = 0; g < 2; ++g) acc[t][g] = mfma16<FMT>(ah, bh[k][g], acc[t][g]);
        }
      }
      const int pl = 4 * mo + q;
      if (pl < planes) {
        const f32x4 b0 = *(const f32x4*)(p.bias + 8 * pl), b1 = *(const f32x4*)(p.bias + 8 * pl + 4);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          float x[8], y[8];
          widen_unit<FMT>(bh[mo][g], bl[mo][g], x);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float z = j < 4 ? acc[0][g][j] + b0[j] : acc[1][g][j - 4] + b1[j - 4];
            const float v = x[j] * sigmoid_exact(z);
            y[j] = v > 0.f ? v : v * p.slope;
          }
          if (live[g]) store_unit<FMT>(out_hi, out_lo, ((int64_t)pl * p.out_plane_stride + pix[g]) * 16, y);
        }
      }
    }
  }
}

// as many workgroups as the device holds at once (LDS = the fragments of this instantiation, so the answer is cached per instantiation)
template <int NCH, int FMT, int NP>
void pa_go(const rsa_smosr_pa_params& p, int64_t steps, int cus, size_t lds, hipStream_t s) {
  static const int per_cu = [lds] {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, smosr_pa_kernel<NCH, FMT, NP>, 256, lds) != hipSuccess || n < 1) n = 1;
    return n;
  }();
  const int64_t resident = (int64_t)per_cu * cus;
  const dim3 grid((unsigned)(steps < resident ? steps : resident), (unsigned)p.batch);
  hipLaunchKernelGGL((smosr_pa_kernel<NCH, FMT, NP>), grid, dim3(256), lds, s, p);
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_smosr_gate(const rsa_smosr_gate_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "smosr_gate: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "smosr_gate: bad geometry (reserved0 0)");
  if (p->C < 8 || p->C > 128 || (p->C & 7)) return set_error(RSA_E_ARG, "smosr_gate: C must be a multiple of 8 from 8 to 128");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "smosr_gate: bad plane format");
  if (!p->a || !p->s_in) return set_error(RSA_E_ARG, "smosr_gate: null operand");
  if (!p->s_out && !p->out_hi) return set_error(RSA_E_ARG, "smosr_gate: no output (s_out and out_hi are both NULL)");
  if (p->out_lo && !p->out_hi) return set_error(RSA_E_ARG, "smosr_gate: out_lo without out_hi");
  if (p->s_out && (const float*)p->s_out == p->a) return set_error(RSA_E_ARG, "smosr_gate: s_out must not be a (in place is s_out == s_in)");
  if (misaligned16(p->a) || misaligned16(p->s_in) || misaligned16(p->s2_in) || misaligned16(p->s_out) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "smosr_gate: maps and planes must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->out_hi && p->out_plane_stride < HW) return set_error(RSA_E_ARG, "smosr_gate: the plane stride is smaller than the map");
  const int64_t blocks = (HW + 255) / 256;
  if (blocks > 0x7fffffff) return set_error(RSA_E_ARG, "smosr_gate: map too large");
  const dim3 grid((unsigned)blocks, (unsigned)p->batch);
  with_fmt(p->fmt, [&](auto F) { hipLaunchKernelGGL((smosr_gate_kernel<decltype(F)::value>), grid, dim3(256), 0, (hipStream_t)stream, *p); });
  return launch_status("smosr_gate: launch failed");
}

extern "C" int rsa_smosr_pad(const rsa_smosr_pad_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "smosr_pad: null params");
  if (p->batch < 1 || p->C < 1 || p->src_h < 1 || p->src_w < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "smosr_pad: bad geometry (reserved0 0)");
  if (p->pad < 0 || p->pad >= p->src_h || p->pad >= p->src_w) return set_error(RSA_E_ARG, "smosr_pad: the reflection needs 0 <= pad < src_h, src_w");
  if (p->dtype != RSA_F32 && p->dtype != RSA_F16 && p->dtype != RSA_BF16) return set_error(RSA_E_ARG, "smosr_pad: bad dtype (f32, f16 or bf16)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "smosr_pad: bad plane format");
  if (!p->x || !p->out_hi) return set_error(RSA_E_ARG, "smosr_pad: null operand");
  if (misaligned16(p->out_hi) || misaligned16(p->out_lo)) return set_error(RSA_E_ALIGN, "smosr_pad: planes must be 16-byte aligned");
  const int64_t HW = (int64_t)(p->src_h + 2 * p->pad) * (p->src_w + 2 * p->pad);
  if (p->out_plane_stride < HW) return set_error(RSA_E_ARG, "smosr_pad: the plane stride is smaller than the padded map");
  const int64_t total = (int64_t)p->batch * ((p->C + 7) / 8) * HW;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(smosr_pad_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("smosr_pad: launch failed");
}

extern "C" int rsa_smosr_pa(const rsa_smosr_pa_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "smosr_pa: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "smosr_pa: bad geometry (reserved0 0)");
  if (p->C < 8 || p->C > 128 || (p->C & 7)) return set_error(RSA_E_ARG, "smosr_pa: C must be a multiple of 8 from 8 to 128");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "smosr_pa: bad plane format");
  if (p->products != 1 && p->products != 3) return set_error(RSA_E_ARG, "smosr_pa: products must be 1 or 3");
  if (!p->w_frag || !p->bias || !p->in_hi || !p->out_hi) return set_error(RSA_E_ARG, "smosr_pa: null operand");
  if (p->products == 3 && !p->in_lo) return set_error(RSA_E_ARG, "smosr_pa: three products need in_lo");
  if (misaligned16(p->w_frag) || misaligned16(p->bias) || misaligned16(p->in_hi) || misaligned16(p->in_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "smosr_pa: weights, bias and planes must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->in_plane_stride < HW || p->out_plane_stride < HW) return set_error(RSA_E_ARG, "smosr_pa: a plane stride is smaller than the map");
  if (p->out_hi == p->in_hi && (p->out_plane_stride != p->in_plane_stride || p->out_batch_stride != p->in_batch_stride || (p->out_lo && p->out_lo != p->in_lo)))
    return set_error(RSA_E_ARG, "smosr_pa: in place needs equal strides and out_lo == in_lo");
  const int64_t steps = (HW + PA_WG_PX - 1) / PA_WG_PX;
  const int nch = (p->C + 31) / 32, np = p->products;
  const size_t lds = (size_t)nch * nch * 2 * (np == 3 ? 2 : 1) * 64 * 16;  // <= 64 KB
  static const int cus = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    return prop.multiProcessorCount;
  }();
  const hipStream_t s = (hipStream_t)stream;
  with_fmt(p->fmt, [&](auto F) {
    constexpr int FMT = decltype(F)::value;
#define PA_GO(NCH, NP) pa_go<NCH, FMT, NP>(*p, steps, cus, lds, s)
#define PA_NP(NCH) \
  if (np == 3)     \
    PA_GO(NCH, 3); \
  else             \
    PA_GO(NCH, 1);
    if (nch == 1) {
      PA_NP(1)
    } else if (nch == 2) {
      PA_NP(2)
    } else if (nch == 3) {
      PA_NP(3)
    } else {
      PA_NP(4)
    }
#undef PA_NP
#undef PA_GO
  });
  return launch_status("smosr_pa: launch failed");
}
