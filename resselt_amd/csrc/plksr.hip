// plksr.hip — the kernels PLKSR / RealPLKSR need beyond the fused convolution (reference resselt/archs/plksr/):
//   rsa_plk_conv           dense K x K convolution of the first pdim channels (PLKConv2d, rplksr.py:22-37, plksr.py:54-93; the sparse
//                          variants are folded into one K x K kernel by the host)
//   rsa_group_norm_stats   per-(image, group) mean / rstd of an f32 map, two deterministic stages     nn.GroupNorm, rplksr.py:94, 103
//   rsa_group_norm_apply   (y - mean) * rstd * gamma + beta + skip -> split planes (+ f32 map)       rplksr.py:103-105
//   rsa_ea_gate            x * sigmoid(g), g = the f32 output of EA's 3x3 convolution                EA.forward, rplksr.py:40-49
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {

// ------------------------------------------------------------------------------------------------------------------ PLK conv
// Implicit GEMM on v_mfma_f32_16x16x32_{bf16,f16}: D[cout 16][pixel 16] += A[cout][k 32] * B[k][pixel], k = 4 taps x 8 channels of one
// input plane (the taps of a plane in row-major order, zero-padded to a multiple of 4).  A workgroup computes a 16 x 32 pixel tile for
// all pdim output channels; its four waves own 8 rows each.  Per input plane the (32 + K - 1) x (16 + K - 1) halo of the tile (hi, and
// lo for three products) is staged in LDS with zeros outside the image; the weights (the A fragments, the same for every workgroup) are
// read from global memory / L2 once per K step and used for 8 rows x CT cout tiles.
constexpr int PLK_TW = 16, PLK_ROWS = 8, PLK_TH = 4 * PLK_ROWS;

__host__ __device__ constexpr int plk_halo_units(int k) { return (PLK_TH + k - 1) * (PLK_TW + k - 1); }

template <int FMT, int PROD, int CT, int KMAX>
__global__ __launch_bounds__(256) void plk_conv_kernel(const rsa_plk_conv_params p) {
  __shared__ uint4 s_in[PROD == 3 ? 2 : 1][plk_halo_units(KMAX)];
  const int K = p.ksize, KK = K * K, S = (KK + 3) >> 2, R = K >> 1;
  const int hw = PLK_TW + K - 1, hh = PLK_TH + K - 1, nunits = hw * hh;
  const int n = blockIdx.z, tx0 = blockIdx.x * PLK_TW, ty0 = blockIdx.y * PLK_TH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 4, col = lane & 15;
  const uint4* in_hi = (const uint4*)p.in_hi + (int64_t)n * p.in_batch_stride;
  const uint4* in_lo = PROD == 3 ? (const uint4*)p.in_lo + (int64_t)n * p.in_batch_stride : nullptr;
  const uint4* wts = (const uint4*)p.w_packed;
  constexpr int HL = PROD == 3 ? 2 : 1;

  f32x4 acc[PLK_ROWS][CT];
#pragma unroll
  for (int r = 0; r < PLK_ROWS; ++r)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[r][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int pl = 0; pl < p.planes; ++pl) {
    __syncthreads();  // the previous plane's halo is no longer read
    for (int u = tid; u < nunits; u += 256) {
      const int yy = u / hw, xx = u - yy * hw;
      const int gy = ty0 + yy - R, gx = tx0 + xx - R;
      uint4 h = {0u, 0u, 0u, 0u}, l = {0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
        const int64_t off = (int64_t)pl * p.in_plane_stride + (int64_t)gy * p.W + gx;
        h = in_hi[off];
        if constexpr (PROD == 3) l = in_lo[off];
      }
      s_in[0][u] = h;
      if constexpr (PROD == 3) s_in[HL - 1][u] = l;
    }
    __syncthreads();
    const uint4* wpl = wts + (int64_t)pl * S * CT * HL * 64;
    // tap of this lane's k group in step s: t = 4 s + grp, clamped to the last tap (its weights are zero) so the LDS read stays inside the halo
    int t = grp, dy = 0, dx = grp;
    while (dx >= K) dx -= K, ++dy;
    for (int s = 0; s < S; ++s) {
      const int cy = t < KK ? dy : K - 1, cx = t < KK ? dx : K - 1;
      bf16x8 ah[CT], al[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const uint4* wf = wpl + ((int64_t)s * CT + c) * HL * 64 + lane;
        ah[c] = __builtin_bit_cast(bf16x8, wf[0]);
        if constexpr (PROD == 3) al[c] = __builtin_bit_cast(bf16x8, wf[64]);
      }
      const int base = (wave * PLK_ROWS + cy) * hw + col + cx;
#pragma unroll
      for (int r = 0; r < PLK_ROWS; ++r) {
        const bf16x8 bh = __builtin_bit_cast(bf16x8, s_in[0][base + r * hw]);
        if constexpr (PROD == 3) {
          const bf16x8 bl = __builtin_bit_cast(bf16x8, s_in[HL - 1][base + r * hw]);
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            acc[r][c] = mfma16<FMT>(ah[c], bh, acc[r][c]);
            acc[r][c] = mfma16<FMT>(ah[c], bl, acc[r][c]);
            acc[r][c] = mfma16<FMT>(al[c], bh, acc[r][c]);
          }
        } else {
#pragma unroll
          for (int c = 0; c < CT; ++c) acc[r][c] = mfma16<FMT>(ah[c], bh, acc[r][c]);
        }
      }
      t += 4;
      dx += 4;
      while (dx >= K) dx -= K, ++dy;
    }
  }

  // epilogue: lane (grp, col) holds pixel column col, output channels 16 c + 4 grp .. +3 = half a unit of plane (16 c + 4 grp) / 8
  const int x = tx0 + col;
  if (x >= p.W) return;
  const int pdim = 8 * p.planes;
  char* ob_hi = (char*)p.out_hi + (int64_t)n * p.out_batch_stride * 16;
  char* ob_lo = p.out_lo ? (char*)p.out_lo + (int64_t)n * p.out_batch_stride * 16 : nullptr;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int c0 = 16 * c + 4 * grp;
    if (c0 >= pdim) continue;
    const f32x4 b = *(const f32x4*)(p.bias + c0);
#pragma unroll
    for (int r = 0; r < PLK_ROWS; ++r) {
      const int y = ty0 + wave * PLK_ROWS + r;
      if (y >= p.H) break;
      const f32x4 v = acc[r][c] + b;
      uint32_t h01, l01, h23, l23;
      split2<FMT>(v[0], v[1], h01, l01);
      split2<FMT>(v[2], v[3], h23, l23);
      const int64_t off = (((int64_t)(p.out_plane_off + (c0 >> 3)) * p.out_plane_stride + (int64_t)y * p.W + x) << 4) + ((c0 & 4) << 1);
      *(uint2*)(ob_hi + off) = make_uint2(h01, h23);
      if (ob_lo) *(uint2*)(ob_lo + off) = make_uint2(l01, l23);
    }
  }
}

template <int FMT, int PROD, int KMAX>
static int plk_launch_k(const rsa_plk_conv_params& p, hipStream_t stream) {
  const dim3 grid((p.W + PLK_TW - 1) / PLK_TW, (p.H + PLK_TH - 1) / PLK_TH, p.batch);
  switch ((p.planes + 1) / 2) {
    case 1:
      plk_conv_kernel<FMT, PROD, 1, KMAX><<<grid, 256, 0, stream>>>(p);
      break;
    case 2:
      plk_conv_kernel<FMT, PROD, 2, KMAX><<<grid, 256, 0, stream>>>(p);
      break;
    case 3:
      plk_conv_kernel<FMT, PROD, 3, KMAX><<<grid, 256, 0, stream>>>(p);
      break;
    default:
      plk_conv_kernel<FMT, PROD, 4, KMAX><<<grid, 256, 0, stream>>>(p);
      break;
  }
  return (int)hipGetLastError();
}

template <int FMT, int PROD>
static int plk_launch(const rsa_plk_conv_params& p, hipStream_t stream) {
  return p.ksize <= 17 ? plk_launch_k<FMT, PROD, 17>(p, stream) : plk_launch_k<FMT, PROD, 31>(p, stream);
}

// ------------------------------------------------------------------------------------------------------------------ GroupNorm
// Stage 1: one workgroup per (chunk of PIX_PER_CHUNK pixels, image).  Each thread sums v - shift and (v - shift)^2 per group in f32, the
// shift being the group's first value in the image (so |v - shift| ~ sigma even when |mean| >> sigma); the per-thread (count, mean, M2)
// are merged in a fixed tree with Chan's pairwise formula in f64.  Stage 2: one workgroup per (group, image) merges the chunks the same way.
constexpr int GN_MAXG = 8, GN_PIX_PER_CHUNK = 1024;  // 2025 workgroups for a 1080p image (4096: 506, 1.2 TB/s)

struct gn_part {
  double n, mean, m2;
};

__device__ __forceinline__ gn_part gn_merge(gn_part a, gn_part b) {
  if (a.n == 0.0) return b;
  if (b.n == 0.0) return a;
  const double n = a.n + b.n, d = b.mean - a.mean;
  return gn_part{n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

__device__ gn_part gn_block_reduce(gn_part v, gn_part* s_red) {
  const int tid = threadIdx.x;
  s_red[tid] = v;
  __syncthreads();
  for (int stride = 128; stride > 0; stride >>= 1) {
    if (tid < stride) s_red[tid] = gn_merge(s_red[tid], s_red[tid + stride]);
    __syncthreads();
  }
  const gn_part r = s_red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void gn_stats_partial_kernel(const f32x4* x, int64_t HW, int C, int G, int chunks, float* ws) {
  __shared__ gn_part s_red[256];
  const int chunk = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int p4 = C >> 2, cpg = C / G;
  const f32x4* xb = x + (int64_t)n * p4 * HW;
  float shift[GN_MAXG], s1[GN_MAXG], s2[GN_MAXG];
  int cnt[GN_MAXG];
  for (int g = 0; g < G; ++g) {
    const int c = g * cpg;
    shift[g] = xb[(int64_t)(c >> 2) * HW][c & 3];
    s1[g] = s2[g] = 0.f;
    cnt[g] = 0;
  }
  const int64_t p0 = (int64_t)chunk * GN_PIX_PER_CHUNK;
  const int64_t p1 = p0 + GN_PIX_PER_CHUNK < HW ? p0 + GN_PIX_PER_CHUNK : HW;
  for (int64_t px = p0 + tid; px < p1; px += 256) {
    for (int q = 0; q < p4; ++q) {
      const f32x4 v = xb[(int64_t)q * HW + px];
      if ((cpg & 3) == 0) {  // whole f32 groups per channel group (every dim the engine builds): one group index per load
        const int g = (4 * q) / cpg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = v[r] - shift[g];
          s1[g] += d;
          s2[g] += d * d;
        }
        cnt[g] += 4;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int g = (4 * q + r) / cpg;
          const float d = v[r] - shift[g];
          s1[g] += d;
          s2[g] += d * d;
          ++cnt[g];
        }
      }
    }
  }
  for (int g = 0; g < G; ++g) {
    gn_part mine{0.0, 0.0, 0.0};
    if (cnt[g] > 0) {
      const double m = (double)s1[g] / cnt[g];
      mine = gn_part{(double)cnt[g], (double)shift[g] + m, fmax((double)s2[g] - (double)s1[g] * m, 0.0)};
    }
    const gn_part tot = gn_block_reduce(mine, s_red);
    if (tid == 0) {
      float* o = ws + (((int64_t)n * chunks + chunk) * G + g) * 4;
      o[0] = (float)tot.n;
      o[1] = (float)tot.mean;
      o[2] = (float)tot.m2;
      o[3] = 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void gn_stats_final_kernel(const float* ws, int chunks, int G, float eps, float* stats) {
  __shared__ gn_part s_red[256];
  const int g = blockIdx.x, n = blockIdx.y;
  gn_part acc{0.0, 0.0, 0.0};
  for (int c = threadIdx.x; c < chunks; c += 256) {
    const float* w = ws + (((int64_t)n * chunks + c) * G + g) * 4;
    acc = gn_merge(acc, gn_part{(double)w[0], (double)w[1], (double)w[2]});
  }
  const gn_part tot = gn_block_reduce(acc, s_red);
  if (threadIdx.x == 0) {
    stats[((int64_t)n * G + g) * 2 + 0] = (float)tot.mean;
    stats[((int64_t)n * G + g) * 2 + 1] = (float)(1.0 / sqrt(tot.m2 / tot.n + (double)eps));
  }
}

// thread = (pixel, output plane of 8 channels); grid (ceil(HW/256), C/8, batch)
template <int FMT>
__global__ __launch_bounds__(256) void gn_apply_kernel(const rsa_group_norm_apply_params p) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t px = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  const int pl = blockIdx.y, n = blockIdx.z, cpg = p.C / p.groups;
  const int64_t f4 = ((int64_t)n * (p.C >> 2) + 2 * pl) * HW + px;  // first of the plane's two f32 groups
  const f32x4 y0 = ((const f32x4*)p.x_f32)[f4], y1 = ((const f32x4*)p.x_f32)[f4 + HW];
  f32x4 k0 = {0.f, 0.f, 0.f, 0.f}, k1 = k0;
  if (p.skip_f32) k0 = ((const f32x4*)p.skip_f32)[f4], k1 = ((const f32x4*)p.skip_f32)[f4 + HW];
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * pl + j, g = c / cpg;
    const float mean = p.stats[((int64_t)n * p.groups + g) * 2], rstd = p.stats[((int64_t)n * p.groups + g) * 2 + 1];
    const float y = j < 4 ? y0[j] : y1[j - 4];
    const float k = j < 4 ? k0[j] : k1[j - 4];
    v[j] = (y - mean) * (rstd * p.gamma[c]) + p.beta[c] + k;
  }
  if (p.out_f32) {
    ((f32x4*)p.out_f32)[f4] = (f32x4){v[0], v[1], v[2], v[3]};
    ((f32x4*)p.out_f32)[f4 + HW] = (f32x4){v[4], v[5], v[6], v[7]};
  }
  if (p.out_hi) {
    const int64_t off = ((int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride + px) << 4;
    store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, off, v);
  }
}

// ------------------------------------------------------------------------------------------------------------------ EA gate
// thread = (pixel, plane); grid (ceil(HW/256), C/8, batch):  out = x * sigmoid(g)
template <int FMT>
__global__ __launch_bounds__(256) void ea_gate_kernel(const rsa_ea_gate_params p) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t px = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  const int pl = blockIdx.y, n = blockIdx.z;
  const int64_t f4 = ((int64_t)n * (p.C >> 2) + 2 * pl) * HW + px;
  const f32x4 g0 = ((const f32x4*)p.g_f32)[f4], g1 = ((const f32x4*)p.g_f32)[f4 + HW];
  float v[8];
  load_unit<FMT>((const char*)p.x_hi, (const char*)p.x_lo, ((int64_t)n * p.x_batch_stride + (int64_t)pl * p.x_plane_stride + px) << 4, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float g = j < 4 ? g0[j] : g1[j - 4];
    v[j] = v[j] / (1.f + expf(-g));
  }
  store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, ((int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride + px) << 4, v);
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_plk_packed_weight_bytes(int32_t ksize, int32_t planes, int32_t products) {
  if (ksize < 3 || ksize > 31 || !(ksize & 1) || planes < 1 || planes > 8 || (products != 1 && products != 3)) return -1;
  const int64_t steps = (ksize * ksize + 3) / 4, ct = (planes + 1) / 2;
  return (int64_t)planes * steps * ct * (products == 3 ? 2 : 1) * 64 * 16;
}

extern "C" int rsa_plk_conv(const rsa_plk_conv_params* p, void* stream) {
  if (!p) return set_error(RSA_E_ARG, "plk_conv: null descriptor");
  if (p->batch < 1 || p->H < 1 || p->W < 1) return set_error(RSA_E_ARG, "plk_conv: bad geometry");
  if (p->ksize < 3 || p->ksize > 31 || !(p->ksize & 1)) return set_error(RSA_E_UNSUPPORTED, "plk_conv: ksize must be odd, 3..31");
  if (p->planes < 1 || p->planes > 8) return set_error(RSA_E_UNSUPPORTED, "plk_conv: planes must be 1..8 (pdim <= 64)");
  if (p->reserved0 != 0) return set_error(RSA_E_ARG, "plk_conv: reserved0 must be 0");
  if (!p->in_hi || !p->w_packed || !p->bias || !p->out_hi || (p->products == 3 && !p->in_lo))
    return set_error(RSA_E_ARG, "plk_conv: null operand");
  if (p->out_plane_off < 0 || p->in_plane_stride < (int64_t)p->H * p->W || p->out_plane_stride < (int64_t)p->H * p->W)
    return set_error(RSA_E_ARG, "plk_conv: bad strides");
  if (misaligned16(p->in_hi) || misaligned16(p->in_lo) || misaligned16(p->w_packed) || misaligned16(p->bias) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "plk_conv: operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (p->fmt == RSA_PF_BF16 && p->products == 3) return plk_launch<RSA_PF_BF16, 3>(*p, s);
  if (p->fmt == RSA_PF_F16 && p->products == 1) return plk_launch<RSA_PF_F16, 1>(*p, s);
  return set_error(RSA_E_UNSUPPORTED, "plk_conv: compiled for bf16 planes with three products and fp16 planes with one product");
}

extern "C" int64_t rsa_group_norm_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t groups) {
  if (batch < 1 || H < 1 || W < 1 || groups < 1) return -1;
  const int64_t chunks = ((int64_t)H * W + GN_PIX_PER_CHUNK - 1) / GN_PIX_PER_CHUNK;
  return (int64_t)batch * chunks * groups * 4 * sizeof(float);
}

extern "C" int rsa_group_norm_stats(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t groups, float eps, float* workspace,
                                    float* stats, void* stream) {
  if (!x_f32 || !workspace || !stats) return set_error(RSA_E_ARG, "group_norm_stats: null operand");
  if (batch < 1 || H < 1 || W < 1 || C < 4 || C % 4 || groups < 1 || groups > GN_MAXG || C % groups)
    return set_error(RSA_E_ARG, "group_norm_stats: bad geometry (C a multiple of 4 and of groups, groups <= 8)");
  if (misaligned16(x_f32)) return set_error(RSA_E_ALIGN, "group_norm_stats: x must be 16-byte aligned");
  const int64_t HW = (int64_t)H * W;
  const int chunks = (int)((HW + GN_PIX_PER_CHUNK - 1) / GN_PIX_PER_CHUNK);
  hipStream_t s = (hipStream_t)stream;
  gn_stats_partial_kernel<<<dim3(chunks, batch), 256, 0, s>>>((const f32x4*)x_f32, HW, C, groups, chunks, workspace);
  int e = (int)hipGetLastError();
  if (e) return e;
  gn_stats_final_kernel<<<dim3(groups, batch), 256, 0, s>>>(workspace, chunks, groups, eps, stats);
  return (int)hipGetLastError();
}

extern "C" int rsa_group_norm_apply(const rsa_group_norm_apply_params* p, void* stream) {
  if (!p || !p->x_f32 || !p->stats || !p->gamma || !p->beta || (!p->out_hi && !p->out_f32)) return set_error(RSA_E_ARG, "group_norm_apply: null operand");
  if (p->batch < 1 || p->H < 1 || p->W < 1 || p->C < 8 || p->C % 8 || p->groups < 1 || p->C % p->groups || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "group_norm_apply: bad geometry (C a multiple of 8 and of groups)");
  if (!plane_fmt_ok(p->out_fmt)) return set_error(RSA_E_ARG, "group_norm_apply: bad out_fmt");
  if (misaligned16(p->x_f32) || misaligned16(p->skip_f32) || misaligned16(p->out_f32) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "group_norm_apply: operands must be 16-byte aligned");
  const dim3 grid((unsigned)(((int64_t)p->H * p->W + 255) / 256), p->C / 8, p->batch);
  with_fmt(p->out_fmt, [&](auto F) { gn_apply_kernel<decltype(F)::value><<<grid, 256, 0, (hipStream_t)stream>>>(*p); });
  return (int)hipGetLastError();
}

extern "C" int rsa_ea_gate(const rsa_ea_gate_params* p, void* stream) {
  if (!p || !p->g_f32 || !p->x_hi || !p->out_hi) return set_error(RSA_E_ARG, "ea_gate: null operand");
  if (p->batch < 1 || p->H < 1 || p->W < 1 || p->C < 8 || p->C % 8 || p->reserved0 != 0) return set_error(RSA_E_ARG, "ea_gate: bad geometry (C a multiple of 8)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "ea_gate: bad fmt");
  if (misaligned16(p->g_f32) || misaligned16(p->x_hi) || misaligned16(p->x_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "ea_gate: operands must be 16-byte aligned");
  const dim3 grid((unsigned)(((int64_t)p->H * p->W + 255) / 256), p->C / 8, p->batch);
  with_fmt(p->fmt, [&](auto F) { ea_gate_kernel<decltype(F)::value><<<grid, 256, 0, (hipStream_t)stream>>>(*p); });
  return (int)hipGetLastError();
}
