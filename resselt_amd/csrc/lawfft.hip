// lawfft.hip — what LAWFFT (reference resselt/archs/lawfft/arch.py) adds to the shared convolution, LayerNorm and DFT paths:
//   rsa_lawfft_wincorr     FSAS, windowed: the 8 x 8 circular convolution of q and k per patch and channel, the channel LayerNorm of
//                          it and the product with v, one launch                                                        FSAS.forward :268-306
//   rsa_lawfft_spec_mul    FSAS, whole image: scale * (rfft2(q) . rfft2(k)) on two of rsa_gfisr_dft's spectral maps      :295-298
//   rsa_lawfft_norm_mul    v * LayerNorm_channels(corr) behind rsa_gfisr_dft's inverse                                   :300-302
//   rsa_lawfft_kernel_gen  DynamicLocal's generator: ordered mean over the map, two tiny linear layers with a ReLU       :223-236
//   rsa_lawfft_dyn_dwconv  depthwise k x k with one weight set per sample, optional f32 residuals and f32 output         :238-242
// Why the windowed form is a direct sum and not 8-point DFT products: per output it is 64 f32 FMAs; a thread that owns one row of a
// channel's patch keeps the 8 accumulators and the current row of q and of the rotated k in 24 registers and reads 128 floats of LDS for
// its 512 FMAs (four FMAs per float read, all as ds_read_b128), so the VALU, not the LDS, bounds the inner loop.  Measured at hidden width
// 48 on 512 x 512: 1.7 x the time of its plane traffic (q, k, v read once, out written once) in hi + lo planes.  The
// DFT form would need the 8 x 5 complex half spectrum of q and of k per channel beside the patch (2.5 x the LDS), twiddles and two more
// passes to save a fifth of the multiplies.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd_lawfft.h"

namespace rsa {
namespace {

constexpr int LF_MAXC = 128;
constexpr int LF_ROW = 68;     // floats per channel row of a patch in LDS: 64 pixels + 4, so that the 128-bit reads of two channels miss each other's banks
constexpr int LF_CHUNK = 32;   // channels of q and k staged per pass: 32 channels x 8 rows = one item per thread
constexpr int LF_GEN_PIX = 4096;  // pixels per chunk of the pooling pass
constexpr int LF_GEN_MAXCHUNKS = 64;

// ---- the channel LayerNorm both FSAS forms end in.  One statement of the arithmetic: the statistics are two ascending sums in one f32
// accumulator each, and every product that could be contracted is spelled as the fma it shall be.
__device__ __forceinline__ float lf_rstd(float ss, int C, float eps) { return 1.f / sqrtf(ss / (float)C + eps); }
__device__ __forceinline__ float lf_norm_mul(float x, float mean, float rstd, float w, float b, float v) {
  return v * __fmaf_rn((x - mean) * rstd, w, b);
}

__host__ __device__ inline int lf_planes(int C) { return (C + 7) >> 3; }

// ---- rsa_lawfft_wincorr: a workgroup owns one patch (64 pixels) and all C channels.
//   1. per pass of 32 channels: thread (pixel, plane) stages one unit of q and of k as f32 rows [channel][y][x];
//      thread (channel, y) then holds k's rows rotated by y -- krot[u] = k[(y - u) & 7] is read with the thread's own row index, so every
//      register index below is a constant -- and accumulates corr[y][0..7] over u, then v, ascending; the row goes to s_corr;
//   2. the first wave computes mean and 1 / sqrt(var + eps) of its pixel over the C channels of s_corr, ascending;
//   3. thread (pixel, plane) normalises, multiplies by v and stores the unit; the tail channels of the last plane are zero.
__global__ __launch_bounds__(256) void lf_wincorr_kernel(const rsa_lawfft_wincorr_params p) {
  extern __shared__ __align__(16) float lf_smem[];
  const int planes = lf_planes(p.C);
  float* s_corr = lf_smem;                          // [8 planes][LF_ROW]
  float* s_q = s_corr + planes * 8 * LF_ROW;        // [LF_CHUNK][LF_ROW]
  float* s_k = s_q + LF_CHUNK * LF_ROW;             // [LF_CHUNK][LF_ROW]
  float* s_st = s_k + LF_CHUNK * LF_ROW;            // [2][64]
  const int n = blockIdx.z, tid = threadIdx.x;
  const int pix = tid & 63, grp = tid >> 6;
  const int64_t gpix = (int64_t)(blockIdx.y * 8 + (pix >> 3)) * p.W + blockIdx.x * 8 + (pix & 7);
  const bf16x8* q_hi = (const bf16x8*)p.q_hi + (int64_t)n * p.q_batch_stride;
  const bf16x8* q_lo = p.q_lo ? (const bf16x8*)p.q_lo + (int64_t)n * p.q_batch_stride : nullptr;
  const bf16x8* k_hi = (const bf16x8*)p.k_hi + (int64_t)n * p.k_batch_stride;
  const bf16x8* k_lo = p.k_lo ? (const bf16x8*)p.k_lo + (int64_t)n * p.k_batch_stride : nullptr;

  for (int c0 = 0; c0 < p.C; c0 += LF_CHUNK) {
    __syncthreads();  // the previous pass no longer reads s_q / s_k
    const int pl = (c0 >> 3) + grp;
    if (pl < planes) {
      float a[8], b[8];
      get_unit(q_hi, q_lo, (int64_t)pl * p.q_plane_stride + gpix, a, p.fmt);
      get_unit(k_hi, k_lo, (int64_t)pl * p.k_plane_stride + gpix, b, p.fmt);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s_q[(grp * 8 + j) * LF_ROW + pix] = a[j];
        s_k[(grp * 8 + j) * LF_ROW + pix] = b[j];
      }
    }
    __syncthreads();
    const int cl = tid >> 3, y = tid & 7;
    if (c0 + cl < p.C) {
      const float* qc = s_q + cl * LF_ROW;
      const float* kc = s_k + cl * LF_ROW;
      float acc[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) acc[x] = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const f32x4 q0 = *(const f32x4*)(qc + u * 8), q1 = *(const f32x4*)(qc + u * 8 + 4);
        const int r = (y - u) & 7;
        const f32x4 k0 = *(const f32x4*)(kc + r * 8), k1 = *(const f32x4*)(kc + r * 8 + 4);
        const float qv[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
        const float kv[8] = {k0[0], k0[1], k0[2], k0[3], k1[0], k1[1], k1[2], k1[3]};
#pragma unroll
        for (int v = 0; v < 8; ++v)
#pragma unroll
          for (int x = 0; x < 8; ++x) acc[x] = __fmaf_rn(qv[v], kv[(x - v) & 7], acc[x]);
      }
      float* dst = s_corr + (c0 + cl) * LF_ROW + y * 8;
      *(f32x4*)dst = (f32x4){acc[0], acc[1], acc[2], acc[3]};
      *(f32x4*)(dst + 4) = (f32x4){acc[4], acc[5], acc[6], acc[7]};
    }
  }
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
    for (int c = 0; c < p.C; ++c) s += s_corr[c * LF_ROW + tid];
    const float mean = s / (float)p.C;
    float ss = 0.f;
    for (int c = 0; c < p.C; ++c) {
      const float d = s_corr[c * LF_ROW + tid] - mean;
      ss = __fmaf_rn(d, d, ss);
    }
    s_st[tid] = mean;
    s_st[64 + tid] = lf_rstd(ss, p.C, p.eps);
  }
  __syncthreads();
  const float mean = s_st[pix], rstd = s_st[64 + pix];
  const bf16x8* v_hi = (const bf16x8*)p.v_hi + (int64_t)n * p.v_batch_stride;
  const bf16x8* v_lo = p.v_lo ? (const bf16x8*)p.v_lo + (int64_t)n * p.v_batch_stride : nullptr;
  bf16x8* o_hi = (bf16x8*)p.out_hi + (int64_t)n * p.out_batch_stride;
  bf16x8* o_lo = p.out_lo ? (bf16x8*)p.out_lo + (int64_t)n * p.out_batch_stride : nullptr;
  for (int pl = grp; pl < planes; pl += 4) {
    float v[8], r[8];
    get_unit(v_hi, v_lo, (int64_t)pl * p.v_plane_stride + gpix, v, p.fmt);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = pl * 8 + j;  // uniform
      r[j] = c < p.C ? lf_norm_mul(s_corr[c * LF_ROW + pix], mean, rstd, p.weight[c], p.bias[c], v[j]) : 0.f;
    }
    put_unit(o_hi, o_lo, (int64_t)pl * p.out_plane_stride + gpix, r, p.fmt);
  }
}

size_t lf_wincorr_lds(int C) { return (size_t)(lf_planes(C) * 8 * LF_ROW + 2 * LF_CHUNK * LF_ROW + 128) * sizeof(float); }

// ---- rsa_lawfft_norm_mul: one thread per pixel, three passes over the pixel's units (the second and third hit the cache)
__global__ __launch_bounds__(256) void lf_norm_mul_kernel(const rsa_lawfft_norm_mul_params p) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int n = blockIdx.y, planes = lf_planes(p.C);
  const bf16x8* c_hi = (const bf16x8*)p.corr_hi + (int64_t)n * p.corr_batch_stride;
  const bf16x8* c_lo = p.corr_lo ? (const bf16x8*)p.corr_lo + (int64_t)n * p.corr_batch_stride : nullptr;
  const bf16x8* v_hi = (const bf16x8*)p.v_hi + (int64_t)n * p.v_batch_stride;
  const bf16x8* v_lo = p.v_lo ? (const bf16x8*)p.v_lo + (int64_t)n * p.v_batch_stride : nullptr;
  bf16x8* o_hi = (bf16x8*)p.out_hi + (int64_t)n * p.out_batch_stride;
  bf16x8* o_lo = p.out_lo ? (bf16x8*)p.out_lo + (int64_t)n * p.out_batch_stride : nullptr;
  float s = 0.f;
  for (int pl = 0; pl < planes; ++pl) {
    float a[8];
    get_unit(c_hi, c_lo, (int64_t)pl * p.corr_plane_stride + pix, a, p.corr_fmt);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (pl * 8 + j < p.C) s += a[j];
  }
  const float mean = s / (float)p.C;
  float ss = 0.f;
  for (int pl = 0; pl < planes; ++pl) {
    float a[8];
    get_unit(c_hi, c_lo, (int64_t)pl * p.corr_plane_stride + pix, a, p.corr_fmt);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (pl * 8 + j < p.C) {
        const float d = a[j] - mean;
        ss = __fmaf_rn(d, d, ss);
      }
  }
  const float rstd = lf_rstd(ss, p.C, p.eps);
  for (int pl = 0; pl < planes; ++pl) {
    float a[8], v[8], r[8];
    get_unit(c_hi, c_lo, (int64_t)pl * p.corr_plane_stride + pix, a, p.corr_fmt);
    get_unit(v_hi, v_lo, (int64_t)pl * p.v_plane_stride + pix, v, p.fmt);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = pl * 8 + j;
      r[j] = c < p.C ? lf_norm_mul(a[j], mean, rstd, p.weight[c], p.bias[c], v[j]) : 0.f;
    }
    put_unit(o_hi, o_lo, (int64_t)pl * p.out_plane_stride + pix, r, p.fmt);
  }
}

// ---- rsa_lawfft_spec_mul: one thread per (image, group of four channels, bin).  The real parts of channels 4u .. 4u + 3 are unit u; their
// imaginary parts are flat channels C + 4u .. C + 4u + 3, which straddle two units when C is no multiple of 4.  Stores are per component:
// a unit that holds the last real parts also holds the first imaginary parts of other threads' channels.
__global__ __launch_bounds__(256) void lf_spec_mul_kernel(const rsa_lawfft_spec_mul_params p) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int u = blockIdx.y, n = blockIdx.z;
  const int units = (2 * p.C + 3) >> 2;
  const int64_t base = (int64_t)n * units * HW;
  const f32x4* A = (const f32x4*)p.a + base;
  const f32x4* B = (const f32x4*)p.b + base;
  float* O = p.out + base * 4;
  const int s = p.C & 3, i0 = (p.C + 4 * u) >> 2;  // i0 < units: 4u < C
  const f32x4 ar = A[(int64_t)u * HW + pix], br = B[(int64_t)u * HW + pix];
  const f32x4 a0 = A[(int64_t)i0 * HW + pix], b0 = B[(int64_t)i0 * HW + pix];
  f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
  if (i0 + 1 < units) a1 = A[(int64_t)(i0 + 1) * HW + pix], b1 = B[(int64_t)(i0 + 1) * HW + pix];
  const float ai8[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  const float bi8[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
  float ore[4], oim[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float ai = 0.f, bi = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)  // (s is uniform: a select, not a register index)
      if (s == t) ai = ai8[t + j], bi = bi8[t + j];
    ore[j] = p.scale * (ar[j] * br[j] - ai * bi);
    oim[j] = p.scale * (ar[j] * bi + ai * br[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 4 * u + j;
    if (c < p.C) {
      O[((int64_t)u * HW + pix) * 4 + j] = ore[j];
      const int ci = p.C + c;
      O[((int64_t)(ci >> 2) * HW + pix) * 4 + (ci & 3)] = oim[j];
    }
  }
}

// ---- rsa_lawfft_kernel_gen, pass 1: the sums of one plane's 8 channels over one chunk of pixels.  A thread adds its pixels in ascending
// order, then the 256 partial sums fold in a fixed tree.
__host__ __device__ inline int lf_gen_chunks(int64_t HW) {
  const int64_t c = (HW + LF_GEN_PIX - 1) / LF_GEN_PIX;
  return (int)(c < 1 ? 1 : c > LF_GEN_MAXCHUNKS ? LF_GEN_MAXCHUNKS : c);
}

__global__ __launch_bounds__(256) void lf_pool_kernel(const rsa_lawfft_kernel_gen_params p) {
  __shared__ float s_red[256][9];
  const int64_t HW = (int64_t)p.H * p.W;
  const int chunks = gridDim.x, ck = blockIdx.x, pl = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
  const int64_t len = (HW + chunks - 1) / chunks;
  const int64_t lo = (int64_t)ck * len, hi = lo + len < HW ? lo + len : HW;
  const bf16x8* in_hi = (const bf16x8*)p.in_hi + (int64_t)n * p.in_batch_stride + (int64_t)pl * p.in_plane_stride;
  const bf16x8* in_lo = p.in_lo ? (const bf16x8*)p.in_lo + (int64_t)n * p.in_batch_stride + (int64_t)pl * p.in_plane_stride : nullptr;
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  for (int64_t i = lo + tid; i < hi; i += 256) {
    float v[8];
    get_unit(in_hi, in_lo, i, v, p.fmt);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += v[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s_red[tid][j] = s[j];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int j = 0; j < 8; ++j) s_red[tid][j] += s_red[tid + w][j];
    }
    __syncthreads();
  }
  if (tid < 8) p.workspace[(((int64_t)n * gridDim.y + pl) * chunks + ck) * 8 + tid] = s_red[0][tid];
}

// pass 2: one workgroup of 128 threads per image
__global__ __launch_bounds__(128) void lf_gen_kernel(const rsa_lawfft_kernel_gen_params p, int chunks) {
  __shared__ float s_mean[LF_MAXC], s_h[LF_MAXC];
  const int n = blockIdx.x, c = threadIdx.x, C = p.C, planes = lf_planes(C), kk = p.ksize * p.ksize;
  const int64_t HW = (int64_t)p.H * p.W;
  if (c < C) {
    const float* part = p.workspace + (((int64_t)n * planes + (c >> 3)) * chunks) * 8 + (c & 7);
    float s = 0.f;
    for (int ck = 0; ck < chunks; ++ck) s += part[ck * 8];
    s_mean[c] = s / (float)HW;
  }
  __syncthreads();
  if (c < C) {
    float a = p.b1[c];
    for (int i = 0; i < C; ++i) a = __fmaf_rn(p.w1_t[i * C + c], s_mean[i], a);
    s_h[c] = fmaxf(a, 0.f);
  }
  __syncthreads();
  const int live = C * kk, total = planes * 8 * kk;
  float* out = p.out + (int64_t)n * total;
  for (int o = c; o < total; o += 128) {
    float a = 0.f;
    if (o < live) {
      a = p.b2[o];
      for (int j = 0; j < C; ++j) a = __fmaf_rn(p.w2_t[(int64_t)j * live + o], s_h[j], a);
    }
    out[o] = a;
  }
}

// ---- rsa_lawfft_dyn_dwconv: one thread per (image, plane, pixel); the weights of the workgroup's plane are uniform
template <int K>
__global__ __launch_bounds__(256) void lf_dyn_dwconv_kernel(const rsa_lawfft_dyn_dwconv_params p) {
  constexpr int KK = K * K, R = K / 2;
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int pl = blockIdx.y, n = blockIdx.z, planes = gridDim.y;
  const int y = (int)(pix / p.W), x = (int)(pix - (int64_t)y * p.W);
  const float* w = p.weight + ((int64_t)n * planes + pl) * 8 * KK;
  const bf16x8* in_hi = (const bf16x8*)p.in_hi + (int64_t)n * p.in_batch_stride + (int64_t)pl * p.in_plane_stride;
  const bf16x8* in_lo = p.in_lo ? (const bf16x8*)p.in_lo + (int64_t)n * p.in_batch_stride + (int64_t)pl * p.in_plane_stride : nullptr;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
  for (int dy = 0; dy < K; ++dy)
#pragma unroll
    for (int dx = 0; dx < K; ++dx) {
      const int yy = y + dy - R, xx = x + dx - R;
      if (yy < 0 || yy >= p.H || xx < 0 || xx >= p.W) continue;
      float v[8];
      get_unit(in_hi, in_lo, (int64_t)yy * p.W + xx, v, p.fmt);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = __fmaf_rn(v[j], w[j * KK + dy * K + dx], acc[j]);
    }
  const int p4 = (p.C + 3) >> 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int u4 = 2 * pl + h;
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (u4 < p4) {
      const int64_t off = ((int64_t)n * p4 + u4) * HW + pix;
      if (p.res1) r = ((const f32x4*)p.res1)[off];
      if (p.res2) r += ((const f32x4*)p.res2)[off];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * h + e;
      acc[j] = pl * 8 + j < p.C ? acc[j] + r[e] : 0.f;
    }
    if (p.out_f32 && u4 < p4) ((f32x4*)p.out_f32)[((int64_t)n * p4 + u4) * HW + pix] = (f32x4){acc[4 * h], acc[4 * h + 1], acc[4 * h + 2], acc[4 * h + 3]};
  }
  if (p.out_hi) {
    bf16x8* o_hi = (bf16x8*)p.out_hi + (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride;
    bf16x8* o_lo = p.out_lo ? (bf16x8*)p.out_lo + (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride : nullptr;
    put_unit(o_hi, o_lo, pix, acc, p.fmt);
  }
}

bool lf_geometry_ok(int batch, int H, int W) { return batch >= 1 && batch <= 65535 && H >= 1 && W >= 1; }
bool lf_blocks_ok(int64_t HW) { return (HW + 255) / 256 <= 0x7fffffff; }

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_lawfft_wincorr(const rsa_lawfft_wincorr_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "lawfft_wincorr: null params");
  if (!lf_geometry_ok(p->batch, p->H, p->W) || p->C < 1 || p->reserved0 != 0 || p->reserved1 != 0)
    return set_error(RSA_E_ARG, "lawfft_wincorr: bad geometry (reserved fields 0)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "lawfft_wincorr: bad plane format");
  if ((p->H & 7) || (p->W & 7)) return set_error(RSA_E_ARG, "lawfft_wincorr: H and W must be multiples of 8");
  if (p->C > LF_MAXC) return set_error(RSA_E_UNSUPPORTED, "lawfft_wincorr: C must be 1..128");
  if (p->H / 8 > 65535) return set_error(RSA_E_UNSUPPORTED, "lawfft_wincorr: map too large");
  if (!p->weight || !p->bias || !p->q_hi || !p->k_hi || !p->v_hi || !p->out_hi) return set_error(RSA_E_ARG, "lawfft_wincorr: null operand");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->q_plane_stride < HW || p->k_plane_stride < HW || p->v_plane_stride < HW || p->out_plane_stride < HW)
    return set_error(RSA_E_ARG, "lawfft_wincorr: a plane stride is smaller than the map");
  if (misaligned16(p->q_hi) || misaligned16(p->q_lo) || misaligned16(p->k_hi) || misaligned16(p->k_lo) || misaligned16(p->v_hi) || misaligned16(p->v_lo) ||
      misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "lawfft_wincorr: planes must be 16-byte aligned");
  const dim3 grid(p->W / 8, p->H / 8, p->batch);
  hipLaunchKernelGGL(lf_wincorr_kernel, grid, dim3(256), lf_wincorr_lds(p->C), (hipStream_t)stream, *p);
  return launch_status("lawfft_wincorr: launch failed");
}

extern "C" int rsa_lawfft_spec_mul(const rsa_lawfft_spec_mul_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "lawfft_spec_mul: null params");
  if (!lf_geometry_ok(p->batch, p->H, p->W) || p->C < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "lawfft_spec_mul: bad geometry (reserved0 0)");
  if (p->C > LF_MAXC) return set_error(RSA_E_UNSUPPORTED, "lawfft_spec_mul: C must be 1..128");
  if (!p->a || !p->b || !p->out) return set_error(RSA_E_ARG, "lawfft_spec_mul: null operand");
  if (misaligned16(p->a) || misaligned16(p->b) || misaligned16(p->out)) return set_error(RSA_E_ALIGN, "lawfft_spec_mul: maps must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (!lf_blocks_ok(HW)) return set_error(RSA_E_UNSUPPORTED, "lawfft_spec_mul: map too large");
  const dim3 grid((unsigned)((HW + 255) / 256), (p->C + 3) / 4, p->batch);
  hipLaunchKernelGGL(lf_spec_mul_kernel, grid, dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("lawfft_spec_mul: launch failed");
}

extern "C" int rsa_lawfft_norm_mul(const rsa_lawfft_norm_mul_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "lawfft_norm_mul: null params");
  if (!lf_geometry_ok(p->batch, p->H, p->W) || p->C < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "lawfft_norm_mul: bad geometry (reserved0 0)");
  if (!plane_fmt_ok(p->fmt) || !plane_fmt_ok(p->corr_fmt)) return set_error(RSA_E_ARG, "lawfft_norm_mul: bad plane format");
  if (p->C > LF_MAXC) return set_error(RSA_E_UNSUPPORTED, "lawfft_norm_mul: C must be 1..128");
  if (!p->weight || !p->bias || !p->corr_hi || !p->v_hi || !p->out_hi) return set_error(RSA_E_ARG, "lawfft_norm_mul: null operand");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->corr_plane_stride < HW || p->v_plane_stride < HW || p->out_plane_stride < HW)
    return set_error(RSA_E_ARG, "lawfft_norm_mul: a plane stride is smaller than the map");
  if (misaligned16(p->corr_hi) || misaligned16(p->corr_lo) || misaligned16(p->v_hi) || misaligned16(p->v_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "lawfft_norm_mul: planes must be 16-byte aligned");
  if (!lf_blocks_ok(HW)) return set_error(RSA_E_UNSUPPORTED, "lawfft_norm_mul: map too large");
  const dim3 grid((unsigned)((HW + 255) / 256), p->batch);
  hipLaunchKernelGGL(lf_norm_mul_kernel, grid, dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("lawfft_norm_mul: launch failed");
}

extern "C" int64_t rsa_lawfft_kernel_gen_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
  if (batch < 1 || C < 1 || C > LF_MAXC || H < 1 || W < 1) return -1;
  return (int64_t)batch * lf_planes(C) * lf_gen_chunks((int64_t)H * W) * 8 * (int64_t)sizeof(float);
}

extern "C" int rsa_lawfft_kernel_gen(const rsa_lawfft_kernel_gen_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "lawfft_kernel_gen: null params");
  if (!lf_geometry_ok(p->batch, p->H, p->W) || p->C < 1 || p->reserved0 != 0 || p->reserved1 != 0)
    return set_error(RSA_E_ARG, "lawfft_kernel_gen: bad geometry (reserved fields 0)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "lawfft_kernel_gen: bad plane format");
  if (p->C > LF_MAXC) return set_error(RSA_E_UNSUPPORTED, "lawfft_kernel_gen: C must be 1..128");
  if (p->ksize != 3 && p->ksize != 5) return set_error(RSA_E_UNSUPPORTED, "lawfft_kernel_gen: ksize must be 3 or 5");
  if (!p->w1_t || !p->b1 || !p->w2_t || !p->b2 || !p->workspace || !p->out || !p->in_hi) return set_error(RSA_E_ARG, "lawfft_kernel_gen: null operand");
  if (p->in_plane_stride < (int64_t)p->H * p->W) return set_error(RSA_E_ARG, "lawfft_kernel_gen: the plane stride is smaller than the map");
  if (misaligned16(p->in_hi) || misaligned16(p->in_lo) || misaligned16(p->workspace))
    return set_error(RSA_E_ALIGN, "lawfft_kernel_gen: planes and the workspace must be 16-byte aligned");
  const int chunks = lf_gen_chunks((int64_t)p->H * p->W);
  hipLaunchKernelGGL(lf_pool_kernel, dim3(chunks, lf_planes(p->C), p->batch), dim3(256), 0, (hipStream_t)stream, *p);
  hipLaunchKernelGGL(lf_gen_kernel, dim3(p->batch), dim3(128), 0, (hipStream_t)stream, *p, chunks);
  return launch_status("lawfft_kernel_gen: launch failed");
}

extern "C" int rsa_lawfft_dyn_dwconv(const rsa_lawfft_dyn_dwconv_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "lawfft_dyn_dwconv: null params");
  if (!lf_geometry_ok(p->batch, p->H, p->W) || p->C < 1 || p->reserved0 != 0 || p->reserved1 != 0)
    return set_error(RSA_E_ARG, "lawfft_dyn_dwconv: bad geometry (reserved fields 0)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "lawfft_dyn_dwconv: bad plane format");
  if (p->C > 8 * 65535) return set_error(RSA_E_UNSUPPORTED, "lawfft_dyn_dwconv: too many channels");
  if (p->ksize != 3 && p->ksize != 5) return set_error(RSA_E_UNSUPPORTED, "lawfft_dyn_dwconv: ksize must be 3 or 5");
  if (!p->weight || !p->in_hi || (!p->out_hi && !p->out_f32)) return set_error(RSA_E_ARG, "lawfft_dyn_dwconv: null operand");
  if (p->out_lo && !p->out_hi) return set_error(RSA_E_ARG, "lawfft_dyn_dwconv: out_lo without out_hi");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->in_plane_stride < HW || (p->out_hi && p->out_plane_stride < HW)) return set_error(RSA_E_ARG, "lawfft_dyn_dwconv: a plane stride is smaller than the map");
  if (p->out_hi == p->in_hi) return set_error(RSA_E_ARG, "lawfft_dyn_dwconv: not in place (a pixel reads its neighbours)");
  if (misaligned16(p->in_hi) || misaligned16(p->in_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo) || misaligned16(p->res1) || misaligned16(p->res2) ||
      misaligned16(p->out_f32))
    return set_error(RSA_E_ALIGN, "lawfft_dyn_dwconv: planes and maps must be 16-byte aligned");
  if (!lf_blocks_ok(HW)) return set_error(RSA_E_UNSUPPORTED, "lawfft_dyn_dwconv: map too large");
  const dim3 grid((unsigned)((HW + 255) / 256), lf_planes(p->C), p->batch);
  if (p->ksize == 3)
    hipLaunchKernelGGL(lf_dyn_dwconv_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL(lf_dyn_dwconv_kernel<5>, grid, dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("lawfft_dyn_dwconv: launch failed");
}
