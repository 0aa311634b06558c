// gater.hip — the non-convolution kernels of the GateR path (reference resselt/archs/gater/arch.py):
//   rsa_rmsnorm_torch     nn.RMSNorm over channels, x * rsqrt(mean(x^2) + eps) * weight, f32 stream -> split planes      GatedCNNBlock.forward :122
//   rsa_pixel_unshuffle2  PixelUnshuffle(2) of an f32 map (the Downsample convolution's output -> the next level's stream) Downsample :142-149
//   rsa_f32map_concat     cat(a, b) as one f32 stream map, a given as a plain NCHW tensor (a depth-to-space store)           GateR.forward :199
//   rsa_fla_reduce        focused linear attention, pass 1: per-head  KV = k^T v / n  and  mean(k)  over ALL tokens          FLPVT2.forward :57-79
//   rsa_fla_apply         pass 2: (q KV) / (q . mean(k) + 1e-6) + the 5x5 depthwise convolution of v, per token              FLPVT2.forward :80-83
// The attention arithmetic is f32 whatever the plane format.  The reduction uses no atomics: workgroups write per-chunk partial sums (a chunk
// is FLA_CHUNK consecutive tokens, a constant, so the partials do not depend on the launch geometry) and a second kernel adds them in
// ascending chunk order -- the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

// thread = pixel; grid (ceil(HW / 256), batch).  Two passes over the pixel's channels (the second one hits the cache)
__global__ __launch_bounds__(256) void rmsnorm_torch_kernel(const f32x4* __restrict__ x, int64_t HW, int C, float eps, const float* __restrict__ weight,
                                                            bf16x8* out_hi, bf16x8* out_lo, int64_t plane_stride, int64_t batch_stride, int fmt) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (pix >= HW) return;
  const int p4 = (C + 3) >> 2;
  const f32x4* xb = x + (int64_t)n * p4 * HW;
  float ss = 0.f;
  for (int g = 0; g < p4; ++g) {
    const f32x4 v = xb[(int64_t)g * HW + pix];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (g * 4 + r < C) ss += v[r] * v[r];
  }
  const float inv = rsqrtf(ss / (float)C + eps);
  const int planes = (C + 7) >> 3;
  for (int pl = 0; pl < planes; ++pl) {
    float o[8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int g = pl * 2 + half;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (g < p4) v = xb[(int64_t)g * HW + pix];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = g * 4 + r;
        o[half * 4 + r] = c < C ? (v[r] * inv) * weight[c] : 0.f;
      }
    }
    const int64_t base = (int64_t)n * batch_stride + (int64_t)pl * plane_stride;
    put_unit(out_hi + base, out_lo ? out_lo + base : nullptr, pix, o, fmt);
  }
}

// thread = (half-resolution pixel, group of 4 input channels); grid (ceil(hw / 256), C / 4, batch).  Output channel 4c + 2i + j at (y, x) is
// input channel c at (2y + i, 2x + j): output group c holds the 2x2 block of input channel c.  A pure permutation of f32 values.
__global__ __launch_bounds__(256) void pixel_unshuffle2_kernel(const f32x4* __restrict__ x, int H, int W, int G, f32x4* __restrict__ out) {
  const int h2 = H >> 1, w2 = W >> 1;
  const int64_t hw = (int64_t)h2 * w2;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int g = blockIdx.y, n = blockIdx.z;
  if (pix >= hw) return;
  const int y = (int)(pix / w2), xx = (int)(pix - (int64_t)y * w2);
  const f32x4* src = x + ((int64_t)n * G + g) * H * W;
  const f32x4 a = src[(int64_t)(2 * y) * W + 2 * xx], b = src[(int64_t)(2 * y) * W + 2 * xx + 1];
  const f32x4 c = src[(int64_t)(2 * y + 1) * W + 2 * xx], d = src[(int64_t)(2 * y + 1) * W + 2 * xx + 1];
  f32x4* dst = out + ((int64_t)n * G * 4 + (int64_t)g * 4) * hw + pix;
#pragma unroll
  for (int r = 0; r < 4; ++r) dst[(int64_t)r * hw] = (f32x4){a[r], b[r], c[r], d[r]};
}

// thread = (pixel, output group of 4 channels); grid (ceil(HW / 256), (Ca + Cb) / 4, batch)
__global__ __launch_bounds__(256) void f32map_concat_kernel(const float* __restrict__ a, int Ga, const f32x4* __restrict__ b, int Gb, int64_t HW,
                                                            f32x4* __restrict__ out) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int g = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  f32x4 v;
  if (g < Ga) {
    const float* src = a + ((int64_t)n * Ga * 4 + (int64_t)g * 4) * HW + pix;
    v = (f32x4){src[0], src[HW], src[2 * HW], src[3 * HW]};
  } else {
    v = b[((int64_t)n * Gb + (g - Ga)) * HW + pix];
  }
  out[((int64_t)n * (Ga + Gb) + g) * HW + pix] = v;
}

// ------------------------------------------------------------------------------------------------ focused linear attention
// the operands of both passes (filled by the entry points from their flat argument lists)
struct FlaParams {
  int batch, H, W, head_dim, fmt;
  const void* qkv_hi;  // planes [q | k | v], C / 8 planes each, C = 8 head_dim
  const void* qkv_lo;  // may be NULL
  int64_t qkv_plane_stride, qkv_batch_stride;
  const float* scale;   // [C], before softplus
  const float* factor;  // [C]
  void* workspace;
  int64_t workspace_bytes;
  const float* dwc_weight;  // [head_dim][25]
  const float* dwc_bias;    // [head_dim]
  void* out_hi;
  void* out_lo;
  int64_t out_plane_stride, out_batch_stride;
};

constexpr int FLA_HEADS = 8;
constexpr int FLA_TT = 32;      // tokens a workgroup holds at a time: thread = (token tid % 32, head tid / 32)
constexpr int FLA_CHUNK = 128;  // tokens per partial sum of the reduction (a constant: the partials do not depend on the grid)
constexpr int FLA_TW = 8, FLA_TH = 4;  // the apply pass's token tile

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

// The focusing step of one token's head slice held by thread (t, h): relu + 1e-6, / softplus(scale), ||.||_2 over ALL C channels (the
// eight head slices of a token meet through `red`), per-channel power exp2(f * log2(t)) (t > 0 by construction), renormalised to the first
// norm.  Every thread of the workgroup calls it (four barriers); the eight partial sums are added in head order.
template <int D>
__device__ __forceinline__ void focus_slice(float (&t)[D], const float* __restrict__ scale, const float* __restrict__ factor, int h, int tok,
                                            float (*red)[FLA_TT]) {
  float s0 = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float v = (fmaxf(t[j], 0.f) + 1e-6f) / softplus_f(scale[h * D + j]);
    t[j] = v;
    s0 += v * v;
  }
  red[h][tok] = s0;
  __syncthreads();
  float n0 = 0.f;
#pragma unroll
  for (int k = 0; k < FLA_HEADS; ++k) n0 += red[k][tok];
  __syncthreads();
  float s1 = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float v = exp2f(factor[h * D + j] * log2f(t[j]));
    t[j] = v;
    s1 += v * v;
  }
  red[h][tok] = s1;
  __syncthreads();
  float n1 = 0.f;
#pragma unroll
  for (int k = 0; k < FLA_HEADS; ++k) n1 += red[k][tok];
  __syncthreads();
  const float r = sqrtf(n0) / sqrtf(n1);
#pragma unroll
  for (int j = 0; j < D; ++j) t[j] *= r;
}

template <int D>
__device__ __forceinline__ void load_slice(const bf16x8* hi, const bf16x8* lo, int64_t plane_stride, int plane0, int64_t pix, bool valid, float (&t)[D], int fmt) {
#pragma unroll
  for (int u = 0; u < D / 8; ++u) {
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) get_unit(hi, lo, (int64_t)(plane0 + u) * plane_stride + pix, v, fmt);
#pragma unroll
    for (int j = 0; j < 8; ++j) t[u * 8 + j] = v[j];
  }
}

// Pass 1a.  grid (chunks, batch), 256 threads.  A chunk is FLA_CHUNK tokens in FLA_TT-token rounds: thread (t, h) focuses its slice of k and
// puts it and its slice of v into LDS; then thread (h, a, b) adds k[.][h][a D/8 ..] x v[.][h][b D/4 ..] over the round's tokens in token
// order into its D/8 x D/4 accumulators, and threads c < C add k[.][c].  Tokens past n contribute zeros.
//   partial[n][chunk][8 D D + 8 D]: KV[h][dd][e] then ksum[c]
template <int D>
__global__ __launch_bounds__(256) void fla_reduce_kernel(const FlaParams p, float* __restrict__ partial, int chunks) {
  constexpr int C = FLA_HEADS * D, KB = D / 8, VB = D / 4, REC = C * D + C;
  __shared__ float ks[FLA_TT][C + 1];  // (+ 1: a row per token, the tokens of a wave on different banks)
  __shared__ float vs[FLA_TT][C + 1];
  __shared__ float red[FLA_HEADS][FLA_TT];
  const int tid = threadIdx.x, tok = tid & (FLA_TT - 1), h = tid / FLA_TT;
  const int chunk = blockIdx.x, n = blockIdx.y;
  const int64_t N = (int64_t)p.H * p.W;
  const bf16x8* hi = (const bf16x8*)p.qkv_hi + (int64_t)n * p.qkv_batch_stride;
  const bf16x8* lo = p.qkv_lo ? (const bf16x8*)p.qkv_lo + (int64_t)n * p.qkv_batch_stride : nullptr;
  const int ah = tid / 32, aa = (tid >> 2) & 7, ab = tid & 3;  // accumulation role: head, k block, v block
  float acc[KB][VB];
#pragma unroll
  for (int i = 0; i < KB; ++i)
#pragma unroll
    for (int j = 0; j < VB; ++j) acc[i][j] = 0.f;
  float ksum[2] = {0.f, 0.f};
  for (int r = 0; r < FLA_CHUNK / FLA_TT; ++r) {
    const int64_t pix = (int64_t)chunk * FLA_CHUNK + r * FLA_TT + tok;
    const bool valid = pix < N;
    float k[D], v[D];
    load_slice<D>(hi, lo, p.qkv_plane_stride, C / 8 + h * (D / 8), pix, valid, k, p.fmt);
    load_slice<D>(hi, lo, p.qkv_plane_stride, 2 * (C / 8) + h * (D / 8), pix, valid, v, p.fmt);
    focus_slice<D>(k, p.scale, p.factor, h, tok, red);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      ks[tok][h * D + j] = valid ? k[j] : 0.f;
      vs[tok][h * D + j] = v[j];
    }
    __syncthreads();
#pragma unroll 2
    for (int t = 0; t < FLA_TT; ++t) {
      float kk[KB], vv[VB];
#pragma unroll
      for (int i = 0; i < KB; ++i) kk[i] = ks[t][ah * D + aa * KB + i];
#pragma unroll
      for (int j = 0; j < VB; ++j) vv[j] = vs[t][ah * D + ab * VB + j];
#pragma unroll
      for (int i = 0; i < KB; ++i)
#pragma unroll
        for (int j = 0; j < VB; ++j) acc[i][j] = fmaf(kk[i], vv[j], acc[i][j]);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = tid + q * 256;
      if (c < C)
        for (int t = 0; t < FLA_TT; ++t) ksum[q] += ks[t][c];
    }
    __syncthreads();
  }
  float* dst = partial + ((int64_t)n * chunks + chunk) * REC;
#pragma unroll
  for (int i = 0; i < KB; ++i)
#pragma unroll
    for (int j = 0; j < VB; ++j) dst[(ah * D + aa * KB + i) * D + ab * VB + j] = acc[i][j];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + q * 256;
    if (c < C) dst[C * D + c] = ksum[q];
  }
}

// Pass 1b.  thread = one element of KV / ksum of one image; grid (ceil(REC / 256), batch).  Chunks in ascending order, then * 1 / n.
__global__ __launch_bounds__(256) void fla_finish_kernel(const float* __restrict__ partial, int chunks, int rec, float inv_n, float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (e >= rec) return;
  const float* src = partial + (int64_t)n * chunks * rec + e;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += src[(int64_t)c * rec];
  out[(int64_t)n * rec + e] = s * inv_n;
}

// Pass 2.  grid (token tiles of 8 x 4, batch), 256 threads: thread (t, h).  KV and mean(k) of the image sit in LDS (8 heads x D x D x 4 B:
// 72 KiB at D = 48); a thread focuses its slice of q, multiplies it by its head's KV (all lanes of a wave but two read the same LDS
// word: broadcasts), scales by z and adds the depthwise 5x5 of v.  The filter of channel c is c % D: the same D filters in every head, so the
// weights are workgroup-uniform.  The halo of v is read through the cache, not staged: at C = 384 a 12 x 8 halo tile is 147 KiB of f32.
template <int D>
__global__ __launch_bounds__(256) void fla_apply_kernel(const FlaParams p, const float* __restrict__ kvmean) {
  constexpr int C = FLA_HEADS * D, REC = C * D + C;
  __shared__ __attribute__((aligned(16))) float kv[C * D];
  __shared__ float km[C];
  __shared__ float red[FLA_HEADS][FLA_TT];
  const int tid = threadIdx.x, tok = tid & (FLA_TT - 1), h = tid / FLA_TT;
  const int n = blockIdx.y;
  const int tiles_x = (p.W + FLA_TW - 1) / FLA_TW;
  const int by = (int)blockIdx.x / tiles_x, bx = (int)blockIdx.x - by * tiles_x;
  const int x = bx * FLA_TW + (tok & (FLA_TW - 1)), y = by * FLA_TH + tok / FLA_TW;
  const bool valid = x < p.W && y < p.H;
  const int64_t pix = (int64_t)y * p.W + x;
  const float* src = kvmean + (int64_t)n * REC;
  for (int i = tid; i < C * D / 4; i += 256) ((f32x4*)kv)[i] = ((const f32x4*)src)[i];
  for (int i = tid; i < C; i += 256) km[i] = src[C * D + i];
  const bf16x8* hi = (const bf16x8*)p.qkv_hi + (int64_t)n * p.qkv_batch_stride;
  const bf16x8* lo = p.qkv_lo ? (const bf16x8*)p.qkv_lo + (int64_t)n * p.qkv_batch_stride : nullptr;
  float q[D];
  load_slice<D>(hi, lo, p.qkv_plane_stride, h * (D / 8), pix, valid, q, p.fmt);
  focus_slice<D>(q, p.scale, p.factor, h, tok, red);  // (its barriers also publish kv / km)
  if (!valid) return;
  float den = 1e-6f;
#pragma unroll
  for (int j = 0; j < D; ++j) den = fmaf(q[j], km[h * D + j], den);
  const float z = 1.f / den;
  float o[D];
#pragma unroll
  for (int e = 0; e < D; ++e) o[e] = 0.f;
  const float* kvh = kv + h * D * D;
#pragma unroll
  for (int j = 0; j < D; ++j) {  // (fully unrolled: q and o stay in registers)
    const f32x4* row = (const f32x4*)(kvh + j * D);
#pragma unroll
    for (int e4 = 0; e4 < D / 4; ++e4) {
      const f32x4 w = row[e4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[e4 * 4 + r] = fmaf(q[j], w[r], o[e4 * 4 + r]);
    }
  }
#pragma unroll
  for (int e = 0; e < D; ++e) o[e] = fmaf(o[e], z, p.dwc_bias[e]);
  const int vplane0 = 2 * (C / 8) + h * (D / 8);
#pragma unroll 1
  for (int dy = -2; dy <= 2; ++dy) {
    const int yy = y + dy;
    if ((unsigned)yy >= (unsigned)p.H) continue;
#pragma unroll 1
    for (int dx = -2; dx <= 2; ++dx) {
      const int xx = x + dx;
      if ((unsigned)xx >= (unsigned)p.W) continue;
      const int tap = (dy + 2) * 5 + dx + 2;
      const int64_t np = (int64_t)yy * p.W + xx;
#pragma unroll
      for (int u = 0; u < D / 8; ++u) {
        float v[8];
        get_unit(hi, lo, (int64_t)(vplane0 + u) * p.qkv_plane_stride + np, v, p.fmt);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[u * 8 + j] = fmaf(p.dwc_weight[(u * 8 + j) * 25 + tap], v[j], o[u * 8 + j]);
      }
    }
  }
  bf16x8* ohi = (bf16x8*)p.out_hi + (int64_t)n * p.out_batch_stride;
  bf16x8* olo = p.out_lo ? (bf16x8*)p.out_lo + (int64_t)n * p.out_batch_stride : nullptr;
#pragma unroll
  for (int u = 0; u < D / 8; ++u) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = o[u * 8 + j];
    put_unit(ohi, olo, (int64_t)(h * (D / 8) + u) * p.out_plane_stride + pix, v, p.fmt);
  }
}

int64_t fla_chunks(int64_t tokens) { return (tokens + FLA_CHUNK - 1) / FLA_CHUNK; }
int64_t fla_rec(int d) { return (int64_t)FLA_HEADS * d * d + FLA_HEADS * d; }

int fla_check(const FlaParams* p, const char* what, bool apply) {
  static thread_local char msg[160];
  auto fail = [&](int code, const char* why) {
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    return set_error(code, msg);
  };
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1) return fail(RSA_E_ARG, "bad geometry");
  if (p->head_dim != 24 && p->head_dim != 48) return fail(RSA_E_UNSUPPORTED, "head_dim must be 24 or 48 (eight heads)");
  if (!plane_fmt_ok(p->fmt)) return fail(RSA_E_ARG, "fmt must be an rsa_plane_fmt");
  if (!p->qkv_hi || !p->scale || !p->factor || !p->workspace) return fail(RSA_E_ARG, "null operand");
  const int64_t N = (int64_t)p->H * p->W;
  if (N > 0x7fffffff / 4) return fail(RSA_E_UNSUPPORTED, "map too large");
  if (p->qkv_plane_stride < N) return fail(RSA_E_ARG, "the qkv plane stride is smaller than the map");
  if (p->workspace_bytes < rsa_fla_workspace_bytes(p->batch, (int32_t)N, p->head_dim)) return fail(RSA_E_ARG, "workspace too small (rsa_fla_workspace_bytes)");
  if (misaligned16(p->qkv_hi) || misaligned16(p->qkv_lo) || misaligned16(p->workspace)) return fail(RSA_E_ALIGN, "planes and the workspace must be 16-byte aligned");
  if (apply) {
    if (!p->out_hi || !p->dwc_weight || !p->dwc_bias) return fail(RSA_E_ARG, "null operand");
    if (p->out_plane_stride < N) return fail(RSA_E_ARG, "the output plane stride is smaller than the map");
    if (misaligned16(p->out_hi) || misaligned16(p->out_lo)) return fail(RSA_E_ALIGN, "planes must be 16-byte aligned");
  }
  return RSA_OK;
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_rmsnorm_torch(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, float eps, const float* weight, void* out_hi, void* out_lo,
                                 int64_t out_plane_stride, int64_t out_batch_stride, int32_t fmt, void* stream) {
  if (!x_f32 || !weight || !out_hi || batch < 1 || batch > 65535 || H < 1 || W < 1 || C < 1 || !(eps >= 0.f)) return set_error(RSA_E_ARG, "rmsnorm_torch: bad argument");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "rmsnorm_torch: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  if (out_plane_stride < HW) return set_error(RSA_E_ARG, "rmsnorm_torch: the plane stride is smaller than the map");
  if (misaligned16(x_f32) || misaligned16(out_hi) || misaligned16(out_lo)) return set_error(RSA_E_ALIGN, "rmsnorm_torch: maps must be 16-byte aligned");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "rmsnorm_torch: map too large");
  hipLaunchKernelGGL(rmsnorm_torch_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, (const f32x4*)x_f32, HW, (int)C, eps,
                     weight, (bf16x8*)out_hi, (bf16x8*)out_lo, out_plane_stride, out_batch_stride, (int)fmt);
  return launch_status("rmsnorm_torch: launch failed");
}

extern "C" int rsa_pixel_unshuffle2(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, float* out_f32, void* stream) {
  if (!x_f32 || !out_f32 || batch < 1 || batch > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 4 || (C & 3) || C / 4 > 65535)
    return set_error(RSA_E_ARG, "pixel_unshuffle2: bad argument (even H and W, C a multiple of 4)");
  if (x_f32 == out_f32) return set_error(RSA_E_ARG, "pixel_unshuffle2: not in place");
  if (misaligned16(x_f32) || misaligned16(out_f32)) return set_error(RSA_E_ALIGN, "pixel_unshuffle2: maps must be 16-byte aligned");
  const int64_t hw = (int64_t)(H / 2) * (W / 2);
  if ((hw + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "pixel_unshuffle2: map too large");
  hipLaunchKernelGGL(pixel_unshuffle2_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)(C / 4), (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                     (const f32x4*)x_f32, (int)H, (int)W, (int)(C / 4), (f32x4*)out_f32);
  return launch_status("pixel_unshuffle2: launch failed");
}

extern "C" int rsa_f32map_concat(const float* a_nchw, int32_t Ca, const float* b_map, int32_t Cb, int32_t batch, int32_t H, int32_t W, float* out_map, void* stream) {
  if (!a_nchw || !b_map || !out_map || batch < 1 || batch > 65535 || H < 1 || W < 1 || Ca < 4 || Cb < 4 || (Ca & 3) || (Cb & 3) || (Ca + Cb) / 4 > 65535)
    return set_error(RSA_E_ARG, "f32map_concat: bad argument (channel counts are multiples of 4)");
  if (out_map == a_nchw || out_map == b_map) return set_error(RSA_E_ARG, "f32map_concat: not in place");
  if (misaligned16(b_map) || misaligned16(out_map) || ((uintptr_t)a_nchw & 3)) return set_error(RSA_E_ALIGN, "f32map_concat: maps must be 16-byte aligned");
  const int64_t HW = (int64_t)H * W;
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "f32map_concat: map too large");
  hipLaunchKernelGGL(f32map_concat_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)((Ca + Cb) / 4), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a_nchw,
                     (int)(Ca / 4), (const f32x4*)b_map, (int)(Cb / 4), HW, (f32x4*)out_map);
  return launch_status("f32map_concat: launch failed");
}

// workspace: [batch][REC] finished KV / mean(k), then [batch][chunks][REC] partials (REC = 8 d d + 8 d floats, a multiple of 4)
extern "C" int64_t rsa_fla_workspace_bytes(int32_t batch, int32_t tokens, int32_t head_dim) {
  if (batch < 1 || tokens < 1 || head_dim < 8 || (head_dim & 7) || head_dim > 1024) return 0;
  return (int64_t)batch * (1 + fla_chunks(tokens)) * fla_rec(head_dim) * 4;
}

extern "C" int rsa_fla_reduce(const void* qkv_hi, const void* qkv_lo, int64_t qkv_plane_stride, int64_t qkv_batch_stride, int32_t batch, int32_t H, int32_t W,
                              int32_t head_dim, int32_t fmt, const float* scale, const float* factor, void* workspace, int64_t workspace_bytes, void* stream) {
  FlaParams fp = {};
  fp.batch = batch, fp.H = H, fp.W = W, fp.head_dim = head_dim, fp.fmt = fmt;
  fp.qkv_hi = qkv_hi, fp.qkv_lo = qkv_lo, fp.qkv_plane_stride = qkv_plane_stride, fp.qkv_batch_stride = qkv_batch_stride;
  fp.scale = scale, fp.factor = factor, fp.workspace = workspace, fp.workspace_bytes = workspace_bytes;
  const FlaParams* p = &fp;
  const int vrc = fla_check(p, "fla_reduce", false);
  if (vrc != RSA_OK) return vrc;
  const int64_t N = (int64_t)p->H * p->W;
  const int chunks = (int)fla_chunks(N), rec = (int)fla_rec(p->head_dim);
  float* fin = (float*)p->workspace;
  float* partial = fin + (int64_t)p->batch * rec;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)chunks, (unsigned)p->batch);
  if (p->head_dim == 24)
    hipLaunchKernelGGL(fla_reduce_kernel<24>, grid, dim3(256), 0, s, *p, partial, chunks);
  else
    hipLaunchKernelGGL(fla_reduce_kernel<48>, grid, dim3(256), 0, s, *p, partial, chunks);
  int rc = (int)hipGetLastError();
  if (rc) return set_error(rc, "fla_reduce: launch failed");
  hipLaunchKernelGGL(fla_finish_kernel, dim3((unsigned)((rec + 255) / 256), (unsigned)p->batch), dim3(256), 0, s, partial, chunks, rec, (float)(1.0 / (double)N), fin);
  rc = (int)hipGetLastError();
  return rc ? set_error(rc, "fla_reduce: second stage launch failed") : RSA_OK;
}

extern "C" int rsa_fla_apply(const void* qkv_hi, const void* qkv_lo, int64_t qkv_plane_stride, int64_t qkv_batch_stride, int32_t batch, int32_t H, int32_t W,
                             int32_t head_dim, int32_t fmt, const float* scale, const float* factor, const void* workspace, int64_t workspace_bytes,
                             const float* dwc_weight, const float* dwc_bias, void* out_hi, void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride,
                             void* stream) {
  FlaParams fp = {};
  fp.batch = batch, fp.H = H, fp.W = W, fp.head_dim = head_dim, fp.fmt = fmt;
  fp.qkv_hi = qkv_hi, fp.qkv_lo = qkv_lo, fp.qkv_plane_stride = qkv_plane_stride, fp.qkv_batch_stride = qkv_batch_stride;
  fp.scale = scale, fp.factor = factor, fp.workspace = (void*)workspace, fp.workspace_bytes = workspace_bytes;
  fp.dwc_weight = dwc_weight, fp.dwc_bias = dwc_bias, fp.out_hi = out_hi, fp.out_lo = out_lo;
  fp.out_plane_stride = out_plane_stride, fp.out_batch_stride = out_batch_stride;
  const FlaParams* p = &fp;
  const int vrc = fla_check(p, "fla_apply", true);
  if (vrc != RSA_OK) return vrc;
  const int64_t tiles = (int64_t)((p->W + FLA_TW - 1) / FLA_TW) * ((p->H + FLA_TH - 1) / FLA_TH);
  const dim3 grid((unsigned)tiles, (unsigned)p->batch);
  hipStream_t s = (hipStream_t)stream;
  if (p->head_dim == 24)
    hipLaunchKernelGGL(fla_apply_kernel<24>, grid, dim3(256), 0, s, *p, (const float*)p->workspace);
  else
    hipLaunchKernelGGL(fla_apply_kernel<48>, grid, dim3(256), 0, s, *p, (const float*)p->workspace);
  return launch_status("fla_apply: launch failed");
}
