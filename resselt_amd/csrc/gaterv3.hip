// gaterv3.hip — what GateRV3 adds to the kernels of the library (reference resselt/archs/gaterv3/arch.py):
//   rsa_gaterv3_local_gate         MetaGated.local's grouped 3x3 (2 in / 2 out per group) + SimpleGate + the tile sums of `sca`   :642-646
//   rsa_gaterv3_sca_apply          the ordered finish of the mean, sca's 1x1 on it, and  s * a + short  on f32 stream maps       :664-665
//   rsa_gaterv3_channel_attention  the latent Attention: 1..16 heads of 1..64 channels over all tokens, three kernels           :549-584
//   rsa_gaterv3_shortcut           + gamma * nearest-upsampled input on the cropped output                                      :801-802
// All arithmetic f32, no atomics, every sum in an order fixed by the map size alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd_gaterv3.h"

namespace rsa {
namespace {

// ---------------------------------------------------------------------------------------------------------------- local gate
constexpr int LG_TW = RSA_GATERV3_TILE_W, LG_TH = RSA_GATERV3_TILE_H, LG_HW = LG_TW + 2, LG_HH = LG_TH + 2, LG_NPIX = LG_HW * LG_HH;

inline int64_t lg_tiles(int H, int W) { return (int64_t)((W + LG_TW - 1) / LG_TW) * ((H + LG_TH - 1) / LG_TH); }

// grid (tiles, dim / 8, batch), 256 threads: plane pl of s on a 32 x 8 tile.  The 34 x 10 halo of input planes pl (x1's channels) and
// pl + dim / 8 (x2's) goes to LDS as f32 [16 channels][340 pixels], zero outside the map: each halo tile is read from memory once.  The 16
// output channels' weights (18 taps each) and biases go to LDS too; their reads are wave-uniform broadcasts.  A lane owns a pixel: per
// group pair it reads the pair's 18 inputs once and runs both outputs' fma chains.  The tile sums: a butterfly over the wave (the same
// order in every lane), then the four waves' sums added in wave order by one lane per channel.
template <int FMT>
__global__ __launch_bounds__(256) void gaterv3_local_gate_kernel(const rsa_gaterv3_local_gate_params p) {
  __shared__ float xs[16 * LG_NPIX];
  __shared__ float wt[16 * 18];
  __shared__ float bt[16];
  __shared__ float red[4][8];
  const int tid = threadIdx.x;
  const int pl = blockIdx.y, n = blockIdx.z;
  const int P = p.dim >> 3;
  for (int i = tid; i < 16 * 18; i += 256) {
    const int r = i / 18, k = i - r * 18;
    const int o = (r < 8 ? 0 : p.dim - 8) + 8 * pl + r;
    wt[i] = p.weight[(int64_t)o * 18 + k];
  }
  if (tid < 16) bt[tid] = p.bias[(tid < 8 ? 0 : p.dim - 8) + 8 * pl + tid];
  const int tiles_x = (p.W + LG_TW - 1) / LG_TW;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int x0 = tx * LG_TW, y0 = ty * LG_TH;
  const char* hi = (const char*)p.x_hi;
  const char* lo = (const char*)p.x_lo;
  for (int idx = tid; idx < 2 * LG_NPIX; idx += 256) {
    const int half = idx >= LG_NPIX ? 1 : 0;
    const int pix = idx - half * LG_NPIX;
    const int hy = pix / LG_HW, hx = pix - hy * LG_HW;
    const int gy = y0 + hy - 1, gx = x0 + hx - 1;
    float v[8];
    if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
      const int64_t u = (int64_t)n * p.x_batch_stride + (int64_t)(pl + half * P) * p.x_plane_stride + (int64_t)gy * p.W + gx;
      load_unit<FMT>(hi, lo, u * 16, v);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) xs[(half * 8 + j) * LG_NPIX + pix] = v[j];
  }
  __syncthreads();
  const int lx = tid & (LG_TW - 1), ly = tid / LG_TW;
  const int x = x0 + lx, y = y0 + ly;
  const bool inside = x < p.W && y < p.H;
  float acc[16];
#pragma unroll
  for (int g = 0; g < 8; ++g) {  // group pair g: channels 2g, 2g + 1 of the 16 staged ones, outputs the same two
    float in[18];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) in[i * 9 + ky * 3 + kx] = xs[(2 * g + i) * LG_NPIX + (ly + ky) * LG_HW + lx + kx];
#pragma unroll
    for (int r = 2 * g; r < 2 * g + 2; ++r) {
      float a = bt[r];
#pragma unroll
      for (int k = 0; k < 18; ++k) a = fmaf(wt[r * 18 + k], in[k], a);
      acc[r] = a;
    }
  }
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = inside ? acc[j] * acc[8 + j] : 0.f;
  if (inside) {
    const int64_t u = (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride + (int64_t)y * p.W + x;
    store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, u * 16, s);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = s[j];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    s[j] = v;
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[tid >> 6][j] = s[j];
  }
  __syncthreads();
  if (tid < 8) {
    const float t = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    p.workspace[((int64_t)n * gridDim.x + blockIdx.x) * p.dim + 8 * pl + tid] = t;
  }
}

// grid (batch), 256 threads: the mean, then a = gamma0 * (sca_w mean + sca_b) into the workspace's tail.  The tile sums of a channel are
// added as K = 256 / dim consecutive runs of ceil(tiles / K) tiles (one lane per channel and run, ascending tiles within a run), the K
// run sums then in ascending order: an order fixed by (H, W, dim) alone.  Above 256 channels K = 1: one ascending pass per channel.
__global__ __launch_bounds__(256) void gaterv3_sca_vector_kernel(const rsa_gaterv3_sca_apply_params p, int tiles) {
  __shared__ float mean[512];
  __shared__ float runs[256];
  const int tid = threadIdx.x, n = blockIdx.x;
  const float* part = p.workspace + (int64_t)n * tiles * p.dim;
  const float hw = (float)((int64_t)p.H * p.W);
  const int K = p.dim <= 256 ? 256 / p.dim : 1;
  if (K > 1) {
    const int per = (tiles + K - 1) / K;
    if (tid < K * p.dim) {
      const int k = tid / p.dim, c = tid - k * p.dim;
      const int t1 = min((k + 1) * per, tiles);
      float s = 0.f;
      for (int t = k * per; t < t1; ++t) s += part[(int64_t)t * p.dim + c];
      runs[tid] = s;
    }
    __syncthreads();
    if (tid < p.dim) {
      float s = 0.f;
      for (int k = 0; k < K; ++k) s += runs[k * p.dim + tid];
      mean[tid] = s / hw;
    }
  } else {
    for (int c = tid; c < p.dim; c += 256) {
      float s = 0.f;
      for (int t = 0; t < tiles; ++t) s += part[(int64_t)t * p.dim + c];
      mean[c] = s / hw;
    }
  }
  __syncthreads();
  float* a = p.workspace + (int64_t)p.batch * tiles * p.dim + (int64_t)n * p.dim;
  for (int o = tid; o < p.dim; o += 256) {
    float acc = p.sca_b[o];
    const float* w = p.sca_w + (int64_t)o * p.dim;
    for (int c = 0; c < p.dim; ++c) acc = fmaf(w[c], mean[c], acc);
    a[o] = p.gamma0[o] * acc;
  }
}

// grid (ceil(H W / 256), dim / 8, batch), 256 threads: a lane owns one plane unit (8 channels of a pixel = two f32x4 of the stream)
template <int FMT>
__global__ __launch_bounds__(256) void gaterv3_sca_apply_kernel(const rsa_gaterv3_sca_apply_params p, int tiles) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const int pl = blockIdx.y, n = blockIdx.z;
  const float* a = p.workspace + (int64_t)p.batch * tiles * p.dim + (int64_t)n * p.dim + 8 * pl;
  float s[8];
  const int64_t u = (int64_t)n * p.s_batch_stride + (int64_t)pl * p.s_plane_stride + i;
  load_unit<FMT>((const char*)p.s_hi, (const char*)p.s_lo, u * 16, s);
  const int64_t m = ((int64_t)n * (p.dim >> 2) + 2 * pl) * HW + i;
  const f32x4* sh = (const f32x4*)p.short_f32;
  f32x4* out = (f32x4*)p.out_f32;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const f32x4 r = sh[m + g * HW];
    f32x4 z;
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = fmaf(s[4 * g + k], a[4 * g + k], r[k]);
    out[m + g * HW] = z;
  }
}

// ---------------------------------------------------------------------------------------------------------------- channel attention
constexpr int CA_CHUNK = RSA_GATERV3_TOKEN_CHUNK, CA_SUB = 64, CA_MAXD = 64, CA_E = CA_MAXD * CA_MAXD / 256;

inline int64_t ca_chunks(int64_t tokens) { return (tokens + CA_CHUNK - 1) / CA_CHUNK; }
__host__ __device__ inline int64_t ca_rec(int d) { return (int64_t)d * d + 2 * d; }

// The d channels of head h of one operand (q, k or v: `plane0` = its first plane) for CA_SUB tokens from t0 into dst[token][ld], zero past
// the last token: whole units are loaded, the slots of other heads dropped.
template <int FMT>
__device__ __forceinline__ void ca_stage(const rsa_gaterv3_attn_params& p, int n, int plane0, int h, int64_t t0, int64_t tokens, float* dst, int ld) {
  const int d = p.head_dim;
  const int c0 = h * d, first = c0 >> 3, np = ((c0 + d - 1) >> 3) - first + 1;
  for (int e = threadIdx.x; e < np * CA_SUB; e += 256) {
    const int q = e / CA_SUB, t = e - q * CA_SUB;
    float v[8];
    if (t0 + t < tokens) {
      const int64_t u = (int64_t)n * p.qkv_batch_stride + (int64_t)(plane0 + first + q) * p.qkv_plane_stride + t0 + t;
      load_unit<FMT>((const char*)p.qkv_hi, (const char*)p.qkv_lo, u * 16, v);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 8 * (first + q) + j - c0;
      if (c >= 0 && c < d) dst[t * ld + c] = v[j];
    }
  }
}

// grid (chunks, heads, batch), 256 threads: the partial record [G d x d | |q|^2 d | |k|^2 d] of one chunk of 128 tokens, staged 64 tokens
// at a time as [token][d | 1] (odd stride: lanes with consecutive j hit consecutive banks).  A thread owns entries tid, tid + 256, ... of G
// and, below 2 d, one squared norm; each is ONE fma chain from 0 over the chunk's tokens in ascending order.
template <int FMT>
__global__ __launch_bounds__(256) void gaterv3_attn_partial_kernel(const rsa_gaterv3_attn_params p, int chunks) {
  __shared__ float qs[CA_SUB * (CA_MAXD + 1)];
  __shared__ float ks[CA_SUB * (CA_MAXD + 1)];
  const int tid = threadIdx.x;
  const int h = blockIdx.y, n = blockIdx.z;
  const int d = p.head_dim, ld = d | 1, dd = d * d;
  const int64_t tokens = (int64_t)p.H * p.W;
  const int P = p.C >> 3;
  int oi[CA_E], oj[CA_E];
  float acc[CA_E];
#pragma unroll
  for (int e = 0; e < CA_E; ++e) {
    const int idx = tid + 256 * e;
    const int i = idx < dd ? idx / d : 0;
    oi[e] = i, oj[e] = idx < dd ? idx - i * d : 0;
    acc[e] = 0.f;
  }
  float nrm = 0.f;
  const bool own_norm = tid < 2 * d;
  const float* nsrc = tid < d ? qs + tid : ks + (own_norm ? tid - d : 0);
  for (int sub = 0; sub < CA_CHUNK / CA_SUB; ++sub) {
    const int64_t t0 = (int64_t)blockIdx.x * CA_CHUNK + sub * CA_SUB;
    if (t0 >= tokens) break;  // (block-uniform)
    __syncthreads();
    ca_stage<FMT>(p, n, 0, h, t0, tokens, qs, ld);
    ca_stage<FMT>(p, n, P, h, t0, tokens, ks, ld);
    __syncthreads();
    for (int t = 0; t < CA_SUB; ++t) {
      const float* qr = qs + t * ld;
      const float* kr = ks + t * ld;
#pragma unroll
      for (int e = 0; e < CA_E; ++e) acc[e] = fmaf(qr[oi[e]], kr[oj[e]], acc[e]);
      if (own_norm) nrm = fmaf(nsrc[t * ld], nsrc[t * ld], nrm);
    }
  }
  float* rec = p.workspace + (((int64_t)n * p.heads + h) * chunks + blockIdx.x) * ca_rec(d);
#pragma unroll
  for (int e = 0; e < CA_E; ++e) {
    const int idx = tid + 256 * e;
    if (idx < dd) rec[idx] = acc[e];
  }
  if (own_norm) rec[dd + tid] = nrm;
}

// grid (heads, batch), 256 threads: the records added in ascending chunk order, then the softmax rows
__global__ __launch_bounds__(256) void gaterv3_attn_finish_kernel(const rsa_gaterv3_attn_params p, int chunks) {
  __shared__ float g[CA_MAXD * CA_MAXD + 2 * CA_MAXD];
  const int tid = threadIdx.x;
  const int h = blockIdx.x, n = blockIdx.y;
  const int d = p.head_dim, dd = d * d;
  const int64_t rec = ca_rec(d);
  const float* part = p.workspace + ((int64_t)n * p.heads + h) * chunks * rec;
  for (int e = tid; e < rec; e += 256) {
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(int64_t)c * rec + e];
    g[e] = s;
  }
  __syncthreads();
  if (tid >= d) return;
  const float T = p.temperature[h];
  const float nq = fmaxf(sqrtf(g[dd + tid]), 1e-12f);
  const float* row = g + tid * d;
  const float* kn = g + dd + d;
  float m = -INFINITY;
  for (int j = 0; j < d; ++j) m = fmaxf(m, T * row[j] / (nq * fmaxf(sqrtf(kn[j]), 1e-12f)));
  float sum = 0.f;
  for (int j = 0; j < d; ++j) sum += expf(T * row[j] / (nq * fmaxf(sqrtf(kn[j]), 1e-12f)) - m);
  float* A = p.workspace + (int64_t)p.batch * p.heads * chunks * rec + (((int64_t)n * p.heads + h) * d + tid) * d;
  for (int j = 0; j < d; ++j) A[j] = expf(T * row[j] / (nq * fmaxf(sqrtf(kn[j]), 1e-12f)) - m) / sum;
}

// grid (ceil(tokens / 256), C / 8, batch), 256 threads: a lane owns a token of output plane pl.  The plane's 8 channels belong to heads
// h_first..h_last; their v channels are walked once in ascending order, every index but the token is block-uniform (A through scalar loads).
template <int FMT>
__global__ __launch_bounds__(256) void gaterv3_attn_apply_kernel(const rsa_gaterv3_attn_params p, int chunks) {
  const int64_t tokens = (int64_t)p.H * p.W;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= tokens) return;
  const int pl = blockIdx.y, n = blockIdx.z;
  const int d = p.head_dim, P = p.C >> 3;
  const float* A = p.workspace + (int64_t)p.batch * p.heads * chunks * ca_rec(d) + (int64_t)n * p.heads * d * d;
  const int c0 = 8 * pl;
  const int h_first = c0 / d, h_last = (c0 + 7) / d;
  const int v_first = h_first * d, v_end = (h_last + 1) * d;
  int hj[8], ij[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) hj[j] = (c0 + j) / d, ij[j] = (c0 + j) - hj[j] * d;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int vp = v_first >> 3; vp <= (v_end - 1) >> 3; ++vp) {
    float v[8];
    const int64_t u = (int64_t)n * p.qkv_batch_stride + (int64_t)(2 * P + vp) * p.qkv_plane_stride + t;
    load_unit<FMT>((const char*)p.qkv_hi, (const char*)p.qkv_lo, u * 16, v);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int cv = 8 * vp + s;
      if (cv < v_first || cv >= v_end) continue;
      const int hv = cv / d, jv = cv - hv * d;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (hj[j] == hv) acc[j] = fmaf(A[((int64_t)hv * d + ij[j]) * d + jv], v[s], acc[j]);
    }
  }
  const int64_t uo = (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride + t;
  store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, uo * 16, acc);
}

// ---------------------------------------------------------------------------------------------------------------- shortcut
// grid (ceil(h s * w s / 256), C, batch): out = round(out + round(gamma * x)), product and sum kept apart
template <class T>
__global__ __launch_bounds__(256) void gaterv3_shortcut_kernel(const rsa_gaterv3_shortcut_params p) {
  const int ow = p.w * p.scale;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.h * p.scale * ow) return;
  const int Y = (int)(i / ow), X = (int)(i - (int64_t)Y * ow);
  const int c = blockIdx.y, n = blockIdx.z;
  const int64_t img = (int64_t)n * p.C + c;
  const T xv = ((const T*)p.x)[(img * p.h + Y / p.scale) * p.w + X / p.scale];
  T* o = (T*)p.out + (img * p.out_H + Y) * p.out_W + X;
  float prod = p.gamma[c] * (float)xv;
  asm volatile("" : "+v"(prod));  // opaque: the product is rounded on its own, never contracted into an fma with the sum
  *o = (T)((float)*o + (float)(T)prod);
}

int lg_check(int batch, int H, int W, int dim, int fmt, int reserved0, const char* what_geo, const char* what_dim) {
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || dim < 1 || reserved0 != 0 || !plane_fmt_ok(fmt) || (int64_t)H * W > 0x7fffffff)
    return set_error(RSA_E_ARG, what_geo);
  if ((dim & 7) || dim > 512) return set_error(RSA_E_UNSUPPORTED, what_dim);
  return RSA_OK;
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_gaterv3_local_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t dim) {
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || dim < 8 || (dim & 7) || dim > 512 || (int64_t)H * W > 0x7fffffff) return 0;
  return ((int64_t)batch * (lg_tiles(H, W) + 1) * dim * 4 + 15) & ~(int64_t)15;
}

extern "C" int rsa_gaterv3_local_gate(const rsa_gaterv3_local_gate_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gaterv3_local_gate: null params");
  const int rc = lg_check(p->batch, p->H, p->W, p->dim, p->fmt, p->reserved0, "gaterv3_local_gate: bad geometry (fmt 0 or 1, reserved0 0)",
                          "gaterv3_local_gate: dim must be a multiple of 8 up to 512");
  if (rc) return rc;
  if (!p->x_hi || !p->weight || !p->bias || !p->out_hi || !p->workspace) return set_error(RSA_E_ARG, "gaterv3_local_gate: null pointer");
  if (misaligned16(p->x_hi) || misaligned16(p->x_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo) || misaligned16(p->weight) ||
      misaligned16(p->bias) || misaligned16(p->workspace))
    return set_error(RSA_E_ALIGN, "gaterv3_local_gate: the planes, the weights and the workspace must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->x_plane_stride < HW || p->out_plane_stride < HW || p->x_batch_stride < 0 || p->out_batch_stride < 0)
    return set_error(RSA_E_ARG, "gaterv3_local_gate: a plane stride is smaller than the map");
  if (p->x_hi == p->out_hi || (p->x_lo && p->x_lo == p->out_lo)) return set_error(RSA_E_ARG, "gaterv3_local_gate: x and out must not overlap");
  if (p->workspace_bytes < rsa_gaterv3_local_workspace_bytes(p->batch, p->H, p->W, p->dim))
    return set_error(RSA_E_ARG, "gaterv3_local_gate: workspace too small (rsa_gaterv3_local_workspace_bytes)");
  const dim3 grid((unsigned)lg_tiles(p->H, p->W), (unsigned)(p->dim >> 3), (unsigned)p->batch);
  with_fmt(p->fmt, [&](auto F) { hipLaunchKernelGGL(gaterv3_local_gate_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, *p); });
  return launch_status("gaterv3_local_gate: launch failed");
}

extern "C" int rsa_gaterv3_sca_apply(const rsa_gaterv3_sca_apply_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gaterv3_sca_apply: null params");
  const int rc = lg_check(p->batch, p->H, p->W, p->dim, p->fmt, p->reserved0, "gaterv3_sca_apply: bad geometry (fmt 0 or 1, reserved0 0)",
                          "gaterv3_sca_apply: dim must be a multiple of 8 up to 512");
  if (rc) return rc;
  if (!p->s_hi || !p->sca_w || !p->sca_b || !p->gamma0 || !p->short_f32 || !p->out_f32 || !p->workspace)
    return set_error(RSA_E_ARG, "gaterv3_sca_apply: null pointer");
  if (misaligned16(p->s_hi) || misaligned16(p->s_lo) || misaligned16(p->short_f32) || misaligned16(p->out_f32) || misaligned16(p->workspace) ||
      misaligned16(p->sca_w) || misaligned16(p->sca_b) || misaligned16(p->gamma0))
    return set_error(RSA_E_ALIGN, "gaterv3_sca_apply: the planes, the maps, the weights and the workspace must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->s_plane_stride < HW || p->s_batch_stride < 0) return set_error(RSA_E_ARG, "gaterv3_sca_apply: a plane stride is smaller than the map");
  if (p->workspace_bytes < rsa_gaterv3_local_workspace_bytes(p->batch, p->H, p->W, p->dim))
    return set_error(RSA_E_ARG, "gaterv3_sca_apply: workspace too small (rsa_gaterv3_local_workspace_bytes)");
  const int tiles = (int)lg_tiles(p->H, p->W);
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gaterv3_sca_vector_kernel, dim3((unsigned)p->batch), dim3(256), 0, s, *p, tiles);
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(p->dim >> 3), (unsigned)p->batch);
  with_fmt(p->fmt, [&](auto F) { hipLaunchKernelGGL(gaterv3_sca_apply_kernel<decltype(F)::value>, grid, dim3(256), 0, s, *p, tiles); });
  return launch_status("gaterv3_sca_apply: launch failed");
}

extern "C" int64_t rsa_gaterv3_attn_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t heads, int32_t head_dim) {
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || heads < 1 || heads > 16 || head_dim < 1 || head_dim > CA_MAXD || (int64_t)H * W > 0x7fffffff)
    return 0;
  const int64_t chunks = ca_chunks((int64_t)H * W);
  return ((int64_t)batch * heads * (chunks * ca_rec(head_dim) + (int64_t)head_dim * head_dim) * 4 + 15) & ~(int64_t)15;
}

extern "C" int rsa_gaterv3_channel_attention(const rsa_gaterv3_attn_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gaterv3_channel_attention: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->C < 1 || p->heads < 1 || p->head_dim < 1 || p->reserved0 != 0 ||
      !plane_fmt_ok(p->fmt) || (int64_t)p->H * p->W > 0x7fffffff)
    return set_error(RSA_E_ARG, "gaterv3_channel_attention: bad geometry (fmt 0 or 1, reserved0 0)");
  if ((p->C & 7) || p->heads > 16 || p->head_dim > CA_MAXD)
    return set_error(RSA_E_UNSUPPORTED, "gaterv3_channel_attention: C must be a multiple of 8, heads 1..16, head_dim 1..64");
  if ((int64_t)p->heads * p->head_dim != p->C) return set_error(RSA_E_ARG, "gaterv3_channel_attention: heads * head_dim must equal C");
  if (!p->qkv_hi || !p->temperature || !p->out_hi || !p->workspace) return set_error(RSA_E_ARG, "gaterv3_channel_attention: null pointer");
  if (misaligned16(p->qkv_hi) || misaligned16(p->qkv_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo) || misaligned16(p->workspace))
    return set_error(RSA_E_ALIGN, "gaterv3_channel_attention: the planes and the workspace must be 16-byte aligned");
  const int64_t tokens = (int64_t)p->H * p->W;
  if (p->qkv_plane_stride < tokens || p->out_plane_stride < tokens || p->qkv_batch_stride < 0 || p->out_batch_stride < 0)
    return set_error(RSA_E_ARG, "gaterv3_channel_attention: a plane stride is smaller than the map");
  if (p->qkv_hi == p->out_hi || (p->qkv_lo && p->qkv_lo == p->out_lo))
    return set_error(RSA_E_ARG, "gaterv3_channel_attention: qkv and out must not overlap");
  if (p->workspace_bytes < rsa_gaterv3_attn_workspace_bytes(p->batch, p->H, p->W, p->heads, p->head_dim))
    return set_error(RSA_E_ARG, "gaterv3_channel_attention: workspace too small (rsa_gaterv3_attn_workspace_bytes)");
  const int chunks = (int)ca_chunks(tokens);
  const hipStream_t s = (hipStream_t)stream;
  with_fmt(p->fmt, [&](auto F) {
    constexpr int FMT = decltype(F)::value;
    hipLaunchKernelGGL(gaterv3_attn_partial_kernel<FMT>, dim3((unsigned)chunks, (unsigned)p->heads, (unsigned)p->batch), dim3(256), 0, s, *p, chunks);
    hipLaunchKernelGGL(gaterv3_attn_finish_kernel, dim3((unsigned)p->heads, (unsigned)p->batch), dim3(256), 0, s, *p, chunks);
    hipLaunchKernelGGL(gaterv3_attn_apply_kernel<FMT>, dim3((unsigned)((tokens + 255) / 256), (unsigned)(p->C >> 3), (unsigned)p->batch), dim3(256), 0, s,
                       *p, chunks);
  });
  return launch_status("gaterv3_channel_attention: launch failed");
}

extern "C" int rsa_gaterv3_shortcut(const rsa_gaterv3_shortcut_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gaterv3_shortcut: null params");
  if (p->batch < 1 || p->batch > 65535 || p->C < 1 || p->C > 65535 || p->h < 1 || p->w < 1 || p->scale < 1 || p->scale > 8 ||
      (int64_t)p->h * p->scale * p->w * p->scale > 0x7fffffff)
    return set_error(RSA_E_ARG, "gaterv3_shortcut: bad geometry (scale 1..8)");
  if (p->out_H < p->h * p->scale || p->out_W < p->w * p->scale) return set_error(RSA_E_ARG, "gaterv3_shortcut: out is smaller than the scaled input");
  if (!p->x || !p->gamma || !p->out) return set_error(RSA_E_ARG, "gaterv3_shortcut: null pointer");
  const int64_t px = (int64_t)p->h * p->scale * p->w * p->scale;
  const dim3 grid((unsigned)((px + 255) / 256), (unsigned)p->C, (unsigned)p->batch);
  const hipStream_t s = (hipStream_t)stream;
  switch (p->dtype) {
    case RSA_F32: hipLaunchKernelGGL(gaterv3_shortcut_kernel<float>, grid, dim3(256), 0, s, *p); break;
    case RSA_F16: hipLaunchKernelGGL(gaterv3_shortcut_kernel<_Float16>, grid, dim3(256), 0, s, *p); break;
    case RSA_BF16: hipLaunchKernelGGL(gaterv3_shortcut_kernel<__bf16>, grid, dim3(256), 0, s, *p); break;
    default: return set_error(RSA_E_UNSUPPORTED, "gaterv3_shortcut: dtype must be f32, f16 or bf16");
  }
  return launch_status("gaterv3_shortcut: launch failed");
}
