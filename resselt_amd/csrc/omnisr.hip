// omnisr.hip — the kernels of OmniSR (reference resselt/archs/omni/arch.py) that the existing kernels do not cover:
//   rsa_omni_window_attention   softmax(q k^T + B) v over block or grid (dilated) ws x ws windows           :514-596, :824, :842
//   rsa_omni_channel_attention  normalised transposed attention over a window or a stride-ws residue class :682-799
//   rsa_gelu_gate_dwconv        GELU(dw3x3(x1)) * dw3x3(x2), the middle of Gated_Conv_FeedForward         :436-439
//   rsa_omni_gate_scale         MBConv's squeeze-excitation applied: h * g[c]                              :460
//   rsa_esa_conv3x3 / rsa_esa_maxpool / rsa_esa_apply   ESA on its small f32 maps                          :18-46
// Every Linear / 1x1 / 3x3 layer, LayerNorm, the depthwise convolutions of MBConv and of the channel attentions and the SE's mean + MLP run
// on the existing kernels (archs/omnisr/arch.py).  Arithmetic is f32 on split-plane operands; no atomics, so results are deterministic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

constexpr int OM_MAXD = 32;     // channels of a head
constexpr int OM_MAXTOK = 64;   // tokens of a window (ws <= 8) and of a channel-attention chunk
constexpr int OM_MAXHEADS = 8;

// byte offset of (image n, plane pl, pixel pix) in a split-plane buffer
__device__ __forceinline__ int64_t om_off(int64_t n, int64_t batch_stride, int64_t pl, int64_t plane_stride, int64_t pix) {
  return (n * batch_stride + pl * plane_stride + pix) * 16;
}

// ------------------------------------------------------------------------------------------------ window attention
// MFMA form (v_mfma_f32_32x32x16_{bf16,f16}), the fragment orders of DAT's rect_attention_kernel: S^T = K Q^T per 32-key x 32-query tile,
// in-lane online softmax over the keys of a query column (the two lane halves joined by one xor-32 shuffle), O^T += V^T P^T with P taken
// straight from the accumulators.  bf16x3: hi*hi + hi*lo + lo*hi (q / k / v lo planes, P split into hi + residual).
//   accumulator element r of lane (lr = lane % 32, lh = lane / 32): key (or channel) = (r & 3) + 8 (r >> 2) + 4 lh, query = lr
// A workgroup holds NW windows of one head (wave w = window w), adjacent along the inner window index: in block mode NW windows side by
// side along x, in grid mode NW windows whose tokens are NEIGHBOURING pixels (token (r, c) of window (wy, wx) sits at pixel
// (r H/ws + wy, c W/ws + wx)).  The q / k / v units of the NW windows are staged in LDS by the whole workgroup with the window index (grid)
// or the in-window column (block) fastest, so the global reads come in runs of adjacent pixels.  KS = K steps of 16 head channels.

template <int FMT>
__device__ __forceinline__ float om_f16v(__bf16 v) {
  if constexpr (FMT == RSA_PF_F16)
    return (float)__builtin_bit_cast(_Float16, v);
  else
    return (float)v;
}

template <int KS>
struct OmWinCfg {
  static constexpr int NW = KS == 1 ? 4 : 2;  // windows per workgroup
  static constexpr int KROW = 16 * KS + 8;    // bf16 per q / k row (+8: staggers the banks of the fragment reads)
  static constexpr int VROW = OM_MAXTOK + 8;  // bf16 per V^T row (one head channel, 64 keys)
};

template <int KS, int PROD, int FMT>
__global__ __launch_bounds__(64 * OmWinCfg<KS>::NW) void omni_window_attn_kernel(const rsa_omni_attn_params p) {
  constexpr int NW = OmWinCfg<KS>::NW, KROW = OmWinCfg<KS>::KROW, VROW = OmWinCfg<KS>::VROW;
  constexpr int NHL = PROD == 3 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) __bf16 s_q[NHL][NW][OM_MAXTOK * KROW];
  __shared__ __attribute__((aligned(16))) __bf16 s_k[NHL][NW][OM_MAXTOK * KROW];
  __shared__ __attribute__((aligned(16))) __bf16 s_v[NHL][NW][16 * KS * VROW];
  __shared__ float s_bias[225];
  const int ws = p.ws, ntok = ws * ws, nb = 2 * ws - 1;
  const int hp = (p.head_dim + 7) >> 3;
  const int nwx = p.W / ws, gx = (nwx + NW - 1) / NW;
  const int wy = blockIdx.x / gx, wx0 = (blockIdx.x - wy * gx) * NW;
  const int h = blockIdx.y, n = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // zero the images: pad channels, pad tokens (keys >= ntok must meet zero V rows) and absent windows
  {
    uint32_t* zq = (uint32_t*)&s_q[0][0][0];
    for (int i = tid; i < NHL * NW * OM_MAXTOK * KROW / 2; i += 64 * NW) zq[i] = 0u;
    uint32_t* zk = (uint32_t*)&s_k[0][0][0];
    for (int i = tid; i < NHL * NW * OM_MAXTOK * KROW / 2; i += 64 * NW) zk[i] = 0u;
    uint32_t* zv = (uint32_t*)&s_v[0][0][0];
    for (int i = tid; i < NHL * NW * 16 * KS * VROW / 2; i += 64 * NW) zv[i] = 0u;
    if (p.bias_table)
      for (int i = tid; i < nb * nb; i += 64 * NW) s_bias[i] = p.bias_table[i * p.heads + h];
  }
  __syncthreads();
  const char* qkv_hi = (const char*)p.qkv_hi;
  const char* qkv_lo = PROD == 3 ? (const char*)p.qkv_lo : nullptr;
  const int per = NW * ntok;  // units of one plane over the workgroup's windows
  for (int idx = tid; idx < 3 * hp * per; idx += 64 * NW) {
    const int e = idx % per, wp = idx / per;  // wp = which * hp + plane
    const int which = wp / hp, pl = wp - which * hp;
    int w, r, c;
    if (p.grid) {
      w = e % NW;
      c = (e / NW) % ws;
      r = e / (NW * ws);
    } else {
      c = e % ws;
      w = (e / ws) % NW;
      r = e / (ws * NW);
    }
    const int wx = wx0 + w;
    if (wx >= nwx) continue;
    const int y = p.grid ? r * (p.H / ws) + wy : wy * ws + r;
    const int x = p.grid ? c * (p.W / ws) + wx : wx * ws + c;
    const int64_t off = om_off(n, p.qkv_batch_stride, (which * p.heads + h) * hp + pl, p.qkv_plane_stride, (int64_t)y * p.W + x);
    const int tok = r * ws + c;
    const bf16x8 vh = *(const bf16x8*)(qkv_hi + off);
    bf16x8 vl;
    if (PROD == 3) vl = *(const bf16x8*)(qkv_lo + off);
    if (which < 2) {
      __bf16* dst = which == 0 ? &s_q[0][w][tok * KROW + pl * 8] : &s_k[0][w][tok * KROW + pl * 8];
      *(bf16x8*)dst = vh;
      if (PROD == 3) *(bf16x8*)(dst + NW * OM_MAXTOK * KROW) = vl;  // the lo image
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s_v[0][w][(pl * 8 + j) * VROW + tok] = vh[j];
        if (PROD == 3) s_v[NHL - 1][w][(pl * 8 + j) * VROW + tok] = vl[j];
      }
    }
  }
  __syncthreads();
  const int wx = wx0 + wave;
  if (wx >= nwx) return;  // wave-uniform
  const int lr = lane & 31, lh = lane >> 5;
  const int QT = (ntok + 31) >> 5;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  char* out_hi = (char*)p.out_hi;
  char* out_lo = (char*)p.out_lo;
  for (int qt = 0; qt < QT; ++qt) {
    const int q = 32 * qt + lr;
    const bool qvalid = q < ntok;
    const int rq = q / ws, cq = q - (q / ws) * ws;
    bf16x8 qh[KS], ql[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qh[s] = *(const bf16x8*)&s_q[0][wave][q * KROW + (2 * s + lh) * 8];
      ql[s] = PROD == 3 ? *(const bf16x8*)&s_q[NHL - 1][wave][q * KROW + (2 * s + lh) * 8] : zero8;
    }
    float m = -INFINITY, l = 0.f;
    f32x16 ot;
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[r] = 0.f;
    for (int kt = 0; kt < QT; ++kt) {
      f32x16 a;
#pragma unroll
      for (int r = 0; r < 16; ++r) a[r] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int off = (32 * kt + lr) * KROW + (2 * s + lh) * 8;
        const bf16x8 kh = *(const bf16x8*)&s_k[0][wave][off];
        if (PROD == 3) {
          const bf16x8 kl = *(const bf16x8*)&s_k[NHL - 1][wave][off];
          a = mfma32<FMT>(kl, qh[s], a);
          a = mfma32<FMT>(kh, ql[s], a);
        }
        a = mfma32<FMT>(kh, qh[s], a);
      }
      float tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float v = a[r];
        if (key >= ntok) {
          v = -INFINITY;
        } else if (p.bias_table && qvalid) {
          const int rk = key / ws, ck = key - rk * ws;
          v += s_bias[(rq - rk + ws - 1) * nb + (cq - ck + ws - 1)];
        }
        a[r] = v;
        tm = fmaxf(tm, v);
      }
      tm = fmaxf(tm, __shfl_xor(tm, 32));
      const float mn = fmaxf(m, tm);  // finite: key tile 0 always holds keys
      const float alpha = expf(m - mn);
      m = mn;
      l *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        ot[r] *= alpha;
        const float e = expf(a[r] - mn);
        a[r] = e;
        l += e;
      }
      // O^T[channel][query] += V^T P^T; A rows = head channels (lr < 16 KS), K = the tile's keys in the accumulator order
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 vh = zero8, vl = zero8;
        if (lr < 16 * KS) {
          const int k0 = 32 * kt + 16 * s + 4 * lh;
#pragma unroll
          for (int g2 = 0; g2 < 2; ++g2) {
            const bf16x4 th = *(const bf16x4*)&s_v[0][wave][lr * VROW + k0 + 8 * g2];
#pragma unroll
            for (int e = 0; e < 4; ++e) vh[g2 * 4 + e] = th[e];
            if (PROD == 3) {
              const bf16x4 tl = *(const bf16x4*)&s_v[NHL - 1][wave][lr * VROW + k0 + 8 * g2];
#pragma unroll
              for (int e = 0; e < 4; ++e) vl[g2 * 4 + e] = tl[e];
            }
          }
        }
        float e8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e8[j] = a[8 * s + j];
        const bf16x8 ph = pack16<FMT>(e8);
        if (PROD == 3) {
          float r8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) r8[j] = e8[j] - om_f16v<FMT>(ph[j]);
          const bf16x8 pl = pack16<FMT>(r8);
          ot = mfma32<FMT>(vl, ph, ot);
          ot = mfma32<FMT>(vh, pl, ot);
        }
        ot = mfma32<FMT>(vh, ph, ot);
      }
    }
    const float lsum = l + __shfl_xor(l, 32);
    if (!qvalid) continue;
    const float inv = 1.f / lsum;
    const int y = p.grid ? rq * (p.H / ws) + wy : wy * ws + rq;
    const int x = p.grid ? cq * (p.W / ws) + wx : wx * ws + cq;
    const int64_t pix = (int64_t)y * p.W + x;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (g >= hp) break;
      float v4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v4[e] = ot[g * 4 + e] * inv;
      uint32_t hw[2], lw[2];
      split2<FMT>(v4[0], v4[1], hw[0], lw[0]);
      split2<FMT>(v4[2], v4[3], hw[1], lw[1]);
      const int64_t off = om_off(n, p.out_batch_stride, h * hp + g, p.out_plane_stride, pix) + lh * 8;
      *(uint2*)(out_hi + off) = make_uint2(hw[0], hw[1]);
      if (out_lo) *(uint2*)(out_lo + off) = make_uint2(lw[0], lw[1]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ channel attention
struct OmSets {
  int nsets, ntok, chunks;
};
__host__ __device__ __forceinline__ OmSets om_sets(int H, int W, int ws, int grid) {
  OmSets s;
  if (grid) {
    s.nsets = ws * ws;
    s.ntok = (H / ws) * (W / ws);
  } else {
    s.nsets = (H / ws) * (W / ws);
    s.ntok = ws * ws;
  }
  s.chunks = (s.ntok + OM_MAXTOK - 1) / OM_MAXTOK;
  return s;
}
// pixel of token t of set s
__device__ __forceinline__ int64_t om_token_pixel(const rsa_omni_attn_params& p, int s, int t) {
  const int ws = p.ws;
  if (p.grid) {
    const int r0 = s / ws, c0 = s - r0 * ws;
    const int gw = p.W / ws;
    const int i = t / gw, j = t - i * gw;
    return (int64_t)(i * ws + r0) * p.W + (j * ws + c0);
  }
  const int nwx = p.W / ws;
  const int sy = s / nwx, sx = s - sy * nwx;
  const int r = t / ws, c = t - r * ws;
  return (int64_t)(sy * ws + r) * p.W + (sx * ws + c);
}

// grid (chunks, sets * heads, batch), 256 threads: partial[n][set][head][chunk][d*d + 2d] = (q k^T, |q|^2, |k|^2) over the chunk's tokens
template <int FMT>
__global__ __launch_bounds__(256) void omni_chan_gram_kernel(const rsa_omni_attn_params p, OmSets S) {
  __shared__ float sq[OM_MAXTOK][OM_MAXD + 1];
  __shared__ float sk[OM_MAXTOK][OM_MAXD + 1];
  const int chunk = blockIdx.x, sh = blockIdx.y, n = blockIdx.z;
  const int set = sh / p.heads, h = sh - set * p.heads;
  const int d = p.head_dim, hp = (d + 7) >> 3;
  const int t = threadIdx.x;
  if (t < OM_MAXTOK) {
    const int tok = chunk * OM_MAXTOK + t;
    const bool live = tok < S.ntok;
    const int64_t pix = live ? om_token_pixel(p, set, tok) : 0;
#pragma unroll
    for (int pl = 0; pl < OM_MAXD / 8; ++pl) {
      float a[8], b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.f;
      if (pl < hp && live) {
        load_unit<FMT>((const char*)p.qkv_hi, (const char*)p.qkv_lo, om_off(n, p.qkv_batch_stride, h * hp + pl, p.qkv_plane_stride, pix), a);
        load_unit<FMT>((const char*)p.qkv_hi, (const char*)p.qkv_lo, om_off(n, p.qkv_batch_stride, (p.heads + h) * hp + pl, p.qkv_plane_stride, pix), b);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) sq[t][pl * 8 + j] = a[j], sk[t][pl * 8 + j] = b[j];
    }
  }
  __syncthreads();
  const int E = d * d + 2 * d;
  float* part = p.workspace + ((((int64_t)n * S.nsets + set) * p.heads + h) * S.chunks + chunk) * E;
  for (int e = t; e < E; e += 256) {
    float s = 0.f;
    if (e < d * d) {
      const int c1 = e / d, c2 = e - c1 * d;
      for (int k = 0; k < OM_MAXTOK; ++k) s = fmaf(sq[k][c1], sk[k][c2], s);
    } else if (e < d * d + d) {
      const int c = e - d * d;
      for (int k = 0; k < OM_MAXTOK; ++k) s = fmaf(sq[k][c], sq[k][c], s);
    } else {
      const int c = e - d * d - d;
      for (int k = 0; k < OM_MAXTOK; ++k) s = fmaf(sk[k][c], sk[k][c], s);
    }
    part[e] = s;
  }
}

// grid (sets * heads, batch), 256 threads: the chunks summed in order, then A = softmax_row(T * G / (max(|q|, eps) max(|k|, eps)))
__global__ __launch_bounds__(256) void omni_chan_finish_kernel(const rsa_omni_attn_params p, OmSets S) {
  __shared__ float g[OM_MAXD * OM_MAXD + 2 * OM_MAXD];
  const int sh = blockIdx.x, n = blockIdx.y;
  const int set = sh / p.heads, h = sh - set * p.heads;
  const int d = p.head_dim, E = d * d + 2 * d;
  const float* part = p.workspace + (((int64_t)n * S.nsets + set) * p.heads + h) * (int64_t)S.chunks * E;
  for (int e = threadIdx.x; e < E; e += 256) {
    float s = 0.f;
    for (int k = 0; k < S.chunks; ++k) s += part[(int64_t)k * E + e];
    g[e] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x >= d) return;
  const int c1 = threadIdx.x;
  const float T = p.temperature[h];
  const float nq = fmaxf(sqrtf(g[d * d + c1]), 1e-12f);
  float* A = p.workspace + (int64_t)p.batch * S.nsets * p.heads * S.chunks * E + (((int64_t)n * S.nsets + set) * p.heads + h) * d * d + c1 * d;
  float mx = -INFINITY;
  for (int c2 = 0; c2 < d; ++c2) {
    const float nk = fmaxf(sqrtf(g[d * d + d + c2]), 1e-12f);
    const float v = g[c1 * d + c2] / (nq * nk) * T;
    A[c2] = v;
    mx = fmaxf(mx, v);
  }
  float sum = 0.f;
  for (int c2 = 0; c2 < d; ++c2) {
    const float e = expf(A[c2] - mx);
    A[c2] = e;
    sum += e;
  }
  const float inv = 1.f / sum;
  for (int c2 = 0; c2 < d; ++c2) A[c2] *= inv;
}

// grid (ceil(HW / 256), heads, batch): thread = pixel; out = A[set(pixel)] v
template <int FMT>
__global__ __launch_bounds__(256) void omni_chan_apply_kernel(const rsa_omni_attn_params p, OmSets S) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int h = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  const int ws = p.ws, d = p.head_dim, hp = (d + 7) >> 3;
  const int y = (int)(pix / p.W), x = (int)(pix - (int64_t)y * p.W);
  const int set = p.grid ? (y % ws) * ws + (x % ws) : (y / ws) * (p.W / ws) + (x / ws);
  const int E = d * d + 2 * d;
  const float* A = p.workspace + (int64_t)p.batch * S.nsets * p.heads * S.chunks * E + (((int64_t)n * S.nsets + set) * p.heads + h) * d * d;
  float v[OM_MAXD];
#pragma unroll
  for (int pl = 0; pl < OM_MAXD / 8; ++pl) {
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = 0.f;
    if (pl < hp) load_unit<FMT>((const char*)p.qkv_hi, (const char*)p.qkv_lo, om_off(n, p.qkv_batch_stride, (2 * p.heads + h) * hp + pl, p.qkv_plane_stride, pix), a);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[pl * 8 + j] = a[j];
  }
#pragma unroll
  for (int pl = 0; pl < OM_MAXD / 8; ++pl) {
    if (pl < hp) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c1 = pl * 8 + j;
        float s = 0.f;
        if (c1 < d) {
#pragma unroll
          for (int c2 = 0; c2 < OM_MAXD; ++c2)
            if (c2 < d) s = fmaf(A[c1 * d + c2], v[c2], s);
        }
        o[j] = s;
      }
      store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, om_off(n, p.out_batch_stride, h * hp + pl, p.out_plane_stride, pix), o);
    }
  }
}

// window mode with <= 64 tokens per window: the whole attention in one workgroup per (window, head, image) -- q, k, v in LDS, the Gram
// matrix and the norms, the row softmax into A (LDS), then A v; nothing goes through the workspace
template <int FMT>
__global__ __launch_bounds__(256) void omni_chan_window_kernel(const rsa_omni_attn_params p) {
  __shared__ float sq[OM_MAXTOK][OM_MAXD + 1];
  __shared__ float sk[OM_MAXTOK][OM_MAXD + 1];
  __shared__ float sv[OM_MAXTOK][OM_MAXD + 1];
  __shared__ float g[OM_MAXD * OM_MAXD + 2 * OM_MAXD];
  __shared__ float sa[OM_MAXD][OM_MAXD + 1];
  const int set = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
  const int d = p.head_dim, hp = (d + 7) >> 3, ntok = p.ws * p.ws;
  const int t = threadIdx.x;
  const char* qhi = (const char*)p.qkv_hi;
  const char* qlo = (const char*)p.qkv_lo;
  if (t < OM_MAXTOK) {
    const bool live = t < ntok;
    const int64_t pix = live ? om_token_pixel(p, set, t) : 0;
#pragma unroll
    for (int pl = 0; pl < OM_MAXD / 8; ++pl) {
      float a[8], b[8], c[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = b[j] = c[j] = 0.f;
      if (pl < hp && live) {
        load_unit<FMT>(qhi, qlo, om_off(n, p.qkv_batch_stride, h * hp + pl, p.qkv_plane_stride, pix), a);
        load_unit<FMT>(qhi, qlo, om_off(n, p.qkv_batch_stride, (p.heads + h) * hp + pl, p.qkv_plane_stride, pix), b);
        load_unit<FMT>(qhi, qlo, om_off(n, p.qkv_batch_stride, (2 * p.heads + h) * hp + pl, p.qkv_plane_stride, pix), c);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) sq[t][pl * 8 + j] = a[j], sk[t][pl * 8 + j] = b[j], sv[t][pl * 8 + j] = c[j];
    }
  }
  __syncthreads();
  const int E = d * d + 2 * d;
  for (int e = t; e < E; e += 256) {
    float s = 0.f;
    if (e < d * d) {
      const int c1 = e / d, c2 = e - c1 * d;
      for (int k = 0; k < OM_MAXTOK; ++k) s = fmaf(sq[k][c1], sk[k][c2], s);
    } else if (e < d * d + d) {
      const int c = e - d * d;
      for (int k = 0; k < OM_MAXTOK; ++k) s = fmaf(sq[k][c], sq[k][c], s);
    } else {
      const int c = e - d * d - d;
      for (int k = 0; k < OM_MAXTOK; ++k) s = fmaf(sk[k][c], sk[k][c], s);
    }
    g[e] = s;
  }
  __syncthreads();
  if (t < d) {
    const float T = p.temperature[h];
    const float nq = fmaxf(sqrtf(g[d * d + t]), 1e-12f);
    float mx = -INFINITY;
    for (int c2 = 0; c2 < d; ++c2) {
      const float v = g[t * d + c2] / (nq * fmaxf(sqrtf(g[d * d + d + c2]), 1e-12f)) * T;
      sa[t][c2] = v;
      mx = fmaxf(mx, v);
    }
    float sum = 0.f;
    for (int c2 = 0; c2 < d; ++c2) {
      const float e = expf(sa[t][c2] - mx);
      sa[t][c2] = e;
      sum += e;
    }
    const float inv = 1.f / sum;
    for (int c2 = 0; c2 < d; ++c2) sa[t][c2] *= inv;
  }
  __syncthreads();
  const int tok = t & (OM_MAXTOK - 1), pl = t >> 6;  // 64 tokens x 4 planes
  if (tok >= ntok || pl >= hp) return;
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c1 = pl * 8 + j;
    float s = 0.f;
    if (c1 < d)
      for (int c2 = 0; c2 < d; ++c2) s = fmaf(sa[c1][c2], sv[tok][c2], s);
    o[j] = s;
  }
  store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, om_off(n, p.out_batch_stride, h * hp + pl, p.out_plane_stride, om_token_pixel(p, set, tok)), o);
}

// ------------------------------------------------------------------------------------------------ gated FFN middle
// grid (ceil(HW / 256), planes, batch): thread = (pixel, output plane); reads plane pl (x1) and plane planes + pl (x2) with a 1-pixel halo
template <int FMT>
__global__ __launch_bounds__(256) void gelu_gate_dwconv_kernel(const rsa_gelu_gate_dwconv_params p) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pl = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  const int y = (int)(pix / p.W), x = (int)(pix - (int64_t)y * p.W);
  const float* w1 = p.weight + (int64_t)pl * 8 * 9;
  const float* w2 = p.weight + (int64_t)(p.planes + pl) * 8 * 9;
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    if (yy < 0 || yy >= p.H || xx < 0 || xx >= p.W) continue;
    const int64_t q = (int64_t)yy * p.W + xx;
    float u[8], v[8];
    load_unit<FMT>((const char*)p.in_hi, (const char*)p.in_lo, om_off(n, p.in_batch_stride, pl, p.in_plane_stride, q), u);
    load_unit<FMT>((const char*)p.in_hi, (const char*)p.in_lo, om_off(n, p.in_batch_stride, p.planes + pl, p.in_plane_stride, q), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = fmaf(w1[j * 9 + tap], u[j], a[j]);
      b[j] = fmaf(w2[j * 9 + tap], v[j], b[j]);
    }
  }
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = gelu_erf(a[j]) * b[j];
  store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, om_off(n, p.out_batch_stride, pl, p.out_plane_stride, pix), o);
}

// ------------------------------------------------------------------------------------------------ SE apply
template <int FMT>
__global__ __launch_bounds__(256) void omni_gate_scale_kernel(const char* ihi, const char* ilo, int64_t plane_stride, int64_t batch_stride, int64_t HW,
                                                              int planes, const float* gate, char* ohi, char* olo) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pl = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  const int64_t off = om_off(n, batch_stride, pl, plane_stride, pix);
  const float* g = gate + ((int64_t)n * planes + pl) * 8;
  float v[8];
  load_unit<FMT>(ihi, ilo, off, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] *= g[j];
  store_unit<FMT>(ohi, olo, off, v);
}

// ------------------------------------------------------------------------------------------------ ESA
// f32 NCHW4c element (n, c, pixel) of a map with p4 channel groups
__device__ __forceinline__ int64_t m4(int64_t n, int p4, int c, int64_t HW, int64_t pix) { return ((n * p4 + (c >> 2)) * HW + pix) * 4 + (c & 3); }

// grid (ceil(HWout / 256), cout, batch)
__global__ __launch_bounds__(256) void esa_conv_kernel(const rsa_esa_conv_params p) {
  const int64_t HWo = (int64_t)p.Hout * p.Wout, HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int co = blockIdx.y, n = blockIdx.z;
  if (pix >= HWo) return;
  const int oy = (int)(pix / p.Wout), ox = (int)(pix - (int64_t)oy * p.Wout);
  const int p4i = (p.cin + 3) >> 2, p4o = (p.cout + 3) >> 2;
  float acc = p.bias[co];
  for (int ci = 0; ci < p.cin; ++ci) {
    const float* w = p.weight + ((int64_t)co * p.cin + ci) * 9;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int iy = oy * p.stride - p.pad + tap / 3, ix = ox * p.stride - p.pad + tap % 3;
      if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) continue;
      acc = fmaf(w[tap], p.in[m4(n, p4i, ci, HW, (int64_t)iy * p.W + ix)], acc);
    }
  }
  p.out[m4(n, p4o, co, HWo, pix)] = acc;
}

// grid (ceil(HWout / 256), C, batch)
__global__ __launch_bounds__(256) void esa_maxpool_kernel(const float* in, int C, int H, int W, int Hout, int Wout, float* out) {
  const int64_t HWo = (int64_t)Hout * Wout, HW = (int64_t)H * W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y, n = blockIdx.z;
  if (pix >= HWo) return;
  const int oy = (int)(pix / Wout), ox = (int)(pix - (int64_t)oy * Wout);
  const int p4 = (C + 3) >> 2;
  float m = -INFINITY;
  for (int ky = 0; ky < 7; ++ky)
    for (int kx = 0; kx < 7; ++kx) m = fmaxf(m, in[m4(n, p4, c, HW, (int64_t)(oy * 3 + ky) * W + ox * 3 + kx)]);
  out[m4(n, p4, c, HWo, pix)] = m;
}

constexpr int ESA_MAXF = 32, ESA_MAXC = 128;

// grid (ceil(HW / 256), batch): thread = pixel
template <int FMT>
__global__ __launch_bounds__(256) void esa_apply_kernel(const rsa_esa_apply_params p) {
  __shared__ float s_wf[ESA_MAXF * ESA_MAXF], s_bf[ESA_MAXF], s_w4[ESA_MAXC * ESA_MAXF], s_b4[ESA_MAXC];
  const int f = p.f, C = p.C;
  for (int i = threadIdx.x; i < f * f; i += 256) s_wf[i] = p.wf[i];
  for (int i = threadIdx.x; i < C * f; i += 256) s_w4[i] = p.w4[i];
  for (int i = threadIdx.x; i < f; i += 256) s_bf[i] = p.bf[i];
  for (int i = threadIdx.x; i < C; i += 256) s_b4[i] = p.b4[i];
  __syncthreads();
  const int64_t HW = (int64_t)p.H * p.W, HWc = (int64_t)p.Hc * p.Wc;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (pix >= HW) return;
  const int y = (int)(pix / p.W), x = (int)(pix - (int64_t)y * p.W);
  // F.interpolate(bilinear, align_corners=False): src = max(scale * (d + 0.5) - 0.5, 0), scale = in / out
  const float sy = fmaxf((float)p.Hc / (float)p.H * ((float)y + 0.5f) - 0.5f, 0.f);
  const float sx = fmaxf((float)p.Wc / (float)p.W * ((float)x + 0.5f) - 0.5f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < p.Hc - 1 ? 1 : 0), x1 = x0 + (x0 < p.Wc - 1 ? 1 : 0);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const int pf = (f + 3) >> 2;
  float c1[ESA_MAXF], u[ESA_MAXF];
#pragma unroll
  for (int k = 0; k < ESA_MAXF; ++k) c1[k] = k < f ? p.c1[m4(n, pf, k, HW, pix)] : 0.f;
#pragma unroll
  for (int k = 0; k < ESA_MAXF; ++k) {
    if (k < f) {
      const float a = p.c3[m4(n, pf, k, HWc, (int64_t)y0 * p.Wc + x0)], b = p.c3[m4(n, pf, k, HWc, (int64_t)y0 * p.Wc + x1)];
      const float c = p.c3[m4(n, pf, k, HWc, (int64_t)y1 * p.Wc + x0)], d = p.c3[m4(n, pf, k, HWc, (int64_t)y1 * p.Wc + x1)];
      float s = (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
      float cf = s_bf[k];
#pragma unroll
      for (int i = 0; i < ESA_MAXF; ++i)
        if (i < f) cf = fmaf(s_wf[k * f + i], c1[i], cf);
      u[k] = s + cf;
    } else {
      u[k] = 0.f;
    }
  }
  const int p4 = (C + 3) >> 2, planes = (C + 7) >> 3;
  for (int pl = 0; pl < planes; ++pl) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = pl * 8 + j;
      float v = 0.f;
      if (c < C) {
        float s = s_b4[c];
#pragma unroll
        for (int k = 0; k < ESA_MAXF; ++k)
          if (k < f) s = fmaf(s_w4[c * f + k], u[k], s);
        v = p.x[m4(n, p4, c, HW, pix)] * sigmoid_exact(s);
      }
      o[j] = v;
      if (c < 4 * p4) p.out[m4(n, p4, c, HW, pix)] = v;
    }
    if (p.out_hi) store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, om_off(n, p.out_batch_stride, pl, p.out_plane_stride, pix), o);
  }
}

int om_planes_ok(const void* hi, const void* lo, int64_t plane_stride, int64_t batch_stride, int64_t HW, int planes) {
  if (misaligned16(hi) || misaligned16(lo)) return RSA_E_ALIGN;
  if (plane_stride < HW || batch_stride < (int64_t)planes * plane_stride) return RSA_E_ARG;
  return RSA_OK;
}

int om_attn_check(const rsa_omni_attn_params* p, const char* who, bool channel) {
  if (p == nullptr) return set_error(RSA_E_ARG, who);
  if (p->batch < 1 || p->batch > 65535 || p->ws < 1 || p->H < p->ws || p->W < p->ws || p->H % p->ws || p->W % p->ws || (p->grid != 0 && p->grid != 1))
    return set_error(RSA_E_ARG, "omni attention: bad geometry (H, W positive multiples of ws, grid 0 or 1)");
  if (p->heads < 1 || p->heads > OM_MAXHEADS || p->head_dim < 1 || p->head_dim > OM_MAXD)
    return set_error(RSA_E_UNSUPPORTED, "omni attention: heads 1..8 and head_dim 1..32");
  if (!channel && (p->ws < 2 || p->ws * p->ws > OM_MAXTOK)) return set_error(RSA_E_UNSUPPORTED, "omni window attention: ws must be 2..8");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "omni attention: bad plane format");
  if (!p->qkv_hi || !p->out_hi || (p->out_lo && !p->out_hi)) return set_error(RSA_E_ARG, "omni attention: null operand");
  const bool one_launch = !p->grid && p->ws * p->ws <= OM_MAXTOK;  // window-mode channel attention needs no workspace
  if (channel ? (!p->temperature || (!p->workspace && !one_launch) || p->bias_table) : (p->temperature || p->workspace))
    return set_error(RSA_E_ARG, "omni attention: temperature / workspace belong to the channel attention, bias_table to the window attention");
  const int hp = (p->head_dim + 7) >> 3;
  const int64_t HW = (int64_t)p->H * p->W;
  if (HW > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "omni attention: map too large");
  int rc = om_planes_ok(p->qkv_hi, p->qkv_lo, p->qkv_plane_stride, p->qkv_batch_stride, HW, 3 * p->heads * hp);
  if (rc == RSA_OK) rc = om_planes_ok(p->out_hi, p->out_lo, p->out_plane_stride, p->out_batch_stride, HW, p->heads * hp);
  if (rc != RSA_OK) return set_error(rc, "omni attention: planes misaligned or strides smaller than the map");
  return RSA_OK;
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_omni_window_attention(const rsa_omni_attn_params* p, void* stream) {
  const int rc0 = om_attn_check(p, "omni_window_attention: null params", false);
  if (rc0 != RSA_OK) return rc0;
  const int64_t nwin = (int64_t)(p->H / p->ws) * (p->W / p->ws);
  if (nwin > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "omni_window_attention: too many windows");
  hipStream_t s = (hipStream_t)stream;
  const int nwx = p->W / p->ws, nwy = p->H / p->ws;
  const int ks = p->head_dim <= 16 ? 1 : 2;
  const int nw = ks == 1 ? OmWinCfg<1>::NW : OmWinCfg<2>::NW;
  const dim3 grid((unsigned)((int64_t)nwy * ((nwx + nw - 1) / nw)), (unsigned)p->heads, (unsigned)p->batch);
  const bool f16 = p->fmt == RSA_PF_F16, three = p->qkv_lo != nullptr;
#define OM_WGO(KS, PROD, FMT) hipLaunchKernelGGL((omni_window_attn_kernel<KS, PROD, FMT>), grid, dim3(64 * OmWinCfg<KS>::NW), 0, s, *p)
  if (ks == 1) {
    if (f16) { if (three) OM_WGO(1, 3, RSA_PF_F16); else OM_WGO(1, 1, RSA_PF_F16); }
    else { if (three) OM_WGO(1, 3, RSA_PF_BF16); else OM_WGO(1, 1, RSA_PF_BF16); }
  } else {
    if (f16) { if (three) OM_WGO(2, 3, RSA_PF_F16); else OM_WGO(2, 1, RSA_PF_F16); }
    else { if (three) OM_WGO(2, 3, RSA_PF_BF16); else OM_WGO(2, 1, RSA_PF_BF16); }
  }
#undef OM_WGO
  return launch_status("omni_window_attention: launch failed");
}

extern "C" int64_t rsa_omni_channel_attn_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t ws, int32_t heads, int32_t head_dim, int32_t grid) {
  if (batch < 1 || ws < 1 || H < ws || W < ws || H % ws || W % ws || heads < 1 || heads > OM_MAXHEADS || head_dim < 1 || head_dim > OM_MAXD ||
      (grid != 0 && grid != 1))
    return RSA_E_ARG;
  if (!grid && ws * ws <= OM_MAXTOK) return 0;  // one launch per window, no workspace
  const OmSets S = om_sets(H, W, ws, grid);
  const int64_t E = (int64_t)head_dim * head_dim + 2 * head_dim;
  return ((int64_t)batch * S.nsets * heads * S.chunks * E + (int64_t)batch * S.nsets * heads * head_dim * head_dim) * 4;
}

extern "C" int rsa_omni_channel_attention(const rsa_omni_attn_params* p, void* stream) {
  const int rc0 = om_attn_check(p, "omni_channel_attention: null params", true);
  if (rc0 != RSA_OK) return rc0;
  const OmSets S = om_sets(p->H, p->W, p->ws, p->grid);
  if ((int64_t)S.nsets * p->heads > 0x7fffffff || S.chunks > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "omni_channel_attention: too many sets");
  hipStream_t s = (hipStream_t)stream;
  if (!p->grid && p->ws * p->ws <= OM_MAXTOK) {
    const dim3 gw((unsigned)S.nsets, (unsigned)p->heads, (unsigned)p->batch);
    with_fmt(p->fmt, [&](auto F) {
      hipLaunchKernelGGL(omni_chan_window_kernel<decltype(F)::value>, gw, dim3(256), 0, s, *p);
    });
    return launch_status("omni_channel_attention: launch failed");
  }
  const int64_t HW = (int64_t)p->H * p->W;
  const dim3 g1((unsigned)S.chunks, (unsigned)(S.nsets * p->heads), (unsigned)p->batch);
  const dim3 g2((unsigned)(S.nsets * p->heads), (unsigned)p->batch);
  const dim3 g3((unsigned)((HW + 255) / 256), (unsigned)p->heads, (unsigned)p->batch);
  with_fmt(p->fmt, [&](auto F) {
    hipLaunchKernelGGL(omni_chan_gram_kernel<decltype(F)::value>, g1, dim3(256), 0, s, *p, S);
    hipLaunchKernelGGL(omni_chan_finish_kernel, g2, dim3(256), 0, s, *p, S);
    hipLaunchKernelGGL(omni_chan_apply_kernel<decltype(F)::value>, g3, dim3(256), 0, s, *p, S);
  });
  return launch_status("omni_channel_attention: launch failed");
}

extern "C" int rsa_gelu_gate_dwconv(const rsa_gelu_gate_dwconv_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gelu_gate_dwconv: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->planes < 1 || p->planes > 65535 || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "gelu_gate_dwconv: bad geometry (reserved0 must be 0)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "gelu_gate_dwconv: bad plane format");
  if (!p->in_hi || !p->weight || !p->out_hi) return set_error(RSA_E_ARG, "gelu_gate_dwconv: null operand");
  const int64_t HW = (int64_t)p->H * p->W;
  int rc0 = om_planes_ok(p->in_hi, p->in_lo, p->in_plane_stride, p->in_batch_stride, HW, 2 * p->planes);
  if (rc0 == RSA_OK) rc0 = om_planes_ok(p->out_hi, p->out_lo, p->out_plane_stride, p->out_batch_stride, HW, p->planes);
  if (rc0 != RSA_OK) return set_error(rc0, "gelu_gate_dwconv: planes misaligned or strides smaller than the map");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "gelu_gate_dwconv: map too large");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)p->planes, (unsigned)p->batch);
  with_fmt(p->fmt, [&](auto F) {
    hipLaunchKernelGGL(gelu_gate_dwconv_kernel<decltype(F)::value>, grid, dim3(256), 0, s, *p);
  });
  return launch_status("gelu_gate_dwconv: launch failed");
}

extern "C" int rsa_omni_gate_scale(const void* in_hi, const void* in_lo, int64_t plane_stride, int64_t batch_stride, int32_t batch, int32_t H, int32_t W,
                                   int32_t planes, const float* gate, int32_t fmt, void* out_hi, void* out_lo, void* stream) {
  if (!in_hi || !gate || !out_hi) return set_error(RSA_E_ARG, "omni_gate_scale: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || planes < 1 || planes > 65535 || !plane_fmt_ok(fmt) || (in_lo == nullptr) != (out_lo == nullptr))
    return set_error(RSA_E_ARG, "omni_gate_scale: bad geometry or plane format (lo planes on both sides or neither)");
  const int64_t HW = (int64_t)H * W;
  int rc0 = om_planes_ok(in_hi, in_lo, plane_stride, batch_stride, HW, planes);
  if (rc0 == RSA_OK) rc0 = om_planes_ok(out_hi, out_lo, plane_stride, batch_stride, HW, planes);
  if (rc0 != RSA_OK) return set_error(rc0, "omni_gate_scale: planes misaligned or strides smaller than the map");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "omni_gate_scale: map too large");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)planes, (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(omni_gate_scale_kernel<decltype(F)::value>, grid, dim3(256), 0, s, (const char*)in_hi, (const char*)in_lo, plane_stride, batch_stride, HW, planes,
                       gate, (char*)out_hi, (char*)out_lo);
  });
  return launch_status("omni_gate_scale: launch failed");
}

extern "C" int rsa_esa_conv3x3(const rsa_esa_conv_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "esa_conv3x3: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->cin < 1 || p->cin > 64 || p->cout < 1 || p->cout > 64 || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "esa_conv3x3: bad geometry (cin, cout 1..64, reserved0 0)");
  if ((p->stride != 1 && p->stride != 2) || (p->pad != 0 && p->pad != 1)) return set_error(RSA_E_UNSUPPORTED, "esa_conv3x3: stride 1 or 2, pad 0 or 1");
  if (p->H + 2 * p->pad < 3 || p->W + 2 * p->pad < 3 || p->Hout != (p->H + 2 * p->pad - 3) / p->stride + 1 || p->Wout != (p->W + 2 * p->pad - 3) / p->stride + 1)
    return set_error(RSA_E_ARG, "esa_conv3x3: Hout / Wout do not match the geometry");
  if (!p->in || !p->weight || !p->bias || !p->out) return set_error(RSA_E_ARG, "esa_conv3x3: null operand");
  if (misaligned16(p->in) || misaligned16(p->out)) return set_error(RSA_E_ALIGN, "esa_conv3x3: maps must be 16-byte aligned");
  const int64_t HWo = (int64_t)p->Hout * p->Wout;
  if ((HWo + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "esa_conv3x3: map too large");
  hipLaunchKernelGGL(esa_conv_kernel, dim3((unsigned)((HWo + 255) / 256), (unsigned)p->cout, (unsigned)p->batch), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("esa_conv3x3: launch failed");
}

extern "C" int rsa_esa_maxpool(const float* in, int32_t batch, int32_t C, int32_t H, int32_t W, float* out, void* stream) {
  if (!in || !out) return set_error(RSA_E_ARG, "esa_maxpool: null operand");
  if (batch < 1 || batch > 65535 || C < 1 || C > 65535 || H < 7 || W < 7) return set_error(RSA_E_ARG, "esa_maxpool: bad geometry (H, W >= 7)");
  if (misaligned16(in) || misaligned16(out)) return set_error(RSA_E_ALIGN, "esa_maxpool: maps must be 16-byte aligned");
  const int Ho = (H - 7) / 3 + 1, Wo = (W - 7) / 3 + 1;
  const int64_t HWo = (int64_t)Ho * Wo;
  hipLaunchKernelGGL(esa_maxpool_kernel, dim3((unsigned)((HWo + 255) / 256), (unsigned)C, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, in, C, H, W, Ho,
                     Wo, out);
  return launch_status("esa_maxpool: launch failed");
}

extern "C" int rsa_esa_apply(const rsa_esa_apply_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "esa_apply: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->Hc < 1 || p->Wc < 1 || p->C < 1 || p->C > ESA_MAXC || p->f < 1 || p->f > ESA_MAXF)
    return set_error(RSA_E_ARG, "esa_apply: bad geometry (C 1..128, f 1..32)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "esa_apply: bad plane format");
  if (!p->x || !p->c1 || !p->c3 || !p->wf || !p->bf || !p->w4 || !p->b4 || !p->out || (p->out_lo && !p->out_hi)) return set_error(RSA_E_ARG, "esa_apply: null operand");
  if (misaligned16(p->x) || misaligned16(p->c1) || misaligned16(p->c3) || misaligned16(p->out)) return set_error(RSA_E_ALIGN, "esa_apply: maps must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->out_hi) {
    const int rc0 = om_planes_ok(p->out_hi, p->out_lo, p->out_plane_stride, p->out_batch_stride, HW, (p->C + 7) / 8);
    if (rc0 != RSA_OK) return set_error(rc0, "esa_apply: planes misaligned or strides smaller than the map");
  }
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "esa_apply: map too large");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)p->batch);
  with_fmt(p->fmt, [&](auto F) {
    hipLaunchKernelGGL(esa_apply_kernel<decltype(F)::value>, grid, dim3(256), 0, s, *p);
  });
  return launch_status("esa_apply: launch failed");
}
