// flexnet.hip — the kernels FlexNet's TransformerBlock needs beside the fused convolution (reference resselt/archs/flexnet/arch.py):
//   rsa_flex_norm_shift    nn.RMSNorm over channels, then the OmniShift as one 5x5 depthwise kernel, f32 stream -> planes, one launch  :271-280, :65-125
//   rsa_flex_window_attn   softmax(q k^T) v + lepe(v) on every 8x8 window, one head as wide as the embedding, both products on MFMA     :172-216
//   rsa_flex_sqrelu        relu(k)^2, optionally RMS-normalised over the hidden width                                                  :256-259
//   rsa_flex_gate_add      stream + sigmoid(r) * kv, as an f32 map and / or planes                                                     :261, :280
// Everything but the two matrix products is f32; no atomics: every sum has a fixed order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

// ------------------------------------------------------------------------------------------------ RMSNorm + 5x5 depthwise
// grid (tiles of 32 x 8 pixels, batch), 256 threads: thread = pixel.  Pass 1 gives every pixel of the (8 + 4) x (32 + 4) halo its
// 1 / rms over all C channels (LDS, 432 floats).  Pass 2 walks the C / 8 planes: the halo of a plane is read again (L2: the tile's
// C x 432 floats were just read), normalised, weighted and staged in LDS as two f32x4 images (13,824 B), zero outside the map -- the padding is
// of the NORMALISED map -- and every thread takes the 25 taps of its pixel.  The normalised map never exists in HBM.
constexpr int NS_TW = 32, NS_TH = 8, NS_HW = NS_TW + 4, NS_HH = NS_TH + 4, NS_HALO = NS_HW * NS_HH;

struct NormShiftArgs {
  const float* x;   // f32 map [batch][C / 4][H][W][4]
  const float* nw;  // [C]: RMSNorm weight
  const float* w;   // [C][25]
  char* o_hi;
  char* o_lo;
  int64_t o_ps, o_bs;
  int H, W, C;
  float eps;
};

template <int FMT>
__global__ __launch_bounds__(256) void flex_norm_shift_kernel(const NormShiftArgs a) {
  __shared__ float s_r[NS_HALO];
  __shared__ f32x4 s_t[2][NS_HALO];
  const int tid = threadIdx.x;
  const int tiles_x = (a.W + NS_TW - 1) / NS_TW;
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * NS_TW, y0 = tyi * NS_TH;
  const int n = blockIdx.y, G = a.C >> 2, P = a.C >> 3;
  const int64_t HW = (int64_t)a.H * a.W;
  const f32x4* xb = (const f32x4*)a.x + (int64_t)n * G * HW;
  const float inv_c = 1.f / (float)a.C;

  for (int idx = tid; idx < NS_HALO; idx += 256) {
    const int hy = idx / NS_HW, hx = idx - hy * NS_HW;
    const int gy = y0 + hy - 2, gx = x0 + hx - 2;
    float r = 0.f;
    if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) {
      const f32x4* p = xb + (int64_t)gy * a.W + gx;
      float ss = 0.f;
      for (int g = 0; g < G; ++g) {
        const f32x4 v = p[(int64_t)g * HW];
#pragma unroll
        for (int j = 0; j < 4; ++j) ss = fmaf(v[j], v[j], ss);
      }
      r = 1.f / sqrtf(ss * inv_c + a.eps);
    }
    s_r[idx] = r;
  }
  __syncthreads();

  const int tx = tid & (NS_TW - 1), ty = tid / NS_TW;
  const int x = x0 + tx, y = y0 + ty;
  const bool inside = x < a.W && y < a.H;
  for (int pl = 0; pl < P; ++pl) {
    const f32x4 w0 = *(const f32x4*)(a.nw + 8 * pl), w1 = *(const f32x4*)(a.nw + 8 * pl + 4);
    for (int idx = tid; idx < NS_HALO; idx += 256) {
      const int hy = idx / NS_HW, hx = idx - hy * NS_HW;
      const int gy = y0 + hy - 2, gx = x0 + hx - 2;
      f32x4 u = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) {
        const float r = s_r[idx];
        const f32x4* p = xb + (int64_t)(2 * pl) * HW + (int64_t)gy * a.W + gx;
        const f32x4 xu = p[0], xv = p[HW];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = xu[j] * r * w0[j], v[j] = xv[j] * r * w1[j];
      }
      s_t[0][idx] = u;
      s_t[1][idx] = v;
    }
    __syncthreads();
    if (inside) {
      const float* w = a.w + (int64_t)pl * 8 * 25;
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
          const int q = (ty + dy) * NS_HW + tx + dx, tap = dy * 5 + dx;
          const f32x4 u = s_t[0][q], v = s_t[1][q];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = fmaf(w[j * 25 + tap], u[j], o[j]);
            o[4 + j] = fmaf(w[(4 + j) * 25 + tap], v[j], o[4 + j]);
          }
        }
      }
      store_unit<FMT>(a.o_hi, a.o_lo, ((int64_t)n * a.o_bs + (int64_t)pl * a.o_ps + (int64_t)y * a.W + x) * 16, o);
    }
    __syncthreads();  // the next plane overwrites the staged halo
  }
}

// ------------------------------------------------------------------------------------------------ window attention + LePE
// One workgroup of 4 waves per (image, 8 x 8 window): 64 tokens, one head of C channels (a multiple of 16, <= 128); wave w owns the
// 16 queries 16 w .. 16 w + 15.  Both products are v_mfma_f32_16x16x32 (A: lane l holds row l & 15, k = 8 (l >> 4) .. + 7; B: column
// l & 15, the same k; D: rows 4 (l >> 4) .. + 3 of column l & 15):
//   S^T[key][query] = K Q^T   A = K, B = Q^T: a fragment is the 16-byte unit of plane 4 chunk + (l >> 4) at the lane's token, loaded straight
//                             from the planes; a chunk is 32 channels, and the planes past C / 8 of the last chunk of C = 16, 48, 80, 112 are
//                             zero fragments (nothing is padded in HBM).  4 key tiles x ceil(C / 32) chunks (x 3 with lo planes).
//   softmax                   a lane holds 16 of the 64 logits of its query (keys 16 kt + 4 (l >> 4) + j); maximum and sum finish with two
//                             xor shuffles (16, 32).  f32, the maximum subtracted; logits and probabilities stay in registers.
//   O^T[chan][query] = V^T P^T  B = the lane's own probabilities: k = 8 g + e of the 32-key chunk c is key 32 c + 16 (e >> 2) + 4 g + (e & 3).
//                             A = V^T from LDS, where v is staged once TRANSPOSED, [hi | lo][C][72] 16-bit, with the keys of a row in exactly
//                             that order, so a fragment is one 16-byte read (row pitch 144 B: 16 rows start in distinct banks).
//   lepe                      3 x 3 depthwise of v with bias, zero-padded at the WINDOW border, for the lane's 4 channels of its query:
//                             8-byte reads of v's planes (L1 / L2: the window's v was just staged), f32.
// LDS: C * 72 * 2 bytes per half: 18,432 B at C = 64 and 36,864 B at C = 128 with lo planes.
constexpr int FA_VROW = 72;

struct AttnArgs {
  const char* hi;  // [q | k | v]: 3 C / 8 planes
  const char* lo;
  int64_t ps, bs;
  char* o_hi;
  char* o_lo;
  int64_t o_ps, o_bs;
  int H, W, C;
  const float* lw;  // [9][C]: tap-major LePE weights
  const float* lb;  // [C]
};

template <int FMT>
__device__ __forceinline__ float fx_elem(const bf16x8 h, int j) {
  if constexpr (FMT == RSA_PF_F16)
    return (float)__builtin_bit_cast(f16x8, h)[j];
  else
    return (float)h[j];
}

template <int PROD, int FMT>
__global__ __launch_bounds__(256) void flex_window_attn_kernel(const AttnArgs a) {
  extern __shared__ __align__(16) unsigned short s_vt[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int C = a.C, P = C >> 3;
  const int wins_x = a.W >> 3;
  const int wy = (int)blockIdx.x / wins_x, wx = (int)blockIdx.x - wy * wins_x, n = blockIdx.y;
  const int64_t nb = (int64_t)n * a.bs;
  const int64_t pix0 = (int64_t)(8 * wy) * a.W + 8 * wx;
  auto pix = [&](int t) -> int64_t { return pix0 + (int64_t)(t >> 3) * a.W + (t & 7); };
  unsigned short* s_h = s_vt;
  unsigned short* s_l = s_vt + C * FA_VROW;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // ---- stage V^T: item = (plane, token), the token fastest ----
  for (int u = tid; u < 64 * P; u += 256) {
    const int t = u & 63, pl = u >> 6, r = t & 31;
    const int pos = (t & 32) + 8 * ((r & 15) >> 2) + 4 * (r >> 4) + (r & 3);
    const int64_t off = (nb + (int64_t)(2 * P + pl) * a.ps + pix(t)) * 16;
    const uint4 h = *(const uint4*)(a.hi + off);
    unsigned short* d = s_h + (8 * pl) * FA_VROW + pos;
    d[0] = (unsigned short)(h.x & 0xffffu), d[FA_VROW] = (unsigned short)(h.x >> 16);
    d[2 * FA_VROW] = (unsigned short)(h.y & 0xffffu), d[3 * FA_VROW] = (unsigned short)(h.y >> 16);
    d[4 * FA_VROW] = (unsigned short)(h.z & 0xffffu), d[5 * FA_VROW] = (unsigned short)(h.z >> 16);
    d[6 * FA_VROW] = (unsigned short)(h.w & 0xffffu), d[7 * FA_VROW] = (unsigned short)(h.w >> 16);
    if (PROD == 3) {
      const uint4 l = *(const uint4*)(a.lo + off);
      unsigned short* e = s_l + (8 * pl) * FA_VROW + pos;
      e[0] = (unsigned short)(l.x & 0xffffu), e[FA_VROW] = (unsigned short)(l.x >> 16);
      e[2 * FA_VROW] = (unsigned short)(l.y & 0xffffu), e[3 * FA_VROW] = (unsigned short)(l.y >> 16);
      e[4 * FA_VROW] = (unsigned short)(l.z & 0xffffu), e[5 * FA_VROW] = (unsigned short)(l.z >> 16);
      e[6 * FA_VROW] = (unsigned short)(l.w & 0xffffu), e[7 * FA_VROW] = (unsigned short)(l.w >> 16);
    }
  }

  // ---- S^T = K Q^T of the wave's 16 queries against the 64 keys ----
  const int tq = 16 * wave + li;
  const int64_t pq = pix(tq);
  f32x4 acc[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) acc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int chunks = (C + 31) >> 5;
  for (int ch = 0; ch < chunks; ++ch) {
    const int plq = 4 * ch + g;
    const bool valid = plq < P;
    bf16x8 qh = zero8, ql = zero8;
    if (valid) {
      const int64_t off = (nb + (int64_t)plq * a.ps + pq) * 16;
      qh = *(const bf16x8*)(a.hi + off);
      if (PROD == 3) ql = *(const bf16x8*)(a.lo + off);
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      bf16x8 kh = zero8, kl = zero8;
      if (valid) {
        const int64_t off = (nb + (int64_t)(P + plq) * a.ps + pix(16 * kt + li)) * 16;
        kh = *(const bf16x8*)(a.hi + off);
        if (PROD == 3) kl = *(const bf16x8*)(a.lo + off);
      }
      if (PROD == 3) {
        acc[kt] = mfma16<FMT>(kl, qh, acc[kt]);
        acc[kt] = mfma16<FMT>(kh, ql, acc[kt]);
      }
      acc[kt] = mfma16<FMT>(kh, qh, acc[kt]);
    }
  }

  // ---- softmax over the 64 keys of the lane's query ----
  float m = acc[0][0];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) m = fmaxf(m, acc[kt][j]);
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float e = expf(acc[kt][j] - m);
      acc[kt][j] = e;
      sum += e;
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.f / sum;
  bf16x8 ph[2], pl2[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float e8[8], r8[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) e8[j] = acc[2 * c][j], e8[4 + j] = acc[2 * c + 1][j];
    ph[c] = pack16<FMT>(e8);
    pl2[c] = zero8;
    if (PROD == 3) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r8[j] = e8[j] - fx_elem<FMT>(ph[c], j);
      pl2[c] = pack16<FMT>(r8);
    }
  }
  __syncthreads();  // V^T is staged

  // ---- O^T = V^T P^T, + lepe, one tile of 16 channels at a time ----
  const int ty = tq >> 3, tx = tq & 7;
  for (int ct = 0; ct < (C >> 4); ++ct) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int so = (16 * ct + li) * FA_VROW + 32 * c + 8 * g;
      const bf16x8 vh = *(const bf16x8*)(s_h + so);
      if (PROD == 3) {
        const bf16x8 vl = *(const bf16x8*)(s_l + so);
        o = mfma16<FMT>(vl, ph[c], o);
        o = mfma16<FMT>(vh, pl2[c], o);
      }
      o = mfma16<FMT>(vh, ph[c], o);
    }
    const int c0 = 16 * ct + 4 * g;  // the lane's 4 channels of query tq
    f32x4 lp = *(const f32x4*)(a.lb + c0);
    const int64_t vb = (nb + (int64_t)(2 * P + (c0 >> 3)) * a.ps) * 16 + (c0 & 4) * 2;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int yy = ty + dy - 1;
      if ((unsigned)yy >= 8u) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int xx = tx + dx - 1;
        if ((unsigned)xx >= 8u) continue;
        const int64_t off = vb + pix(yy * 8 + xx) * 16;
        const uint2 h = *(const uint2*)(a.hi + off);
        const uint2 l = (PROD == 3) ? *(const uint2*)(a.lo + off) : make_uint2(0u, 0u);
        const f32x4 v = widen4<FMT>(h, l);
        const f32x4 w = *(const f32x4*)(a.lw + (dy * 3 + dx) * C + c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) lp[j] = fmaf(w[j], v[j], lp[j]);
      }
    }
    uint32_t h2[2], l2[2];
    split2<FMT>(fmaf(o[0], inv, lp[0]), fmaf(o[1], inv, lp[1]), h2[0], l2[0]);
    split2<FMT>(fmaf(o[2], inv, lp[2]), fmaf(o[3], inv, lp[3]), h2[1], l2[1]);
    const int64_t oo = ((int64_t)n * a.o_bs + (int64_t)(c0 >> 3) * a.o_ps + pq) * 16 + (c0 & 4) * 2;
    *(uint2*)(a.o_hi + oo) = make_uint2(h2[0], h2[1]);
    if (a.o_lo) *(uint2*)(a.o_lo + oo) = make_uint2(l2[0], l2[1]);
  }
}

// ------------------------------------------------------------------------------------------------ relu^2 (+ RMS over the hidden width)
// Without the norm: grid (ceil(HW / 256), planes, batch), thread = one 16-byte unit.  With it: grid (ceil(HW / 256), 1, batch), thread = pixel:
// one pass sums k^2 over the planes in ascending order, a second reads the units again (L2) and writes k / rms.  A thread writes a unit only
// after its last read of it, so in place is safe.
template <int FMT>
__global__ __launch_bounds__(256) void flex_sqrelu_kernel(const char* hi, const char* lo, int64_t ps, int64_t bs, char* ohi, char* olo, int64_t o_ps,
                                                          int64_t o_bs, int64_t HW, int P, int norm, float eps) {
  const int64_t pixel = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.z;
  if (pixel >= HW) return;
  const int64_t ib = ((int64_t)n * bs + pixel) * 16, ob = ((int64_t)n * o_bs + pixel) * 16;
  float v[8];
  if (!norm) {
    const int pl = blockIdx.y;
    load_unit<FMT>(hi, lo, ib + (int64_t)pl * ps * 16, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float k = fmaxf(v[j], 0.f);
      v[j] = k * k;
    }
    store_unit<FMT>(ohi, olo, ob + (int64_t)pl * o_ps * 16, v);
    return;
  }
  float ss = 0.f;
  for (int pl = 0; pl < P; ++pl) {
    load_unit<FMT>(hi, lo, ib + (int64_t)pl * ps * 16, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float k = fmaxf(v[j], 0.f), k2 = k * k;
      ss = fmaf(k2, k2, ss);
    }
  }
  const float r = 1.f / sqrtf(ss / (float)(8 * P) + eps);
  for (int pl = 0; pl < P; ++pl) {
    load_unit<FMT>(hi, lo, ib + (int64_t)pl * ps * 16, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float k = fmaxf(v[j], 0.f);
      v[j] = k * k * r;
    }
    store_unit<FMT>(ohi, olo, ob + (int64_t)pl * o_ps * 16, v);
  }
}

// ------------------------------------------------------------------------------------------------ stream + sigmoid(r) * kv
// grid (ceil(HW / 256), C / 8, batch): thread = one unit of r and kv and the two f32x4 of the stream it belongs to.  The sum goes to an f32
// map (the next block's stream; may be the base itself: a thread reads its two f32x4 before it writes them) and / or to planes (what the
// convolutions behind the last block of a group read).
template <int FMT>
__global__ __launch_bounds__(256) void flex_gate_add_kernel(const char* rhi, const char* rlo, int64_t r_ps, int64_t r_bs, const char* khi, const char* klo,
                                                            int64_t k_ps, int64_t k_bs, const f32x4* base, f32x4* out, char* ohi, char* olo, int64_t o_ps,
                                                            int64_t o_bs, int64_t HW, int P) {
  const int64_t pixel = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pl = blockIdx.y, n = blockIdx.z;
  if (pixel >= HW) return;
  float r[8], kv[8], o[8];
  load_unit<FMT>(rhi, rlo, ((int64_t)n * r_bs + (int64_t)pl * r_ps + pixel) * 16, r);
  load_unit<FMT>(khi, klo, ((int64_t)n * k_bs + (int64_t)pl * k_ps + pixel) * 16, kv);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t i = ((int64_t)n * 2 * P + 2 * pl + h) * HW + pixel;
    f32x4 b = base[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[j] = fmaf(1.f / (1.f + expf(-r[4 * h + j])), kv[4 * h + j], b[j]);  // e^30: finite; e^89 and up: inf, 1 / inf = 0
      o[4 * h + j] = b[j];
    }
    if (out) out[i] = b;
  }
  if (ohi) store_unit<FMT>(ohi, olo, ((int64_t)n * o_bs + (int64_t)pl * o_ps + pixel) * 16, o);
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_flex_norm_shift(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, float eps, const float* norm_weight,
                                   const float* weight, void* out_hi, void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride, int32_t fmt,
                                   void* stream) {
  if (!x_f32 || !norm_weight || !weight || !out_hi) return set_error(RSA_E_ARG, "flex_norm_shift: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || C < 8 || (C & 7) || !(eps >= 0.f))
    return set_error(RSA_E_ARG, "flex_norm_shift: bad geometry (C a multiple of 8, eps >= 0)");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "flex_norm_shift: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  if (out_plane_stride < HW) return set_error(RSA_E_ARG, "flex_norm_shift: the plane stride is smaller than the map");
  if (batch > 1 && out_batch_stride < (int64_t)(C / 8) * out_plane_stride)
    return set_error(RSA_E_ARG, "flex_norm_shift: the batch stride is smaller than the planes of an image");
  if (misaligned16(x_f32) || misaligned16(norm_weight) || misaligned16(out_hi) || misaligned16(out_lo))
    return set_error(RSA_E_ALIGN, "flex_norm_shift: the map, the norm weight and the planes must be 16-byte aligned");
  const int64_t tiles = (int64_t)((W + NS_TW - 1) / NS_TW) * ((H + NS_TH - 1) / NS_TH);
  if (tiles > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "flex_norm_shift: map too large");
  NormShiftArgs a;
  a.x = x_f32, a.nw = norm_weight, a.w = weight, a.o_hi = (char*)out_hi, a.o_lo = (char*)out_lo, a.o_ps = out_plane_stride, a.o_bs = out_batch_stride;
  a.H = H, a.W = W, a.C = C, a.eps = eps;
  const dim3 grid((unsigned)tiles, (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(flex_norm_shift_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, a);
  });
  return launch_status("flex_norm_shift: launch failed");
}

extern "C" int64_t rsa_flex_window_attn_lds_bytes(int32_t C, int32_t products) {
  if (C < 16 || C > 128 || (C & 15) || (products != 1 && products != 3)) return RSA_E_ARG;
  return (int64_t)(products == 3 ? 2 : 1) * C * FA_VROW * 2;
}

extern "C" int rsa_flex_window_attn(const void* qkv_hi, const void* qkv_lo, int64_t qkv_plane_stride, int64_t qkv_batch_stride, void* out_hi, void* out_lo,
                                    int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t products,
                                    int32_t fmt, const float* lepe_w, const float* lepe_b, void* stream) {
  if (!qkv_hi || !out_hi || !lepe_w || !lepe_b) return set_error(RSA_E_ARG, "flex_window_attn: null operand");
  if (batch < 1 || batch > 65535 || H < 8 || W < 8 || (H & 7) || (W & 7)) return set_error(RSA_E_ARG, "flex_window_attn: H and W must be multiples of 8");
  if (C < 16 || C > 128 || (C & 15)) return set_error(RSA_E_ARG, "flex_window_attn: C must be a multiple of 16 from 16 to 128");
  if (products != 1 && products != 3) return set_error(RSA_E_ARG, "flex_window_attn: products must be 1 or 3");
  if (products == 3 && !qkv_lo) return set_error(RSA_E_ARG, "flex_window_attn: three products need lo planes");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "flex_window_attn: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  const int P = C / 8;
  if (qkv_plane_stride < HW || out_plane_stride < HW) return set_error(RSA_E_ARG, "flex_window_attn: a plane stride is smaller than the map");
  if (batch > 1 && (qkv_batch_stride < 3 * (int64_t)P * qkv_plane_stride || out_batch_stride < (int64_t)P * out_plane_stride))
    return set_error(RSA_E_ARG, "flex_window_attn: a batch stride is smaller than the planes of an image");
  if (out_hi == qkv_hi) return set_error(RSA_E_ARG, "flex_window_attn: not in place");
  if (misaligned16(qkv_hi) || misaligned16(qkv_lo) || misaligned16(out_hi) || misaligned16(out_lo) || misaligned16(lepe_w) || misaligned16(lepe_b))
    return set_error(RSA_E_ALIGN, "flex_window_attn: planes and the LePE weights must be 16-byte aligned");
  const int64_t windows = (int64_t)(H / 8) * (W / 8);
  if (windows > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "flex_window_attn: map too large");
  AttnArgs a;
  a.hi = (const char*)qkv_hi, a.lo = products == 3 ? (const char*)qkv_lo : nullptr, a.ps = qkv_plane_stride, a.bs = qkv_batch_stride;
  a.o_hi = (char*)out_hi, a.o_lo = (char*)out_lo, a.o_ps = out_plane_stride, a.o_bs = out_batch_stride;
  a.H = H, a.W = W, a.C = C, a.lw = lepe_w, a.lb = lepe_b;
  const size_t lds = (size_t)(products == 3 ? 2 : 1) * C * FA_VROW * 2;
  const dim3 grid((unsigned)windows, (unsigned)batch);
  const hipStream_t st = (hipStream_t)stream;
  if (products == 3 && fmt == RSA_PF_F16)
    hipLaunchKernelGGL((flex_window_attn_kernel<3, RSA_PF_F16>), grid, dim3(256), lds, st, a);
  else if (products == 3)
    hipLaunchKernelGGL((flex_window_attn_kernel<3, RSA_PF_BF16>), grid, dim3(256), lds, st, a);
  else if (fmt == RSA_PF_F16)
    hipLaunchKernelGGL((flex_window_attn_kernel<1, RSA_PF_F16>), grid, dim3(256), lds, st, a);
  else
    hipLaunchKernelGGL((flex_window_attn_kernel<1, RSA_PF_BF16>), grid, dim3(256), lds, st, a);
  return launch_status("flex_window_attn: launch failed");
}

extern "C" int rsa_flex_sqrelu(const void* in_hi, const void* in_lo, int64_t in_plane_stride, int64_t in_batch_stride, void* out_hi, void* out_lo,
                               int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t hidden, int32_t norm,
                               float eps, int32_t fmt, void* stream) {
  if (!in_hi || !out_hi) return set_error(RSA_E_ARG, "flex_sqrelu: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || hidden < 8 || (hidden & 7) || hidden > 8 * 65535 || !(eps >= 0.f))
    return set_error(RSA_E_ARG, "flex_sqrelu: bad geometry (hidden a multiple of 8, eps >= 0)");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "flex_sqrelu: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  const int P = hidden / 8;
  if (in_plane_stride < HW || out_plane_stride < HW) return set_error(RSA_E_ARG, "flex_sqrelu: a plane stride is smaller than the map");
  if (batch > 1 && (in_batch_stride < (int64_t)P * in_plane_stride || out_batch_stride < (int64_t)P * out_plane_stride))
    return set_error(RSA_E_ARG, "flex_sqrelu: a batch stride is smaller than the planes of an image");
  if (out_hi == in_hi && (out_plane_stride != in_plane_stride || out_batch_stride != in_batch_stride))
    return set_error(RSA_E_ARG, "flex_sqrelu: in place needs the same strides");
  if (misaligned16(in_hi) || misaligned16(in_lo) || misaligned16(out_hi) || misaligned16(out_lo))
    return set_error(RSA_E_ALIGN, "flex_sqrelu: planes must be 16-byte aligned");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "flex_sqrelu: map too large");
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(norm ? 1 : P), (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(flex_sqrelu_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)in_hi, (const char*)in_lo, in_plane_stride,
                       in_batch_stride, (char*)out_hi, (char*)out_lo, out_plane_stride, out_batch_stride, HW, P, (int)(norm != 0), eps);
  });
  return launch_status("flex_sqrelu: launch failed");
}

extern "C" int rsa_flex_gate_add(const void* r_hi, const void* r_lo, int64_t r_plane_stride, int64_t r_batch_stride, const void* kv_hi, const void* kv_lo,
                                 int64_t kv_plane_stride, int64_t kv_batch_stride, const float* base_f32, float* out_f32, void* out_hi, void* out_lo,
                                 int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t fmt,
                                 void* stream) {
  if (!r_hi || !kv_hi || !base_f32 || (!out_f32 && !out_hi)) return set_error(RSA_E_ARG, "flex_gate_add: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || C < 8 || (C & 7) || C > 8 * 65535) return set_error(RSA_E_ARG, "flex_gate_add: bad geometry (C a multiple of 8)");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "flex_gate_add: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  const int P = C / 8;
  if (r_plane_stride < HW || kv_plane_stride < HW || (out_hi && out_plane_stride < HW))
    return set_error(RSA_E_ARG, "flex_gate_add: a plane stride is smaller than the map");
  if (batch > 1 && (r_batch_stride < (int64_t)P * r_plane_stride || kv_batch_stride < (int64_t)P * kv_plane_stride ||
                    (out_hi && out_batch_stride < (int64_t)P * out_plane_stride)))
    return set_error(RSA_E_ARG, "flex_gate_add: a batch stride is smaller than the planes of an image");
  if (misaligned16(r_hi) || misaligned16(r_lo) || misaligned16(kv_hi) || misaligned16(kv_lo) || misaligned16(base_f32) || misaligned16(out_f32) ||
      misaligned16(out_hi) || misaligned16(out_lo))
    return set_error(RSA_E_ALIGN, "flex_gate_add: planes and maps must be 16-byte aligned");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "flex_gate_add: map too large");
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)P, (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(flex_gate_add_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)r_hi, (const char*)r_lo, r_plane_stride,
                       r_batch_stride, (const char*)kv_hi, (const char*)kv_lo, kv_plane_stride, kv_batch_stride, (const f32x4*)base_f32, (f32x4*)out_f32,
                       (char*)out_hi, (char*)out_lo, out_plane_stride, out_batch_stride, HW, P);
  });
  return launch_status("flex_gate_add: launch failed");
}
