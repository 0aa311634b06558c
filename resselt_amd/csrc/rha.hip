// rha.hip — the kernels RHA's HybridAttention needs beside the fused convolution (reference resselt/archs/rha/arch.py):
//   rsa_rha_window_attn   MaxPool(down) -> roll(-shift) -> FocusedLinearAttention per window -> roll(+shift), one launch      :188-302, :398-407
//   rsa_rha_mix           cat(OmniShift(x1) as one 5x5 depthwise kernel, bilinear x down of the attention map)                 :408-415
//   rsa_rha_gate          mish(g) * cat(i, a * c)                                                                              :449
// Arithmetic is f32 on split-plane operands and f32 maps; no atomics: every sum has a fixed order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

// ------------------------------------------------------------------------------------------------ pooled window attention
// One workgroup of 256 threads per (image, window) of the pooled map.  N = window^2 tokens (16 or 64), C2 channels (8 .. 32), 8 heads of
// d = C2 / 8.  Every operand sits in LDS as f32, CHANNEL-major ([channel][token]): consecutive lanes are consecutive tokens, so a row
// access is conflict-free and a weight read is a broadcast.  LDS floats (RHA_LDS_FLOATS; the launch passes 4 x that as dynamic LDS):
//   tokens / attention output [C2][N] + q|k|v [3 C2][N] + Wqkv^T [C2][3 C2] + Wproj^T [C2][C2] + kv [8][d][d] + mean(k) [C2]
//   + qkv bias [3 C2] + proj bias [C2] + 1/softplus(scale) [C2] + dwc [d][25] + its bias [d]
// = 4 C2 N + 4 C2^2 + C2 d + 6 C2 + 26 d:  C2 = 8: 2,386 (9,544 B);  16: 5,300 (21,200 B);  24: 8,742 (34,968 B);  32: 12,712 (50,848 B)
// at N = 64, so three workgroups of the widest form share a CU's 160 KB.
struct WinArgs {
  const char* x_hi;
  const char* x_lo;
  int64_t x_ps, x_bs;
  int H, W, C2, down, ws, shift, Hd, Wd;
  const float* wqkv_t;  // [C2][3 C2]
  const float* bqkv;    // [3 C2]
  const float* pos_t;   // [C2][N]
  const float* isc;     // [C2]: 1 / softplus(scale)
  const float* dww;     // [d][25]
  const float* dwb;     // [d]
  const float* wproj_t; // [C2][C2]
  const float* bproj;   // [C2]
  float* out;           // f32 map [batch][C2 / 4][Hd][Wd][4]
};

inline int64_t rha_lds_floats(int C2, int N) {
  const int d = C2 / 8;
  return (int64_t)4 * C2 * N + 4 * C2 * C2 + C2 * d + 6 * C2 + 26 * d;
}

// out[4 o4 .. 4 o4 + 3][t] = sum_c in[c][t] * wt[c][4 o4 ..]: item = (o4, t), t fastest; `epi(o4, t, acc)` finishes (bias, stores)
template <class Epi>
__device__ __forceinline__ void rh_linear(const float* s_in, const float* s_wt, int Cin, int Cout, int N, Epi epi) {
  const int items = (Cout >> 2) * N;
  for (int it = threadIdx.x; it < items; it += 256) {
    const int o4 = it / N, t = it - o4 * N;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* xp = s_in + t;
    const f32x4* wp = (const f32x4*)(s_wt + 4 * o4);
    for (int c = 0; c < Cin; ++c) {
      const float xv = xp[c * N];
      const f32x4 w = wp[c * (Cout >> 2)];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(xv, w[j], acc[j]);
    }
    epi(o4, t, acc);
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void rha_window_attn_kernel(const WinArgs a) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x;
  const int C2 = a.C2, ws = a.ws, N = ws * ws, d = C2 >> 3, C3 = 3 * C2, P = C2 >> 3;
  float* s_x = smem;                // [C2][N]
  float* s_q = s_x + C2 * N;        // [3 C2][N]: q, k, v
  float* s_wq = s_q + C3 * N;       // [C2][3 C2]
  float* s_wp = s_wq + C2 * C3;     // [C2][C2]
  float* s_kv = s_wp + C2 * C2;     // [8][d][d]
  float* s_km = s_kv + C2 * d;      // [C2]
  float* s_bq = s_km + C2;          // [3 C2]
  float* s_bp = s_bq + C3;          // [C2]
  float* s_isc = s_bp + C2;         // [C2]
  float* s_dww = s_isc + C2;        // [d][25]
  float* s_dwb = s_dww + 25 * d;    // [d]
  const int wins_x = a.Wd / ws;
  const int wy = (int)blockIdx.x / wins_x, wx = (int)blockIdx.x - wy * wins_x, n = blockIdx.y;

  // weights and small vectors
  for (int i = tid; i < (C2 * C3) >> 2; i += 256) ((f32x4*)s_wq)[i] = ((const f32x4*)a.wqkv_t)[i];
  for (int i = tid; i < (C2 * C2) >> 2; i += 256) ((f32x4*)s_wp)[i] = ((const f32x4*)a.wproj_t)[i];
  for (int i = tid; i < C3; i += 256) s_bq[i] = a.bqkv[i];
  for (int i = tid; i < C2; i += 256) s_bp[i] = a.bproj[i], s_isc[i] = a.isc[i];
  for (int i = tid; i < 25 * d; i += 256) s_dww[i] = a.dww[i];
  if (tid < d) s_dwb[tid] = a.dwb[tid];

  // tokens: item = (plane, token, row of the pool cell), the row fastest: a lane reads `down` consecutive units of one full-resolution row, and
  // the `down` lanes of a cell take the maximum over its rows with xor shuffles.  Every full-resolution value is read once.
  {
    const int dn = a.down;
    const int total = P * N * dn;  // a multiple of dn; 256 is one too, so the lanes of a cell are all live or all dead
    for (int base = 0; base < total; base += 256) {
      const bool live = base + tid < total;
      const int idx = live ? base + tid : total - 1;
      const int s = idx % dn, rest = idx / dn, t = rest % N, p = rest / N;
      const int r = t / ws, c = t - r * ws;
      const int py = (wy * ws + r + a.shift) % a.Hd, px = (wx * ws + c + a.shift) % a.Wd;
      const int64_t off = (((int64_t)n * a.x_bs + (int64_t)p * a.x_ps) + (int64_t)(py * dn + s) * a.W + (int64_t)px * dn) * 16;
      float m[8];
      load_unit<FMT>(a.x_hi, a.x_lo, off, m);  // the maximum starts from the first element
      for (int dx = 1; dx < dn; ++dx) {
        float v[8];
        load_unit<FMT>(a.x_hi, a.x_lo, off + (int64_t)dx * 16, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], v[j]);
      }
      for (int mask = 1; mask < dn; mask <<= 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], __shfl_xor(m[j], mask, 64));
      }
      if (live && s == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s_x[(8 * p + j) * N + t] = m[j];
      }
    }
  }
  __syncthreads();

  // q | k | v = tokens Wqkv^T + b;  k += positional encoding;  q, k = (relu(.) + 1e-6) / softplus(scale)
  rh_linear(s_x, s_wq, C2, C3, N, [&](int o4, int t, const f32x4& acc) {
    const int o = 4 * o4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = acc[j] + s_bq[o + j];
      if (o < 2 * C2) {  // (4 o4 never straddles q | k | v: C2 is a multiple of 8)
        const int c = o + j < C2 ? o + j : o + j - C2;
        if (o >= C2) v += a.pos_t[c * N + t];
        v = (fmaxf(v, 0.f) + 1e-6f) * s_isc[c];
      }
      s_q[(o + j) * N + t] = v;
    }
  });
  __syncthreads();

  // focusing: u <- u^3 / ||u^3|| * ||u|| over ALL C2 channels of a token.  With r = u / max(u) in (0, 1]: u^3 / ||u^3|| = r^3 / ||r^3|| (scale-
  // free) and ||u|| = max ||r||, so no cube of a small u is formed: sum r^6 >= 1 (the maximum contributes exactly 1; squares below 2^-126
  // beside it flush to nothing of consequence) and nothing divides by a flushed norm.
  if (tid < 2 * N) {
    float* base = s_q + (tid >= N ? C2 * N + tid - N : tid);
    float m = 0.f;
    for (int c = 0; c < C2; ++c) m = fmaxf(m, base[c * N]);
    float s2 = 0.f, s6 = 0.f;
    for (int c = 0; c < C2; ++c) {
      const float r = base[c * N] / m, r3 = r * r * r;
      s2 = fmaf(r, r, s2);
      s6 = fmaf(r3, r3, s6);
    }
    const float f = m * sqrtf(s2) / sqrtf(s6);
    for (int c = 0; c < C2; ++c) {
      const float r = base[c * N] / m;
      base[c * N] = r * r * r * f;
    }
  }
  __syncthreads();

  // per head: kv = k^T v / N and mean(k): one entry per thread, the token loop rotated by the lane so that the lanes hit distinct banks
  {
    const int E = C2 * d;  // 8 d d
    const float inv_n = 1.f / (float)N;
    for (int e = tid; e < E + C2; e += 256) {
      float acc = 0.f;
      if (e < E) {
        const int h = e / (d * d), i = (e / d) % d, j = e % d;
        const float* kr = s_q + (C2 + h * d + i) * N;
        const float* vr = s_q + (2 * C2 + h * d + j) * N;
        for (int it = 0; it < N; ++it) {
          const int t = (it + tid) & (N - 1);
          acc = fmaf(kr[t], vr[t], acc);
        }
        s_kv[e] = acc * inv_n;
      } else {
        const float* kr = s_q + (C2 + e - E) * N;
        for (int it = 0; it < N; ++it) acc += kr[(it + tid) & (N - 1)];
        s_km[e - E] = acc * inv_n;
      }
    }
  }
  __syncthreads();

  // out = (q kv) / (q . mean(k) + 1e-6) + dwc(v): the 5x5 depthwise filter of channel c % d, zero-padded at the WINDOW border
  for (int it = tid; it < C2 * N; it += 256) {
    const int c = it / N, t = it - c * N;
    const int h = c / d, j = c - h * d;
    float den = 0.f, num = 0.f;
    for (int i = 0; i < d; ++i) {
      const float qv = s_q[(h * d + i) * N + t];
      den = fmaf(qv, s_km[h * d + i], den);
      num = fmaf(qv, s_kv[(h * d + i) * d + j], num);
    }
    const int ty = t / ws, tx = t - ty * ws;
    const float* vr = s_q + (2 * C2 + c) * N;
    const float* wr = s_dww + 25 * j;
    float conv = s_dwb[j];
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
      const int yy = ty + dy - 2;
      if ((unsigned)yy >= (unsigned)ws) continue;
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int xx = tx + dx - 2;
        if ((unsigned)xx < (unsigned)ws) conv = fmaf(wr[dy * 5 + dx], vr[yy * ws + xx], conv);
      }
    }
    s_x[it] = num / (den + 1e-6f) + conv;
  }
  __syncthreads();

  // proj, written at the UN-ROLLED pooled coordinates
  float* outp = a.out + (int64_t)n * (C2 >> 2) * a.Hd * a.Wd * 4;
  rh_linear(s_x, s_wp, C2, C2, N, [&](int o4, int t, const f32x4& acc) {
    const int r = t / ws, c = t - r * ws;
    const int py = (wy * ws + r + a.shift) % a.Hd, px = (wx * ws + c + a.shift) % a.Wd;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = acc[j] + s_bp[4 * o4 + j];
    *(f32x4*)(outp + (((int64_t)o4 * a.Hd + py) * a.Wd + px) * 4) = v;
  });
}

// ------------------------------------------------------------------------------------------------ mix: [dw5x5(x1) | bilinear(att)]
// grid (tiles of 32 x 8 pixels, 2 * C2 / 8 output planes, batch), 256 threads: thread = pixel.  A plane of the first half stages its
// (8 + 4) x (32 + 4) halo once in LDS as f32 in two 4-channel halves (hi + lo summed, zero outside the map); a plane of the second half
// samples the pooled f32 map (L2-resident: down^2 times smaller) and never stores the upsampled map as f32.
constexpr int MX_TW = 32, MX_TH = 8, MX_HW = MX_TW + 4, MX_HH = MX_TH + 4;

struct MixArgs {
  const char* x_hi;
  const char* x_lo;
  int64_t x_ps, x_bs;
  const float* att;
  char* o_hi;
  char* o_lo;
  int64_t o_ps, o_bs;
  int H, W, C2, down, Hd, Wd;
  const float* w;  // [C2][25]
  const float* b;  // [C2]
};

template <int FMT>
__global__ __launch_bounds__(256) void rha_mix_kernel(const MixArgs a) {
  __shared__ f32x4 s_t[2][MX_HH * MX_HW];
  const int tid = threadIdx.x;
  const int tiles_x = (a.W + MX_TW - 1) / MX_TW;
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * MX_TW, y0 = tyi * MX_TH;
  const int pl = blockIdx.y, n = blockIdx.z, P = a.C2 >> 3;
  const int tx = tid & (MX_TW - 1), ty = tid / MX_TW;
  const int x = x0 + tx, y = y0 + ty;
  const bool inside = x < a.W && y < a.H;
  float o[8];
  if (pl < P) {  // (uniform over the workgroup)
    const int64_t base = ((int64_t)n * a.x_bs + (int64_t)pl * a.x_ps) * 16;
    for (int idx = tid; idx < MX_HH * MX_HW; idx += 256) {
      const int hy = idx / MX_HW, hx = idx - hy * MX_HW;
      const int gy = y0 + hy - 2, gx = x0 + hx - 2;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) load_unit<FMT>(a.x_hi, a.x_lo, base + ((int64_t)gy * a.W + gx) * 16, v);
      s_t[0][idx] = (f32x4){v[0], v[1], v[2], v[3]};
      s_t[1][idx] = (f32x4){v[4], v[5], v[6], v[7]};
    }
    __syncthreads();
    if (!inside) return;
    const float* w = a.w + (int64_t)pl * 8 * 25;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = a.b[pl * 8 + j];
#pragma unroll 1
    for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int q = (ty + dy) * MX_HW + tx + dx, tap = dy * 5 + dx;
        const f32x4 u = s_t[0][q], v = s_t[1][q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = fmaf(w[j * 25 + tap], u[j], o[j]);
          o[4 + j] = fmaf(w[(4 + j) * 25 + tap], v[j], o[4 + j]);
        }
      }
    }
  } else {
    if (!inside) return;
    // F.interpolate(bilinear, align_corners=False): src = (dst + 0.5) / down - 0.5, clamped at 0; the upper neighbour is clamped to the edge
    const float inv = 1.f / (float)a.down;
    const float sy = fmaxf((y + 0.5f) * inv - 0.5f, 0.f), sx = fmaxf((x + 0.5f) * inv - 0.5f, 0.f);
    const int yA = (int)sy, xA = (int)sx;
    const int yB = yA + 1 < a.Hd ? yA + 1 : a.Hd - 1, xB = xA + 1 < a.Wd ? xA + 1 : a.Wd - 1;
    const float ly = sy - (float)yA, lx = sx - (float)xA;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const int q = pl - P;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4* m = (const f32x4*)a.att + ((int64_t)n * (a.C2 >> 2) + 2 * q + h) * a.Hd * a.Wd;
      const f32x4 vAA = m[(int64_t)yA * a.Wd + xA], vAB = m[(int64_t)yA * a.Wd + xB];
      const f32x4 vBA = m[(int64_t)yB * a.Wd + xA], vBB = m[(int64_t)yB * a.Wd + xB];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[4 * h + j] = hy * (hx * vAA[j] + lx * vAB[j]) + ly * (hx * vBA[j] + lx * vBB[j]);
    }
  }
  store_unit<FMT>(a.o_hi, a.o_lo, ((int64_t)n * a.o_bs + (int64_t)pl * a.o_ps + (int64_t)y * a.W + x) * 16, o);
}

// ------------------------------------------------------------------------------------------------ gate
// grid (ceil(HW / 256), hidden planes, batch): thread = one 16-byte unit.  f holds [g | i | c] (hp, ip and hp - ip planes), a the hp - ip
// planes of mish(aggr(.)).
template <int FMT>
__global__ __launch_bounds__(256) void rha_gate_kernel(const char* fhi, const char* flo, int64_t f_ps, int64_t f_bs, const char* ahi, const char* alo,
                                                       int64_t a_ps, int64_t a_bs, char* ohi, char* olo, int64_t o_ps, int64_t o_bs, int64_t HW, int hp,
                                                       int ip) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pl = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  float g[8], m[8], o[8];
  load_unit<FMT>(fhi, flo, ((int64_t)n * f_bs + (int64_t)pl * f_ps + pix) * 16, g);
  load_unit<FMT>(fhi, flo, ((int64_t)n * f_bs + (int64_t)(hp + pl) * f_ps + pix) * 16, m);
  if (pl >= ip) {
    float av[8];
    load_unit<FMT>(ahi, alo, ((int64_t)n * a_bs + (int64_t)(pl - ip) * a_ps + pix) * 16, av);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] *= av[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = mish_exact(g[j]) * m[j];
  store_unit<FMT>(ohi, olo, ((int64_t)n * o_bs + (int64_t)pl * o_ps + pix) * 16, o);
}

bool rha_pow2_le8(int v) { return v == 1 || v == 2 || v == 4 || v == 8; }

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_rha_window_attn_lds_bytes(int32_t C2, int32_t window) {
  if (C2 < 8 || C2 > 32 || (C2 & 7) || (window != 4 && window != 8)) return RSA_E_ARG;
  return rha_lds_floats(C2, window * window) * (int64_t)sizeof(float);
}

extern "C" int rsa_rha_window_attn(const void* x_hi, const void* x_lo, int64_t x_plane_stride, int64_t x_batch_stride, int32_t batch, int32_t H, int32_t W,
                                   int32_t C2, int32_t down, int32_t window, int32_t shift, int32_t fmt, const float* wqkv_t, const float* bqkv,
                                   const float* pos_t, const float* inv_scale, const float* dwc_w, const float* dwc_b, const float* wproj_t,
                                   const float* bproj, float* out, void* stream) {
  if (!x_hi || !wqkv_t || !bqkv || !pos_t || !inv_scale || !dwc_w || !dwc_b || !wproj_t || !bproj || !out)
    return set_error(RSA_E_ARG, "rha_window_attn: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1) return set_error(RSA_E_ARG, "rha_window_attn: bad geometry");
  if (C2 < 8 || C2 > 32 || (C2 & 7)) return set_error(RSA_E_ARG, "rha_window_attn: C2 must be 8, 16, 24 or 32");
  if (!rha_pow2_le8(down)) return set_error(RSA_E_ARG, "rha_window_attn: down must be 1, 2, 4 or 8");
  if (window != 4 && window != 8) return set_error(RSA_E_ARG, "rha_window_attn: window must be 4 or 8");
  if (shift < 0 || shift >= window) return set_error(RSA_E_ARG, "rha_window_attn: shift must be in [0, window)");
  if (H % (down * window) || W % (down * window)) return set_error(RSA_E_ARG, "rha_window_attn: H and W must be multiples of down * window");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "rha_window_attn: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  if (x_plane_stride < HW) return set_error(RSA_E_ARG, "rha_window_attn: the plane stride is smaller than the map");
  if (batch > 1 && x_batch_stride < (int64_t)(C2 / 8) * x_plane_stride)
    return set_error(RSA_E_ARG, "rha_window_attn: the batch stride is smaller than the planes of an image");
  if (misaligned16(x_hi) || misaligned16(x_lo) || misaligned16(wqkv_t) || misaligned16(wproj_t) || misaligned16(out))
    return set_error(RSA_E_ALIGN, "rha_window_attn: planes, the two matrices and the output map must be 16-byte aligned");
  const int Hd = H / down, Wd = W / down;
  const int64_t windows = (int64_t)(Hd / window) * (Wd / window);
  if (windows > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "rha_window_attn: map too large");
  WinArgs a;
  a.x_hi = (const char*)x_hi, a.x_lo = (const char*)x_lo, a.x_ps = x_plane_stride, a.x_bs = x_batch_stride;
  a.H = H, a.W = W, a.C2 = C2, a.down = down, a.ws = window, a.shift = shift, a.Hd = Hd, a.Wd = Wd;
  a.wqkv_t = wqkv_t, a.bqkv = bqkv, a.pos_t = pos_t, a.isc = inv_scale, a.dww = dwc_w, a.dwb = dwc_b, a.wproj_t = wproj_t, a.bproj = bproj, a.out = out;
  const size_t lds = (size_t)rha_lds_floats(C2, window * window) * sizeof(float);
  const dim3 grid((unsigned)windows, (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(rha_window_attn_kernel<decltype(F)::value>, grid, dim3(256), lds, (hipStream_t)stream, a);
  });
  return launch_status("rha_window_attn: launch failed");
}

extern "C" int rsa_rha_mix(const void* x_hi, const void* x_lo, int64_t x_plane_stride, int64_t x_batch_stride, const float* att, void* out_hi, void* out_lo,
                           int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C2, int32_t down, int32_t fmt,
                           const float* weight, const float* bias, void* stream) {
  if (!x_hi || !att || !out_hi || !weight || !bias) return set_error(RSA_E_ARG, "rha_mix: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || C2 < 8 || (C2 & 7) || C2 > 8 * 16383) return set_error(RSA_E_ARG, "rha_mix: bad geometry");
  if (!rha_pow2_le8(down)) return set_error(RSA_E_ARG, "rha_mix: down must be 1, 2, 4 or 8");
  if (H % down || W % down) return set_error(RSA_E_ARG, "rha_mix: H and W must be multiples of down");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "rha_mix: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  const int P = C2 / 8;
  if (x_plane_stride < HW || out_plane_stride < HW) return set_error(RSA_E_ARG, "rha_mix: a plane stride is smaller than the map");
  if (batch > 1 && (x_batch_stride < (int64_t)P * x_plane_stride || out_batch_stride < 2 * (int64_t)P * out_plane_stride))
    return set_error(RSA_E_ARG, "rha_mix: a batch stride is smaller than the planes of an image");
  if (x_hi == out_hi) return set_error(RSA_E_ARG, "rha_mix: not in place (a tile reads its neighbours' pixels)");
  if (misaligned16(x_hi) || misaligned16(x_lo) || misaligned16(out_hi) || misaligned16(out_lo) || misaligned16(att))
    return set_error(RSA_E_ALIGN, "rha_mix: planes and the attention map must be 16-byte aligned");
  const int64_t tiles = (int64_t)((W + MX_TW - 1) / MX_TW) * ((H + MX_TH - 1) / MX_TH);
  if (tiles > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "rha_mix: map too large");
  MixArgs a;
  a.x_hi = (const char*)x_hi, a.x_lo = (const char*)x_lo, a.x_ps = x_plane_stride, a.x_bs = x_batch_stride, a.att = att;
  a.o_hi = (char*)out_hi, a.o_lo = (char*)out_lo, a.o_ps = out_plane_stride, a.o_bs = out_batch_stride;
  a.H = H, a.W = W, a.C2 = C2, a.down = down, a.Hd = H / down, a.Wd = W / down, a.w = weight, a.b = bias;
  const dim3 grid((unsigned)tiles, (unsigned)(2 * P), (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(rha_mix_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, a);
  });
  return launch_status("rha_mix: launch failed");
}

extern "C" int rsa_rha_gate(const void* f_hi, const void* f_lo, int64_t f_plane_stride, int64_t f_batch_stride, const void* a_hi, const void* a_lo,
                            int64_t a_plane_stride, int64_t a_batch_stride, void* out_hi, void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride,
                            int32_t batch, int32_t H, int32_t W, int32_t hidden_planes, int32_t i_planes, int32_t fmt, void* stream) {
  if (!f_hi || !a_hi || !out_hi) return set_error(RSA_E_ARG, "rha_gate: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || hidden_planes < 1 || hidden_planes > 32767 || i_planes < 0 || i_planes >= hidden_planes)
    return set_error(RSA_E_ARG, "rha_gate: bad geometry (0 <= i_planes < hidden_planes)");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "rha_gate: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  const int64_t hp = hidden_planes, cp = hidden_planes - i_planes;
  if (f_plane_stride < HW || a_plane_stride < HW || out_plane_stride < HW) return set_error(RSA_E_ARG, "rha_gate: a plane stride is smaller than the map");
  if (batch > 1 && (f_batch_stride < 2 * hp * f_plane_stride || a_batch_stride < cp * a_plane_stride || out_batch_stride < hp * out_plane_stride))
    return set_error(RSA_E_ARG, "rha_gate: a batch stride is smaller than the planes of an image");
  if (out_hi == f_hi || out_hi == a_hi) return set_error(RSA_E_ARG, "rha_gate: not in place");
  if (misaligned16(f_hi) || misaligned16(f_lo) || misaligned16(a_hi) || misaligned16(a_lo) || misaligned16(out_hi) || misaligned16(out_lo))
    return set_error(RSA_E_ALIGN, "rha_gate: planes must be 16-byte aligned");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "rha_gate: map too large");
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)hidden_planes, (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(rha_gate_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)f_hi, (const char*)f_lo, f_plane_stride, f_batch_stride,
                       (const char*)a_hi, (const char*)a_lo, a_plane_stride, a_batch_stride, (char*)out_hi, (char*)out_lo, out_plane_stride, out_batch_stride, HW,
                       (int)hidden_planes, (int)i_planes);
  });
  return launch_status("rha_gate: launch failed");
}
