// eimn.hip — the kernels EIMN needs beside the fused convolution (reference resselt/archs/eimn/arch.py):
//   rsa_eimn_query_chain   MOLRCM's depthwise chain: 5x5, then per channel group 5x5 dilation 2 / identity / 7x7 dilation 3   :112-130, :141-145
//   rsa_eimn_sal           SADFFM's middle: GELU(dw3x3(x1) + b1) * (dw3x3(x2) + b2)                                            :43-51, :58-59
//   rsa_eimn_silu_mul      silu(fusion) * value                                                                                :145-146
//   rsa_eimn_dffm_reduce / _gates / _apply   DFFM (:65-92) with the block's layer-scaled residual (:171) and the stage LayerNorm (:237-239)
// Arithmetic is f32 on split-plane operands and f32 maps (f64 where a reduction is pooled over the map); no atomics: every sum has a fixed order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

// ------------------------------------------------------------------------------------------------ the depthwise chain
// A workgroup is a 32 x 16 pixel tile of one HALF plane (four channels: the low or the high 8 bytes of the 16-byte units), 256 threads, two
// output rows per thread.  It stages its input once in LDS as f32 (hi + lo summed, GELU applied when asked for, zero outside the map),
// evaluates stage 1 (5x5, bias) on the tile grown by the reach of ITS group's stage 2 into a second LDS tile -- 0 where the position lies
// outside the map: stage 2 zero-pads the stage-1 MAP, not its bias and not stage 1 of the padded input -- and stage 2 reads that tile.
// Reach staged per group: 2 + 4 (5x5 dilation 2), 2 (identity), 2 + 9 (7x7 dilation 3).
// LDS per workgroup, sized by the widest group: input (16 + 22) x (32 + 22) + intermediate (16 + 18) x (32 + 18) four-channel f32 units
// = (2052 + 1700) * 16 B = 60032 B, two workgroups per CU.  A whole plane in f32 would be 120 KB (one workgroup per CU); an 8-row tile
// evaluates stage 1 on 5.1 positions per output pixel instead of 3.3.  A tap is one 16-byte LDS read of consecutive units by consecutive
// lanes (conflict-free, dilated or not); the weights are workgroup-uniform [tap][4 channels] rows.
constexpr int EQ_TW = 32, EQ_TH = 16;
constexpr int EQ_R1 = 2;    // stage 1: 5x5, padding 2
constexpr int EQ_RMAX = 9;  // stage 2 of the widest group: 7x7, dilation 3, padding 9
constexpr int EQ_IN_UNITS = (EQ_TH + 2 * (EQ_R1 + EQ_RMAX)) * (EQ_TW + 2 * (EQ_R1 + EQ_RMAX));
constexpr int EQ_MID_UNITS = (EQ_TH + 2 * EQ_RMAX) * (EQ_TW + 2 * EQ_RMAX);
constexpr int EQ_K1 = 25, EQ_K2 = 49;  // taps of a weight row of stage 1 / stage 2 (a 5x5 second stage uses the first 25)
static_assert((EQ_IN_UNITS + EQ_MID_UNITS) * 16 == 60032, "the LDS budget stated above");

struct ChainArgs {
  const char* q_hi;
  const char* q_lo;
  int64_t q_ps, q_bs;
  char* o_hi;
  char* o_lo;
  int64_t o_ps, o_bs;
  int H, W, planes_a, planes_b, gelu_in;
  const f32x4* w1;  // [half plane][25]
  const f32x4* b1;  // [half plane]
  const f32x4* w2;  // [half plane][49]
  const f32x4* b2;  // [half plane]
};

template <int FMT, int K2, int DIL>
__device__ __forceinline__ void chain_tile(const char* qhi, const char* qlo, char* ohi, char* olo, int H, int W, int x0, int y0, bool gelu,
                                           const f32x4* __restrict__ w1, const f32x4 b1, const f32x4* __restrict__ w2, const f32x4 b2, f32x4* s_in,
                                           f32x4* s_mid) {
  constexpr int R2 = (K2 / 2) * DIL, R = R2 + EQ_R1;
  constexpr int IH = EQ_TH + 2 * R, IW = EQ_TW + 2 * R, MH = EQ_TH + 2 * R2, MW = EQ_TW + 2 * R2;
  static_assert(IH * IW <= EQ_IN_UNITS && MH * MW <= EQ_MID_UNITS, "tile exceeds the LDS arrays");
  const int tid = threadIdx.x;
  for (int idx = tid; idx < IH * IW; idx += 256) {
    const int hy = idx / IW, hx = idx - hy * IW;
    const int gy = y0 + hy - R, gx = x0 + hx - R;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
      const int64_t off = ((int64_t)gy * W + gx) * 16;
      const uint2 h = *(const uint2*)(qhi + off);
      const uint2 l = qlo ? *(const uint2*)(qlo + off) : make_uint2(0u, 0u);
      v = widen4<FMT>(h, l);
      if (gelu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = gelu_erf(v[j]);
      }
    }
    s_in[idx] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < MH * MW; idx += 256) {
    const int my = idx / MW, mx = idx - my * MW;
    const int gy = y0 + my - R2, gx = x0 + mx - R2;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};  // outside the map the second stage reads 0
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
      a = b1;
#pragma unroll
      for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
          const f32x4 wv = w1[dy * 5 + dx], xv = s_in[(my + dy) * IW + mx + dx];
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = fmaf(wv[j], xv[j], a[j]);
        }
      }
    }
    s_mid[idx] = a;
  }
  __syncthreads();
  const int tx = tid & (EQ_TW - 1), ty = tid / EQ_TW;
  const int x = x0 + tx;
  if (x >= W) return;
#pragma unroll
  for (int r = 0; r < EQ_TH / 8; ++r) {
    const int oy = ty + 8 * r, y = y0 + oy;
    if (y >= H) continue;
    f32x4 acc;
    if constexpr (K2 == 1) {
      acc = s_mid[oy * MW + tx];
    } else {
      acc = b2;
#pragma unroll 1
      for (int dy = 0; dy < K2; ++dy) {  // (one row of taps at a time, as rsa_gated_dwconv)
#pragma unroll
        for (int dx = 0; dx < K2; ++dx) {
          const f32x4 wv = w2[dy * K2 + dx], xv = s_mid[(oy + dy * DIL) * MW + tx + dx * DIL];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(wv[j], xv[j], acc[j]);
        }
      }
    }
    uint32_t h0, h1, l0, l1;
    split2<FMT>(acc[0], acc[1], h0, l0);
    split2<FMT>(acc[2], acc[3], h1, l1);
    const int64_t off = ((int64_t)y * W + x) * 16;
    *(uint2*)(ohi + off) = make_uint2(h0, h1);
    if (olo) *(uint2*)(olo + off) = make_uint2(l0, l1);
  }
}

// grid (tiles, 2 * planes, batch), 256 threads
template <int FMT>
__global__ __launch_bounds__(256) void eimn_chain_kernel(const ChainArgs a) {
  __shared__ f32x4 s_in[EQ_IN_UNITS];
  __shared__ f32x4 s_mid[EQ_MID_UNITS];
  const int tiles_x = (a.W + EQ_TW - 1) / EQ_TW;
  const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
  const int x0 = txi * EQ_TW, y0 = tyi * EQ_TH;
  const int hp = blockIdx.y, pl = hp >> 1, half = hp & 1, n = blockIdx.z;
  const int64_t qo = ((int64_t)n * a.q_bs + (int64_t)pl * a.q_ps) * 16 + half * 8, oo = ((int64_t)n * a.o_bs + (int64_t)pl * a.o_ps) * 16 + half * 8;
  const char* qhi = a.q_hi + qo;
  const char* qlo = a.q_lo ? a.q_lo + qo : nullptr;
  char* ohi = a.o_hi + oo;
  char* olo = a.o_lo ? a.o_lo + oo : nullptr;
  const f32x4* w1 = a.w1 + (int64_t)hp * EQ_K1;
  const f32x4* w2 = a.w2 + (int64_t)hp * EQ_K2;
  const f32x4 b1 = a.b1[hp], b2 = a.b2[hp];
  const bool gelu = a.gelu_in != 0;
  if (pl < a.planes_a)
    chain_tile<FMT, 5, 2>(qhi, qlo, ohi, olo, a.H, a.W, x0, y0, gelu, w1, b1, w2, b2, s_in, s_mid);
  else if (pl < a.planes_a + a.planes_b)
    chain_tile<FMT, 1, 1>(qhi, qlo, ohi, olo, a.H, a.W, x0, y0, gelu, w1, b1, w2, b2, s_in, s_mid);
  else
    chain_tile<FMT, 7, 3>(qhi, qlo, ohi, olo, a.H, a.W, x0, y0, gelu, w1, b1, w2, b2, s_in, s_mid);
}

// ------------------------------------------------------------------------------------------------ SAL gate, multiply
// grid (ceil(HW / 256), planes, batch): thread = (pixel, output plane); reads plane pl (x1) and plane planes + pl (x2) with a 1-pixel halo
template <int FMT>
__global__ __launch_bounds__(256) void eimn_sal_kernel(const char* ihi, const char* ilo, int64_t i_ps, int64_t i_bs, char* ohi, char* olo, int64_t o_ps,
                                                       int64_t o_bs, int H, int W, int planes, const float* __restrict__ weight,
                                                       const float* __restrict__ bias) {
  const int64_t HW = (int64_t)H * W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pl = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
  const float* w1 = weight + (int64_t)pl * 8 * 9;
  const float* w2 = weight + (int64_t)(planes + pl) * 8 * 9;
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = bias[pl * 8 + j], b[j] = bias[(planes + pl) * 8 + j];
  const int64_t base1 = ((int64_t)n * i_bs + (int64_t)pl * i_ps) * 16, base2 = ((int64_t)n * i_bs + (int64_t)(planes + pl) * i_ps) * 16;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
    const int64_t q = ((int64_t)yy * W + xx) * 16;
    float u[8], v[8];
    load_unit<FMT>(ihi, ilo, base1 + q, u);
    load_unit<FMT>(ihi, ilo, base2 + q, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = fmaf(w1[j * 9 + tap], u[j], a[j]);
      b[j] = fmaf(w2[j * 9 + tap], v[j], b[j]);
    }
  }
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = gelu_erf(a[j]) * b[j];
  store_unit<FMT>(ohi, olo, ((int64_t)n * o_bs + (int64_t)pl * o_ps + pix) * 16, o);
}

// grid (ceil(HW / 256), planes, batch): thread = one 16-byte unit; out may be f or v
template <int FMT>
__global__ __launch_bounds__(256) void eimn_silu_mul_kernel(const char* fhi, const char* flo, int64_t f_ps, int64_t f_bs, const char* vhi, const char* vlo,
                                                            int64_t v_ps, int64_t v_bs, char* ohi, char* olo, int64_t o_ps, int64_t o_bs, int64_t HW) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pl = blockIdx.y, n = blockIdx.z;
  if (pix >= HW) return;
  float f[8], v[8], o[8];
  load_unit<FMT>(fhi, flo, ((int64_t)n * f_bs + (int64_t)pl * f_ps + pix) * 16, f);
  load_unit<FMT>(vhi, vlo, ((int64_t)n * v_bs + (int64_t)pl * v_ps + pix) * 16, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (f[j] * sigmoid_exact(f[j])) * v[j];
  store_unit<FMT>(ohi, olo, ((int64_t)n * o_bs + (int64_t)pl * o_ps + pix) * 16, o);
}

// ------------------------------------------------------------------------------------------------ DFFM
constexpr int ED_THREADS = 256;
constexpr int ED_MAX_C = 128, ED_MAX_RC = 32;

// Reduce pass.  grid (slots = ceil(HW / 256), batch), 256 threads: thread = pixel.  The channels-first LayerNorm of a pixel is evaluated in
// f64 from the f32 map and each normalised, affine-applied value is rounded to f32 ONCE; a channel's 256 values are then added in f32: an
// xor butterfly over the 64 lanes of a wave (6 levels, the same bits in every lane), and the four wave partials in order (3 additions).
// Depth of the f32 tree behind a workspace entry: 1 + 6 + 3 = 10 (RSA_EIMN_DFFM_DEPTH; tests/test_eimn_kernels_gpu.py quotes it).
// Every entry workspace[n][slot][c] is written by exactly one workgroup; dead pixels of the last slot add 0.
__global__ __launch_bounds__(ED_THREADS) void dffm_reduce_kernel(const float* __restrict__ z, int64_t HW, int C, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, double eps, float* __restrict__ ws) {
  __shared__ float s_part[ED_THREADS / 64][ED_MAX_C];
  const int n = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t pix = (int64_t)blockIdx.x * ED_THREADS + t;
  const bool live = pix < HW;
  const int P4 = C >> 2;
  const f32x4* zp = (const f32x4*)z + (int64_t)n * P4 * HW + (live ? pix : 0);
  double mean = 0.0, rstd = 0.0;
  if (live) {
    double s = 0.0;
    for (int g = 0; g < P4; ++g) {
      const f32x4 v = zp[(int64_t)g * HW];
      s += (((double)v[0] + (double)v[1]) + (double)v[2]) + (double)v[3];
    }
    mean = s / (double)C;
    double q = 0.0;
    for (int g = 0; g < P4; ++g) {
      const f32x4 v = zp[(int64_t)g * HW];
#pragma unroll
      for (int j = 0; j < 4; ++j) q += ((double)v[j] - mean) * ((double)v[j] - mean);
    }
    rstd = 1.0 / sqrt(q / (double)C + eps);
  }
  for (int g = 0; g < P4; ++g) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      const f32x4 zz = zp[(int64_t)g * HW];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (float)(((double)zz[j] - mean) * rstd * (double)gamma[4 * g + j] + (double)beta[4 * g + j]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += __shfl_xor(v[j], m, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s_part[wv][4 * g + j] = v[j];
    }
  }
  __syncthreads();
  float* dst = ws + ((int64_t)n * gridDim.x + blockIdx.x) * C;
  for (int c = t; c < C; c += ED_THREADS) dst[c] = ((s_part[0][c] + s_part[1][c]) + s_part[2][c]) + s_part[3][c];
}

__device__ __forceinline__ double ed_gelu(double v) { return 0.5 * v * (1.0 + erf(v * 0.70710678118654752440)); }

// Finish.  grid (batch), 256 threads, f64 throughout.  Thread t owns channel t % C of the slots t / C, + NSL, + 2 NSL ... (NSL = 256 / C) in
// ascending order; the NSL partials of a channel are then added in order by one thread: a fixed order for a given slot count.
// gates[n]: c_attn[0 .. C), then the scalar s_g at [C] ([C + 1 .. C + 4) are written as 0): a row of C + 4 floats.
__global__ __launch_bounds__(ED_THREADS) void dffm_gates_kernel(const float* __restrict__ ws, int slots, int C, int rc, double inv_hw,
                                                                const float* __restrict__ wg, const float* __restrict__ bg,
                                                                const float* __restrict__ wc, const float* __restrict__ bc,
                                                                const float* __restrict__ wsp, const float* __restrict__ bsp, float* __restrict__ gates) {
  __shared__ double s_part[ED_THREADS];
  __shared__ double s_mean[ED_MAX_C];
  __shared__ double s_g[ED_MAX_RC];
  const int n = blockIdx.x, t = threadIdx.x;
  const int NSL = ED_THREADS / C;
  const int c0 = t % C, sl = t / C;
  if (sl < NSL) {
    const float* src = ws + (int64_t)n * slots * C + c0;
    double a = 0.0;
    for (int64_t s = sl; s < slots; s += NSL) a += (double)src[s * C];
    s_part[sl * C + c0] = a;
  }
  __syncthreads();
  if (t < C) {
    double s = 0.0;
    for (int k = 0; k < NSL; ++k) s += s_part[k * C + t];
    s_mean[t] = s * inv_hw;
  }
  __syncthreads();
  if (t < rc) {
    double s = (double)bg[t];
    for (int c = 0; c < C; ++c) s += (double)wg[(int64_t)t * C + c] * s_mean[c];
    s_g[t] = ed_gelu(s);
  }
  __syncthreads();
  float* dst = gates + (int64_t)n * (C + 4);
  if (t < C) {
    double s = (double)bc[t];
    for (int k = 0; k < rc; ++k) s += (double)wc[(int64_t)t * rc + k] * s_g[k];
    dst[t] = (float)(1.0 / (1.0 + exp(-s)));
  } else if (t == C) {
    double s = (double)bsp[0];
    for (int k = 0; k < rc; ++k) s += (double)wsp[rc + k] * s_g[k];
    dst[C] = (float)s;
    dst[C + 1] = dst[C + 2] = dst[C + 3] = 0.f;
  }
}

struct ApplyArgs {
  const float* z;       // f32 map: linear_out's output
  const float* x;       // f32 map: the residual stream
  const float* add;     // f32 map added last, or NULL
  float* out;           // f32 map (may be x)
  int64_t HW;
  int C, rc;
  const float* gamma;   // DFFM.norm
  const float* beta;
  float eps;
  const float* wl;      // local_reduce [rc][C]
  const float* bl;      // [rc]
  const float* wsp;     // spatial_expand [2 rc]: the first rc multiply the local branch
  const float* gates;   // [batch][C + 4] from the finish pass
  const float* scale;   // layer_scale_2 [C]
  const float* ngamma;  // stage LayerNorm, or NULL
  const float* nbeta;
  float neps;
  char* o_hi;
  char* o_lo;
  int64_t o_ps, o_bs;
};

// Apply pass.  grid (ceil(HW / 256), batch), 256 threads: thread = pixel, all C channels.  local_reduce's matrix sits transposed in LDS
// ([c][RCP], zero past rc) and is read as broadcast 16-byte rows; RCP = 16 or 32.  With the stage norm the thread writes x_new to `out`,
// re-reads its own values for the variance and overwrites them with the normalised ones.
template <int FMT, int RCP>
__global__ __launch_bounds__(ED_THREADS) void dffm_apply_kernel(const ApplyArgs a) {
  __shared__ f32x4 s_wl[ED_MAX_C * RCP / 4];
  __shared__ float s_bl[RCP], s_ws[RCP];
  __shared__ float s_k[ED_MAX_C];  // layer_scale_2[c] * c_attn[n][c]
  const int n = blockIdx.y, t = threadIdx.x;
  const int C = a.C, rc = a.rc, P4 = C >> 2;
  const float* gates = a.gates + (int64_t)n * (C + 4);
  for (int i = t; i < C * RCP; i += ED_THREADS) {
    const int c = i / RCP, r = i - c * RCP;
    ((float*)s_wl)[i] = r < rc ? a.wl[(int64_t)r * C + c] : 0.f;
  }
  if (t < RCP) s_bl[t] = t < rc ? a.bl[t] : 0.f, s_ws[t] = t < rc ? a.wsp[t] : 0.f;
  for (int c = t; c < C; c += ED_THREADS) s_k[c] = a.scale[c] * gates[c];
  __syncthreads();
  const int64_t HW = a.HW;
  const int64_t pix = (int64_t)blockIdx.x * ED_THREADS + t;
  if (pix >= HW) return;
  const int64_t base = (int64_t)n * P4 * HW + pix;
  const f32x4* zp = (const f32x4*)a.z + base;
  const f32x4* xp = (const f32x4*)a.x + base;
  const f32x4* ap = a.add ? (const f32x4*)a.add + base : nullptr;
  f32x4* op = (f32x4*)a.out + base;
  float sum = 0.f;
  for (int g = 0; g < P4; ++g) {
    const f32x4 v = zp[(int64_t)g * HW];
    sum += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = sum / (float)C;
  float q = 0.f;
  for (int g = 0; g < P4; ++g) {
    const f32x4 v = zp[(int64_t)g * HW];
    q += ((v[0] - mean) * (v[0] - mean) + (v[1] - mean) * (v[1] - mean)) + ((v[2] - mean) * (v[2] - mean) + (v[3] - mean) * (v[3] - mean));
  }
  const float rstd = 1.f / sqrtf(q / (float)C + a.eps);
  float l[RCP];
#pragma unroll
  for (int r = 0; r < RCP; ++r) l[r] = 0.f;
  for (int g = 0; g < P4; ++g) {
    const f32x4 v = zp[(int64_t)g * HW];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float nv = fmaf((v[j] - mean) * rstd, a.gamma[4 * g + j], a.beta[4 * g + j]);
#pragma unroll
      for (int r4 = 0; r4 < RCP / 4; ++r4) {
        const f32x4 w = s_wl[(4 * g + j) * (RCP / 4) + r4];
#pragma unroll
        for (int i = 0; i < 4; ++i) l[4 * r4 + i] = fmaf(w[i], nv, l[4 * r4 + i]);
      }
    }
  }
  float pre = gates[C];  // s_g
#pragma unroll
  for (int r = 0; r < RCP; ++r) pre = fmaf(s_ws[r], gelu_erf(l[r] + s_bl[r]), pre);
  const float s = sigmoid_exact(pre);
  const bool norm = a.ngamma != nullptr;
  char* ohi = a.o_hi + ((int64_t)n * a.o_bs + pix) * 16;
  char* olo = a.o_lo ? a.o_lo + ((int64_t)n * a.o_bs + pix) * 16 : nullptr;
  if (!norm) {
    for (int p = 0; p < (C >> 3); ++p) {
      float o[8];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int g = 2 * p + h;
        const f32x4 zz = zp[(int64_t)g * HW], xx = xp[(int64_t)g * HW];
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = fmaf(s_k[4 * g + j] * zz[j], s, xx[j]);
        if (ap) r += ap[(int64_t)g * HW];
        op[(int64_t)g * HW] = r;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[4 * h + j] = r[j];
      }
      store_unit<FMT>(ohi, olo, (int64_t)p * a.o_ps * 16, o);
    }
    return;
  }
  float sum2 = 0.f;
  for (int g = 0; g < P4; ++g) {
    const f32x4 zz = zp[(int64_t)g * HW], xx = xp[(int64_t)g * HW];
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = fmaf(s_k[4 * g + j] * zz[j], s, xx[j]);
    op[(int64_t)g * HW] = r;
    sum2 += (r[0] + r[1]) + (r[2] + r[3]);
  }
  const float mean2 = sum2 / (float)C;
  float q2 = 0.f;
  for (int g = 0; g < P4; ++g) {
    const f32x4 v = op[(int64_t)g * HW];
    q2 += ((v[0] - mean2) * (v[0] - mean2) + (v[1] - mean2) * (v[1] - mean2)) + ((v[2] - mean2) * (v[2] - mean2) + (v[3] - mean2) * (v[3] - mean2));
  }
  const float rstd2 = 1.f / sqrtf(q2 / (float)C + a.neps);
  for (int p = 0; p < (C >> 3); ++p) {
    float o[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int g = 2 * p + h;
      const f32x4 v = op[(int64_t)g * HW];
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = fmaf((v[j] - mean2) * rstd2, a.ngamma[4 * g + j], a.nbeta[4 * g + j]);
      if (ap) r += ap[(int64_t)g * HW];
      op[(int64_t)g * HW] = r;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[4 * h + j] = r[j];
    }
    store_unit<FMT>(ohi, olo, (int64_t)p * a.o_ps * 16, o);
  }
}

int dffm_geometry(int32_t batch, int32_t H, int32_t W, int32_t C) {
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || C < 8 || (C & 7) || C > ED_MAX_C) return RSA_E_ARG;
  if (((int64_t)H * W + ED_THREADS - 1) / ED_THREADS > 0x7fffffff) return RSA_E_UNSUPPORTED;
  return RSA_OK;
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_eimn_query_chain(const void* q_hi, const void* q_lo, int64_t q_plane_stride, int64_t q_batch_stride, void* out_hi, void* out_lo,
                                    int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t planes_a,
                                    int32_t planes_b, int32_t planes_c, int32_t gelu_in, int32_t fmt, const float* w1, const float* b1, const float* w2,
                                    const float* b2, void* stream) {
  if (!q_hi || !out_hi || !w1 || !b1 || !w2 || !b2) return set_error(RSA_E_ARG, "eimn_query_chain: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || planes_a < 0 || planes_b < 0 || planes_c < 0) return set_error(RSA_E_ARG, "eimn_query_chain: bad geometry");
  const int64_t planes = (int64_t)planes_a + planes_b + planes_c;
  if (planes < 1 || 2 * planes > 65535) return set_error(RSA_E_ARG, "eimn_query_chain: total planes must be in [1, 32767]");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "eimn_query_chain: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  if (q_plane_stride < HW || out_plane_stride < HW) return set_error(RSA_E_ARG, "eimn_query_chain: a plane stride is smaller than the map");
  if (batch > 1 && (q_batch_stride < planes * q_plane_stride || out_batch_stride < planes * out_plane_stride))
    return set_error(RSA_E_ARG, "eimn_query_chain: a batch stride is smaller than the planes of an image");
  if (q_hi == out_hi) return set_error(RSA_E_ARG, "eimn_query_chain: not in place (a tile reads its neighbours' pixels)");
  if (misaligned16(q_hi) || misaligned16(q_lo) || misaligned16(out_hi) || misaligned16(out_lo) || misaligned16(w1) || misaligned16(b1) ||
      misaligned16(w2) || misaligned16(b2))
    return set_error(RSA_E_ALIGN, "eimn_query_chain: planes and weights must be 16-byte aligned");
  const int64_t tiles = (int64_t)((W + EQ_TW - 1) / EQ_TW) * ((H + EQ_TH - 1) / EQ_TH);
  if (tiles > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "eimn_query_chain: map too large");
  ChainArgs a;
  a.q_hi = (const char*)q_hi, a.q_lo = (const char*)q_lo, a.q_ps = q_plane_stride, a.q_bs = q_batch_stride;
  a.o_hi = (char*)out_hi, a.o_lo = (char*)out_lo, a.o_ps = out_plane_stride, a.o_bs = out_batch_stride;
  a.H = H, a.W = W, a.planes_a = planes_a, a.planes_b = planes_b, a.gelu_in = gelu_in;
  a.w1 = (const f32x4*)w1, a.b1 = (const f32x4*)b1, a.w2 = (const f32x4*)w2, a.b2 = (const f32x4*)b2;
  const dim3 grid((unsigned)tiles, (unsigned)(2 * planes), (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(eimn_chain_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, a);
  });
  return launch_status("eimn_query_chain: launch failed");
}

extern "C" int rsa_eimn_sal(const void* in_hi, const void* in_lo, int64_t in_plane_stride, int64_t in_batch_stride, void* out_hi, void* out_lo,
                            int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t planes, int32_t fmt,
                            const float* weight, const float* bias, void* stream) {
  if (!in_hi || !out_hi || !weight || !bias) return set_error(RSA_E_ARG, "eimn_sal: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || planes < 1 || planes > 32767) return set_error(RSA_E_ARG, "eimn_sal: bad geometry");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "eimn_sal: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  if (in_plane_stride < HW || out_plane_stride < HW) return set_error(RSA_E_ARG, "eimn_sal: a plane stride is smaller than the map");
  if (batch > 1 && (in_batch_stride < 2 * (int64_t)planes * in_plane_stride || out_batch_stride < (int64_t)planes * out_plane_stride))
    return set_error(RSA_E_ARG, "eimn_sal: a batch stride is smaller than the planes of an image");
  if (in_hi == out_hi) return set_error(RSA_E_ARG, "eimn_sal: not in place (a pixel reads its neighbours)");
  if (misaligned16(in_hi) || misaligned16(in_lo) || misaligned16(out_hi) || misaligned16(out_lo)) return set_error(RSA_E_ALIGN, "eimn_sal: planes must be 16-byte aligned");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "eimn_sal: map too large");
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)planes, (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(eimn_sal_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)in_hi, (const char*)in_lo, in_plane_stride, in_batch_stride,
                       (char*)out_hi, (char*)out_lo, out_plane_stride, out_batch_stride, (int)H, (int)W, (int)planes, weight, bias);
  });
  return launch_status("eimn_sal: launch failed");
}

extern "C" int rsa_eimn_silu_mul(const void* f_hi, const void* f_lo, int64_t f_plane_stride, int64_t f_batch_stride, const void* v_hi, const void* v_lo,
                                 int64_t v_plane_stride, int64_t v_batch_stride, void* out_hi, void* out_lo, int64_t out_plane_stride,
                                 int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t planes, int32_t fmt, void* stream) {
  if (!f_hi || !v_hi || !out_hi) return set_error(RSA_E_ARG, "eimn_silu_mul: null operand");
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || planes < 1 || planes > 65535) return set_error(RSA_E_ARG, "eimn_silu_mul: bad geometry");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "eimn_silu_mul: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  if (f_plane_stride < HW || v_plane_stride < HW || out_plane_stride < HW) return set_error(RSA_E_ARG, "eimn_silu_mul: a plane stride is smaller than the map");
  if (batch > 1 && (f_batch_stride < (int64_t)planes * f_plane_stride || v_batch_stride < (int64_t)planes * v_plane_stride ||
                    out_batch_stride < (int64_t)planes * out_plane_stride))
    return set_error(RSA_E_ARG, "eimn_silu_mul: a batch stride is smaller than the planes of an image");
  if (misaligned16(f_hi) || misaligned16(f_lo) || misaligned16(v_hi) || misaligned16(v_lo) || misaligned16(out_hi) || misaligned16(out_lo))
    return set_error(RSA_E_ALIGN, "eimn_silu_mul: planes must be 16-byte aligned");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "eimn_silu_mul: map too large");
  const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)planes, (unsigned)batch);
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(eimn_silu_mul_kernel<decltype(F)::value>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)f_hi, (const char*)f_lo, f_plane_stride, f_batch_stride,
                       (const char*)v_hi, (const char*)v_lo, v_plane_stride, v_batch_stride, (char*)out_hi, (char*)out_lo, out_plane_stride, out_batch_stride, HW);
  });
  return launch_status("eimn_silu_mul: launch failed");
}

extern "C" int64_t rsa_eimn_dffm_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t C) {
  if (dffm_geometry(batch, H, W, C) != RSA_OK) return RSA_E_ARG;
  return (int64_t)batch * (((int64_t)H * W + ED_THREADS - 1) / ED_THREADS) * C * (int64_t)sizeof(float);
}

extern "C" int rsa_eimn_dffm_reduce(const float* z, int32_t batch, int32_t H, int32_t W, int32_t C, const float* gamma, const float* beta, float eps,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  const int g = dffm_geometry(batch, H, W, C);
  if (g != RSA_OK) return set_error(g, "eimn_dffm_reduce: bad geometry (C % 8 == 0, 8 <= C <= 128)");
  if (!z || !gamma || !beta || !workspace) return set_error(RSA_E_ARG, "eimn_dffm_reduce: null operand");
  if (workspace_bytes < rsa_eimn_dffm_workspace_bytes(batch, H, W, C)) return set_error(RSA_E_ARG, "eimn_dffm_reduce: workspace too small");
  if (misaligned16(z) || misaligned16(workspace)) return set_error(RSA_E_ALIGN, "eimn_dffm_reduce: the map and the workspace must be 16-byte aligned");
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(dffm_reduce_kernel, dim3((unsigned)((HW + ED_THREADS - 1) / ED_THREADS), (unsigned)batch), dim3(ED_THREADS), 0, (hipStream_t)stream, z, HW,
                     (int)C, gamma, beta, (double)eps, (float*)workspace);
  return launch_status("eimn_dffm_reduce: launch failed");
}

extern "C" int rsa_eimn_dffm_gates(const void* workspace, int64_t workspace_bytes, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t rc,
                                   const float* wg, const float* bg, const float* wc, const float* bc, const float* ws, const float* bs, float* gates,
                                   void* stream) {
  const int g = dffm_geometry(batch, H, W, C);
  if (g != RSA_OK) return set_error(g, "eimn_dffm_gates: bad geometry (C % 8 == 0, 8 <= C <= 128)");
  if (rc < 1 || rc > ED_MAX_RC) return set_error(RSA_E_ARG, "eimn_dffm_gates: the reduced width must be in 1..32");
  if (!workspace || !wg || !bg || !wc || !bc || !ws || !bs || !gates) return set_error(RSA_E_ARG, "eimn_dffm_gates: null operand");
  if (workspace_bytes < rsa_eimn_dffm_workspace_bytes(batch, H, W, C)) return set_error(RSA_E_ARG, "eimn_dffm_gates: workspace too small");
  if (misaligned16(workspace) || misaligned16(gates)) return set_error(RSA_E_ALIGN, "eimn_dffm_gates: the workspace and the gates must be 16-byte aligned");
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(dffm_gates_kernel, dim3((unsigned)batch), dim3(ED_THREADS), 0, (hipStream_t)stream, (const float*)workspace,
                     (int)((HW + ED_THREADS - 1) / ED_THREADS), (int)C, (int)rc, 1.0 / (double)HW, wg, bg, wc, bc, ws, bs, gates);
  return launch_status("eimn_dffm_gates: launch failed");
}

extern "C" int rsa_eimn_dffm_apply(const float* z, const float* x, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t rc, const float* gamma,
                                   const float* beta, float eps, const float* wl, const float* bl, const float* ws, const float* gates,
                                   const float* scale, const float* norm_gamma, const float* norm_beta, float norm_eps, const float* add, float* out_f32,
                                   void* out_hi, void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride, int32_t fmt, void* stream) {
  const int g = dffm_geometry(batch, H, W, C);
  if (g != RSA_OK) return set_error(g, "eimn_dffm_apply: bad geometry (C % 8 == 0, 8 <= C <= 128)");
  if (rc < 1 || rc > ED_MAX_RC) return set_error(RSA_E_ARG, "eimn_dffm_apply: the reduced width must be in 1..32");
  if (!z || !x || !gamma || !beta || !wl || !bl || !ws || !gates || !scale || !out_f32 || !out_hi) return set_error(RSA_E_ARG, "eimn_dffm_apply: null operand");
  if ((norm_gamma == nullptr) != (norm_beta == nullptr)) return set_error(RSA_E_ARG, "eimn_dffm_apply: the stage norm needs both gamma and beta");
  if (!plane_fmt_ok(fmt)) return set_error(RSA_E_ARG, "eimn_dffm_apply: fmt must be an rsa_plane_fmt");
  const int64_t HW = (int64_t)H * W;
  if (out_plane_stride < HW) return set_error(RSA_E_ARG, "eimn_dffm_apply: the plane stride is smaller than the map");
  if (batch > 1 && out_batch_stride < (int64_t)(C / 8) * out_plane_stride)
    return set_error(RSA_E_ARG, "eimn_dffm_apply: the batch stride is smaller than the planes of an image");
  if (out_f32 == z || out_f32 == add) return set_error(RSA_E_ARG, "eimn_dffm_apply: out_f32 may alias x only");
  if (misaligned16(z) || misaligned16(x) || misaligned16(add) || misaligned16(out_f32) || misaligned16(out_hi) || misaligned16(out_lo) || misaligned16(gates))
    return set_error(RSA_E_ALIGN, "eimn_dffm_apply: maps, planes and gates must be 16-byte aligned");
  ApplyArgs a;
  a.z = z, a.x = x, a.add = add, a.out = out_f32, a.HW = HW, a.C = C, a.rc = rc, a.gamma = gamma, a.beta = beta, a.eps = eps, a.wl = wl, a.bl = bl, a.wsp = ws;
  a.gates = gates, a.scale = scale, a.ngamma = norm_gamma, a.nbeta = norm_beta, a.neps = norm_eps;
  a.o_hi = (char*)out_hi, a.o_lo = (char*)out_lo, a.o_ps = out_plane_stride, a.o_bs = out_batch_stride;
  const dim3 grid((unsigned)((HW + ED_THREADS - 1) / ED_THREADS), (unsigned)batch);
  hipStream_t s = (hipStream_t)stream;
  if (fmt == RSA_PF_F16) {
    if (rc <= 16)
      hipLaunchKernelGGL((dffm_apply_kernel<RSA_PF_F16, 16>), grid, dim3(ED_THREADS), 0, s, a);
    else
      hipLaunchKernelGGL((dffm_apply_kernel<RSA_PF_F16, 32>), grid, dim3(ED_THREADS), 0, s, a);
  } else {
    if (rc <= 16)
      hipLaunchKernelGGL((dffm_apply_kernel<RSA_PF_BF16, 16>), grid, dim3(ED_THREADS), 0, s, a);
    else
      hipLaunchKernelGGL((dffm_apply_kernel<RSA_PF_BF16, 32>), grid, dim3(ED_THREADS), 0, s, a);
  }
  return launch_status("eimn_dffm_apply: launch failed");
}
