// fdat.hip — the kernels of FDAT (reference resselt/archs/fdat/arch.py) that the DAT kernels do not cover:
//   rsa_fdat_interact  SimplifiedAIM + the residual add + norm2 in one pass over the C-wide stream        :521-548, :600-606
//   rsa_pa_gate        PA (x * sigmoid(conv1x1(x))) and the LeakyReLU(0.2) of the pa_up head             :282-288, :425-433
//   rsa_lda_offsets    LDA_AQU: upsampled q -> depthwise 3x3 -> group LayerNorm -> SiLU, per HR pixel     :251-259
//   rsa_lda_attention  LDA_AQU: nine deformable samples of k and v per group, softmax(q k) v             :261-279
// The window and channel attention, the channel gate, the depthwise convolutions and every Linear layer run on DAT's kernels and the
// convolution kernels (archs/fdat/arch.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

// one unit (8 channels) of a split plane at byte offset `off`: hi (+ lo) -> f32

// ------------------------------------------------------------------------------------------------ AIM interaction + residual + norm2
// A workgroup (4 waves) owns 64 pixels of ONE image; wave w holds planes w, w + 4, ... of its lane's pixel in registers (MAXP per wave),
// so the stream is read once and written once.  Per-pixel sums (the mode-1 dot product, the mean, the centred variance) are combined
// across the four waves through LDS.
template <int MAXP, int MODE, int FMT>
__global__ __launch_bounds__(256) void fdat_interact_kernel(const rsa_fdat_interact_params p) {
  __shared__ float s_red[3][4][64];
  const uint32_t HW = (uint32_t)p.H * (uint32_t)p.W;
  const int C = p.C;
  const int planes = (C + 7) >> 3, p4 = (C + 3) >> 2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t bpi = (HW + 63u) >> 6;
  const uint32_t n = blockIdx.x / bpi;
  const uint32_t pix = (blockIdx.x - n * bpi) * 64u + (uint32_t)lane;
  const bool live = pix < HW;
  const int64_t px = live ? pix : 0;
  const char* ahi = (const char*)p.a_hi + ((int64_t)n * p.a_batch_stride + px) * 16;
  const char* alo = p.a_lo ? (const char*)p.a_lo + ((int64_t)n * p.a_batch_stride + px) * 16 : nullptr;
  const char* chi = (const char*)p.c_hi + ((int64_t)n * p.c_batch_stride + px) * 16;
  const char* clo = p.c_lo ? (const char*)p.c_lo + ((int64_t)n * p.c_batch_stride + px) * 16 : nullptr;

  float v[MAXP][8], cv[MAXP][8];
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int pl = wave + 4 * k;  // uniform
#pragma unroll
    for (int j = 0; j < 8; ++j) v[k][j] = cv[k][j] = 0.f;
    if (pl < planes) {
      load_unit<FMT>(ahi, alo, (int64_t)pl * p.a_plane_stride * 16, v[k]);
      load_unit<FMT>(chi, clo, (int64_t)pl * p.c_plane_stride * 16, cv[k]);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (pl * 8 + j >= C) v[k][j] = cv[k][j] = 0.f;  // uniform test
    }
  }
  float gate = 0.f;
  if constexpr (MODE == 1) {
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
      const int pl = wave + 4 * k;
      if (pl < planes) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (pl * 8 + j < C) dot = fmaf(p.w[pl * 8 + j], v[k][j], dot);
      }
    }
    s_red[0][wave][lane] = dot;
    __syncthreads();
    gate = sigmoid_exact((s_red[0][0][lane] + s_red[0][1][lane]) + (s_red[0][2][lane] + s_red[0][3][lane]));
  }
  const float* cm = MODE == 0 ? p.cm + (int64_t)n * planes * 8 : nullptr;  // rows of rsa_channel_gate's gate: 8 * planes
  const f32x4* xb = p.x ? (const f32x4*)p.x + (int64_t)n * p4 * HW + px : nullptr;  // NULL: x_out receives f alone
  f32x4* xo = (f32x4*)p.x_out + (int64_t)n * p4 * HW + px;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int pl = wave + 4 * k;
    if (pl < planes) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int g = 2 * pl + h;
        if (g < p4) {
          f32x4 xv = xb ? xb[(int64_t)g * HW] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = 4 * h + r, ch = 8 * pl + j;
            float f;
            if constexpr (MODE == 0)
              f = fmaf(v[k][j], ch < C ? cm[ch] : 0.f, cv[k][j]);
            else
              f = fmaf(cv[k][j], gate, v[k][j]);
            xv[r] = ch < C ? xv[r] + f : 0.f;
            v[k][j] = xv[r];
            sum += xv[r];
          }
          if (live) xo[(int64_t)g * HW] = xv;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[k][4 * h + r] = 0.f;
        }
      }
    }
  }
  if (p.out_hi == nullptr) return;  // uniform: the unfused path normalises in rsa_layernorm
  s_red[1][wave][lane] = sum;
  __syncthreads();
  const float inv_c = 1.f / (float)C;
  const float mean = ((s_red[1][0][lane] + s_red[1][1][lane]) + (s_red[1][2][lane] + s_red[1][3][lane])) * inv_c;
  float var = 0.f;
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int pl = wave + 4 * k;
    if (pl < planes) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[k][j] - mean;
        var += (pl * 8 + j < C) ? d * d : 0.f;
      }
    }
  }
  s_red[2][wave][lane] = var;
  __syncthreads();
  const float rstd = 1.f / sqrtf(((s_red[2][0][lane] + s_red[2][1][lane]) + (s_red[2][2][lane] + s_red[2][3][lane])) * inv_c + p.eps);
  if (!live) return;
  char* ohi = (char*)p.out_hi + ((int64_t)n * p.out_batch_stride + px) * 16;
  char* olo = p.out_lo ? (char*)p.out_lo + ((int64_t)n * p.out_batch_stride + px) * 16 : nullptr;
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int pl = wave + 4 * k;
    if (pl < planes) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = pl * 8 + j;
        o[j] = ch < C ? (v[k][j] - mean) * rstd * p.gamma[ch] + p.beta[ch] : 0.f;
      }
      store_unit<FMT>(ohi, olo, (int64_t)pl * p.out_plane_stride * 16, o);
    }
  }
}

// ------------------------------------------------------------------------------------------------ PA gate
template <int FMT>
__global__ __launch_bounds__(256) void pa_gate_kernel(const char* xhi, const char* xlo, const char* ghi, const char* glo, int64_t plane_stride,
                                                      int64_t batch_stride, int64_t HW, int planes, int64_t total, float slope, char* ohi, char* olo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t per_img = (int64_t)planes * HW;
  const int64_t n = i / per_img, r = i - n * per_img;
  const int64_t pl = r / HW, pix = r - pl * HW;
  const int64_t off = (n * batch_stride + pl * plane_stride + pix) * 16;
  float x[8], g[8], o[8];
  load_unit<FMT>(xhi, xlo, off, x);
  load_unit<FMT>(ghi, glo, off, g);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = x[j] * sigmoid_exact(g[j]);
    o[j] = v > 0.f ? v : v * slope;
  }
  store_unit<FMT>(ohi, olo, off, o);
}

// ------------------------------------------------------------------------------------------------ LDA_AQU
constexpr int LDA_MAX_HIDDEN = 64;

// F.interpolate(..., mode='bilinear', align_corners=True) source coordinate of destination index d: the taps and weights of one axis
struct Lerp {
  int i0, i1;
  float w0, w1;
};
__device__ __forceinline__ Lerp lerp_ac(int d, float scale, int n_in) {
  const float src = scale * (float)d;
  const int i0 = min((int)src, n_in - 1);
  const float l1 = fminf(src - (float)i0, 1.f);
  return {i0, i0 + (i0 < n_in - 1 ? 1 : 0), 1.f - l1, l1};
}

// q of `hidden` channels at output pixel (y, x), bilinear from the H x W planes
template <int FMT>
__device__ __forceinline__ void lda_q_at(const char* hi, const char* lo, int64_t plane_stride, int W, int hp, const Lerp& ly, const Lerp& lx,
                                         float (&q)[LDA_MAX_HIDDEN]) {
#pragma unroll
  for (int pl = 0; pl < LDA_MAX_HIDDEN / 8; ++pl) {
    if (pl >= hp) break;
    float a[8], b[8], c[8], d[8];
    const int64_t base = (int64_t)pl * plane_stride;
    load_unit<FMT>(hi, lo, (base + (int64_t)ly.i0 * W + lx.i0) * 16, a);
    load_unit<FMT>(hi, lo, (base + (int64_t)ly.i0 * W + lx.i1) * 16, b);
    load_unit<FMT>(hi, lo, (base + (int64_t)ly.i1 * W + lx.i0) * 16, c);
    load_unit<FMT>(hi, lo, (base + (int64_t)ly.i1 * W + lx.i1) * 16, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[pl * 8 + j] = ly.w0 * (lx.w0 * a[j] + lx.w1 * b[j]) + ly.w1 * (lx.w0 * c[j] + lx.w1 * d[j]);
  }
}

// thread = output pixel
template <int FMT>
__global__ __launch_bounds__(256) void lda_offsets_kernel(const rsa_lda_offsets_params p) {
  const int64_t HWo = (int64_t)p.Hout * p.Wout;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.batch * HWo) return;
  const int64_t n = idx / HWo, pix = idx - n * HWo;
  const int i = (int)(pix / p.Wout), j = (int)(pix - (int64_t)i * p.Wout);
  const float sy = p.Hout > 1 ? (float)(p.H - 1) / (float)(p.Hout - 1) : 0.f;
  const float sx = p.Wout > 1 ? (float)(p.W - 1) / (float)(p.Wout - 1) : 0.f;
  const int hp = (p.hidden + 7) >> 3, gc = p.hidden / p.groups;
  const char* qhi = (const char*)p.q_hi + n * p.q_batch_stride * 16;
  const char* qlo = p.q_lo ? (const char*)p.q_lo + n * p.q_batch_stride * 16 : nullptr;
  float acc[LDA_MAX_HIDDEN];
#pragma unroll
  for (int c = 0; c < LDA_MAX_HIDDEN; ++c) acc[c] = 0.f;
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = i + tap / 3 - 1, xx = j + tap % 3 - 1;
    if (yy < 0 || yy >= p.Hout || xx < 0 || xx >= p.Wout) continue;  // the depthwise conv's zero padding at the output resolution
    float q[LDA_MAX_HIDDEN];
    lda_q_at<FMT>(qhi, qlo, p.q_plane_stride, p.W, hp, lerp_ac(yy, sy, p.H), lerp_ac(xx, sx, p.W), q);
#pragma unroll
    for (int c = 0; c < LDA_MAX_HIDDEN; ++c)
      if (c < p.hidden) acc[c] = fmaf(p.dw_weight[(c % gc) * 9 + tap], q[c], acc[c]);
  }
  // LayerNorm over each group's channels (the module runs on the (B * groups) batch), then SiLU
  for (int g = 0; g < p.groups; ++g) {
    float mean = 0.f;
#pragma unroll
    for (int c = 0; c < LDA_MAX_HIDDEN; ++c)
      if (c >= g * gc && c < (g + 1) * gc) mean += acc[c];
    mean /= (float)gc;
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < LDA_MAX_HIDDEN; ++c)
      if (c >= g * gc && c < (g + 1) * gc) var = fmaf(acc[c] - mean, acc[c] - mean, var);
    const float rstd = 1.f / sqrtf(var / (float)gc + p.eps);
#pragma unroll
    for (int c = 0; c < LDA_MAX_HIDDEN; ++c)
      if (c >= g * gc && c < (g + 1) * gc) {
        const float t = (acc[c] - mean) * rstd * p.gamma[c - g * gc] + p.beta[c - g * gc];
        acc[c] = t * sigmoid_exact(t);
      }
  }
  char* ohi = (char*)p.out_hi + (n * p.out_batch_stride + pix) * 16;
  char* olo = p.out_lo ? (char*)p.out_lo + (n * p.out_batch_stride + pix) * 16 : nullptr;
#pragma unroll
  for (int pl = 0; pl < LDA_MAX_HIDDEN / 8; ++pl) {
    if (pl >= hp) break;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = pl * 8 + e < p.hidden ? acc[pl * 8 + e] : 0.f;
    store_unit<FMT>(ohi, olo, (int64_t)pl * p.out_plane_stride * 16, o);
  }
}

// grid_sample(bilinear, zeros, align_corners=True) corners of the H x W map at (iy, ix); weights of corners outside the map are 0
struct Corners {
  int64_t o[4];  // pixel offsets y * W + x (0 for corners outside)
  float w[4];
};
__device__ __forceinline__ Corners corners_at(float iy, float ix, int H, int W) {
  const float fy = floorf(iy), fx = floorf(ix);
  const int y0 = (int)fy, x0 = (int)fx;
  const float ty = iy - fy, tx = ix - fx;
  Corners c;
  const int ys[2] = {y0, y0 + 1}, xs[2] = {x0, x0 + 1};
  const float wy[2] = {1.f - ty, ty}, wx[2] = {1.f - tx, tx};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const bool in = ys[a] >= 0 && ys[a] < H && xs[b] >= 0 && xs[b] < W;
      c.o[2 * a + b] = in ? (int64_t)ys[a] * W + xs[b] : 0;
      c.w[2 * a + b] = in ? wy[a] * wx[b] : 0.f;
    }
  return c;
}

// thread = output pixel; both groups, nine taps each
template <int FMT>
__global__ __launch_bounds__(256) void lda_attention_kernel(const rsa_lda_attn_params p) {
  constexpr int G = 2;
  const int64_t HWo = (int64_t)p.Hout * p.Wout;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.batch * HWo) return;
  const int64_t n = idx / HWo, pix = idx - n * HWo;
  const int i = (int)(pix / p.Wout), j = (int)(pix - (int64_t)i * p.Wout);
  const int hp = (p.hidden + 7) >> 3, hk = p.hidden / G, vc = p.C / G;
  float q[LDA_MAX_HIDDEN];
  {
    const float sy = (float)(p.H - 1) / (float)(p.Hout - 1), sx = (float)(p.W - 1) / (float)(p.Wout - 1);
    const char* qhi = (const char*)p.q_hi + n * p.q_batch_stride * 16;
    const char* qlo = p.q_lo ? (const char*)p.q_lo + n * p.q_batch_stride * 16 : nullptr;
    lda_q_at<FMT>(qhi, qlo, p.q_plane_stride, p.W, hp, lerp_ac(i, sy, p.H), lerp_ac(j, sx, p.W), q);
  }
  // sample points in the H x W maps: get_offset (:218-236) normalises by Hout - 1 / Wout - 1, grid_sample(align_corners=True) scales by
  // H - 1 / W - 1
  float py[G][9], px[G][9];
  const int p4o = (18 * G + 3) >> 2;
  const float* ob = p.offset + (n * p4o * HWo + pix) * 4;
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int cy = 18 * g + 2 * t, cx = cy + 1;
      const float dy = tanhf(ob[(int64_t)(cy >> 2) * HWo * 4 + (cy & 3)]) * p.range + (float)(t / 3 - 1);
      const float dx = tanhf(ob[(int64_t)(cx >> 2) * HWo * 4 + (cx & 3)]) * p.range + (float)(t % 3 - 1);
      const float gy = 2.f * ((float)i + dy) / (float)(p.Hout - 1) - 1.f;
      const float gx = 2.f * ((float)j + dx) / (float)(p.Wout - 1) - 1.f;
      py[g][t] = (gy + 1.f) / 2.f * (float)(p.H - 1);
      px[g][t] = (gx + 1.f) / 2.f * (float)(p.W - 1);
    }
  // scores: one head over all hidden channels, each group's k sampled at its own points
  const char* khi = (const char*)p.k_hi + n * p.k_batch_stride * 16;
  const char* klo = p.k_lo ? (const char*)p.k_lo + n * p.k_batch_stride * 16 : nullptr;
  float s[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    float acc = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const Corners cr = corners_at(py[g][t], px[g][t], p.H, p.W);
      const int pl0 = (g * hk) >> 3, pl1 = ((g + 1) * hk - 1) >> 3;
#pragma unroll
      for (int pl = 0; pl < LDA_MAX_HIDDEN / 8; ++pl) {
        if (pl < pl0 || pl > pl1) continue;
        float kv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float u[8];
          load_unit<FMT>(khi, klo, ((int64_t)pl * p.k_plane_stride + cr.o[k]) * 16, u);
#pragma unroll
          for (int e = 0; e < 8; ++e) kv[e] = fmaf(cr.w[k], u[e], kv[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int ch = pl * 8 + e;
          if (ch >= g * hk && ch < (g + 1) * hk) acc = fmaf(q[ch], kv[e] + p.rpb[t * p.hidden + ch], acc);
        }
      }
    }
    s[t] = acc * p.scale;
  }
  float m = s[0];
#pragma unroll
  for (int t = 1; t < 9; ++t) m = fmaxf(m, s[t]);
  float den = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    s[t] = expf(s[t] - m);
    den += s[t];
  }
  const float inv = 1.f / den;
#pragma unroll
  for (int t = 0; t < 9; ++t) s[t] *= inv;
  // out = P v, plane by plane of each group's v channels
  const char* vhi = (const char*)p.v_hi + n * p.v_batch_stride * 16;
  const char* vlo = p.v_lo ? (const char*)p.v_lo + n * p.v_batch_stride * 16 : nullptr;
  char* ohi = (char*)p.out_hi + (n * p.out_batch_stride + pix) * 16;
  char* olo = p.out_lo ? (char*)p.out_lo + (n * p.out_batch_stride + pix) * 16 : nullptr;
  for (int g = 0; g < G; ++g) {
    Corners cr[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) cr[t] = corners_at(py[g][t], px[g][t], p.H, p.W);
    for (int pl = (g * vc) >> 3; pl < ((g + 1) * vc) >> 3; ++pl) {
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float u[8];
          load_unit<FMT>(vhi, vlo, ((int64_t)pl * p.v_plane_stride + cr[t].o[k]) * 16, u);
          const float wk = s[t] * cr[t].w[k];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = fmaf(wk, u[e], o[e]);
        }
      store_unit<FMT>(ohi, olo, (int64_t)pl * p.out_plane_stride * 16, o);
    }
  }
}

int fd_grid(int64_t threads, unsigned& blocks) {
  const int64_t b = (threads + 255) / 256;
  if (b < 1 || b > 0x7fffffff) return RSA_E_ARG;
  blocks = (unsigned)b;
  return RSA_OK;
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_fdat_interact(const rsa_fdat_interact_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "fdat_interact: null params");
  if (p->batch < 1 || p->H < 1 || p->W < 1 || p->C < 1 || p->C > 256 || (p->mode != 0 && p->mode != 1) || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "fdat_interact: bad geometry (C 1..256, mode 0 or 1, reserved0 0)");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "fdat_interact: bad plane format");
  if (!p->a_hi || !p->c_hi || !p->x_out || (p->mode == 0 && !p->cm) || (p->mode == 1 && !p->w))
    return set_error(RSA_E_ARG, "fdat_interact: null operand");
  if (!p->x && p->out_hi) return set_error(RSA_E_ARG, "fdat_interact: norm2 needs the stream x (x NULL writes the interaction alone)");
  if (p->out_hi && (!p->gamma || !p->beta || !(p->eps > 0.f))) return set_error(RSA_E_ARG, "fdat_interact: norm2 needs gamma, beta and eps > 0");
  if (p->out_lo && !p->out_hi) return set_error(RSA_E_ARG, "fdat_interact: out_lo without out_hi");
  if (misaligned16(p->a_hi) || misaligned16(p->a_lo) || misaligned16(p->c_hi) || misaligned16(p->c_lo) || misaligned16(p->x) ||
      misaligned16(p->x_out) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "fdat_interact: maps must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->a_plane_stride < HW || p->c_plane_stride < HW || (p->out_hi && p->out_plane_stride < HW))
    return set_error(RSA_E_ARG, "fdat_interact: a plane stride is smaller than the map");
  if (HW > 0x7fffffff) return set_error(RSA_E_ARG, "fdat_interact: map too large");
  const int64_t blocks = (int64_t)p->batch * ((HW + 63) / 64);
  if (blocks > 0x7fffffff) return set_error(RSA_E_ARG, "fdat_interact: map too large");
  const int per_wave = (((p->C + 7) >> 3) + 3) >> 2;
  const dim3 grid((unsigned)blocks);
  const hipStream_t s = (hipStream_t)stream;
#define FD_GO(MAXP, MODE, FMT) hipLaunchKernelGGL((fdat_interact_kernel<MAXP, MODE, FMT>), grid, dim3(256), 0, s, *p)
#define FD_MODE(MAXP, FMT) \
  if (p->mode == 0)        \
    FD_GO(MAXP, 0, FMT);   \
  else                     \
    FD_GO(MAXP, 1, FMT);
#define FD_FMT(MAXP)             \
  if (p->fmt == RSA_PF_F16) {    \
    FD_MODE(MAXP, RSA_PF_F16)    \
  } else {                       \
    FD_MODE(MAXP, RSA_PF_BF16)   \
  }
  if (per_wave <= 2) {
    FD_FMT(2)
  } else if (per_wave <= 4) {
    FD_FMT(4)
  } else {
    FD_FMT(8)
  }
#undef FD_FMT
#undef FD_MODE
#undef FD_GO
  return launch_status("fdat_interact: launch failed");
}

extern "C" int rsa_pa_gate(const void* x_hi, const void* x_lo, const void* logit_hi, const void* logit_lo, int64_t plane_stride, int64_t batch_stride,
                           int32_t batch, int32_t H, int32_t W, int32_t planes, float slope, int32_t fmt, void* out_hi, void* out_lo, void* stream) {
  if (!x_hi || !logit_hi || !out_hi) return set_error(RSA_E_ARG, "pa_gate: null operand");
  if (batch < 1 || H < 1 || W < 1 || planes < 1 || !plane_fmt_ok(fmt))
    return set_error(RSA_E_ARG, "pa_gate: bad geometry or plane format");
  const int64_t HW = (int64_t)H * W;
  if (plane_stride < HW || batch_stride < (int64_t)planes * plane_stride) return set_error(RSA_E_ARG, "pa_gate: strides smaller than the map");
  if (misaligned16(x_hi) || misaligned16(x_lo) || misaligned16(logit_hi) || misaligned16(logit_lo) || misaligned16(out_hi) || misaligned16(out_lo))
    return set_error(RSA_E_ALIGN, "pa_gate: planes must be 16-byte aligned");
  const int64_t total = (int64_t)batch * planes * HW;
  unsigned blocks;
  if (fd_grid(total, blocks)) return set_error(RSA_E_ARG, "pa_gate: map too large");
  const hipStream_t s = (hipStream_t)stream;
  with_fmt(fmt, [&](auto F) {
    hipLaunchKernelGGL(pa_gate_kernel<decltype(F)::value>, dim3(blocks), dim3(256), 0, s, (const char*)x_hi, (const char*)x_lo, (const char*)logit_hi,
                       (const char*)logit_lo, plane_stride, batch_stride, HW, planes, total, slope, (char*)out_hi, (char*)out_lo);
  });
  return launch_status("pa_gate: launch failed");
}

extern "C" int rsa_lda_offsets(const rsa_lda_offsets_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "lda_offsets: null params");
  if (p->batch < 1 || p->H < 1 || p->W < 1 || p->Hout < 2 || p->Wout < 2 || p->reserved0 != 0 || !(p->eps > 0.f))
    return set_error(RSA_E_ARG, "lda_offsets: bad geometry (Hout, Wout >= 2, eps > 0, reserved0 0)");
  if (p->groups != 2 || p->hidden < 2 || p->hidden > LDA_MAX_HIDDEN || p->hidden % 2)
    return set_error(RSA_E_ARG, "lda_offsets: groups must be 2 and hidden even in 2..64");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "lda_offsets: bad plane format");
  if (!p->q_hi || !p->dw_weight || !p->gamma || !p->beta || !p->out_hi) return set_error(RSA_E_ARG, "lda_offsets: null operand");
  if (misaligned16(p->q_hi) || misaligned16(p->q_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "lda_offsets: planes must be 16-byte aligned");
  if (p->q_plane_stride < (int64_t)p->H * p->W || p->out_plane_stride < (int64_t)p->Hout * p->Wout)
    return set_error(RSA_E_ARG, "lda_offsets: a plane stride is smaller than its map");
  unsigned blocks;
  if (fd_grid((int64_t)p->batch * p->Hout * p->Wout, blocks)) return set_error(RSA_E_ARG, "lda_offsets: map too large");
  const hipStream_t s = (hipStream_t)stream;
  with_fmt(p->fmt, [&](auto F) {
    hipLaunchKernelGGL(lda_offsets_kernel<decltype(F)::value>, dim3(blocks), dim3(256), 0, s, *p);
  });
  return launch_status("lda_offsets: launch failed");
}

extern "C" int rsa_lda_attention(const rsa_lda_attn_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "lda_attention: null params");
  if (p->batch < 1 || p->H < 1 || p->W < 1 || p->Hout < 2 || p->Wout < 2 || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "lda_attention: bad geometry (Hout, Wout >= 2, reserved0 0)");
  if (p->groups != 2 || p->hidden < 2 || p->hidden > LDA_MAX_HIDDEN || p->hidden % 2 || p->C < 16 || p->C > 256 || p->C % 16)
    return set_error(RSA_E_ARG, "lda_attention: groups 2, hidden even in 2..64, C a multiple of 16 up to 256");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "lda_attention: bad plane format");
  if (!p->q_hi || !p->k_hi || !p->v_hi || !p->offset || !p->rpb || !p->out_hi) return set_error(RSA_E_ARG, "lda_attention: null operand");
  if (misaligned16(p->q_hi) || misaligned16(p->q_lo) || misaligned16(p->k_hi) || misaligned16(p->k_lo) || misaligned16(p->v_hi) ||
      misaligned16(p->v_lo) || misaligned16(p->offset) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "lda_attention: maps must be 16-byte aligned");
  const int64_t hw = (int64_t)p->H * p->W;
  if (p->q_plane_stride < hw || p->k_plane_stride < hw || p->v_plane_stride < hw || p->out_plane_stride < (int64_t)p->Hout * p->Wout)
    return set_error(RSA_E_ARG, "lda_attention: a plane stride is smaller than its map");
  unsigned blocks;
  if (fd_grid((int64_t)p->batch * p->Hout * p->Wout, blocks)) return set_error(RSA_E_ARG, "lda_attention: map too large");
  const hipStream_t s = (hipStream_t)stream;
  with_fmt(p->fmt, [&](auto F) {
    hipLaunchKernelGGL(lda_attention_kernel<decltype(F)::value>, dim3(blocks), dim3(256), 0, s, *p);
  });
  return launch_status("lda_attention: launch failed");
}
