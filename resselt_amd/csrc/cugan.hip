// cugan.hip — the kernels Real-CUGAN needs beyond the fused convolution (reference resselt/archs/cugan/arch.py):
//   rsa_deconv        nn.ConvTranspose2d (k2 s2 p0, k4 s2 p3, k5 s3 p2) as stride^2 phase convolutions       arch.py:126, 130, 181, 185, 213-214
//   rsa_conv_s2       nn.Conv2d(k=2, s=2) on a window of any origin parity                                    arch.py:124, 204-206
//   rsa_region_se     SEBlock over a window, applied in place                                                 arch.py:58-69
//   rsa_cugan_input   pro affine + reflect pad + pixel_unshuffle -> split planes                              arch.py:300-306, 426-431
//   rsa_cugan_output  final crop + PixelShuffle + nearest base + pro inverse -> dtype / 8-bit store           arch.py:307-315, 395-410
// Every operand is a window (origin + size) of a larger grid: include/resselt_amd.h, "Real-CUGAN ops".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "conv_common.h"
#include "resselt_amd.h"

namespace rsa {

// ------------------------------------------------------------------------------------------------------------------ deconv / conv_s2
// Implicit GEMM on v_mfma_f32_16x16x32_{bf16,f16}: D[cout 16][cell 16] += A[cout][k 32] * B[k][cell], k = 4 units of 8 channels, a unit
// being (tap, input plane) in tap-major order.  A "cell" is one output pixel of one phase: rsa_deconv's output pixel o = stride * q + r - pad
// of phase r reads the input pixels q - d through the weight taps stride * d + r (d = 0 .. ceil((k - r) / stride) - 1 per axis);
// rsa_conv_s2's output pixel q reads 2 q + d, d = 0, 1.  A workgroup computes 4 x ROWS cell rows x 16 cell columns of one phase for all
// cout tiles; each wave owns ROWS rows; the phases of a tile are consecutive workgroups.  The B fragments come straight from global memory
// (16 consecutive pixels of one unit per 16 lanes: 256 contiguous bytes for rsa_deconv, a 32-byte stride for rsa_conv_s2); the A fragments
// of a K step are read once per wave and used for ROWS rows x CT cout tiles.
template <int CT>
struct rs_rows {
  static constexpr int value = CT >= 8 ? 2 : 4;  // 8 cout tiles: 64 accumulator VGPRs per row in three products
};

template <int FMT, int PROD, int CT, bool TRANS, bool GELU = false>
__global__ __launch_bounds__(256) void resample_conv_kernel(const rsa_resample_conv_params p, int smax) {
  constexpr int ROWS = rs_rows<CT>::value;
  constexpr int HL = PROD == 3 ? 2 : 1;
  const int s = p.stride, K = p.ksize;
  const int nphase = TRANS ? s * s : 1;
  // the phases of one tile are neighbours in the launch order: they read the same input rows and fill the same output lines in L2
  const int phase = blockIdx.x % nphase, bx = blockIdx.x / nphase, n = blockIdx.z;
  const int ry = TRANS ? phase / s : 0, rx = TRANS ? phase - ry * s : 0;
  const int tyn = TRANS ? (K - ry + s - 1) / s : K, txn = TRANS ? (K - rx + s - 1) / s : K;
  const int units = tyn * txn * p.cin_planes, steps = (units + 3) >> 2;
  const int out_h = TRANS ? (p.in_h - 1) * s - 2 * p.pad + K : p.in_h / 2;
  const int out_w = TRANS ? (p.in_w - 1) * s - 2 * p.pad + K : p.in_w / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, col = lane & 15;
  const int qx = bx * 16 + col, qy0 = (blockIdx.y * 4 + wave) * ROWS;
  const uint4* in_hi = (const uint4*)p.in_hi + (int64_t)n * p.in_batch_stride;
  const uint4* in_lo = PROD == 3 ? (const uint4*)p.in_lo + (int64_t)n * p.in_batch_stride : nullptr;
  const uint4* wph = (const uint4*)p.w_packed + (int64_t)phase * smax * CT * HL * 64;

  f32x4 acc[ROWS][CT];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[r][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int st = 0; st < steps; ++st) {
    const int u = 4 * st + grp;
    const bool uval = u < units;
    const int t = uval ? u / p.cin_planes : 0, pl = uval ? u - t * p.cin_planes : 0;
    const int dy = t / txn, dx = t - dy * txn;
    bf16x8 ah[CT], al[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const uint4* wf = wph + ((int64_t)st * CT + c) * HL * 64 + lane;
      ah[c] = __builtin_bit_cast(bf16x8, wf[0]);
      if constexpr (PROD == 3) al[c] = __builtin_bit_cast(bf16x8, wf[64]);
    }
    const int ix = TRANS ? qx - dx : 2 * qx + dx;
    const bool xval = uval && ix >= 0 && ix < p.in_w;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int qy = qy0 + r;
      const int iy = TRANS ? qy - dy : 2 * qy + dy;
      uint4 h = {0u, 0u, 0u, 0u}, l = {0u, 0u, 0u, 0u};
      if (xval && iy >= 0 && iy < p.in_h) {
        const int64_t off = (int64_t)pl * p.in_plane_stride + (int64_t)(p.in_y0 + iy) * p.in_W + p.in_x0 + ix;
        h = in_hi[off];
        if constexpr (PROD == 3) l = in_lo[off];
      }
      const bf16x8 bh = __builtin_bit_cast(bf16x8, h);
      if constexpr (PROD == 3) {
        const bf16x8 bl = __builtin_bit_cast(bf16x8, l);
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
  }

  // epilogue: lane (grp, col) holds cell column col, output channels 16 c + 4 grp .. +3 = half a unit of plane (16 c + 4 grp) / 8
  const int ox = TRANS ? s * qx + rx - p.pad : qx;
  if (ox < 0 || ox >= out_w) return;
  const int planes_out = (p.cout + 7) >> 3, p4_out = (p.cout + 3) >> 2;
  char* ob_hi = p.out_hi ? (char*)p.out_hi + (int64_t)n * p.out_batch_stride * 16 : nullptr;
  char* ob_lo = p.out_lo ? (char*)p.out_lo + (int64_t)n * p.out_batch_stride * 16 : nullptr;
  const char* rb_hi = p.res_hi ? (const char*)p.res_hi + (int64_t)n * p.res_batch_stride * 16 : nullptr;
  const char* rb_lo = p.res_lo ? (const char*)p.res_lo + (int64_t)n * p.res_batch_stride * 16 : nullptr;
  const int64_t map_hw = (int64_t)p.out_H * p.out_W;
  f32x4* of = p.out_f32 ? (f32x4*)p.out_f32 + (int64_t)n * p4_out * map_hw : nullptr;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int c0 = 16 * c + 4 * grp;
    if (c0 >= 8 * planes_out) continue;
    const f32x4 b = *(const f32x4*)(p.bias + c0);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int oy = TRANS ? s * (qy0 + r) + ry - p.pad : qy0 + r;
      if (oy < 0 || oy >= out_h) continue;
      f32x4 v = acc[r][c] + b;
      if constexpr (GELU) {  // a separate instantiation: the LeakyReLU / linear kernels keep their code
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = gelu_fast(v[j]);
      } else if (p.act == RSA_ACT_LRELU) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : v[j] * p.act_param;
      }
      if (rb_hi) {
        const int64_t roff = (((int64_t)(c0 >> 3) * p.res_plane_stride + (int64_t)(p.res_y0 + oy) * p.res_W + p.res_x0 + ox) << 4) + ((c0 & 4) << 1);
        const uint2 h = *(const uint2*)(rb_hi + roff);
        const uint2 l = rb_lo ? *(const uint2*)(rb_lo + roff) : make_uint2(0u, 0u);
        v += widen4<FMT>(h, l);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j >= p.cout) v[j] = 0.f;
      const int gy = p.out_y0 + oy, gx = p.out_x0 + ox;
      if (ob_hi) {
        uint32_t h01, l01, h23, l23;
        split2<FMT>(v[0], v[1], h01, l01);
        split2<FMT>(v[2], v[3], h23, l23);
        const int64_t off = (((int64_t)(c0 >> 3) * p.out_plane_stride + (int64_t)gy * p.out_W + gx) << 4) + ((c0 & 4) << 1);
        *(uint2*)(ob_hi + off) = make_uint2(h01, h23);
        if (ob_lo) *(uint2*)(ob_lo + off) = make_uint2(l01, l23);
      }
      if (of && c0 < 4 * p4_out) of[(int64_t)(c0 >> 2) * map_hw + (int64_t)gy * p.out_W + gx] = v;
    }
  }
}

static int rs_smax(int ksize, int stride, bool trans, int cin_planes) {
  const int t = trans ? (ksize + stride - 1) / stride : ksize;
  return (t * t * cin_planes + 3) / 4;
}

template <int FMT, int PROD, bool TRANS, bool GELU = false>
static int rs_launch(const rsa_resample_conv_params& p, hipStream_t stream) {
  const int s = p.stride, K = p.ksize;
  const int out_h = TRANS ? (p.in_h - 1) * s - 2 * p.pad + K : p.in_h / 2;
  const int out_w = TRANS ? (p.in_w - 1) * s - 2 * p.pad + K : p.in_w / 2;
  const int qh = TRANS ? (out_h - 1 + p.pad) / s + 1 : out_h, qw = TRANS ? (out_w - 1 + p.pad) / s + 1 : out_w;
  const int nphase = TRANS ? s * s : 1, smax = rs_smax(K, s, TRANS, p.cin_planes);
  const int ct = (p.cout + 15) / 16;
#define RS_GO(CT_)                                                                                                      \
  {                                                                                                                     \
    constexpr int rows = rs_rows<CT_>::value;                                                                           \
    const dim3 grid((qw + 15) / 16 * nphase, (qh + 4 * rows - 1) / (4 * rows), p.batch);                                \
    resample_conv_kernel<FMT, PROD, CT_, TRANS, GELU><<<grid, 256, 0, stream>>>(p, smax);                               \
  }
  if (ct <= 1)
    RS_GO(1)
  else if (ct <= 2)
    RS_GO(2)
  else if (ct <= 4)
    RS_GO(4)
  else
    RS_GO(8)
#undef RS_GO
  return (int)hipGetLastError();
}

static int rs_validate(const rsa_resample_conv_params* p, bool trans, const char* what) {
  (void)what;
  if (!p) return set_error(RSA_E_ARG, "resample conv: null descriptor");
  if (p->batch < 1 || p->cin_planes < 1 || p->cin_planes > 32 || p->cout < 1 || p->cout > 128 || p->in_W < 1)
    return set_error(RSA_E_ARG, "resample conv: bad geometry (cin_planes 1..32, cout 1..128)");
  if (p->reserved0 != 0 || p->reserved1 != 0) return set_error(RSA_E_ARG, "resample conv: reserved fields must be 0");
  if (trans) {
    if (p->ksize < 1 || p->ksize > 6 || p->stride < 1 || p->stride > 3 || p->pad < 0 || p->pad >= p->ksize)
      return set_error(RSA_E_UNSUPPORTED, "deconv: ksize 1..6, stride 1..3, 0 <= pad < ksize");
  } else if (p->ksize != 2 || p->stride != 2 || p->pad != 0) {
    return set_error(RSA_E_UNSUPPORTED, "conv_s2: only ksize 2, stride 2, pad 0");
  }
  if (p->in_h < 1 || p->in_w < 1 || p->in_y0 < 0 || p->in_x0 < 0 || p->in_x0 + p->in_w > p->in_W) return set_error(RSA_E_ARG, "resample conv: bad input window");
  const int out_h = trans ? (p->in_h - 1) * p->stride - 2 * p->pad + p->ksize : p->in_h / 2;
  const int out_w = trans ? (p->in_w - 1) * p->stride - 2 * p->pad + p->ksize : p->in_w / 2;
  if (out_h < 1 || out_w < 1) return set_error(RSA_E_ARG, "resample conv: empty output");
  if (p->out_y0 < 0 || p->out_x0 < 0 || p->out_y0 + out_h > p->out_H || p->out_x0 + out_w > p->out_W)
    return set_error(RSA_E_ARG, "resample conv: the output window leaves the output grid");
  if (p->in_plane_stride < (int64_t)(p->in_y0 + p->in_h) * p->in_W) return set_error(RSA_E_ARG, "resample conv: the input window leaves the input planes");
  if (p->out_hi && p->out_plane_stride < (int64_t)p->out_H * p->out_W) return set_error(RSA_E_ARG, "resample conv: bad output plane stride");
  if (p->res_hi && (p->res_y0 < 0 || p->res_x0 < 0 || p->res_x0 + out_w > p->res_W || p->res_plane_stride < (int64_t)(p->res_y0 + out_h) * p->res_W))
    return set_error(RSA_E_ARG, "resample conv: the residual window leaves its planes");
  if (p->act != RSA_ACT_NONE && p->act != RSA_ACT_LRELU && !(trans && p->act == RSA_ACT_GELU))
    return set_error(RSA_E_UNSUPPORTED, "resample conv: act must be none or LeakyReLU (rsa_deconv: or GELU)");
  if (!p->in_hi || !p->w_packed || !p->bias || (!p->out_hi && !p->out_f32) || (p->products == 3 && !p->in_lo) || (p->res_lo && !p->res_hi) ||
      (p->out_lo && !p->out_hi))
    return set_error(RSA_E_ARG, "resample conv: null operand");
  if (misaligned16(p->in_hi) || misaligned16(p->in_lo) || misaligned16(p->w_packed) || misaligned16(p->bias) || misaligned16(p->out_hi) ||
      misaligned16(p->out_lo) || misaligned16(p->out_f32) || misaligned16(p->res_hi) || misaligned16(p->res_lo))
    return set_error(RSA_E_ALIGN, "resample conv: operands must be 16-byte aligned");
  if (!((p->fmt == RSA_PF_BF16 && p->products == 3) || (p->fmt == RSA_PF_F16 && p->products == 1)))
    return set_error(RSA_E_UNSUPPORTED, "resample conv: compiled for bf16 planes with three products and fp16 planes with one product");
  return RSA_OK;
}

// ------------------------------------------------------------------------------------------------------------------ region SE
constexpr int SE_ROWS_PER_CHUNK = 16;

// stage 1: grid (chunks, planes, batch); the 8 channel sums of one plane over SE_ROWS_PER_CHUNK window rows, a fixed-shape tree in LDS
template <int FMT>
__global__ __launch_bounds__(256) void region_se_sum_kernel(const rsa_region_se_params p, int chunks) {
  __shared__ float s_red[8][256];
  const int chunk = blockIdx.x, pl = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
  const int r0 = chunk * SE_ROWS_PER_CHUNK, r1 = min(r0 + SE_ROWS_PER_CHUNK, p.h);
  const int64_t npx = (int64_t)(r1 - r0) * p.w;
  const char* hi = (const char*)p.x_hi + ((int64_t)n * p.x_batch_stride + (int64_t)pl * p.x_plane_stride) * 16;
  const char* lo = p.x_lo ? (const char*)p.x_lo + ((int64_t)n * p.x_batch_stride + (int64_t)pl * p.x_plane_stride) * 16 : nullptr;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t i = tid; i < npx; i += 256) {
    const int yy = r0 + (int)(i / p.w), xx = (int)(i % p.w);
    float v[8];
    load_unit<FMT>(hi, lo, ((int64_t)(p.y0 + yy) * p.W + p.x0 + xx) << 4, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += v[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s_red[j][tid] = acc[j];
  __syncthreads();
  for (int stride = 128; stride > 0; stride >>= 1) {
    if (tid < stride)
#pragma unroll
      for (int j = 0; j < 8; ++j) s_red[j][tid] += s_red[j][tid + stride];
    __syncthreads();
  }
  if (tid < 8) p.workspace[((int64_t)n * chunks + chunk) * (8 * p.planes) + 8 * pl + tid] = s_red[tid][0];
}

// stage 2: one workgroup per image: ordered f64 sum of the chunks -> mean; relu(W1 m + b1); sigmoid(W2 h + b2)
__global__ __launch_bounds__(256) void region_se_gate_kernel(const rsa_region_se_params p, int chunks) {
  __shared__ float s_mean[256];
  __shared__ float s_hid[64];
  const int n = blockIdx.x, tid = threadIdx.x, C = 8 * p.planes;
  if (tid < C) {
    double sum = 0.0;
    for (int k = 0; k < chunks; ++k) sum += (double)p.workspace[((int64_t)n * chunks + k) * C + tid];
    s_mean[tid] = (float)(sum / ((double)p.h * p.w));
  }
  __syncthreads();
  if (tid < p.hidden) {
    float a = p.b1[tid];
    for (int c = 0; c < C; ++c) a += p.w1[tid * C + c] * s_mean[c];
    s_hid[tid] = a > 0.f ? a : 0.f;
  }
  __syncthreads();
  if (tid < C) {
    float g = p.b2[tid];
    for (int j = 0; j < p.hidden; ++j) g += p.w2[tid * p.hidden + j] * s_hid[j];
    p.gate[(int64_t)n * C + tid] = 1.f / (1.f + expf(-g));
  }
}

// stage 3: grid (ceil(h w / 256), planes, batch): x[window] *= gate, in place
template <int FMT>
__global__ __launch_bounds__(256) void region_se_apply_kernel(const rsa_region_se_params p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.h * p.w) return;
  const int pl = blockIdx.y, n = blockIdx.z;
  const int yy = (int)(i / p.w), xx = (int)(i % p.w);
  const int64_t off = ((int64_t)n * p.x_batch_stride + (int64_t)pl * p.x_plane_stride + (int64_t)(p.y0 + yy) * p.W + p.x0 + xx) << 4;
  float v[8];
  load_unit<FMT>((const char*)p.x_hi, (const char*)p.x_lo, off, v);
  const float* g = p.gate + (int64_t)n * 8 * p.planes + 8 * pl;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] *= g[j];
  store_unit<FMT>((char*)p.x_hi, (char*)p.x_lo, off, v);
}

// ------------------------------------------------------------------------------------------------------------------ input / output stages
__device__ __forceinline__ float cg_read(const void* x, int dtype, int64_t i) {
  switch (dtype) {
    case RSA_F32:
      return ((const float*)x)[i];
    case RSA_F16:
      return (float)((const _Float16*)x)[i];
    case RSA_BF16:
      return __builtin_bit_cast(float, (uint32_t)((const uint16_t*)x)[i] << 16);
    default:
      return (float)((const uint8_t*)x)[i] / 255.f;
  }
}

__device__ __forceinline__ int cg_reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

// thread = one pixel of the out_H x out_W grid, every plane; grid (ceil(out_H out_W / 256), batch)
template <int FMT>
__global__ __launch_bounds__(256) void cugan_input_kernel(const rsa_cugan_input_params p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.out_H * p.out_W) return;
  const int n = blockIdx.y, y = (int)(i / p.out_W), x = (int)(i % p.out_W);
  const int r = p.unshuffle, cr = p.C * r * r, planes = (cr + 7) >> 3;
  const bool u8 = p.dtype == RSA_U8;
  for (int pl = 0; pl < planes; ++pl) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int co = 8 * pl + j;
      v[j] = 0.f;
      if (co < cr) {
        const int c = co / (r * r), ij = co - c * r * r, di = ij / r, dj = ij - di * r;
        const int sy = cg_reflect(y * r + di - p.pad_top, p.h), sx = cg_reflect(x * r + dj - p.pad_left, p.w);
        const int64_t src = u8 ? (((int64_t)n * p.h + sy) * p.w + sx) * p.C + c : (((int64_t)n * p.C + c) * p.h + sy) * p.w + sx;
        v[j] = cg_read(p.x, p.dtype, src) * p.in_scale + p.in_shift;
      }
    }
    store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, ((int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride + i) << 4, v);
  }
}

// thread = one output pixel, every channel; grid (ceil(out_h out_w / 256), batch)
__global__ __launch_bounds__(256) void cugan_output_kernel(const rsa_cugan_output_params p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.out_h * p.out_w) return;
  const int n = blockIdx.y, Y = (int)(i / p.out_w), X = (int)(i % p.out_w);
  const int r = p.pixel_shuffle, cm = p.C * r * r, p4 = (cm + 3) >> 2;
  const int64_t map_hw = (int64_t)p.map_H * p.map_W;
  const int64_t mpx = (int64_t)(p.y0 + Y / r) * p.map_W + p.x0 + X / r;
  const bool u8 = p.dtype == RSA_U8;
  for (int c = 0; c < p.C; ++c) {
    const int ch = c * r * r + (Y % r) * r + X % r;
    float v = p.map[(((int64_t)n * p4 + (ch >> 2)) * map_hw + mpx) * 4 + (ch & 3)];
    if (p.base) {
      const int by = Y / p.base_div, bx = X / p.base_div;
      const int64_t bi = u8 ? (((int64_t)n * p.base_h + by) * p.base_w + bx) * p.C + c : (((int64_t)n * p.C + c) * p.base_h + by) * p.base_w + bx;
      v += cg_read(p.base, p.dtype, bi) * p.base_scale + p.base_shift;
    }
    v = (v - p.out_shift) / p.out_div;
    switch (p.dtype) {
      case RSA_F32:
        ((float*)p.out)[(((int64_t)n * p.C + c) * p.out_h + Y) * p.out_w + X] = v;
        break;
      case RSA_F16:
        ((_Float16*)p.out)[(((int64_t)n * p.C + c) * p.out_h + Y) * p.out_w + X] = (_Float16)v;
        break;
      case RSA_BF16:
        ((__bf16*)p.out)[(((int64_t)n * p.C + c) * p.out_h + Y) * p.out_w + X] = (__bf16)v;
        break;
      default: {
        const float q = __builtin_rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
        ((uint8_t*)p.out)[(((int64_t)n * p.out_h + Y) * p.out_w + X) * p.C + c] = (uint8_t)q;
      }
    }
  }
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_resample_packed_weight_bytes(int32_t ksize, int32_t stride, int32_t transposed, int32_t cin_planes, int32_t cout, int32_t products) {
  if (ksize < 1 || ksize > 6 || stride < 1 || stride > 3 || cin_planes < 1 || cin_planes > 32 || cout < 1 || cout > 128 || (products != 1 && products != 3))
    return -1;
  const int64_t nphase = transposed ? stride * stride : 1;
  const int ct = (cout + 15) / 16, cts = ct <= 1 ? 1 : ct <= 2 ? 2 : ct <= 4 ? 4 : 8;
  return nphase * rs_smax(ksize, stride, transposed != 0, cin_planes) * cts * (products == 3 ? 2 : 1) * 64 * 16;
}

extern "C" int rsa_deconv(const rsa_resample_conv_params* p, void* stream) {
  const int e = rs_validate(p, true, "deconv");
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
  if (p->act == RSA_ACT_GELU)
    return p->fmt == RSA_PF_BF16 ? rs_launch<RSA_PF_BF16, 3, true, true>(*p, s) : rs_launch<RSA_PF_F16, 1, true, true>(*p, s);
  return p->fmt == RSA_PF_BF16 ? rs_launch<RSA_PF_BF16, 3, true>(*p, s) : rs_launch<RSA_PF_F16, 1, true>(*p, s);
}

extern "C" int rsa_conv_s2(const rsa_resample_conv_params* p, void* stream) {
  const int e = rs_validate(p, false, "conv_s2");
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
  return p->fmt == RSA_PF_BF16 ? rs_launch<RSA_PF_BF16, 3, false>(*p, s) : rs_launch<RSA_PF_F16, 1, false>(*p, s);
}

extern "C" int64_t rsa_region_se_workspace_bytes(int32_t batch, int32_t h, int32_t planes) {
  if (batch < 1 || h < 1 || planes < 1) return -1;
  return (int64_t)batch * ((h + SE_ROWS_PER_CHUNK - 1) / SE_ROWS_PER_CHUNK) * 8 * planes * sizeof(float);
}

extern "C" int rsa_region_se(const rsa_region_se_params* p, void* stream) {
  if (!p || !p->x_hi || !p->w1 || !p->b1 || !p->w2 || !p->b2 || !p->workspace || !p->gate) return set_error(RSA_E_ARG, "region_se: null operand");
  if (p->batch < 1 || p->planes < 1 || p->planes > 32 || p->hidden < 1 || p->hidden > 64 || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "region_se: bad geometry (C = 8 planes <= 256, hidden <= 64)");
  if (p->h < 1 || p->w < 1 || p->y0 < 0 || p->x0 < 0 || p->x0 + p->w > p->W || p->x_plane_stride < (int64_t)(p->y0 + p->h) * p->W)
    return set_error(RSA_E_ARG, "region_se: the window leaves the planes");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "region_se: bad fmt");
  if (misaligned16(p->x_hi) || misaligned16(p->x_lo)) return set_error(RSA_E_ALIGN, "region_se: planes must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (p->h + SE_ROWS_PER_CHUNK - 1) / SE_ROWS_PER_CHUNK;
  with_fmt(p->fmt, [&](auto F) { region_se_sum_kernel<decltype(F)::value><<<dim3(chunks, p->planes, p->batch), 256, 0, s>>>(*p, chunks); });
  int e = (int)hipGetLastError();
  if (e) return e;
  region_se_gate_kernel<<<p->batch, 256, 0, s>>>(*p, chunks);
  e = (int)hipGetLastError();
  if (e) return e;
  const dim3 grid((unsigned)(((int64_t)p->h * p->w + 255) / 256), p->planes, p->batch);
  with_fmt(p->fmt, [&](auto F) { region_se_apply_kernel<decltype(F)::value><<<grid, 256, 0, s>>>(*p); });
  return (int)hipGetLastError();
}

extern "C" int rsa_cugan_input(const rsa_cugan_input_params* p, void* stream) {
  if (!p || !p->x || !p->out_hi) return set_error(RSA_E_ARG, "cugan_input: null operand");
  if (p->dtype < RSA_F32 || p->dtype > RSA_U8 || !plane_fmt_ok(p->fmt) || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "cugan_input: bad dtype / fmt");
  if (p->batch < 1 || p->C < 1 || p->h < 1 || p->w < 1 || (p->unshuffle != 1 && p->unshuffle != 2) || p->out_H < 1 || p->out_W < 1)
    return set_error(RSA_E_ARG, "cugan_input: bad geometry");
  const int r = p->unshuffle, pb = r * p->out_H - p->pad_top - p->h, pr = r * p->out_W - p->pad_left - p->w;
  if (p->pad_top < 0 || p->pad_left < 0 || pb < 0 || pr < 0 || p->pad_top >= p->h || pb >= p->h || p->pad_left >= p->w || pr >= p->w)
    return set_error(RSA_E_ARG, "cugan_input: reflect pads must be in [0, size)");
  if (p->C * r * r > 8 * 32 || p->out_plane_stride < (int64_t)p->out_H * p->out_W) return set_error(RSA_E_ARG, "cugan_input: bad planes");
  if (misaligned16(p->out_hi) || misaligned16(p->out_lo)) return set_error(RSA_E_ALIGN, "cugan_input: planes must be 16-byte aligned");
  const dim3 grid((unsigned)(((int64_t)p->out_H * p->out_W + 255) / 256), p->batch);
  with_fmt(p->fmt, [&](auto F) { cugan_input_kernel<decltype(F)::value><<<grid, 256, 0, (hipStream_t)stream>>>(*p); });
  return (int)hipGetLastError();
}

extern "C" int rsa_cugan_output(const rsa_cugan_output_params* p, void* stream) {
  if (!p || !p->map || !p->out) return set_error(RSA_E_ARG, "cugan_output: null operand");
  if (p->dtype < RSA_F32 || p->dtype > RSA_U8 || p->reserved0 != 0 || p->out_div == 0.f) return set_error(RSA_E_ARG, "cugan_output: bad dtype / out_div");
  if (p->batch < 1 || p->C < 1 || p->out_h < 1 || p->out_w < 1 || (p->pixel_shuffle != 1 && p->pixel_shuffle != 2) || p->y0 < 0 || p->x0 < 0)
    return set_error(RSA_E_ARG, "cugan_output: bad geometry");
  const int r = p->pixel_shuffle;
  if (p->y0 + (p->out_h + r - 1) / r > p->map_H || p->x0 + (p->out_w + r - 1) / r > p->map_W) return set_error(RSA_E_ARG, "cugan_output: the crop leaves the map");
  if (p->base && (p->base_div < 1 || (p->out_h - 1) / p->base_div >= p->base_h || (p->out_w - 1) / p->base_div >= p->base_w))
    return set_error(RSA_E_ARG, "cugan_output: the base image does not cover the output");
  if (misaligned16(p->map)) return set_error(RSA_E_ALIGN, "cugan_output: the map must be 16-byte aligned");
  const dim3 grid((unsigned)(((int64_t)p->out_h * p->out_w + 255) / 256), p->batch);
  cugan_output_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(*p);
  return (int)hipGetLastError();
}
