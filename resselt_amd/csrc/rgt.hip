// rgt.hip — the kernels of RGT's recursive-generalisation self-attention (reference resselt/archs/rgt/arch.py, RG_SA :500-544):
//   rsa_rg_attention   softmax(Q K^T) V of every full-resolution token against the pooled key / value set of its image   :534-542
//   rsa_rg_reduce      the t-fold depthwise 4x4 stride-4 reduction (`reduction1` applied t times) in one launch          :522-523
//   rsa_layernorm_gelu GELU(LayerNorm(x)) of an f32 token map into split planes (norm_act of the pooled map)              :525-526
//   rsa_scale_add      out += gamma[c] * res: the HAI term of Block.forward                                                :612-619
// The L_SA half of RGT and the MLP run on DAT's kernels (csrc/dat.hip).
//
// rsa_rg_attention is flash-style: a workgroup (4 waves) owns 256 queries of one (image, head); the key / value set of the image (at most
// 3,969 tokens, the same for every workgroup of the image, so it is served from L2) is staged in LDS 128 keys at a time; each wave keeps
// the running max / sum / output of its two 32-query tiles in registers across the chunks.  The arithmetic is rect_attention_kernel's
// (csrc/dat.hip): S^T = K Q^T on v_mfma_f32_32x32x16, in-lane softmax, the S^T accumulators reused as the B operand of O^T = V^T P^T.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

// ------------------------------------------------------------------------------------------------ global-token cross-attention
constexpr int RG_CHUNK_T = 4;                // key tiles of 32 staged per chunk
constexpr int RG_QBLOCK = 256;               // queries per workgroup: 4 waves x 2 tiles of 32

// grid (ceil(H*W / 256), heads, batch).  Wave w owns query tiles w and w + 4 of the block.  Every key tile holds at least one real key
// (there are ceil(N' / 32) of them), so the running max is finite after the first tile; keys >= N' get -1e30 before the max.
template <int PROD, int FMT>
__global__ __launch_bounds__(256, 2) void rg_attention_kernel(const rsa_rg_attn_params p) {
  constexpr int NT = 32 * RG_CHUNK_T;
  constexpr int KROW = 40;  // bf16 per K row = 80 bytes: ds_read_b128 of 16 consecutive rows touches every bank once
  constexpr int NHL = PROD == 3 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) __bf16 s_k[NHL][NT * KROW];
  __shared__ __attribute__((aligned(16))) __bf16 s_v[NHL][NT * 32];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int head = blockIdx.y;
  const int n = blockIdx.z;
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t q0 = (int64_t)blockIdx.x * RG_QBLOCK;
  const int KT = (p.nkeys + 31) >> 5;

  const bf16x8* q_hi = (const bf16x8*)p.q_hi + (int64_t)n * p.q_batch_stride + (int64_t)head * 4 * p.q_plane_stride;
  const bf16x8* q_lo = PROD == 3 ? (const bf16x8*)p.q_lo + (int64_t)n * p.q_batch_stride + (int64_t)head * 4 * p.q_plane_stride : nullptr;
  const bf16x8* k_hi = (const bf16x8*)p.k_hi + (int64_t)n * p.k_batch_stride + (int64_t)head * 4 * p.k_plane_stride;
  const bf16x8* k_lo = PROD == 3 ? (const bf16x8*)p.k_lo + (int64_t)n * p.k_batch_stride + (int64_t)head * 4 * p.k_plane_stride : nullptr;
  const bf16x8* v_hi = (const bf16x8*)p.v_hi + (int64_t)n * p.v_batch_stride + (int64_t)head * 4 * p.v_plane_stride;
  const bf16x8* v_lo = PROD == 3 ? (const bf16x8*)p.v_lo + (int64_t)n * p.v_batch_stride + (int64_t)head * 4 * p.v_plane_stride : nullptr;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  const int lr = lane & 31;
  const int lh = lane >> 5;
  const int g16 = lane >> 4;
  const int li16 = lane & 15;
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

  // ---- per-wave state of its two query tiles ----
  bool qvalid[2];
  int64_t qpix[2];
  bf16x8 qh[2][2], ql[2][2];
  float m[2], l[2];
  f32x16 ot[2];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    qpix[qi] = q0 + 32 * (wave + 4 * qi) + lr;
    qvalid[qi] = qpix[qi] < HW;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // Q fragments (B operand): query qpix, channels 16s + 8lh .. +7 = plane 2s + lh
      qh[qi][s] = zero8;
      ql[qi][s] = zero8;
      if (qvalid[qi]) {
        qh[qi][s] = q_hi[(2 * s + lh) * p.q_plane_stride + qpix[qi]];
        if (PROD == 3) ql[qi][s] = q_lo[(2 * s + lh) * p.q_plane_stride + qpix[qi]];
      }
    }
    m[qi] = -3.0e38f;
    l[qi] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[qi][r] = 0.f;
  }
  // a wave whose two tiles are both past the map still takes part in staging and barriers; it skips the arithmetic
  const bool wave_live = q0 + 32 * wave < HW;

  for (int kt0 = 0; kt0 < KT; kt0 += RG_CHUNK_T) {
    // ---- stage K (threads 0..127) and V (threads 128..255) of key tiles [kt0, kt0 + 4): thread = key token ----
    if (kt0 > 0) __syncthreads();  // everybody is done with the previous chunk
    {
      const int t = tid & (NT - 1);
      const int key = 32 * kt0 + t;
      const bool valid = key < p.nkeys;
      if (tid < NT) {
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) {
          bf16x8 kh = zero8, kl = zero8;
          if (valid) {
            kh = k_hi[pl * p.k_plane_stride + key];
            if (PROD == 3) kl = k_lo[pl * p.k_plane_stride + key];
          }
          *(bf16x8*)&s_k[0][t * KROW + pl * 8] = kh;
          if (PROD == 3) *(bf16x8*)&s_k[NHL - 1][t * KROW + pl * 8] = kl;
        }
      } else {
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) {
          bf16x8 vh = zero8, vl = zero8;
          if (valid) {
            vh = v_hi[pl * p.v_plane_stride + key];
            if (PROD == 3) vl = v_lo[pl * p.v_plane_stride + key];
          }
          *(bf16x8*)&s_v[0][t * 32 + pl * 8] = vh;
          if (PROD == 3) *(bf16x8*)&s_v[NHL - 1][t * 32 + pl * 8] = vl;
        }
      }
    }
    __syncthreads();
    if (!wave_live) continue;
    const int ktn = (KT - kt0 < RG_CHUNK_T) ? KT - kt0 : RG_CHUNK_T;  // key tiles in this chunk

#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      // accumulator element r of lane (lr, lh): key = 32kt + (r&3) + 8(r>>2) + 4lh, query = tile row lr (one query column per lane)
      for (int kt = 0; kt < ktn; ++kt) {
        f32x16 a;
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int off = (32 * kt + lr) * KROW + (2 * s + lh) * 8;
          const bf16x8 kh = *(const bf16x8*)&s_k[0][off];
          if (PROD == 3) {
            const bf16x8 kl = *(const bf16x8*)&s_k[NHL - 1][off];
            a = mfma32<FMT>(kl, qh[qi][s], a);
            a = mfma32<FMT>(kh, ql[qi][s], a);
          }
          a = mfma32<FMT>(kh, qh[qi][s], a);
        }
        const int kbase = 32 * (kt0 + kt);
        const bool ragged = kbase + 32 > p.nkeys;  // only the last tile
        float tm = -3.0e38f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (ragged && kbase + (r & 3) + 8 * (r >> 2) + 4 * lh >= p.nkeys) a[r] = -1.0e30f;
          tm = fmaxf(tm, a[r]);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32));
        const float mn = fmaxf(m[qi], tm);
        const float alpha = expf(m[qi] - mn);  // 0 on the first tile
        m[qi] = mn;
        l[qi] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          ot[qi][r] *= alpha;
          const float e = expf(a[r] - mn);
          a[r] = e;
          l[qi] += e;
        }
        // O^T[channel][query] += V^T P^T: A = V^T through transpose reads, B = the P tile straight from the accumulators
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 vh, vl;
#pragma unroll
          for (int g2 = 0; g2 < 2; ++g2) {
            const int row = 32 * kt + 16 * s + 8 * g2 + 4 * lh + (li16 >> 2);
            const int col = 16 * (g16 & 1) + 4 * (li16 & 3);
            const bf16x4 th = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)&s_v[0][row * 32 + col]);
#pragma unroll
            for (int e = 0; e < 4; ++e) vh[g2 * 4 + e] = th[e];
            if (PROD == 3) {
              const bf16x4 tl = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)&s_v[NHL - 1][row * 32 + col]);
#pragma unroll
              for (int e = 0; e < 4; ++e) vl[g2 * 4 + e] = tl[e];
            }
          }
          float e8[8], r8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) e8[j] = a[8 * s + j];
          const bf16x8 ph = pack16<FMT>(e8);
          if (PROD == 3) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r8[j] = e8[j] - (float)ph[j];
            const bf16x8 pl = pack16<FMT>(r8);
            ot[qi] = mfma32<FMT>(vl, ph, ot[qi]);
            ot[qi] = mfma32<FMT>(vh, pl, ot[qi]);
          }
          ot[qi] = mfma32<FMT>(vh, ph, ot[qi]);
        }
      }
    }
  }

  // ---- normalise and store: lane owns query qpix, channels 8g + 4lh .. +3 ----
  char* out_hi = (char*)p.out_hi + ((int64_t)n * p.out_batch_stride + (int64_t)head * 4 * p.out_plane_stride) * 16;
  char* out_lo = p.out_lo != nullptr ? (char*)p.out_lo + ((int64_t)n * p.out_batch_stride + (int64_t)head * 4 * p.out_plane_stride) * 16 : nullptr;
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const float lsum = l[qi] + __shfl_xor(l[qi], 32);  // the two halves of a query column share m, so their partial sums just add
    if (!qvalid[qi]) continue;
    const float inv_l = 1.f / lsum;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 h, lo4;
      float v4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v4[e] = ot[qi][g * 4 + e] * inv_l;
      round4<FMT>(v4, h, lo4);
      const int64_t off = ((int64_t)g * p.out_plane_stride + qpix[qi]) * 16 + lh * 8;
      *(bf16x4*)(out_hi + off) = h;
      if (out_lo != nullptr) *(bf16x4*)(out_lo + off) = lo4;
    }
  }
}

// ------------------------------------------------------------------------------------------------ t-fold 4x4 stride-4 reduction
// Value of one pixel of the level-LV map (level 0 = the input, level k = reduction1 applied k times) whose block starts at (y0, x0) of
// the input: bias + sum of the 16 taps over the level-(LV-1) values, i.e. the reference's per-step bias, recursively.
// w / b: the taps and biases of the workgroup's 8 channels in LDS.
template <int LV>
__device__ __forceinline__ void level_value(const bf16x8* hi, const bf16x8* lo, int fmt, int W, int y0, int x0, const float (*w)[16], const float* b,
                                            float (&out)[8]) {
  if constexpr (LV == 0) {
    get_unit(hi, lo, (int64_t)y0 * W + x0, out, fmt);
  } else {
    constexpr int S = 1 << (2 * (LV - 1));  // input pixels per side of a level-(LV-1) pixel
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = 0.f;
#pragma unroll 1
    for (int a = 0; a < 16; ++a) {
      float v[8];
      level_value<LV - 1>(hi, lo, fmt, W, y0 + (a >> 2) * S, x0 + (a & 3) * S, w, b, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = fmaf(w[j][a], v[j], out[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] += b[j];
  }
}

// grid (h' * w', planes, batch); one workgroup = one output pixel x 8 channels.  Thread j computes the level-L0 pixel j of the block
// (L0 = t - 2: a 16 x 16 grid of them; t = 1: L0 = 0, a 4 x 4 grid), the last steps run in LDS.
__global__ __launch_bounds__(256) void rg_reduce_kernel(const rsa_rg_reduce_params p, int ow) {
  __shared__ float s_a[256][8];
  __shared__ float s_b[16][8];
  const int tid = threadIdx.x;
  const int opix = blockIdx.x, plane = blockIdx.y, n = blockIdx.z;
  const int oy = opix / ow, ox = opix - oy * ow;
  const int t = p.times;
  const int S = 1 << (2 * t);  // input pixels per side of an output pixel
  const bf16x8* hi = (const bf16x8*)p.in_hi + (int64_t)n * p.in_batch_stride + (int64_t)plane * p.in_plane_stride;
  const bf16x8* lo = p.in_lo != nullptr ? (const bf16x8*)p.in_lo + (int64_t)n * p.in_batch_stride + (int64_t)plane * p.in_plane_stride : nullptr;
  __shared__ float w[8][16], b[8];
  if (tid < 128) w[tid >> 4][tid & 15] = p.weight[plane * 128 + tid];
  if (tid < 8) b[tid] = p.bias[plane * 8 + tid];
  __syncthreads();
  const int grid = t == 1 ? 4 : 16;  // level-L0 pixels per side of the block
  const int side = S / grid;         // input pixels per side of a level-L0 pixel
  if (tid < grid * grid) {
    const int y0 = oy * S + (tid / grid) * side, x0 = ox * S + (tid % grid) * side;
    float v[8];
    switch (t) {
      case 1:
      case 2: level_value<0>(hi, lo, p.fmt, p.W, y0, x0, w, b, v); break;
      case 3: level_value<1>(hi, lo, p.fmt, p.W, y0, x0, w, b, v); break;
      case 4: level_value<2>(hi, lo, p.fmt, p.W, y0, x0, w, b, v); break;
      case 5: level_value<3>(hi, lo, p.fmt, p.W, y0, x0, w, b, v); break;
      default: level_value<4>(hi, lo, p.fmt, p.W, y0, x0, w, b, v); break;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_a[tid][j] = v[j];
  }
  __syncthreads();
  const float* src = &s_a[0][0];
  int g = grid;
  if (g == 16) {  // 16 x 16 -> 4 x 4
    if (tid < 128) {
      const int o = tid >> 3, j = tid & 7;
      const int y = (o >> 2) * 4, x = (o & 3) * 4;
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 16; ++a) acc = fmaf(w[j][a], s_a[(y + (a >> 2)) * 16 + x + (a & 3)][j], acc);
      s_b[o][j] = acc + b[j];
    }
    __syncthreads();
    src = &s_b[0][0];
    g = 4;
  }
  // 4 x 4 -> 1 (the output pixel); the unit is stored by thread 0
  __shared__ float s_o[8];
  if (tid < 8) {
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 16; ++a) acc = fmaf(w[tid][a], src[a * 8 + tid], acc);
    s_o[tid] = acc + b[tid];
  }
  __syncthreads();
  if (tid == 0) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = s_o[j];
    const int64_t u = (int64_t)n * p.out_batch_stride + (int64_t)plane * p.out_plane_stride + (int64_t)oy * ow + ox;
    put_unit((bf16x8*)p.out_hi, (bf16x8*)p.out_lo, u, v, p.fmt);
  }
}

// ------------------------------------------------------------------------------------------------ small elementwise kernels
// thread = pixel; two passes over the channels of an f32 NCHW4c map (the pooled map: at most 3,969 pixels per image)
__global__ __launch_bounds__(256) void layernorm_gelu_kernel(const rsa_layernorm_params p) {
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.batch * HW) return;
  const int n = (int)(idx / HW);
  const int64_t pix = idx - (int64_t)n * HW;
  const int p4 = (p.C + 3) >> 2;
  const float* x = p.x_f32 + ((int64_t)n * p4 * HW + pix) * 4;
  float sum = 0.f;
  for (int c = 0; c < p.C; ++c) sum += x[(int64_t)(c >> 2) * HW * 4 + (c & 3)];
  const float mean = sum / (float)p.C;
  float var = 0.f;
  for (int c = 0; c < p.C; ++c) {
    const float d = x[(int64_t)(c >> 2) * HW * 4 + (c & 3)] - mean;
    var = fmaf(d, d, var);
  }
  const float rstd = 1.f / sqrtf(var / (float)p.C + p.eps);
  const int planes = (p.C + 7) >> 3;
  for (int pl = 0; pl < planes; ++pl) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = pl * 8 + j;
      v[j] = c < p.C ? gelu_erf((x[(int64_t)(c >> 2) * HW * 4 + (c & 3)] - mean) * rstd * p.gamma[c] + p.beta[c]) : 0.f;
    }
    put_unit((bf16x8*)p.out_hi, (bf16x8*)p.out_lo, (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride + pix, v, p.out_fmt);
  }
}

// thread = one f32x4 of an NCHW4c map: out += gamma[c] * res
__global__ __launch_bounds__(256) void scale_add_kernel(const f32x4* res, const float* gamma, f32x4* out, int64_t HW, int p4, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int g = (int)((i / HW) % p4);
  const f32x4 r = res[i], gm = *(const f32x4*)(gamma + 4 * g);
  f32x4 o = out[i];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = fmaf(r[e], gm[e], o[e]);
  out[i] = o;
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_rg_attention(const rsa_rg_attn_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "rg_attention: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->heads < 1 || p->heads > 65535)
    return set_error(RSA_E_ARG, "rg_attention: bad geometry");
  if (p->nkeys < 1 || p->nkeys > RSA_RG_MAX_KEYS) return set_error(RSA_E_ARG, "rg_attention: nkeys must be in [1, 3969]");
  if (p->dim_qk < 1 || p->dim_qk > 32 || p->dim_v < 1 || p->dim_v > 32)
    return set_error(RSA_E_UNSUPPORTED, "rg_attention: per-head q/k and v widths must be in [1, 32]");
  if (p->reserved0 != 0) return set_error(RSA_E_ARG, "rg_attention: reserved0 must be 0");
  const bool f16 = p->fmt == RSA_PF_F16;
  if (p->fmt != RSA_PF_BF16 && !f16) return set_error(RSA_E_ARG, "rg_attention: bad plane format");
  if (p->products != 1 && (p->products != 3 || f16)) return set_error(RSA_E_UNSUPPORTED, "rg_attention: products must be 3 (bf16) or 1");
  if (!p->q_hi || !p->k_hi || !p->v_hi || !p->out_hi || (p->products == 3 && (!p->q_lo || !p->k_lo || !p->v_lo)))
    return set_error(RSA_E_ARG, "rg_attention: null pointer");
  if (misaligned16(p->q_hi) || misaligned16(p->q_lo) || misaligned16(p->k_hi) || misaligned16(p->k_lo) || misaligned16(p->v_hi) || misaligned16(p->v_lo) ||
      misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "rg_attention: pointers must be 16-byte aligned");
  if (p->k_plane_stride < p->nkeys || p->v_plane_stride < p->nkeys || p->q_plane_stride < (int64_t)p->H * p->W ||
      p->out_plane_stride < (int64_t)p->H * p->W)
    return set_error(RSA_E_ARG, "rg_attention: a plane stride is smaller than its map");
  const int64_t blocks = ((int64_t)p->H * p->W + RG_QBLOCK - 1) / RG_QBLOCK;
  if (blocks > 0x7fffffff) return set_error(RSA_E_ARG, "rg_attention: map too large");
  const dim3 grid((unsigned)blocks, (unsigned)p->heads, (unsigned)p->batch);
  const hipStream_t s = (hipStream_t)stream;
  if (f16)
    hipLaunchKernelGGL((rg_attention_kernel<1, RSA_PF_F16>), grid, dim3(256), 0, s, *p);
  else if (p->products == 3)
    hipLaunchKernelGGL((rg_attention_kernel<3, RSA_PF_BF16>), grid, dim3(256), 0, s, *p);
  else
    hipLaunchKernelGGL((rg_attention_kernel<1, RSA_PF_BF16>), grid, dim3(256), 0, s, *p);
  return launch_status("rg_attention: launch failed");
}

extern "C" int rsa_rg_reduce(const rsa_rg_reduce_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "rg_reduce: null params");
  if (p->times < 1 || p->times > 6) return set_error(RSA_E_UNSUPPORTED, "rg_reduce: times must be in [1, 6]");
  if (p->batch < 1 || p->batch > 65535 || p->planes < 1 || p->planes > 65535 || p->H < 1 || p->W < 1 || !plane_fmt_ok(p->fmt))
    return set_error(RSA_E_ARG, "rg_reduce: bad geometry");
  const int oh = p->H >> (2 * p->times), ow = p->W >> (2 * p->times);
  if (oh < 1 || ow < 1) return set_error(RSA_E_ARG, "rg_reduce: the map reduces to nothing (H or W < 4^times)");
  if (!p->in_hi || !p->out_hi || !p->weight || !p->bias) return set_error(RSA_E_ARG, "rg_reduce: null pointer");
  if (misaligned16(p->in_hi) || misaligned16(p->in_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "rg_reduce: planes must be 16-byte aligned");
  if ((int64_t)oh * ow > 0x7fffffff) return set_error(RSA_E_ARG, "rg_reduce: map too large");
  hipLaunchKernelGGL(rg_reduce_kernel, dim3((unsigned)(oh * ow), (unsigned)p->planes, (unsigned)p->batch), dim3(256), 0, (hipStream_t)stream, *p, ow);
  return launch_status("rg_reduce: launch failed");
}

extern "C" int rsa_layernorm_gelu(const rsa_layernorm_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "layernorm_gelu: null params");
  if (p->batch < 1 || p->H < 1 || p->W < 1 || p->C < 1 || !(p->eps > 0.f) || p->reserved0 != 0 || !plane_fmt_ok(p->out_fmt))
    return set_error(RSA_E_ARG, "layernorm_gelu: bad geometry");
  if (!p->x_f32 || !p->gamma || !p->beta || !p->out_hi || p->out_f32) return set_error(RSA_E_ARG, "layernorm_gelu: needs x, gamma, beta, out_hi (no out_f32)");
  if (misaligned16(p->x_f32) || misaligned16(p->out_hi) || misaligned16(p->out_lo)) return set_error(RSA_E_ALIGN, "layernorm_gelu: pointers must be 16-byte aligned");
  const int64_t total = (int64_t)p->batch * p->H * p->W;
  if ((total + 255) / 256 > 0x7fffffff) return set_error(RSA_E_ARG, "layernorm_gelu: map too large");
  hipLaunchKernelGGL(layernorm_gelu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("layernorm_gelu: launch failed");
}

extern "C" int rsa_scale_add(const float* res, const float* gamma, float* out, int32_t batch, int32_t H, int32_t W, int32_t C, void* stream) {
  if (!res || !gamma || !out) return set_error(RSA_E_ARG, "scale_add: null pointer");
  if (batch < 1 || H < 1 || W < 1 || C < 1) return set_error(RSA_E_ARG, "scale_add: bad geometry");
  if (misaligned16(res) || misaligned16(gamma) || misaligned16(out)) return set_error(RSA_E_ALIGN, "scale_add: pointers must be 16-byte aligned");
  const int p4 = (C + 3) >> 2;
  const int64_t HW = (int64_t)H * W, total = (int64_t)batch * p4 * HW;
  if ((total + 255) / 256 > 0x7fffffff) return set_error(RSA_E_ARG, "scale_add: map too large");
  hipLaunchKernelGGL(scale_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)res, gamma, (f32x4*)out,
                     HW, p4, total);
  return launch_status("scale_add: launch failed");
}
