// gaterv2.hip — what GateRv2 adds to the kernels of the library (reference resselt/archs/gaterv2/arch.py):
//   rsa_gaterv2_linear_attention   the latent Attention: l2-normalised linear attention, m <= 64 query / key channels, C <= 1024 value
//                                  channels, over all tokens; three kernels                                                     :215-250
// All arithmetic f32, no atomics, every sum in an order fixed by the map size alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd_gaterv2.h"

namespace rsa {
namespace {

constexpr int LA_CHUNK = RSA_GATERV2_TOKEN_CHUNK, LA_SUB = 64, LA_MAXM = 64;
constexpr int LA_VG = 64;                 // value channels of one workgroup: 8 planes
constexpr int LA_KLD = LA_MAXM + 4;       // row stride of the staged kn: a multiple of 4 (16-byte rows), 4 banks apart
constexpr int LA_VLD = LA_VG + 1;         // row stride of the staged v: odd, so lanes with consecutive tokens hit consecutive banks

__host__ __device__ inline int64_t la_chunks(int64_t tokens) { return (tokens + LA_CHUNK - 1) / LA_CHUNK; }
// one record [M m x C | ksum m | vsum C]; an image owns 1 + chunks of them: the finished one, then one per chunk
__host__ __device__ inline int64_t la_rec(int C, int m) { return (int64_t)m * C + m + C; }

// The first m channels of operand `plane0` (q: 0, k: mp) of token t, scaled by the inverse of their l2 norm: the sum of squares is one fma
// chain from 0 over ascending channels.  dst[j * stride], j < m.
template <int FMT>
__device__ __forceinline__ void la_unit_vector(const rsa_gaterv2_attn_params& p, int n, int plane0, int64_t t, float* dst, int stride) {
  const int m = p.m, mp = (m + 7) >> 3;
  const int64_t base = (int64_t)n * p.qkv_batch_stride + (int64_t)plane0 * p.qkv_plane_stride + t;
  float v[LA_MAXM / 8][8];  // every unit of the token is in flight at once: the loads do not wait for one another
#pragma unroll
  for (int q = 0; q < LA_MAXM / 8; ++q)
    if (q < mp) load_unit<FMT>((const char*)p.qkv_hi, (const char*)p.qkv_lo, (base + (int64_t)q * p.qkv_plane_stride) * 16, v[q]);
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < LA_MAXM / 8; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (8 * q + j < m) ss = fmaf(v[q][j], v[q][j], ss);
  const float inv = 1.f / sqrtf(ss);
#pragma unroll
  for (int q = 0; q < LA_MAXM / 8; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (8 * q + j < m) dst[(8 * q + j) * stride] = v[q][j] * inv;
}

// grid (chunks, ceil(C / 64), batch), 256 threads: the part of one chunk's record that belongs to 64 value channels, 64 tokens at a time.
// kn of the sub-chunk goes to LDS once ([token][LA_KLD], columns >= m stay zero), v as f32 [token][LA_VLD].  A thread owns value channel
// tid & 63 and the `jper` consecutive key channels of its wave (a multiple of 4: kn is read as wave-uniform 16-byte rows); each entry of M
// is ONE fma chain from 0 over the chunk's tokens in ascending order.  Wave 0 also sums v, and in value group 0 wave 1 sums kn.
template <int FMT>
__global__ __launch_bounds__(256) void gaterv2_attn_partial_kernel(const rsa_gaterv2_attn_params p, int chunks) {
  __shared__ __attribute__((aligned(16))) float ks[LA_SUB * LA_KLD];
  __shared__ float vs[LA_SUB * LA_VLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.y, n = blockIdx.z;
  const int m = p.m, mp = (m + 7) >> 3, C = p.C;
  const int64_t tokens = (int64_t)p.H * p.W;
  const int planes = min(LA_VG >> 3, (C >> 3) - 8 * g);  // value planes of this group
  const int jper = (((m + 3) >> 2) + 3) & ~3;              // key channels per wave
  const int j0 = wave * jper, jn = max(0, min(jper, m - j0));
  for (int e = tid; e < LA_SUB * LA_KLD; e += 256) ks[e] = 0.f;
  for (int e = tid; e < LA_SUB * LA_VLD; e += 256) vs[e] = 0.f;
  float acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  float side = 0.f;  // wave 0: vsum of channel `lane`; wave 1 of group 0: ksum of key channel `lane`
  for (int sub = 0; sub < LA_CHUNK / LA_SUB; ++sub) {
    const int64_t t0 = (int64_t)blockIdx.x * LA_CHUNK + sub * LA_SUB;
    if (t0 >= tokens) break;  // (block-uniform)
    const int nt = (int)min((int64_t)LA_SUB, tokens - t0);
    __syncthreads();
    if (tid < nt) la_unit_vector<FMT>(p, n, mp, t0 + tid, ks + tid * LA_KLD, 1);
    for (int e = tid; e < planes * LA_SUB; e += 256) {
      const int pl = e / LA_SUB, t = e - pl * LA_SUB;
      if (t >= nt) continue;
      float v[8];
      const int64_t u = (int64_t)n * p.qkv_batch_stride + (int64_t)(2 * mp + 8 * g + pl) * p.qkv_plane_stride + t0 + t;
      load_unit<FMT>((const char*)p.qkv_hi, (const char*)p.qkv_lo, u * 16, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) vs[t * LA_VLD + 8 * pl + j] = v[j];
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < nt; ++t) {
      const float v = vs[t * LA_VLD + lane];
      const float* kr = ks + t * LA_KLD + j0;
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        if (4 * e4 < jn) {  // (wave-uniform)
          const f32x4 k4 = *(const f32x4*)(kr + 4 * e4);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[4 * e4 + i] = fmaf(k4[i], v, acc[4 * e4 + i]);
        }
      }
      if (wave == 0)
        side += v;
      else if (wave == 1 && g == 0)
        side += ks[t * LA_KLD + lane];
    }
  }
  float* rec = p.workspace + ((int64_t)n * (chunks + 1) + 1 + blockIdx.x) * la_rec(C, m);
  const int c = LA_VG * g + lane;
  if (c < C) {
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e < jn) rec[(int64_t)(j0 + e) * C + c] = acc[e];
    if (wave == 0) rec[(int64_t)m * C + m + c] = side;
  }
  if (wave == 1 && g == 0 && lane < m) rec[(int64_t)m * C + lane] = side;
}

// grid (ceil(record / 256), batch), 256 threads: every entry of the records added in ascending chunk order from 0, eps added to ksum
__global__ __launch_bounds__(256) void gaterv2_attn_finish_kernel(const rsa_gaterv2_attn_params p, int chunks) {
  const int64_t rec = la_rec(p.C, p.m);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rec) return;
  float* head = p.workspace + (int64_t)blockIdx.y * (chunks + 1) * rec;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += head[(int64_t)(1 + c) * rec + e];
  const int64_t k0 = (int64_t)p.m * p.C;
  if (e >= k0 && e < k0 + p.m) s += p.eps;
  head[e] = s;
}

// grid (ceil(tokens / 64), ceil(C / 64), batch), 256 threads: 64 tokens x 64 value channels.  M of the group ([m][64], 16 KB at most) and
// the tokens' qn ([m][64 tokens]) go to LDS; wave 0 forms qn and t.  A lane owns a token, wave w the group's planes 2 w and 2 w + 1: 16 fma
// chains from vsum over ascending j, M read as wave-uniform 16-byte rows, then the product with t.
template <int FMT>
__global__ __launch_bounds__(256) void gaterv2_attn_apply_kernel(const rsa_gaterv2_attn_params p, int chunks) {
  __shared__ __attribute__((aligned(16))) float Ms[LA_MAXM * LA_VG];
  __shared__ float qs[LA_MAXM * 64];
  __shared__ float ts[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.y, n = blockIdx.z;
  const int m = p.m, C = p.C;
  const int64_t tokens = (int64_t)p.H * p.W;
  const int64_t t = (int64_t)blockIdx.x * 64 + lane;
  const float* head = p.workspace + (int64_t)n * (chunks + 1) * la_rec(C, m);
  const int width = min(LA_VG, C - LA_VG * g);  // value channels of this group
  for (int e = tid; e < m * LA_VG; e += 256) {
    const int j = e >> 6, cc = e & 63;
    Ms[e] = cc < width ? head[(int64_t)j * C + LA_VG * g + cc] : 0.f;
  }
  if (wave == 0) {
    float tv = 0.f;
    if (t < tokens) {
      la_unit_vector<FMT>(p, n, 0, t, qs + lane, 64);
      const float* ksum = head + (int64_t)m * C;
      float d = 0.f;
      for (int j = 0; j < m; ++j) d = fmaf(qs[j * 64 + lane], ksum[j], d);
      tv = 1.f / ((float)tokens + d);
    }
    ts[lane] = tv;
  }
  __syncthreads();
  if (t >= tokens) return;
  const int c0 = 16 * wave;  // of the group
  if (c0 >= width) return;
  const float* vsum = head + (int64_t)m * C + m + LA_VG * g + c0;
  const bool second = c0 + 8 < width;
  float acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = (e < 8 || second) ? vsum[e] : 0.f;
#pragma unroll 4
  for (int j = 0; j < m; ++j) {
    const float qj = qs[j * 64 + lane];
    const float* mr = Ms + j * LA_VG + c0;
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      const f32x4 m4 = *(const f32x4*)(mr + 4 * e4);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[4 * e4 + i] = fmaf(qj, m4[i], acc[4 * e4 + i]);
    }
  }
  const float tv = ts[lane];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] *= tv;
  const int pl = (LA_VG >> 3) * g + 2 * wave;
  const int64_t uo = (int64_t)n * p.out_batch_stride + (int64_t)pl * p.out_plane_stride + t;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = acc[e];
  store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, uo * 16, o);
  if (second) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = acc[8 + e];
    store_unit<FMT>((char*)p.out_hi, (char*)p.out_lo, (uo + p.out_plane_stride) * 16, o);
  }
}

inline bool la_geometry_ok(int batch, int H, int W, int C, int m) {
  return batch >= 1 && batch <= 65535 && H >= 1 && W >= 1 && C >= 1 && m >= 1 && (int64_t)H * W <= 0x7fffffff;
}
inline bool la_supported(int C, int m) { return !(C & 7) && C >= 16 && C <= 1024 && m <= LA_MAXM; }

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_gaterv2_attn_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t C, int32_t m) {
  if (!la_geometry_ok(batch, H, W, C, m) || !la_supported(C, m) || m > C) return 0;
  return ((int64_t)batch * (la_chunks((int64_t)H * W) + 1) * la_rec(C, m) * 4 + 15) & ~(int64_t)15;
}

extern "C" int rsa_gaterv2_linear_attention(const rsa_gaterv2_attn_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gaterv2_linear_attention: null params");
  if (!la_geometry_ok(p->batch, p->H, p->W, p->C, p->m) || p->reserved0 != 0 || !plane_fmt_ok(p->fmt))
    return set_error(RSA_E_ARG, "gaterv2_linear_attention: bad geometry (fmt 0 or 1, reserved0 0)");
  if (!la_supported(p->C, p->m))
    return set_error(RSA_E_UNSUPPORTED, "gaterv2_linear_attention: C must be a multiple of 8 in 16..1024, m 1..64");
  if (p->m > p->C) return set_error(RSA_E_ARG, "gaterv2_linear_attention: m must not exceed C");
  if (!p->qkv_hi || !p->out_hi || !p->workspace) return set_error(RSA_E_ARG, "gaterv2_linear_attention: null pointer");
  if (misaligned16(p->qkv_hi) || misaligned16(p->qkv_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo) || misaligned16(p->workspace))
    return set_error(RSA_E_ALIGN, "gaterv2_linear_attention: the planes and the workspace must be 16-byte aligned");
  const int64_t tokens = (int64_t)p->H * p->W;
  if (p->qkv_plane_stride < tokens || p->out_plane_stride < tokens || p->qkv_batch_stride < 0 || p->out_batch_stride < 0)
    return set_error(RSA_E_ARG, "gaterv2_linear_attention: a plane stride is smaller than the map");
  if (p->qkv_hi == p->out_hi || (p->qkv_lo && p->qkv_lo == p->out_lo))
    return set_error(RSA_E_ARG, "gaterv2_linear_attention: qkv and out must not overlap");
  if (p->workspace_bytes < rsa_gaterv2_attn_workspace_bytes(p->batch, p->H, p->W, p->C, p->m))
    return set_error(RSA_E_ARG, "gaterv2_linear_attention: workspace too small (rsa_gaterv2_attn_workspace_bytes)");
  const int chunks = (int)la_chunks(tokens);
  const unsigned groups = (unsigned)((p->C + LA_VG - 1) / LA_VG);
  const hipStream_t s = (hipStream_t)stream;
  with_fmt(p->fmt, [&](auto F) {
    constexpr int FMT = decltype(F)::value;
    hipLaunchKernelGGL(gaterv2_attn_partial_kernel<FMT>, dim3((unsigned)chunks, groups, (unsigned)p->batch), dim3(256), 0, s, *p, chunks);
    hipLaunchKernelGGL(gaterv2_attn_finish_kernel, dim3((unsigned)((la_rec(p->C, p->m) + 255) / 256), (unsigned)p->batch), dim3(256), 0, s, *p, chunks);
    hipLaunchKernelGGL(gaterv2_attn_apply_kernel<FMT>, dim3((unsigned)((tokens + 63) / 64), groups, (unsigned)p->batch), dim3(256), 0, s, *p, chunks);
  });
  return launch_status("gaterv2_linear_attention: launch failed");
}
