// atd.hip — the kernels of ATD (reference resselt/archs/atd/arch.py) that the existing kernels do not cover:
//   rsa_atd_dict       k^ = normalize(wk td + bk) and V^T = (wv td + bv)^T of the per-image token dictionary               :236-241
//   rsa_atd_ca         ATD_CA: cosine logits against the dictionary, softmax, category id (first maximum), sim V on MFMA     :234-249
//   rsa_atd_sort       stable counting sort of the category ids: permutation and inverse                                    :304-307
//   rsa_atd_attention  softmax(scale q k^T + bias + mask) v over token groups (shifted windows, or categories through perm)  :151-188, :297-331
//   rsa_atd_dwconv     x + GELU(dw5x5(x)): ConvFFN's middle                                                                  :81-85
//   rsa_atd_refine     adaptive token refinement of the dictionary                                                           :483-487
// The similarity path is f32 (VALU) in every precision mode, so category ids do not depend on the precision policy.  No atomics decide a
// result: the only ones are integer histogram counts in LDS, whose sum does not depend on the order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd.h"

namespace rsa {
namespace {

constexpr int ATD_MAX_C = 256, ATD_MAX_M = 128, ATD_MAX_RC = 16;

// ------------------------------------------------------------------------------------------------ dictionary
// grid (Cp * 128 / 256 + 1, batch).  Blocks [0, Cp/2): one V^T element per thread; the last block: the normalised keys.
__global__ __launch_bounds__(256) void atd_dict_kernel(const rsa_atd_dict_params p, int Cp) {
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const float* td = p.td + (int64_t)n * p.m * p.C;
  if ((int)blockIdx.x == Cp / 2) {
    if (tid < ATD_MAX_M) {
      float k[ATD_MAX_RC];
      float nrm = 0.f;
#pragma unroll
      for (int j = 0; j < ATD_MAX_RC; ++j) {
        float acc = 0.f;
        if (j < p.rc && tid < p.m) {
          for (int c = 0; c < p.C; ++c) acc = fmaf(p.wk[j * p.C + c], td[tid * p.C + c], acc);
          if (p.bk != nullptr) acc += p.bk[j];
        }
        k[j] = acc;
        nrm = fmaf(acc, acc, nrm);
      }
      const float d = fmaxf(sqrtf(nrm), 1e-12f);
      if (tid < p.m) {
#pragma unroll
        for (int j = 0; j < ATD_MAX_RC; ++j) p.kn[((int64_t)n * p.m + tid) * 16 + j] = k[j] / d;
      }
    }
    return;
  }
  const int idx = blockIdx.x * 256 + tid;  // < Cp * 128
  const int c = idx >> 7, k = idx & 127;
  float v = 0.f;
  if (c < p.C && k < p.m) {
    for (int i = 0; i < p.C; ++i) v = fmaf(p.wv[c * p.C + i], td[k * p.C + i], v);
    if (p.bv != nullptr) v += p.bv[c];
  }
  const __bf16 h = (__bf16)v;
  const int64_t o = (int64_t)n * Cp * 128 + idx;
  ((__bf16*)p.vt_hi)[o] = h;
  ((__bf16*)p.vt_lo)[o] = (__bf16)(v - (float)h);
}

// ------------------------------------------------------------------------------------------------ dictionary cross-attention
// grid (ceil(HW / 128), batch); a wave owns 32 pixels, the lane pair (lr, lr + 32) one pixel: lane half lh holds the dictionary tokens
// 16s + 8lh + j (s < MS, j < 8), which is the B operand order of v_mfma_f32_32x32x16 (k = 8lh + j), so the softmax output feeds sim V
// straight from registers.  A = V^T rows from global memory (at most 64 KB per image and half: L2).
template <int MS, int PROD>
__global__ __launch_bounds__(256) void atd_ca_kernel(const rsa_atd_ca_params p) {
  __shared__ __attribute__((aligned(16))) float s_wq[ATD_MAX_C][16];
  __shared__ __attribute__((aligned(16))) float s_kn[ATD_MAX_M][16];
  __shared__ float s_sc[ATD_MAX_M];
  __shared__ float s_bq[16];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int n = blockIdx.y;
  const int64_t HW = (int64_t)p.H * p.W;
  const int P4 = (p.C + 3) >> 2;
  const int Cp = (p.C + 31) & ~31;
  for (int i = tid; i < ATD_MAX_C * 16; i += 256) {
    const int c = i >> 4, j = i & 15;
    s_wq[c][j] = (c < p.C && j < p.rc) ? p.wq[j * p.C + c] : 0.f;
  }
  for (int i = tid; i < ATD_MAX_M * 16; i += 256) {
    const int k = i >> 4;
    s_kn[k][i & 15] = k < p.m ? p.kn[((int64_t)n * p.m + k) * 16 + (i & 15)] : 0.f;
  }
  if (tid < ATD_MAX_M) s_sc[tid] = tid < p.m ? p.scale[tid] : 0.f;
  if (tid < 16) s_bq[tid] = (p.bq != nullptr && tid < p.rc) ? p.bq[tid] : 0.f;
  __syncthreads();

  const int64_t pix = (int64_t)blockIdx.x * 128 + wave * 32 + lr;
  const bool valid = pix < HW;
  const int64_t pc = valid ? pix : HW - 1;
  const f32x4* xn = (const f32x4*)p.xn + (int64_t)n * P4 * HW;

  float q[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) q[j] = 0.f;
  for (int g = lh; g < P4; g += 2) {
    const f32x4 x = xn[(int64_t)g * HW + pc];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * g + e;
      const float xe = c < p.C ? x[e] : 0.f;
      const f32x4* w = (const f32x4*)&s_wq[c < p.C ? c : 0][0];
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4) {
        const f32x4 wv = w[j4];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) q[4 * j4 + e2] = fmaf(xe, wv[e2], q[4 * j4 + e2]);
      }
    }
  }
  float nrm = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    q[j] += __shfl_xor(q[j], 32);
    q[j] += s_bq[j];
    nrm = fmaf(q[j], q[j], nrm);
  }
  const float den = fmaxf(sqrtf(nrm), 1e-12f);
#pragma unroll
  for (int j = 0; j < 16; ++j) q[j] /= den;

  float pr[MS][8];
  float mx = -3.0e38f;
#pragma unroll
  for (int s = 0; s < MS; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = 16 * s + 8 * lh + j;
      const f32x4* kr = (const f32x4*)&s_kn[key][0];
      float d = 0.f;
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4) {
        const f32x4 kv = kr[j4];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) d = fmaf(q[4 * j4 + e2], kv[e2], d);
      }
      const float lg = key < p.m ? d * s_sc[key] : -3.0e38f;
      pr[s][j] = lg;
      mx = fmaxf(mx, lg);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < MS; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = 16 * s + 8 * lh + j;
      const float e = key < p.m ? expf(pr[s][j] - mx) : 0.f;
      pr[s][j] = e;
      sum += e;
    }
  }
  sum += __shfl_xor(sum, 32);
  float best = -1.f;
  int bi = 0;
#pragma unroll
  for (int s = 0; s < MS; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = 16 * s + 8 * lh + j;
      const float v = pr[s][j] / sum;
      pr[s][j] = v;
      if (key < p.m && v > best) {
        best = v;
        bi = key;
      }
    }
  }
  {
    const float ob = __shfl_xor(best, 32);
    const int oi = __shfl_xor(bi, 32);
    if (ob > best || (ob == best && oi < bi)) bi = oi;
  }
  if (valid) {
    if (p.ids != nullptr && lh == 0) p.ids[(int64_t)n * HW + pix] = bi;
    if (p.sim != nullptr) {
      float* sb = p.sim + ((int64_t)n * HW + pix) * p.m;
#pragma unroll
      for (int s = 0; s < MS; ++s) {
        const int key0 = 16 * s + 8 * lh;
        if ((p.m & 3) == 0) {
          if (key0 + 4 <= p.m) *(f32x4*)(sb + key0) = (f32x4){pr[s][0], pr[s][1], pr[s][2], pr[s][3]};
          if (key0 + 8 <= p.m) *(f32x4*)(sb + key0 + 4) = (f32x4){pr[s][4], pr[s][5], pr[s][6], pr[s][7]};
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (key0 + j < p.m) sb[key0 + j] = pr[s][j];
        }
      }
    }
  }

  bf16x8 ph[MS], pl[MS];
#pragma unroll
  for (int s = 0; s < MS; ++s) {
    ph[s] = pack16<RSA_PF_BF16>(pr[s]);
    if (PROD == 3) {
      float r8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r8[j] = pr[s][j] - (float)ph[s][j];
      pl[s] = pack16<RSA_PF_BF16>(r8);
    }
  }
  const __bf16* vth = (const __bf16*)p.vt_hi + (int64_t)n * Cp * 128;
  const __bf16* vtl = (const __bf16*)p.vt_lo + (int64_t)n * Cp * 128;
  f32x4* out = (f32x4*)p.out + (int64_t)n * P4 * HW;
  for (int ct = 0; ct < (Cp >> 5); ++ct) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int64_t row = (int64_t)(32 * ct + lr) * 128 + 8 * lh;
#pragma unroll
    for (int s = 0; s < MS; ++s) {
      const bf16x8 vh = *(const bf16x8*)(vth + row + 16 * s);
      if (PROD == 3) {
        const bf16x8 vl = *(const bf16x8*)(vtl + row + 16 * s);
        acc = mfma32<RSA_PF_BF16>(vl, ph[s], acc);
        acc = mfma32<RSA_PF_BF16>(vh, pl[s], acc);
      }
      acc = mfma32<RSA_PF_BF16>(vh, ph[s], acc);
    }
    if (valid) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int G = 8 * ct + 2 * g + lh;  // channels 32ct + 8g + 4lh .. +3
        if (G < P4) out[(int64_t)G * HW + pix] = (f32x4){acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ stable counting sort
constexpr int SORT_CHUNK = 2048;

__device__ __forceinline__ int clamp_id(int id) { return id < 0 ? 0 : id > ATD_MAX_M - 1 ? ATD_MAX_M - 1 : id; }

// grid (chunks, batch): counts of every category in a chunk of 2048 tokens
__global__ __launch_bounds__(256) void atd_sort_hist_kernel(const int32_t* ids, int64_t n, int32_t* hist) {
  __shared__ int s_h[ATD_MAX_M];
  const int tid = threadIdx.x;
  if (tid < ATD_MAX_M) s_h[tid] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * SORT_CHUNK;
  for (int i = tid; i < SORT_CHUNK; i += 256)
    if (t0 + i < n) atomicAdd(&s_h[clamp_id(ids[(int64_t)blockIdx.y * n + t0 + i])], 1);  // integer counts: the order does not matter
  __syncthreads();
  if (tid < ATD_MAX_M) hist[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ATD_MAX_M + tid] = s_h[tid];
}

// grid (batch), 128 threads: counts -> first sorted position of every (chunk, category), in place
__global__ __launch_bounds__(128) void atd_sort_scan_kernel(int32_t* hist, int chunks) {
  __shared__ int s_tot[ATD_MAX_M];
  const int bin = threadIdx.x;
  int32_t* h = hist + (int64_t)blockIdx.x * chunks * ATD_MAX_M;
  int tot = 0;
  for (int c = 0; c < chunks; ++c) tot += h[c * ATD_MAX_M + bin];
  s_tot[bin] = tot;
  __syncthreads();
  int base = 0;
  for (int b = 0; b < bin; ++b) base += s_tot[b];
  for (int c = 0; c < chunks; ++c) {
    const int v = h[c * ATD_MAX_M + bin];
    h[c * ATD_MAX_M + bin] = base;
    base += v;
  }
}

// grid (chunks, batch): tokens of a chunk in ascending order, 256 at a time; the rank of a token among the equal ids of its wave comes
// from ballots, the waves of a tile are ordered through per-wave counts in LDS
__global__ __launch_bounds__(256) void atd_sort_scatter_kernel(const int32_t* ids, int64_t n, const int32_t* hist, int32_t* perm, int32_t* inv) {
  __shared__ int s_base[ATD_MAX_M];
  __shared__ int s_cnt[4][ATD_MAX_M];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < ATD_MAX_M) s_base[tid] = hist[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ATD_MAX_M + tid];
  const int64_t b0 = (int64_t)blockIdx.y * n;
  for (int tile = 0; tile < SORT_CHUNK / 256; ++tile) {
    const int64_t tok = (int64_t)blockIdx.x * SORT_CHUNK + tile * 256 + tid;
    const bool valid = tok < n;
    const int id = valid ? clamp_id(ids[b0 + tok]) : ATD_MAX_M;  // bit 7: matches no real id
    s_cnt[tid >> 7][tid & 127] = 0;
    s_cnt[2 + (tid >> 7)][tid & 127] = 0;
    unsigned long long peers = ~0ull;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (id >> bit) & 1;
      const unsigned long long b = __ballot(on);
      peers &= on ? b : ~b;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    const bool leader = lane == 63 - __clzll(peers);
    __syncthreads();  // counts zeroed (and s_base loaded / updated)
    if (valid && leader) s_cnt[wave][id] = __popcll(peers);
    __syncthreads();
    if (valid) {
      int pos = s_base[id] + rank;
      for (int w = 0; w < wave; ++w) pos += s_cnt[w][id];
      if (pos >= 0 && pos < n) {  // (always, for ids that the histogram pass saw)
        perm[b0 + pos] = (int32_t)tok;
        inv[b0 + tok] = pos;
      }
    }
    __syncthreads();
    if (tid < ATD_MAX_M) s_base[tid] += s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ group attention
// grid (groups, heads, batch), 4 waves; wave w owns the query tiles w and w + 4 of the group (32 tokens each), keys are staged 128 at a time.
// The arithmetic is rg_attention_kernel's (csrc/rgt.hip): S^T = K Q^T, in-lane online softmax, O^T = V^T P^T with P from the accumulators.
// KS = 16-channel steps of q k^T (2: head_dim <= 32, 4: <= 64).
template <int KS, int PROD>
__global__ __launch_bounds__(256) void atd_attention_kernel(const rsa_atd_attn_params p, int hp, int G, int64_t n_tok) {
  constexpr int NT = 128;
  constexpr int KROW = 16 * KS + 8;  // bf16 per K row: 80 / 144 bytes, conflict-free ds_read_b128 over 16 consecutive rows
  constexpr int VROW = 16 * KS;
  constexpr int DT = KS > 2 ? 2 : 1;  // 32-channel tiles of the output
  constexpr int NHL = PROD == 3 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) __bf16 s_k[NHL][NT * KROW];
  __shared__ __attribute__((aligned(16))) __bf16 s_v[NHL][NT * VROW];
  __shared__ int s_tok[256];
  __shared__ int s_code[256];
  __shared__ float s_bias[31 * 31];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = blockIdx.x, head = blockIdx.y, n = blockIdx.z;
  const bool win = p.mode == 0;
  const bool use_bias = win && p.bias_table != nullptr;
  const bool use_mask = win && p.shift > 0;
  const int nb = 2 * p.ws - 1;

  // ---- the group's index list ----
  {
    int tok = -1, code = 0;
    if (tid < G) {
      if (win) {
        const int wpr = p.W / p.ws;
        const int wy = grp / wpr, wx = grp - wy * wpr;
        const int ty = tid / p.ws, tx = tid - ty * p.ws;
        const int ys = wy * p.ws + ty, xs = wx * p.ws + tx;  // in the rolled map
        int y = ys + p.shift, x = xs + p.shift;
        if (y >= p.H) y -= p.H;
        if (x >= p.W) x -= p.W;
        tok = y * p.W + x;
        const int ry = ys < p.H - p.ws ? 0 : ys < p.H - p.shift ? 1 : 2;
        const int rx = xs < p.W - p.ws ? 0 : xs < p.W - p.shift ? 1 : 2;
        code = ty | (tx << 5) | ((3 * ry + rx) << 10);
      } else {
        const int64_t pos = (int64_t)grp * G + tid;
        const int64_t src = pos < n_tok ? pos : 2 * n_tok - 1 - pos;  // the flipped tail pads the last group
        int t = p.perm[(int64_t)n * n_tok + (src < 0 ? 0 : src)];
        t = t < 0 ? 0 : t >= n_tok ? (int)(n_tok - 1) : t;
        tok = t;
        code = pos < n_tok ? 0 : 1;  // 1: a padding position (a key, not a query)
      }
    }
    s_tok[tid] = tok;
    s_code[tid] = code;
    if (use_bias)
      for (int i = tid; i < nb * nb; i += 256) s_bias[i] = p.bias_table[(int64_t)head * nb * nb + i];
  }
  __syncthreads();

  const int KT = (G + 31) >> 5;
  const int64_t qoff = (int64_t)n * p.qkv_batch_stride + (int64_t)head * hp * p.qkv_plane_stride;
  const int64_t hstride = (int64_t)p.heads * hp * p.qkv_plane_stride;
  const bf16x8* q_hi = (const bf16x8*)p.qkv_hi + qoff;
  const bf16x8* k_hi = q_hi + hstride;
  const bf16x8* v_hi = k_hi + hstride;
  const bf16x8* q_lo = PROD == 3 ? (const bf16x8*)p.qkv_lo + qoff : nullptr;
  const bf16x8* k_lo = PROD == 3 ? q_lo + hstride : nullptr;
  const bf16x8* v_lo = PROD == 3 ? k_lo + hstride : nullptr;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  const int lr = lane & 31;
  const int lh = lane >> 5;
  const int g16 = lane >> 4;
  const int li16 = lane & 15;
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

  bool qvalid[2];
  int qtok[2], qcode[2];
  bf16x8 qh[2][KS], ql[2][KS];
  float m[2], l[2];
  f32x16 ot[2][DT];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const int tq = 32 * (wave + 4 * qi) + lr;  // < 256
    qtok[qi] = s_tok[tq];
    qcode[qi] = s_code[tq];
    qvalid[qi] = tq < G && (win || qcode[qi] == 0);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qh[qi][s] = zero8;
      ql[qi][s] = zero8;
      const int pl = 2 * s + lh;
      if (qvalid[qi] && pl < hp) {
        qh[qi][s] = q_hi[pl * p.qkv_plane_stride + qtok[qi]];
        if (PROD == 3) ql[qi][s] = q_lo[pl * p.qkv_plane_stride + qtok[qi]];
      }
    }
    m[qi] = -3.0e38f;
    l[qi] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[qi][dt][r] = 0.f;
  }
  const bool wave_live = 32 * wave < G;

  for (int kt0 = 0; kt0 < KT; kt0 += 4) {
    if (kt0 > 0) __syncthreads();
    {
      const int t = tid & (NT - 1);
      const int key = 32 * kt0 + t;  // < 256
      const int tok = s_tok[key];
      const bool valid = key < G;
      if (tid < NT) {
#pragma unroll
        for (int pl = 0; pl < 2 * KS; ++pl) {
          bf16x8 kh = zero8, kl = zero8;
          if (valid && pl < hp) {
            kh = k_hi[pl * p.qkv_plane_stride + tok];
            if (PROD == 3) kl = k_lo[pl * p.qkv_plane_stride + tok];
          }
          *(bf16x8*)&s_k[0][t * KROW + pl * 8] = kh;
          if (PROD == 3) *(bf16x8*)&s_k[NHL - 1][t * KROW + pl * 8] = kl;
        }
      } else {
#pragma unroll
        for (int pl = 0; pl < 2 * KS; ++pl) {
          bf16x8 vh = zero8, vl = zero8;
          if (valid && pl < hp) {
            vh = v_hi[pl * p.qkv_plane_stride + tok];
            if (PROD == 3) vl = v_lo[pl * p.qkv_plane_stride + tok];
          }
          *(bf16x8*)&s_v[0][t * VROW + pl * 8] = vh;
          if (PROD == 3) *(bf16x8*)&s_v[NHL - 1][t * VROW + pl * 8] = vl;
        }
      }
    }
    __syncthreads();
    if (!wave_live) continue;
    const int ktn = (KT - kt0 < 4) ? KT - kt0 : 4;

#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      if (32 * (wave + 4 * qi) >= G) continue;  // wave-uniform: this tile holds no query
      const int qty = qcode[qi] & 31, qtx = (qcode[qi] >> 5) & 31, qreg = qcode[qi] >> 10;
      for (int kt = 0; kt < ktn; ++kt) {
        f32x16 a;
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int off = (32 * kt + lr) * KROW + (2 * s + lh) * 8;
          const bf16x8 kh = *(const bf16x8*)&s_k[0][off];
          if (PROD == 3) {
            const bf16x8 kl = *(const bf16x8*)&s_k[NHL - 1][off];
            a = mfma32<RSA_PF_BF16>(kl, qh[qi][s], a);
            a = mfma32<RSA_PF_BF16>(kh, ql[qi][s], a);
          }
          a = mfma32<RSA_PF_BF16>(kh, qh[qi][s], a);
        }
        const int kbase = 32 * (kt0 + kt);
        float tm = -3.0e38f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kidx = kbase + (r & 3) + 8 * (r >> 2) + 4 * lh;  // < 256
          float v = a[r] * p.scale;
          if (win) {
            const int kc = s_code[kidx];
            if (use_bias) v += s_bias[(qty - (kc & 31) + p.ws - 1) * nb + (qtx - ((kc >> 5) & 31) + p.ws - 1)];
            if (use_mask && (kc >> 10) != qreg) v -= 100.f;
          }
          if (kidx >= G) v = -1.0e30f;
          a[r] = v;
          tm = fmaxf(tm, v);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32));
        const float mn = fmaxf(m[qi], tm);
        const float alpha = expf(m[qi] - mn);
        m[qi] = mn;
        l[qi] *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) ot[qi][dt][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = expf(a[r] - mn);
          a[r] = e;
          l[qi] += e;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float e8[8], r8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) e8[j] = a[8 * s + j];
          const bf16x8 ph = pack16<RSA_PF_BF16>(e8);
          bf16x8 pl8 = zero8;
          if (PROD == 3) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r8[j] = e8[j] - (float)ph[j];
            pl8 = pack16<RSA_PF_BF16>(r8);
          }
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            bf16x8 vh, vl;
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
              const int row = 32 * kt + 16 * s + 8 * g2 + 4 * lh + (li16 >> 2);
              const int col = 32 * dt + 16 * (g16 & 1) + 4 * (li16 & 3);
              const bf16x4 th = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)&s_v[0][row * VROW + col]);
#pragma unroll
              for (int e = 0; e < 4; ++e) vh[g2 * 4 + e] = th[e];
              if (PROD == 3) {
                const bf16x4 tl = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)&s_v[NHL - 1][row * VROW + col]);
#pragma unroll
                for (int e = 0; e < 4; ++e) vl[g2 * 4 + e] = tl[e];
              }
            }
            if (PROD == 3) {
              ot[qi][dt] = mfma32<RSA_PF_BF16>(vl, ph, ot[qi][dt]);
              ot[qi][dt] = mfma32<RSA_PF_BF16>(vh, pl8, ot[qi][dt]);
            }
            ot[qi][dt] = mfma32<RSA_PF_BF16>(vh, ph, ot[qi][dt]);
          }
        }
      }
    }
  }

  // ---- normalise and store on the token's own pixel: lane owns channels 32dt + 8g + 4lh .. +3 = plane 4dt + g, half lh ----
  const int64_t ooff = ((int64_t)n * p.out_batch_stride + (int64_t)head * hp * p.out_plane_stride) * 16;
  char* out_hi = (char*)p.out_hi + ooff;
  char* out_lo = p.out_lo != nullptr ? (char*)p.out_lo + ooff : nullptr;
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const float lsum = l[qi] + __shfl_xor(l[qi], 32);
    if (!qvalid[qi]) continue;
    const float inv_l = 1.f / lsum;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (4 * dt + g >= hp) continue;
        bf16x4 h, lo4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = ot[qi][dt][g * 4 + e] * inv_l;
          const __bf16 hb = (__bf16)v;
          h[e] = hb;
          lo4[e] = (__bf16)(v - (float)hb);
        }
        const int64_t off = ((int64_t)(4 * dt + g) * p.out_plane_stride + qtok[qi]) * 16 + lh * 8;
        *(bf16x4*)(out_hi + off) = h;
        if (out_lo != nullptr) *(bf16x4*)(out_lo + off) = lo4;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ ConvFFN middle
// grid (ceil(HW / 256), planes, batch): thread = pixel x 8 channels
__global__ __launch_bounds__(256) void atd_dwconv_kernel(const rsa_atd_dwconv_params p) {
  __shared__ float s_w[25][8];
  __shared__ float s_b[8];
  const int tid = threadIdx.x;
  const int plane = blockIdx.y, n = blockIdx.z;
  if (tid < 200) s_w[tid % 25][tid / 25] = p.weight[(int64_t)plane * 200 + tid];
  if (tid < 8) s_b[tid] = p.bias[plane * 8 + tid];
  __syncthreads();
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + tid;
  if (pix >= HW) return;
  const int y = (int)(pix / p.W), x = (int)(pix - (int64_t)y * p.W);
  const bf16x8* hi = (const bf16x8*)p.in_hi + (int64_t)n * p.in_batch_stride + (int64_t)plane * p.in_plane_stride;
  const bf16x8* lo = p.in_lo != nullptr ? (const bf16x8*)p.in_lo + (int64_t)n * p.in_batch_stride + (int64_t)plane * p.in_plane_stride : nullptr;
  float acc[8], ctr[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = s_b[j], ctr[j] = 0.f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= p.H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= p.W) continue;
      const int64_t u = (int64_t)yy * p.W + xx;
      const bf16x8 h = hi[u];
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
      if (lo != nullptr) {
        const bf16x8 lw = lo[u];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += (float)lw[j];
      }
      const int tap = (dy + 2) * 5 + dx + 2;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(s_w[tap][j], v[j], acc[j]);
      if (dy == 0 && dx == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ctr[j] = v[j];
      }
    }
  }
  bf16x8 oh, ol;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = ctr[j] + gelu_erf(acc[j]);
    const __bf16 hb = (__bf16)v;
    oh[j] = hb;
    ol[j] = (__bf16)(v - (float)hb);
  }
  const int64_t o = (int64_t)n * p.out_batch_stride + (int64_t)plane * p.out_plane_stride + pix;
  ((bf16x8*)p.out_hi)[o] = oh;
  if (p.out_lo != nullptr) ((bf16x8*)p.out_lo)[o] = ol;
}

// ------------------------------------------------------------------------------------------------ dictionary refinement
constexpr int RF_CHUNK = 1024;

struct RfWs {
  int chunks, Cp;
  int64_t off_dsum, off_fmm, off_coef, off_acc, off_se, total;
};

RfWs rf_layout(int batch, int64_t n, int C) {
  RfWs w;
  w.chunks = (int)((n + RF_CHUNK - 1) / RF_CHUNK);
  w.Cp = (C + 31) & ~31;
  int64_t o = 0;
  w.off_dsum = o, o += (int64_t)batch * w.chunks * 2 * ATD_MAX_M * 8;
  w.off_fmm = o, o += (int64_t)batch * w.chunks * 2 * ATD_MAX_M * 4;
  w.off_coef = o, o += (int64_t)batch * 3 * ATD_MAX_M * 4;
  w.off_acc = o, o += (int64_t)batch * w.chunks * ATD_MAX_M * w.Cp * 4;
  w.off_se = o, o += (int64_t)batch * w.chunks * ATD_MAX_M * 4;
  w.total = o;
  return w;
}

// grid (chunks, batch): per column of sim, sum and sum of squares (f64), minimum and maximum over a chunk of 1024 pixels
__global__ __launch_bounds__(256) void atd_refine_stats_kernel(const rsa_atd_refine_params p, double* dsum, float* fmm) {
  __shared__ double s_d[2][2][ATD_MAX_M];
  __shared__ float s_f[2][2][ATD_MAX_M];
  const int tid = threadIdx.x, col = tid & 127, half = tid >> 7;
  const int chunk = blockIdx.x, n = blockIdx.y;
  const int64_t HW = (int64_t)p.H * p.W;
  const int64_t p0 = (int64_t)chunk * RF_CHUNK;
  const int rows = (int)(HW - p0 < RF_CHUNK ? HW - p0 : RF_CHUNK);
  double s = 0.0, ss = 0.0;
  float mn = 3.0e38f, mx = -3.0e38f;
  if (col < p.m) {
    const float* sim = p.sim + ((int64_t)n * HW + p0) * p.m + col;
    for (int r = half; r < rows; r += 2) {
      const float v = sim[(int64_t)r * p.m];
      s += (double)v;
      ss += (double)v * (double)v;
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  }
  s_d[half][0][col] = s, s_d[half][1][col] = ss;
  s_f[half][0][col] = mn, s_f[half][1][col] = mx;
  __syncthreads();
  if (half == 0) {
    const int64_t o = ((int64_t)n * gridDim.x + chunk) * 2 * ATD_MAX_M;
    dsum[o + col] = s_d[0][0][col] + s_d[1][0][col];
    dsum[o + ATD_MAX_M + col] = s_d[0][1][col] + s_d[1][1][col];
    fmm[o + col] = fminf(s_f[0][0][col], s_f[1][0][col]);
    fmm[o + ATD_MAX_M + col] = fmaxf(s_f[0][1][col], s_f[1][1][col]);
  }
}

// grid (batch), 128 threads: z = a x + b of InstanceNorm1d (biased variance) and the maximum of z over the pixels
__global__ __launch_bounds__(128) void atd_refine_coef_kernel(const rsa_atd_refine_params p, const double* dsum, const float* fmm, float* coef, int chunks) {
  const int col = threadIdx.x, n = blockIdx.x;
  const int64_t HW = (int64_t)p.H * p.W;
  double s = 0.0, ss = 0.0;
  float mn = 3.0e38f, mx = -3.0e38f;
  for (int c = 0; c < chunks; ++c) {
    const int64_t o = ((int64_t)n * chunks + c) * 2 * ATD_MAX_M;
    s += dsum[o + col];
    ss += dsum[o + ATD_MAX_M + col];
    mn = fminf(mn, fmm[o + col]);
    mx = fmaxf(mx, fmm[o + ATD_MAX_M + col]);
  }
  float a = 0.f, b = 0.f, zmax = 0.f;
  if (col < p.m) {
    const double mean = s / (double)HW;
    double var = ss / (double)HW - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + (double)p.eps);
    a = (float)((double)p.gamma[col] * rstd);
    b = (float)((double)p.beta[col] - mean * (double)p.gamma[col] * rstd);
    zmax = fmaxf(fmaf(a, mn, b), fmaf(a, mx, b));
  }
  float* c3 = coef + (int64_t)n * 3 * ATD_MAX_M;
  c3[col] = a;
  c3[ATD_MAX_M + col] = b;
  c3[2 * ATD_MAX_M + col] = zmax;
}

// grid (chunks, Cp / 32, batch): sum over a chunk of pixels of exp(z - zmax) x for every dictionary token and 32 channels.
// Thread (tg = tid >> 3, cg = tid & 7) owns tokens 4tg .. +3 and channels 4cg .. +3 of the tile.
__global__ __launch_bounds__(256) void atd_refine_accum_kernel(const rsa_atd_refine_params p, const float* coef, float* pacc, float* pse, int Cp) {
  constexpr int SUB = 64;
  __shared__ __attribute__((aligned(16))) float s_e[SUB][ATD_MAX_M];
  __shared__ __attribute__((aligned(16))) float s_x[SUB][32];
  __shared__ float s_c[3][ATD_MAX_M];
  const int tid = threadIdx.x, tg = tid >> 3, cg = tid & 7;
  const int chunk = blockIdx.x, ct = blockIdx.y, n = blockIdx.z;
  const int64_t HW = (int64_t)p.H * p.W;
  const int P4 = (p.C + 3) >> 2;
  for (int i = tid; i < 3 * ATD_MAX_M; i += 256) s_c[i >> 7][i & 127] = coef[(int64_t)n * 3 * ATD_MAX_M + i];
  float acc[4][4], se[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    se[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  }
  const f32x4* x4 = (const f32x4*)p.x + (int64_t)n * P4 * HW;
  for (int sub = 0; sub < RF_CHUNK / SUB; ++sub) {
    const int64_t p0 = (int64_t)chunk * RF_CHUNK + sub * SUB;
    if (p0 >= HW) break;  // block-uniform
    __syncthreads();
    for (int i = tid; i < SUB * ATD_MAX_M; i += 256) {
      const int pl = i >> 7, col = i & 127;
      float e = 0.f;
      if (col < p.m && p0 + pl < HW) e = expf(fmaf(s_c[0][col], p.sim[((int64_t)n * HW + p0 + pl) * p.m + col], s_c[1][col]) - s_c[2][col]);
      s_e[pl][col] = e;
    }
    for (int i = tid; i < SUB * 8; i += 256) {
      const int g = i >> 6, pl = i & 63;
      const int G = ct * 8 + g;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (G < P4 && p0 + pl < HW) v = x4[(int64_t)G * HW + p0 + pl];
      *(f32x4*)&s_x[pl][4 * g] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int pl = 0; pl < SUB; ++pl) {
      const f32x4 e4 = *(const f32x4*)&s_e[pl][4 * tg];
      const f32x4 xv = *(const f32x4*)&s_x[pl][4 * cg];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        se[i] += e4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(e4[i], xv[j], acc[i][j]);
      }
    }
  }
  const int64_t o = ((int64_t)n * gridDim.x + chunk) * ATD_MAX_M;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *(f32x4*)&pacc[(o + 4 * tg + i) * Cp + ct * 32 + 4 * cg] = (f32x4){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
    if (ct == 0 && cg == 0) pse[o + 4 * tg + i] = se[i];
  }
}

// grid (m, batch), 256 threads: the partial sums in chunk order, then the blend with the old dictionary
__global__ __launch_bounds__(256) void atd_refine_finish_kernel(const rsa_atd_refine_params p, const float* pacc, const float* pse, int chunks, int Cp) {
  const int t = blockIdx.x, n = blockIdx.y, c = threadIdx.x;
  if (c >= p.C) return;
  float acc = 0.f, se = 0.f;
  for (int k = 0; k < chunks; ++k) {
    const int64_t o = ((int64_t)n * chunks + k) * ATD_MAX_M + t;
    acc += pacc[o * Cp + c];
    se += pse[o];
  }
  const float sg = 1.f / (1.f + expf(-p.sigma[t]));
  float* td = p.td + ((int64_t)n * p.m + t) * p.C + c;
  *td = sg * *td + (1.f - sg) * (acc / se);
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int rsa_atd_dict(const rsa_atd_dict_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "atd_dict: null params");
  if (p->batch < 1 || p->batch > 65535) return set_error(RSA_E_ARG, "atd_dict: bad batch");
  if (p->C < 1 || p->C > ATD_MAX_C || p->m < 1 || p->m > ATD_MAX_M || p->rc < 1 || p->rc > ATD_MAX_RC)
    return set_error(RSA_E_UNSUPPORTED, "atd_dict: C in [1, 256], m in [1, 128], rc in [1, 16]");
  if (!p->td || !p->wk || !p->wv || !p->kn || !p->vt_hi || !p->vt_lo) return set_error(RSA_E_ARG, "atd_dict: null pointer");
  if (misaligned16(p->kn) || misaligned16(p->vt_hi) || misaligned16(p->vt_lo)) return set_error(RSA_E_ALIGN, "atd_dict: outputs must be 16-byte aligned");
  const int Cp = (p->C + 31) & ~31;
  hipLaunchKernelGGL(atd_dict_kernel, dim3((unsigned)(Cp / 2 + 1), (unsigned)p->batch), dim3(256), 0, (hipStream_t)stream, *p, Cp);
  return launch_status("atd_dict: launch failed");
}

extern "C" int rsa_atd_ca(const rsa_atd_ca_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "atd_ca: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->reserved0 != 0) return set_error(RSA_E_ARG, "atd_ca: bad geometry");
  if (p->C < 1 || p->C > ATD_MAX_C || p->m < 1 || p->m > ATD_MAX_M || p->rc < 1 || p->rc > ATD_MAX_RC)
    return set_error(RSA_E_UNSUPPORTED, "atd_ca: C in [1, 256], m in [1, 128], rc in [1, 16]");
  if (p->products != 1 && p->products != 3) return set_error(RSA_E_UNSUPPORTED, "atd_ca: products must be 3 or 1");
  if (!p->xn || !p->wq || !p->kn || !p->scale || !p->vt_hi || !p->vt_lo || !p->out) return set_error(RSA_E_ARG, "atd_ca: null pointer");
  if (misaligned16(p->xn) || misaligned16(p->kn) || misaligned16(p->vt_hi) || misaligned16(p->vt_lo) || misaligned16(p->out) || misaligned16(p->sim))
    return set_error(RSA_E_ALIGN, "atd_ca: pointers must be 16-byte aligned");
  const int64_t blocks = ((int64_t)p->H * p->W + 127) / 128;
  if (blocks > 0x7fffffff || (int64_t)p->H * p->W > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "atd_ca: map too large");
  const dim3 grid((unsigned)blocks, (unsigned)p->batch);
  const hipStream_t s = (hipStream_t)stream;
  if (p->m <= 64) {
    if (p->products == 3)
      hipLaunchKernelGGL((atd_ca_kernel<4, 3>), grid, dim3(256), 0, s, *p);
    else
      hipLaunchKernelGGL((atd_ca_kernel<4, 1>), grid, dim3(256), 0, s, *p);
  } else {
    if (p->products == 3)
      hipLaunchKernelGGL((atd_ca_kernel<8, 3>), grid, dim3(256), 0, s, *p);
    else
      hipLaunchKernelGGL((atd_ca_kernel<8, 1>), grid, dim3(256), 0, s, *p);
  }
  return launch_status("atd_ca: launch failed");
}

extern "C" int64_t rsa_atd_sort_workspace_bytes(int32_t batch, int64_t n) {
  if (batch < 1 || n < 1) return 0;
  return (int64_t)batch * ((n + SORT_CHUNK - 1) / SORT_CHUNK) * ATD_MAX_M * 4;
}

extern "C" int rsa_atd_sort(const int32_t* ids, int32_t batch, int64_t n, int32_t m, int32_t* perm, int32_t* inv, void* workspace, void* stream) {
  if (!ids || !perm || !inv || !workspace) return set_error(RSA_E_ARG, "atd_sort: null pointer");
  if (batch < 1 || batch > 65535 || n < 1 || n > 0x7fffffff) return set_error(RSA_E_ARG, "atd_sort: bad geometry");
  if (m < 1 || m > ATD_MAX_M) return set_error(RSA_E_UNSUPPORTED, "atd_sort: m must be in [1, 128]");
  const int64_t chunks = (n + SORT_CHUNK - 1) / SORT_CHUNK;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)chunks, (unsigned)batch);
  hipLaunchKernelGGL(atd_sort_hist_kernel, grid, dim3(256), 0, s, ids, n, (int32_t*)workspace);
  hipLaunchKernelGGL(atd_sort_scan_kernel, dim3((unsigned)batch), dim3(128), 0, s, (int32_t*)workspace, (int)chunks);
  hipLaunchKernelGGL(atd_sort_scatter_kernel, grid, dim3(256), 0, s, ids, n, (const int32_t*)workspace, perm, inv);
  return launch_status("atd_sort: launch failed");
}

extern "C" int rsa_atd_attention(const rsa_atd_attn_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "atd_attention: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->heads < 1 || p->heads > 65535 || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "atd_attention: bad geometry");
  if (p->head_dim < 1 || p->head_dim > 64) return set_error(RSA_E_UNSUPPORTED, "atd_attention: head_dim must be in [1, 64]");
  if (p->products != 1 && p->products != 3) return set_error(RSA_E_UNSUPPORTED, "atd_attention: products must be 3 or 1");
  const int64_t n_tok = (int64_t)p->H * p->W;
  if (n_tok > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "atd_attention: map too large");
  int G;
  int64_t groups;
  if (p->mode == 0) {
    if (p->ws < 2 || p->ws > 16 || p->shift < 0 || p->shift >= p->ws || p->H % p->ws || p->W % p->ws)
      return set_error(RSA_E_ARG, "atd_attention: ws in [2, 16], 0 <= shift < ws, H and W multiples of ws");
    G = p->ws * p->ws;
    groups = (int64_t)(p->H / p->ws) * (p->W / p->ws);
  } else if (p->mode == 1) {
    if (p->gs < 1 || p->gs > 256 || p->gs > n_tok || !p->perm) return set_error(RSA_E_ARG, "atd_attention: gs in [1, min(256, H*W)] and perm");
    G = p->gs;
    groups = (n_tok + G - 1) / G;
  } else {
    return set_error(RSA_E_ARG, "atd_attention: mode must be 0 or 1");
  }
  if (groups > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "atd_attention: too many groups");
  if (!p->qkv_hi || !p->out_hi || (p->products == 3 && !p->qkv_lo)) return set_error(RSA_E_ARG, "atd_attention: null pointer");
  if (misaligned16(p->qkv_hi) || misaligned16(p->qkv_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "atd_attention: planes must be 16-byte aligned");
  if (p->qkv_plane_stride < n_tok || p->out_plane_stride < n_tok) return set_error(RSA_E_ARG, "atd_attention: a plane stride is smaller than the map");
  const int hp = (p->head_dim + 7) >> 3;
  const dim3 grid((unsigned)groups, (unsigned)p->heads, (unsigned)p->batch);
  const hipStream_t s = (hipStream_t)stream;
  if (hp <= 4) {
    if (p->products == 3)
      hipLaunchKernelGGL((atd_attention_kernel<2, 3>), grid, dim3(256), 0, s, *p, hp, G, n_tok);
    else
      hipLaunchKernelGGL((atd_attention_kernel<2, 1>), grid, dim3(256), 0, s, *p, hp, G, n_tok);
  } else {
    if (p->products == 3)
      hipLaunchKernelGGL((atd_attention_kernel<4, 3>), grid, dim3(256), 0, s, *p, hp, G, n_tok);
    else
      hipLaunchKernelGGL((atd_attention_kernel<4, 1>), grid, dim3(256), 0, s, *p, hp, G, n_tok);
  }
  return launch_status("atd_attention: launch failed");
}

extern "C" int rsa_atd_dwconv(const rsa_atd_dwconv_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "atd_dwconv: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->planes < 1 || p->planes > 65535) return set_error(RSA_E_ARG, "atd_dwconv: bad geometry");
  if (!p->in_hi || !p->weight || !p->bias || !p->out_hi) return set_error(RSA_E_ARG, "atd_dwconv: null pointer");
  if (misaligned16(p->in_hi) || misaligned16(p->in_lo) || misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "atd_dwconv: planes must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->in_plane_stride < HW || p->out_plane_stride < HW) return set_error(RSA_E_ARG, "atd_dwconv: a plane stride is smaller than the map");
  if ((HW + 255) / 256 > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "atd_dwconv: map too large");
  hipLaunchKernelGGL(atd_dwconv_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)p->planes, (unsigned)p->batch), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("atd_dwconv: launch failed");
}

extern "C" int64_t rsa_atd_refine_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t C, int32_t m) {
  if (batch < 1 || H < 1 || W < 1 || C < 1 || C > ATD_MAX_C || m < 1 || m > ATD_MAX_M) return 0;
  return rf_layout(batch, (int64_t)H * W, C).total;
}

extern "C" int rsa_atd_refine(const rsa_atd_refine_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "atd_refine: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || !(p->eps > 0.f)) return set_error(RSA_E_ARG, "atd_refine: bad geometry");
  if (p->C < 1 || p->C > ATD_MAX_C || p->m < 1 || p->m > ATD_MAX_M) return set_error(RSA_E_UNSUPPORTED, "atd_refine: C in [1, 256], m in [1, 128]");
  if (!p->sim || !p->x || !p->gamma || !p->beta || !p->sigma || !p->td || !p->workspace) return set_error(RSA_E_ARG, "atd_refine: null pointer");
  if (misaligned16(p->x) || misaligned16(p->workspace)) return set_error(RSA_E_ALIGN, "atd_refine: x and workspace must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (HW > 0x7fffffff) return set_error(RSA_E_UNSUPPORTED, "atd_refine: map too large");
  const RfWs w = rf_layout(p->batch, HW, p->C);
  char* ws = (char*)p->workspace;
  double* dsum = (double*)(ws + w.off_dsum);
  float* fmm = (float*)(ws + w.off_fmm);
  float* coef = (float*)(ws + w.off_coef);
  float* pacc = (float*)(ws + w.off_acc);
  float* pse = (float*)(ws + w.off_se);
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(atd_refine_stats_kernel, dim3((unsigned)w.chunks, (unsigned)p->batch), dim3(256), 0, s, *p, dsum, fmm);
  hipLaunchKernelGGL(atd_refine_coef_kernel, dim3((unsigned)p->batch), dim3(128), 0, s, *p, (const double*)dsum, (const float*)fmm, coef, w.chunks);
  hipLaunchKernelGGL(atd_refine_accum_kernel, dim3((unsigned)w.chunks, (unsigned)(w.Cp / 32), (unsigned)p->batch), dim3(256), 0, s, *p, (const float*)coef,
                     pacc, pse, w.Cp);
  hipLaunchKernelGGL(atd_refine_finish_kernel, dim3((unsigned)p->m, (unsigned)p->batch), dim3(256), 0, s, *p, (const float*)pacc, (const float*)pse, w.chunks,
                     w.Cp);
  return launch_status("atd_refine: launch failed");
}
