// gfisr.hip — the kernels of GFISRv2's FourierUnit (reference resselt/archs/gfisrv2/arch.py:449-496):
//   rsa_gfisr_dft        rfft2 / irfft2 (norm='ortho') of a whole map as dense DFT-matrix products on the f32-input MFMA; the inverse
//                        ends in post_norm (RMSNorm over the channels) and writes split planes                     FourierUnit.forward :477, :494-495
//   rsa_gfisr_spectral   rn (RMSNorm over the 2c spectral channels) + fpe (depthwise 3x3 + bias) + its residual      FourierUnit.forward :485-486
// (fdc + GELU between them is a 1x1 launch of the fused convolution; the gate of the block is csrc/mosr.hip with silu(g).)
//
// The transform costs O(HW (H + W)) per channel: 2 (H W 2Wf + 4 H H Wf) FLOP, every one an exact f32 fma.  Two passes per direction, all
// four the same batched product D[M x N] = A[M x K] B[K x N] per (image, channel), told apart by where A, B and D live (Pass):
//   forward  row pass     A = the image from split planes [H x W],  B = tab_row [W x 2Wf],     D -> scratch [2H x Wf] (rows re | im)
//            column pass  A = tab_col [2H x 2H] (k-major),          B = scratch [2H x Wf],      D -> spec, channels [re of all | im of all]
//   inverse  column pass  A = tab_col [2H x 2H],                    B = spec as [2H x Wf],      D -> scratch [H x 2Wf] (columns re | im)
//            row pass     A = scratch [H x 2Wf],                    B = tab_row [2Wf x W],      D -> raw f32 [H x W], then post_norm -> planes
// The inverse row pass walks ALL channels of its pixel tile in one workgroup: it keeps the sum of squares of each of its pixels in registers,
// parks the raw values in scratch (every lane re-reads only what it wrote itself), and normalises them into plane units at the end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "plane_unit.h"
#include "resselt_amd_gfisr.h"

namespace rsa {
namespace {

// A workgroup of four waves owns a 2 WT x 2 WT tile of D, a wave a WT x WT quarter of it in ONE accumulator: WT = 32 on
// v_mfma_f32_32x32x2_f32 (16 registers; its issue interval equals its dependent latency, 64 cycles, so one chain runs at the issue rate),
// WT = 16 on v_mfma_f32_16x16x4_f32 (4 registers; 32-cycle issue, 40-cycle dependent latency) where a pass has too few 64 x 64 tiles to
// fill the machine.  K advances in steps of BK through LDS: A as [k][m] with a row of 2 WT + 1 floats, B as [k][n], so the operand reads
// of an MFMA -- consecutive lanes one k, the next lane group the next k -- are conflict-free.  The operands of step k + 1 are loaded into
// registers before the MFMAs of step k are issued, so their latency runs under the matrix pipe.
constexpr int BK = 32;
constexpr int BM = 64, BN = 64;  // the tile of the passes on WT = 32
template <int WT>
struct Frag {
  typedef f32x16 acc_t;
  static constexpr int R = 16;
};
template <>
struct Frag<16> {
  typedef f32x4 acc_t;
  static constexpr int R = 4;
};
// C/D layout: element r of lane l is D[row][col]
template <int WT>
__device__ __forceinline__ int acc_row(int lane, int r) {
  if constexpr (WT == 32) return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
  return 4 * (lane >> 4) + r;
}
template <int WT>
__device__ __forceinline__ int acc_col(int lane) {
  return lane & (WT - 1);
}
enum Pass { FWD_ROW = 0, FWD_COL = 1, INV_COL = 2, INV_ROW = 3 };

struct Geo {
  int H, W, Wf, C, P4, fmt;     // P4 = ceil(2C / 4): groups of the spectral map
  int M, N, K;
  const float* tab;             // the table operand of this pass
  const float* spec_in;         // INV_COL
  float* spec_out;              // FWD_COL
  const float* s_in;            // FWD_COL, INV_ROW: scratch the previous pass wrote
  float* s_out;                 // FWD_ROW, INV_COL; INV_ROW: the raw values
  const char* pl_hi;            // FWD_ROW reads, INV_ROW writes
  const char* pl_lo;
  int64_t pl_ps, pl_bs;         // 16-byte units
  const float* nscale;
  const float* noffset;
  float eps;
};

__device__ __forceinline__ float plane_elem(const Geo& g, int n, int ch, int64_t pix) {
  const int64_t e = (((int64_t)n * g.pl_bs + (int64_t)(ch >> 3) * g.pl_ps + pix) << 3) + (ch & 7);
  if (g.fmt == RSA_PF_F16) {
    float v = (float)((const _Float16*)g.pl_hi)[e];
    if (g.pl_lo) v += (float)((const _Float16*)g.pl_lo)[e];
    return v;
  }
  float v = (float)((const __bf16*)g.pl_hi)[e];
  if (g.pl_lo) v += (float)((const __bf16*)g.pl_lo)[e];
  return v;
}

template <int PASS>
__device__ __forceinline__ float load_a(const Geo& g, int n, int ch, int m, int k) {
  if (m >= g.M || k >= g.K) return 0.f;
  if constexpr (PASS == FWD_ROW) return plane_elem(g, n, ch, (int64_t)m * g.W + k);
  if constexpr (PASS == FWD_COL || PASS == INV_COL) return g.tab[(int64_t)k * g.M + m];
  return g.s_in[(((int64_t)n * g.C + ch) * g.H + m) * (2 * g.Wf) + k];  // INV_ROW
}

template <int PASS>
__device__ __forceinline__ float load_b(const Geo& g, int n, int ch, int k, int j) {
  if (k >= g.K || j >= g.N) return 0.f;
  if constexpr (PASS == FWD_ROW || PASS == INV_ROW) return g.tab[(int64_t)k * g.N + j];
  if constexpr (PASS == FWD_COL) return g.s_in[(((int64_t)n * g.C + ch) * (2 * g.H) + k) * g.Wf + j];
  const int chan = k < g.H ? ch : g.C + ch, y = k < g.H ? k : k - g.H;  // INV_COL
  return g.spec_in[((((int64_t)n * g.P4 + (chan >> 2)) * g.H + y) * g.Wf + j) * 4 + (chan & 3)];
}

template <int PASS>
__device__ __forceinline__ void store_d(const Geo& g, int n, int ch, int m, int j, float v) {
  if (m >= g.M || j >= g.N) return;
  if constexpr (PASS == FWD_ROW) {
    const int row = j < g.Wf ? m : g.H + m, col = j < g.Wf ? j : j - g.Wf;
    g.s_out[(((int64_t)n * g.C + ch) * (2 * g.H) + row) * g.Wf + col] = v;
  } else if constexpr (PASS == FWD_COL) {
    const int chan = m < g.H ? ch : g.C + ch, y = m < g.H ? m : m - g.H;
    g.spec_out[((((int64_t)n * g.P4 + (chan >> 2)) * g.H + y) * g.Wf + j) * 4 + (chan & 3)] = v;
  } else if constexpr (PASS == INV_COL) {
    const int row = m < g.H ? m : m - g.H, col = m < g.H ? j : g.Wf + j;
    g.s_out[(((int64_t)n * g.C + ch) * g.H + row) * (2 * g.Wf) + col] = v;
  } else {
    g.s_out[(((int64_t)n * g.C + ch) * g.H + m) * g.W + j] = v;
  }
}

// One 2 WT x 2 WT tile of D for one (image, channel): the wave's WT x WT quarter in acc.
template <int PASS, int WT>
__device__ __forceinline__ void tile_product(const Geo& g, int n, int ch, int m0, int j0, float* As, float* Bs, typename Frag<WT>::acc_t& acc) {
  constexpr int TM = 2 * WT, TN = 2 * WT, AS = TM + 1, NL = TM * BK / 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WT, wn = (wave & 1) * WT;
#pragma unroll
  for (int r = 0; r < Frag<WT>::R; ++r) acc[r] = 0.f;
  float ra[NL], rb[NL];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      int am, ak;
      if constexpr (PASS == FWD_ROW || PASS == INV_ROW) {  // data, contiguous along k
        ak = tid & (BK - 1), am = tid / BK + (256 / BK) * i;
      } else {  // a k-major table, contiguous along m
        am = tid & (TM - 1), ak = tid / TM + (256 / TM) * i;
      }
      ra[i] = load_a<PASS>(g, n, ch, m0 + am, k0 + ak);
      rb[i] = load_b<PASS>(g, n, ch, k0 + tid / TN + (256 / TN) * i, j0 + (tid & (TN - 1)));
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < g.K; k0 += BK) {
    __syncthreads();  // the previous step's operands have been read
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      int am, ak;
      if constexpr (PASS == FWD_ROW || PASS == INV_ROW) {
        ak = tid & (BK - 1), am = tid / BK + (256 / BK) * i;
      } else {
        am = tid & (TM - 1), ak = tid / TM + (256 / TM) * i;
      }
      As[ak * AS + am] = ra[i];
      Bs[(tid / TN + (256 / TN) * i) * TN + (tid & (TN - 1))] = rb[i];
    }
    __syncthreads();
    if (k0 + BK < g.K) fetch(k0 + BK);  // in flight under the MFMAs below
    if constexpr (WT == 32) {
#pragma unroll
      for (int s = 0; s < BK / 2; ++s) {
        const int kk = 2 * s + (lane >> 5);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk * AS + wm + (lane & 31)], Bs[kk * TN + wn + (lane & 31)], acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int s = 0; s < BK / 4; ++s) {
        const int kk = 4 * s + (lane >> 4);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(As[kk * AS + wm + (lane & 15)], Bs[kk * TN + wn + (lane & 15)], acc, 0, 0, 0);
      }
    }
  }
}

// grid (tiles of D, batch * C), 256 threads
template <int PASS>
__global__ __launch_bounds__(256) void gfisr_dft_kernel(const Geo g) {
  __shared__ float As[BK * (BM + 1)];
  __shared__ float Bs[BK * BN];
  const int tiles_n = (g.N + BN - 1) / BN;
  const int tm = (int)blockIdx.x / tiles_n, tn = (int)blockIdx.x - tm * tiles_n;
  const int n = (int)blockIdx.y / g.C, ch = (int)blockIdx.y - n * g.C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = tm * BM, j0 = tn * BN;
  f32x16 acc;
  tile_product<PASS, 32>(g, n, ch, m0, j0, As, Bs, acc);
  const int col = j0 + (wave & 1) * 32 + acc_col<32>(lane), row0 = m0 + (wave >> 1) * 32;
#pragma unroll
  for (int r = 0; r < 16; ++r) store_d<PASS>(g, n, ch, row0 + acc_row<32>(lane, r), col, acc[r]);
}

// The inverse row pass with post_norm: grid (32 x 32 tiles of the H x W map, batch), 256 threads; the workgroup walks the channels.  (WT = 16:
// a 512 x 512 map has 64 tiles of 64 x 64 for 256 compute units, and every workgroup is a serial chain of C products.)
constexpr int OT = 32;
template <int FMT>
__global__ __launch_bounds__(256) void gfisr_dft_out_kernel(const Geo g) {
  __shared__ float As[BK * (OT + 1)];
  __shared__ float Bs[BK * OT];
  const int tiles_n = (g.N + OT - 1) / OT;
  const int tm = (int)blockIdx.x / tiles_n, tn = (int)blockIdx.x - tm * tiles_n;
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = tm * OT, j0 = tn * OT;
  const int col = j0 + (wave & 1) * 16 + acc_col<16>(lane), row0 = m0 + (wave >> 1) * 16;
  float ss[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) ss[r] = 0.f;
  for (int ch = 0; ch < g.C; ++ch) {
    f32x4 acc;
    tile_product<INV_ROW, 16>(g, n, ch, m0, j0, As, Bs, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      store_d<INV_ROW>(g, n, ch, row0 + acc_row<16>(lane, r), col, acc[r]);
      ss[r] = fmaf(acc[r], acc[r], ss[r]);
    }
  }
  // every raw value this lane reads below it stored itself above (same addresses, program order): no barrier, no fence
  if (col >= g.W) return;
  const int planes = (g.C + 7) >> 3;
  const float rc = 1.f / sqrtf((float)g.C);
  char* hi = (char*)g.pl_hi;
  char* lo = (char*)g.pl_lo;
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // (unrolled: ss stays in registers)
    const int y = row0 + acc_row<16>(lane, r);
    if (y >= g.H) continue;
    const float inv = g.nscale ? 1.f / (sqrtf(ss[r]) * rc + g.eps) : 1.f;
    const int64_t pix = (int64_t)y * g.W + col;
    for (int pl = 0; pl < planes; ++pl) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = 8 * pl + j;
        float t = 0.f;  // the tail channels of the last plane are zero
        if (ch < g.C) {
          t = g.s_out[(((int64_t)n * g.C + ch) * g.H + y) * g.W + col];
          if (g.nscale) t = fmaf(t * inv, g.nscale[ch], g.noffset[ch]);
        }
        v[j] = t;
      }
      store_unit<FMT>(hi, lo, ((int64_t)n * g.pl_bs + (int64_t)pl * g.pl_ps + pix) * 16, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- rn + fpe + residual
constexpr int SP_TW = 32, SP_TH = 8, SP_HW = SP_TW + 2, SP_HH = SP_TH + 2;

// grid (tiles, batch), 256 threads: a 32 x 8 tile of the spectral grid.  Phase 1 puts 1 / (rms + eps) of the tile's 34 x 10 halo pixels in
// LDS (0 outside the grid: the depthwise convolution pads the NORMALISED map with zeros, offset included); phase 2: a lane owns a pixel and
// walks its channel groups, reading the nine neighbours of a group straight from the map (the L1 / L2 hold the tile).
__global__ __launch_bounds__(256) void gfisr_spectral_kernel(const rsa_gfisr_spectral_params p) {
  __shared__ float inv[SP_HH * SP_HW];
  const int tiles_x = (p.W + SP_TW - 1) / SP_TW;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int n = blockIdx.y;
  const int x0 = tx * SP_TW, y0 = ty * SP_TH;
  const int64_t HW = (int64_t)p.H * p.W;
  const int p4 = (p.C + 3) >> 2;
  const f32x4* xm = (const f32x4*)p.x + (int64_t)n * p4 * HW;
  const float rc = 1.f / sqrtf((float)p.C);
  for (int idx = threadIdx.x; idx < SP_HH * SP_HW; idx += 256) {
    const int hy = idx / SP_HW, hx = idx - hy * SP_HW;
    const int gy = y0 + hy - 1, gx = x0 + hx - 1;
    float r = 0.f;
    if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
      float ss = 0.f;
      for (int g = 0; g < p4; ++g) {
        const f32x4 v = xm[(int64_t)g * HW + (int64_t)gy * p.W + gx];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (4 * g + c < p.C) ss = fmaf(v[c], v[c], ss);  // (a select, not a product: a NaN in an unused component stays out)
      }
      r = 1.f / (sqrtf(ss) * rc + p.eps);
    }
    inv[idx] = r;
  }
  __syncthreads();
  const int lx = threadIdx.x & (SP_TW - 1), ly = threadIdx.x / SP_TW;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= p.W || y >= p.H) return;
  const int planes = (p.C + 7) >> 3;
  const int64_t pix = (int64_t)y * p.W + x;
  char* hi = (char*)p.out_hi + ((int64_t)n * p.out_batch_stride + pix) * 16;
  char* lo = p.out_lo ? (char*)p.out_lo + ((int64_t)n * p.out_batch_stride + pix) * 16 : nullptr;
  for (int pl = 0; pl < planes; ++pl) {
    float o[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int g = 2 * pl + h;
      float acc[4] = {0.f, 0.f, 0.f, 0.f}, ctr[4] = {0.f, 0.f, 0.f, 0.f};
      if (g < p4) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float r = inv[(ly + dy) * SP_HW + lx + dx];
            if (r == 0.f) continue;  // outside the grid (inside it r > 0: eps > 0 bounds the denominator)
            const f32x4 v = xm[(int64_t)g * HW + (int64_t)(y + dy - 1) * p.W + (x + dx - 1)];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int ch = 4 * g + c;
              if (ch < p.C) {
                const float t = fmaf(v[c] * r, p.scale[ch], p.offset[ch]);
                acc[c] = fmaf(p.weight[ch * 9 + dy * 3 + dx], t, acc[c]);
                if (dy == 1 && dx == 1) ctr[c] = t;
              }
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ch = 4 * g + c;
        o[4 * h + c] = ch < p.C ? acc[c] + p.bias[ch] + ctr[c] : 0.f;
      }
    }
    store_unit<RSA_PF_BF16>(hi, lo, (int64_t)pl * p.out_plane_stride * 16, o);
  }
}

bool dft_sizes_ok(int64_t batch, int64_t C, int64_t H, int64_t W) {
  const int64_t Wf = W / 2 + 1, lim = 0x7fffffff;
  return 4 * H * H <= lim && 2 * Wf * W <= lim && batch * C * 2 * H * Wf <= lim && batch * C * H * W <= lim && batch * C <= 65535;
}

}  // namespace
}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_gfisr_dft_scratch_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
  if (batch < 1 || C < 1 || C > 128 || H < 1 || W < 1 || !dft_sizes_ok(batch, C, H, W)) return -1;
  return (int64_t)batch * C * ((int64_t)2 * H * (W / 2 + 1) + (int64_t)H * W) * 4;
}

extern "C" int rsa_gfisr_dft(const rsa_gfisr_dft_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gfisr_dft: null params");
  if (p->batch < 1 || p->H < 1 || p->W < 1 || p->C < 1 || (p->inverse != 0 && p->inverse != 1) || p->reserved0 != 0)
    return set_error(RSA_E_ARG, "gfisr_dft: bad geometry (inverse 0 or 1, reserved0 0)");
  if (p->C > 128) return set_error(RSA_E_UNSUPPORTED, "gfisr_dft: C must be in 1..128");
  if (!dft_sizes_ok(p->batch, p->C, p->H, p->W)) return set_error(RSA_E_UNSUPPORTED, "gfisr_dft: the map is too large for the dense transform");
  if (!plane_fmt_ok(p->fmt)) return set_error(RSA_E_ARG, "gfisr_dft: bad plane format");
  if (!p->tab_row || !p->tab_col || !p->spec || !p->scratch || !p->plane_hi) return set_error(RSA_E_ARG, "gfisr_dft: null pointer");
  if (p->norm_scale && (!p->norm_offset || !(p->eps > 0.f))) return set_error(RSA_E_ARG, "gfisr_dft: the norm needs norm_offset and eps > 0");
  if (misaligned16(p->tab_row) || misaligned16(p->tab_col) || misaligned16(p->spec) || misaligned16(p->scratch) || misaligned16(p->plane_hi) ||
      misaligned16(p->plane_lo) || misaligned16(p->norm_scale) || misaligned16(p->norm_offset))
    return set_error(RSA_E_ALIGN, "gfisr_dft: tables, maps, scratch and planes must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->plane_plane_stride < HW) return set_error(RSA_E_ARG, "gfisr_dft: the plane stride is smaller than the map");
  const hipStream_t s = (hipStream_t)stream;
  Geo g{};
  g.H = p->H, g.W = p->W, g.Wf = p->W / 2 + 1, g.C = p->C, g.P4 = (2 * p->C + 3) / 4, g.fmt = p->fmt;
  g.pl_hi = (const char*)p->plane_hi, g.pl_lo = (const char*)p->plane_lo, g.pl_ps = p->plane_plane_stride, g.pl_bs = p->plane_batch_stride;
  g.nscale = p->norm_scale, g.noffset = p->norm_offset, g.eps = p->eps;
  float* col_scratch = p->scratch;                                          // [batch][C][2H Wf]
  float* raw = p->scratch + (int64_t)p->batch * p->C * 2 * p->H * g.Wf;     // [batch][C][H][W]
  auto tiles = [](int M, int N, int T = BM) { return (unsigned)(((M + T - 1) / T) * ((N + T - 1) / T)); };
  const unsigned nb = (unsigned)(p->batch * p->C);
  if (!p->inverse) {
    Geo a = g;
    a.M = g.H, a.N = 2 * g.Wf, a.K = g.W, a.tab = p->tab_row, a.s_out = col_scratch;
    hipLaunchKernelGGL(gfisr_dft_kernel<FWD_ROW>, dim3(tiles(a.M, a.N), nb), dim3(256), 0, s, a);
    Geo b = g;
    b.M = 2 * g.H, b.N = g.Wf, b.K = 2 * g.H, b.tab = p->tab_col, b.s_in = col_scratch, b.spec_out = p->spec;
    hipLaunchKernelGGL(gfisr_dft_kernel<FWD_COL>, dim3(tiles(b.M, b.N), nb), dim3(256), 0, s, b);
  } else {
    Geo a = g;
    a.M = 2 * g.H, a.N = g.Wf, a.K = 2 * g.H, a.tab = p->tab_col, a.spec_in = p->spec, a.s_out = col_scratch;
    hipLaunchKernelGGL(gfisr_dft_kernel<INV_COL>, dim3(tiles(a.M, a.N), nb), dim3(256), 0, s, a);
    Geo b = g;
    b.M = g.H, b.N = g.W, b.K = 2 * g.Wf, b.tab = p->tab_row, b.s_in = col_scratch, b.s_out = raw;
    with_fmt(p->fmt, [&](auto F) {
      hipLaunchKernelGGL((gfisr_dft_out_kernel<decltype(F)::value>), dim3(tiles(b.M, b.N, OT), (unsigned)p->batch), dim3(256), 0, s, b);
    });
  }
  return launch_status("gfisr_dft: launch failed");
}

extern "C" int rsa_gfisr_spectral(const rsa_gfisr_spectral_params* p, void* stream) {
  if (p == nullptr) return set_error(RSA_E_ARG, "gfisr_spectral: null params");
  if (p->batch < 1 || p->batch > 65535 || p->H < 1 || p->W < 1 || p->C < 1 || p->reserved0 != 0 || !(p->eps > 0.f))
    return set_error(RSA_E_ARG, "gfisr_spectral: bad geometry (eps > 0, reserved0 0)");
  if (p->C > 256) return set_error(RSA_E_UNSUPPORTED, "gfisr_spectral: C must be in 1..256");
  if (!p->x || !p->scale || !p->offset || !p->weight || !p->bias || !p->out_hi) return set_error(RSA_E_ARG, "gfisr_spectral: null pointer");
  if (misaligned16(p->x) || misaligned16(p->scale) || misaligned16(p->offset) || misaligned16(p->weight) || misaligned16(p->bias) ||
      misaligned16(p->out_hi) || misaligned16(p->out_lo))
    return set_error(RSA_E_ALIGN, "gfisr_spectral: the map, the channel vectors and the planes must be 16-byte aligned");
  const int64_t HW = (int64_t)p->H * p->W;
  if (p->out_plane_stride < HW) return set_error(RSA_E_ARG, "gfisr_spectral: the plane stride is smaller than the map");
  const int64_t tiles = (int64_t)((p->W + SP_TW - 1) / SP_TW) * ((p->H + SP_TH - 1) / SP_TH);
  if (tiles > 0x7fffffff) return set_error(RSA_E_ARG, "gfisr_spectral: map too large");
  hipLaunchKernelGGL(gfisr_spectral_kernel, dim3((unsigned)tiles, (unsigned)p->batch), dim3(256), 0, (hipStream_t)stream, *p);
  return launch_status("gfisr_spectral: launch failed");
}
