/*
 * resselt_amd_gfisr.h — the entry points of the GFISR family (GFISRv2's FourierUnit first) in libresselt_amd.so, an extension of the C-ABI
 * in resselt_amd.h (same conventions, same library): the reference's archs/gfisrv2/arch.py; resselt_amd/csrc/gfisr.hip (and csrc/mosr.hip
 * for rsa_gfisr_gate).  The ctypes mirrors and signature rows live in resselt_amd/engine/lib_gfisr.py, and tests/test_gfisrv2_capi.py
 * compares the two field by field and argument by argument.
 */
#ifndef RESSELT_AMD_GFISR_H
#define RESSELT_AMD_GFISR_H

#include "resselt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The whole-image real 2-D DFT of torch.fft.rfft2 / irfft2 with norm='ortho', as dense DFT-matrix products on the f32-input MFMA
 * (v_mfma_f32_32x32x2_f32, and v_mfma_f32_16x16x4_f32 in the last inverse pass: an exact f32 fma chain in k order).  One arithmetic for every H and W: no radix cases, no padding.
 * H x W is the image, Wf = W/2 + 1 the width of the half spectrum, C the channel count of the image (1..128).
 *
 * Tables (f32, built by the host in float64 with the index product reduced mod the length before the angle is taken, 1/sqrt(W) folded
 * into the row tables and 1/sqrt(H) into the column table, rounded once; resselt_amd/engine/lib_gfisr.py dft_tables):
 *   tab_row  forward [W][2 Wf]:   [x][k] = cos(2 pi xk/W)/sqrt(W),  [x][Wf + k] = -sin(2 pi xk/W)/sqrt(W)
 *            inverse [2 Wf][W]:   [k][x] = c_k cos(2 pi kx/W)/sqrt(W),  [Wf + k][x] = -c_k sin(2 pi kx/W)/sqrt(W);  c_0 = 1, c_{W/2} = 1 for
 *            even W, every other c_k = 2 -- irfft2's reading of a non-Hermitian half spectrum (the imaginary parts of column 0 and of the
 *            Nyquist column do not contribute)
 *   tab_col  [2H][2H], k-major ([k][m]):  forward the transpose of G = [[Cc, Sc], [-Sc, Cc]] / sqrt(H), inverse G itself (= the transpose
 *            of conj), Cc / Sc = cos / sin(2 pi vy/H): a complex column transform as one real product on stacked [re; im] rows
 *
 * inverse = 0, forward:  planes (split planes of format fmt, the ceil(C/8) planes from plane_hi; plane_lo may be NULL; value = hi + lo)
 *     -> spec, an f32 map [N][ceil(2C/4)][H][Wf][4] whose channels are [real of all C | imag of all C]; components past 2C are not written.
 * inverse = 1:  spec (same layout, same channel order) -> irfft2(s = (H, W)) -> RMSNorm over the C channels,
 *     y / (||y||_2 / sqrt(C) + eps) * norm_scale[c] + norm_offset[c]  (norm_scale NULL: no norm), -> planes; the tail channels of the last
 *     plane are written as zero.  Components of spec past 2C are never read.
 * scratch: rsa_gfisr_dft_scratch_bytes(batch, C, H, W) bytes, 16-byte aligned, private layout, no state kept between calls.
 * Errors: RSA_E_ARG null pointer / bad geometry / reserved field; RSA_E_UNSUPPORTED C outside 1..128 or a size whose tables or scratch
 * pass 2^31 elements; RSA_E_ALIGN. */
typedef struct rsa_gfisr_dft_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                   /* channels of the image: 1..128 */
  int32_t inverse;             /* 0 or 1 */
  int32_t fmt;                 /* enum rsa_plane_fmt of plane_hi / plane_lo */
  float eps;                   /* inverse, with norm_scale */
  int32_t reserved0;           /* must be 0 */
  const float* tab_row;
  const float* tab_col;
  float* spec;                 /* written (forward) / read (inverse) */
  float* scratch;
  const float* norm_scale;     /* inverse: [8 ceil(C/8)], may be NULL */
  const float* norm_offset;    /* with norm_scale */
  void* plane_hi;              /* read (forward) / written (inverse) */
  void* plane_lo;              /* may be NULL */
  int64_t plane_plane_stride;  /* 16-byte units, >= H*W */
  int64_t plane_batch_stride;
} rsa_gfisr_dft_params;
int rsa_gfisr_dft(const rsa_gfisr_dft_params* p, void* stream);
int64_t rsa_gfisr_dft_scratch_bytes(int32_t batch, int32_t C, int32_t H, int32_t W);

/* FourierUnit's rn and fpe with its residual in one launch (gfisrv2/arch.py:485-486), on the H x W spectral grid (W here is Wf):
 *   v = x / (||x||_2 / sqrt(C) + eps) * scale + offset      over the true C channels of the f32 map x [N][ceil(C/4)][H][W][4]
 *   out = depthwise3x3(v) + bias + v                        zero padding of v at the border of the grid
 * written as bf16 split planes [N][ceil(C/8)][H][W][8] (out_lo may be NULL).  Components past C are never used (a NaN there reaches no
 * output) and the tail channels of the last plane are written as zero.  scale / offset / bias f32 [8 ceil(C/8)], weight f32
 * [8 ceil(C/8)][9].  C: 1..256.  Errors as above. */
typedef struct rsa_gfisr_spectral_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;
  float eps;
  int32_t reserved0;           /* must be 0 */
  const float* x;
  const float* scale;
  const float* offset;
  const float* weight;
  const float* bias;
  void* out_hi;
  void* out_lo;                /* may be NULL */
  int64_t out_plane_stride;    /* 16-byte units, >= H*W */
  int64_t out_batch_stride;
} rsa_gfisr_spectral_params;
int rsa_gfisr_spectral(const rsa_gfisr_spectral_params* p, void* stream);

/* rsa_gated_dwconv (resselt_amd.h) with the gate activation as an argument:  out = act(g) * cat(x[0 : i_planes), seg_0(x), ...).
 * act: RSA_ACT_MISH (then it IS rsa_gated_dwconv) or RSA_ACT_SILU (GFISRv2, gfisrv2/arch.py:615); anything else RSA_E_UNSUPPORTED. */
int rsa_gfisr_gate(const rsa_gated_dwconv_params* p, int32_t act, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESSELT_AMD_GFISR_H */
