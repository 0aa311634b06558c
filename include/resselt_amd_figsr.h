/*
 * resselt_amd_figsr.h — the FIGSR entry points of libresselt_amd.so, an extension of the C-ABI in resselt_amd.h (same conventions, same
 * library): the reference's archs/figsr/arch.py; resselt_amd/csrc/figsr.hip.  Their ctypes mirrors and signature rows live in
 * resselt_amd/engine/lib_figsr.py, and tests/test_figsr_capi.py compares the two field by field and argument by argument.
 * The FourierUnit of FIGSR is GFISRv2's: rsa_gfisr_dft and rsa_gfisr_spectral (resselt_amd_gfisr.h) serve it unchanged.
 */
#ifndef RESSELT_AMD_FIGSR_H
#define RESSELT_AMD_FIGSR_H

#include "resselt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gate of a FIGSR block with both dense band convolutions of its Inception step in one launch (GatedCNNBlock.gated_forward :612-618,
 * InceptionConv2d :563-591):
 *     out = silu(g) * cat(x[0 : pass_planes), hw, bandw(x_w) + bias_w, bandh(x_h) + bias_h)
 * Every operand is split planes [N][planes][H][W][8] of format fmt (value = hi + lo; a lo pointer may be NULL where noted).  With
 * P = gc / 8, g, x and out have planes = pass_planes + 3 P planes each; x is fc1's cat(i, c, c_hw, c_w, c_h) range in that order:
 *     x planes [0, pass_planes)                       passed through (i, and the Fourier branch, which holds post_norm's output by now)
 *     x planes [pass_planes, + P)                     c_hw: NOT read -- hw, a separate operand of P planes, is convhw(c_hw) (rsa_plk_conv)
 *     x planes [pass_planes + P, + 2 P)               x_w: bandw, a dense gc -> gc 1 x K convolution, zero padding (0, K / 2)
 *     x planes [pass_planes + 2 P, + 3 P)             x_h: bandh, a dense gc -> gc K x 1 convolution, zero padding (K / 2, 0)
 * K = ksize odd, 3..31; gc 8 or 16.  The bands run on v_mfma_f32_16x16x32_{bf16,f16} with f32 accumulation, in the arithmetic of
 * rsa_plk_conv: fmt RSA_PF_BF16 with products = 3 (w_hi x_hi + w_hi x_lo + w_lo x_hi; x_lo required) or fmt RSA_PF_F16 with
 * products = 1 (the hi halves alone; lo halves of g, hw and the passed-through planes are still read where given).  SiLU is
 * g / (1 + exp(-g)) in f32 on g_hi + g_lo.
 * w_packed: rsa_figsr_band_packed_weight_bytes(ksize, gc, products) bytes of A fragments, 16-bit values of format fmt,
 *     [2 bands (w, h)][P input planes][S = ceil(K / 4) steps][products == 3 ? 2 : 1 halves][64 lanes][8]:
 *     lane l of (band, plane p, step s) holds W_band[l & 15][8 p + j][tap 4 s + (l >> 4)], j = 0..7: 8 input channels of one tap per lane,
 *     four taps per K step, zero past K and past output channel gc -- one B fragment is one plane unit at a shifted pixel
 *     (resselt_amd/engine/lib_figsr.py: pack_band_weights).  bias_w, bias_h: f32 [16], zero past gc.
 * No plane outside [0, planes) of out is touched, and nothing outside H x W of a plane.  out must not be g, x or hw.
 * Errors: RSA_E_ARG null pointer / bad geometry, format or products / planes != pass_planes + 3 gc / 8 / x_lo missing for three
 * products / a plane stride below H*W / out aliasing an input / reserved field; RSA_E_UNSUPPORTED ksize even or outside 3..31, gc not
 * 8 or 16, or another (fmt, products) pair than the two above; RSA_E_ALIGN. */
typedef struct rsa_figsr_mix_params {
  int32_t batch;
  int32_t H, W;
  int32_t fmt;                /* enum rsa_plane_fmt of every plane operand and of w_packed */
  int32_t products;           /* 3 with RSA_PF_BF16, 1 with RSA_PF_F16 */
  int32_t ksize;              /* K of both bands: odd, 3..31 */
  int32_t gc;                 /* 8 or 16 */
  int32_t planes;             /* of g, x and out: pass_planes + 3 gc / 8 */
  int32_t pass_planes;        /* >= 0 */
  int32_t reserved0;          /* must be 0 */
  const void* w_packed;
  const float* bias_w;
  const float* bias_h;
  const void* g_hi;
  const void* g_lo;           /* may be NULL */
  int64_t g_plane_stride;     /* 16-byte units, >= H*W */
  int64_t g_batch_stride;
  const void* x_hi;
  const void* x_lo;           /* may be NULL with products == 1 */
  int64_t x_plane_stride;
  int64_t x_batch_stride;
  const void* hw_hi;          /* gc / 8 planes */
  const void* hw_lo;          /* may be NULL */
  int64_t hw_plane_stride;
  int64_t hw_batch_stride;
  void* out_hi;
  void* out_lo;               /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_figsr_mix_params;
int rsa_figsr_mix(const rsa_figsr_mix_params* p, void* stream);
int64_t rsa_figsr_band_packed_weight_bytes(int32_t ksize, int32_t gc, int32_t products);

/* The front end (FIGSR.forward :672-690): a plain [N][C][src_h][src_w] tensor of `dtype` (enum rsa_dtype: f32, f16 or bf16) ->
 *     v = (x - shift[c]) / scale_norm[c]                       a true f32 division, as the reference divides
 *     F.pad(v, (pad, pad + src_w % 2, pad, pad + src_h % 2), 'reflect')    fused into the read
 * -> one split plane [N][1][H][W][8], H = src_h + 2 pad + src_h % 2, W likewise (both even); the channels past C are written as zero.
 * C: 1..8; shift, scale_norm: f32 [C].
 * Errors: RSA_E_ARG null pointer / bad geometry / pad < 0 or pad + src % 2 >= src in either direction (the reflection needs that many
 * pixels) / bad dtype or format / a plane stride below H*W / reserved field; RSA_E_UNSUPPORTED C above 8; RSA_E_ALIGN for planes that
 * are not 16-byte aligned. */
typedef struct rsa_figsr_input_params {
  int32_t batch;
  int32_t C;
  int32_t src_h, src_w;
  int32_t pad;
  int32_t dtype;              /* enum rsa_dtype of x */
  int32_t fmt;                /* enum rsa_plane_fmt of out_hi / out_lo */
  int32_t reserved0;          /* must be 0 */
  const void* x;
  const float* shift;
  const float* scale_norm;
  void* out_hi;
  void* out_lo;               /* may be NULL */
  int64_t out_plane_stride;   /* 16-byte units, >= H*W */
  int64_t out_batch_stride;
} rsa_figsr_input_params;
int rsa_figsr_input(const rsa_figsr_input_params* p, void* stream);

/* The back end (FIGSR.forward :701-708): the window rows [y0, y0 + out_h), columns [x0, x0 + out_w) of the head's f32 result
 * y [N][C][H][W] ->  y * scale_norm[c] + shift[c]  (a product and a sum, each rounded to f32) -> out [N][C][out_h][out_w] of `dtype`
 * (f32, f16 or bf16; rounded once).  shift, scale_norm: f32 [C].
 * Errors: RSA_E_ARG null pointer / bad geometry / a window that leaves the map / bad dtype / reserved field. */
typedef struct rsa_figsr_output_params {
  int32_t batch;
  int32_t C;
  int32_t H, W;               /* of y */
  int32_t y0, x0;
  int32_t out_h, out_w;
  int32_t dtype;              /* enum rsa_dtype of out */
  int32_t reserved0;          /* must be 0 */
  const float* y;
  const float* shift;
  const float* scale_norm;
  void* out;
} rsa_figsr_output_params;
int rsa_figsr_output(const rsa_figsr_output_params* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESSELT_AMD_FIGSR_H */
