/*
 * resselt_amd_lawfft.h — the entry points of LAWFFT (the reference's archs/lawfft/arch.py) in libresselt_amd.so, an extension of the C-ABI
 * in resselt_amd.h (same conventions, same library): resselt_amd/csrc/lawfft.hip.  The ctypes mirrors and signature rows live in
 * resselt_amd/engine/lib_lawfft.py, and tests/test_lawfft_capi.py compares the two field by field and argument by argument.
 *
 * Conventions, as resselt_amd_gfisr.h and resselt_amd_figsr.h: split planes of 8 channels in format `fmt` (enum rsa_plane_fmt), value =
 * hi + lo, a lo pointer may be NULL; strides in 16-byte units; C is the TRUE channel count of a plane range of ceil(C/8) planes: the tail
 * channels of the last plane are never used as values (a NaN there reaches no output) and are written as zero.  Every argument check
 * happens before any launch: RSA_E_ARG null pointer / bad geometry / a reserved field that is not 0, RSA_E_UNSUPPORTED a size that is not
 * built, RSA_E_ALIGN a plane or map pointer that is not 16-byte aligned.
 */
#ifndef RESSELT_AMD_LAWFFT_H
#define RESSELT_AMD_LAWFFT_H

#include "resselt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The windowed FSAS core (arch.py:268-306) in one launch.  For every 8 x 8 patch and every channel c < C
 *     corr[y][x] = sum_{u, v} q[u][v] * k[(y - u) mod 8][(x - v) mod 8]
 * (= irfft2(rfft2(q) * rfft2(k), s = (8, 8)): the circular convolution of the patch), in f32 FMAs over u, then v, ascending: the result
 * is the same bits from run to run.  Then, per pixel, the LayerNorm over the C channels (biased variance) and the product with v:
 *     out = v * ((corr - mean) / sqrt(var + eps) * weight[c] + bias[c])
 * with exactly the arithmetic of rsa_lawfft_norm_mul.  H and W are multiples of 8, C is 1..128, weight / bias f32 [C].  out may be v. */
typedef struct rsa_lawfft_wincorr_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                   /* channels of q, of k, of v and of out: 1..128 */
  int32_t fmt;                 /* enum rsa_plane_fmt of every plane operand */
  int32_t reserved0;           /* must be 0 */
  float eps;
  int32_t reserved1;           /* must be 0 */
  const float* weight;
  const float* bias;
  const void* q_hi;
  const void* q_lo;            /* may be NULL */
  int64_t q_plane_stride;      /* 16-byte units, >= H*W */
  int64_t q_batch_stride;
  const void* k_hi;
  const void* k_lo;            /* may be NULL */
  int64_t k_plane_stride;
  int64_t k_batch_stride;
  const void* v_hi;
  const void* v_lo;            /* may be NULL */
  int64_t v_plane_stride;
  int64_t v_batch_stride;
  void* out_hi;
  void* out_lo;                /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_lawfft_wincorr_params;
int rsa_lawfft_wincorr(const rsa_lawfft_wincorr_params* p, void* stream);

/* out = scale * (a (.) b), a complex product per bin of two f32 spectral maps in rsa_gfisr_dft's layout [N][ceil(2C/4)][H][W][4] (W here
 * is Wf) whose channels are [real of all C | imag of all C].  Components past 2C are neither used as values nor written.  out may be a
 * (in place) or b.  C: 1..128. */
typedef struct rsa_lawfft_spec_mul_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;
  float scale;
  int32_t reserved0;           /* must be 0 */
  const float* a;
  const float* b;
  float* out;
} rsa_lawfft_spec_mul_params;
int rsa_lawfft_spec_mul(const rsa_lawfft_spec_mul_params* p, void* stream);

/* out = v * LayerNorm_channels(corr) over the true C channels (the whole-image FSAS: corr is what rsa_gfisr_dft's inverse wrote), per pixel:
 *     mean = (sum_c corr[c]) / C,  var = (sum_c (corr[c] - mean)^2) / C   (both sums over c ascending, one f32 accumulator)
 *     out[c] = v[c] * fma((corr[c] - mean) * (1 / sqrt(var + eps)), weight[c], bias[c])
 * corr planes are of format corr_fmt, v and out of format fmt.  C: 1..128.  out may be v or corr. */
typedef struct rsa_lawfft_norm_mul_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;
  int32_t corr_fmt;
  int32_t fmt;
  float eps;
  int32_t reserved0;           /* must be 0 */
  const float* weight;
  const float* bias;
  const void* corr_hi;
  const void* corr_lo;         /* may be NULL */
  int64_t corr_plane_stride;
  int64_t corr_batch_stride;
  const void* v_hi;
  const void* v_lo;            /* may be NULL */
  int64_t v_plane_stride;
  int64_t v_batch_stride;
  void* out_hi;
  void* out_lo;                /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_lawfft_norm_mul_params;
int rsa_lawfft_norm_mul(const rsa_lawfft_norm_mul_params* p, void* stream);

/* DynamicLocal's kernel generator (arch.py:223-236), two kernels on `stream`, no atomics:
 *     m[b][c] = mean over H*W of channel c          (per plane, per chunk of pixels, a fixed tree; then the chunks in ascending order)
 *     h = relu(W1 m + b1),  out[b] = W2 h + b2      (f32 FMAs over the input index, ascending)
 * w1_t f32 [C][C] and w2_t f32 [C][C k^2] are the TRANSPOSES of the two 1x1 convolutions' matrices (w1_t[i][j] = W1[j][i]), b1 [C],
 * b2 [C k^2].  out: f32 [batch][8 ceil(C/8)][k^2], the layout rsa_lawfft_dyn_dwconv reads; the tail channels are written as zero.
 * workspace: rsa_lawfft_kernel_gen_workspace_bytes(batch, C, H, W) bytes, 16-byte aligned.  C: 1..128, ksize 3 or 5. */
typedef struct rsa_lawfft_kernel_gen_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;
  int32_t ksize;
  int32_t fmt;
  int32_t reserved0;           /* must be 0 */
  int32_t reserved1;           /* must be 0 */
  const float* w1_t;
  const float* b1;
  const float* w2_t;
  const float* b2;
  float* workspace;
  float* out;
  const void* in_hi;
  const void* in_lo;           /* may be NULL */
  int64_t in_plane_stride;
  int64_t in_batch_stride;
} rsa_lawfft_kernel_gen_params;
int rsa_lawfft_kernel_gen(const rsa_lawfft_kernel_gen_params* p, void* stream);
int64_t rsa_lawfft_kernel_gen_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W);

/* Depthwise k x k (k = 3 or 5), zero padding k / 2, no bias, one weight set per batch sample (arch.py:238-242):
 *     y[b][c] = sum_taps x[b][c] * weight[b][c][tap]        taps row-major, ascending, f32 FMAs
 *     value = y (+ res1) (+ res2),  written to out planes and / or out_f32
 * weight: f32 [batch][8 ceil(C/8)][k^2] (rsa_lawfft_kernel_gen's output).  res1, res2 and out_f32 are f32 maps [N][ceil(C/4)][H][W][4]
 * and may be NULL; at least one of out_hi and out_f32 is given.  Channels past C of an f32 map are never read and are written as zero.
 * Not in place on the planes (a pixel reads its neighbours); out_f32 may be res1 or res2. */
typedef struct rsa_lawfft_dyn_dwconv_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;
  int32_t ksize;
  int32_t fmt;
  int32_t reserved0;           /* must be 0 */
  int32_t reserved1;           /* must be 0 */
  const float* weight;
  const float* res1;
  const float* res2;
  float* out_f32;
  const void* in_hi;
  const void* in_lo;           /* may be NULL */
  int64_t in_plane_stride;
  int64_t in_batch_stride;
  void* out_hi;                /* may be NULL (then out_f32) */
  void* out_lo;                /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_lawfft_dyn_dwconv_params;
int rsa_lawfft_dyn_dwconv(const rsa_lawfft_dyn_dwconv_params* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESSELT_AMD_LAWFFT_H */
