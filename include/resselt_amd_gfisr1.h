/*
 * resselt_amd_gfisr1.h — the entry points GFISR (v1) adds to the GFISR family in libresselt_amd.so, an extension of the C-ABI in
 * resselt_amd.h (same conventions, same library): the reference's archs/gfisr/arch.py; resselt_amd/csrc/gfisr1.hip.  The transforms
 * themselves are rsa_gfisr_dft of resselt_amd_gfisr.h.  The ctypes mirrors and signature rows live in resselt_amd/engine/lib_gfisr1.py,
 * and tests/test_gfisr_capi.py compares the two field by field and argument by argument.
 */
#ifndef RESSELT_AMD_GFISR1_H
#define RESSELT_AMD_GFISR1_H

#include "resselt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* FourierUnit's spectral stage in one launch, all f32 (gfisr/arch.py:459-465), on the H x W spectral grid (W here is Wf); C = 2 gc
 * spectral channels in the order both transforms use, [real of all | imag of all]:
 *   v = (x - mean_c x) / sqrt(var_c x + eps) * ln_w + ln_b     mean and biased variance over the true C channels, centred two-pass form
 *   u = depthwise3x3(v) + fpe_b + v                            v is ZERO outside the grid (not ln_b)
 *   z = gelu_erf(fdc_w u + fdc_b)                              C -> C; per output an f32 fma chain from the bias over c = 0, 1, ...
 * x and out are f32 maps [N][ceil(C/4)][H][W][4] (out is what rsa_gfisr_dft(inverse = 1) reads) and must not overlap: a pixel reads its
 * eight neighbours.  Components past C of x are never used (a NaN there reaches no output); components past C of out are not written.
 * ln_w / ln_b / fpe_b / fdc_b f32 [C], fpe_w f32 [C][9] (row-major taps), fdc_w f32 [C][C] ([output][input]).  The softmax-weighted
 * einsum of the reference (:462-464) is the identity for its one group and has no part here.
 * Errors: RSA_E_ARG null pointer / bad geometry / eps <= 0 / reserved field; RSA_E_UNSUPPORTED C outside 2..32 or odd; RSA_E_ALIGN. */
typedef struct rsa_gfisr_ln_spectral_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                   /* 2..32, even */
  float eps;
  int32_t reserved0;           /* must be 0 */
  const float* x;
  const float* ln_w;
  const float* ln_b;
  const float* fpe_w;
  const float* fpe_b;
  const float* fdc_w;
  const float* fdc_b;
  float* out;
} rsa_gfisr_ln_spectral_params;
int rsa_gfisr_ln_spectral(const rsa_gfisr_ln_spectral_params* p, void* stream);

/* A window of split planes with torch's 'reflect' rule applied once: the pad in front of FourierUnit's transform and the crop behind it
 * (gfisr/arch.py:385-413).  For y < out_H, x < out_W of each of the `planes` planes:
 *   out[n][p][y][x] = in[n][p][r(y - top, H)][r(x - left, W)],   r(t, S) = -t for t < 0, 2 (S - 1) - t for t >= S, else t
 * in 16-byte units, hi and (where both lo pointers are given) lo: the plane format does not matter.  pad: (top, left) = (2, 2) and
 * out = (H + 4 + H % 2, W + 4 + W % 2); crop: (top, left) = (-2, -2) and out = the unpadded size.  Nothing is written outside
 * [out_H][out_W] of a plane.  in and out must not overlap.
 * Errors: RSA_E_ARG null pointer / bad geometry / one lo pointer without the other / a stride smaller than its map / an index that
 * would need a second reflection (a pad >= the side); RSA_E_ALIGN. */
typedef struct rsa_plane_window_params {
  int32_t batch;
  int32_t planes;
  int32_t H, W;                /* of in */
  int32_t out_H, out_W;
  int32_t top, left;
  const void* in_hi;
  const void* in_lo;           /* may be NULL (then out_lo too) */
  int64_t in_plane_stride;     /* 16-byte units, >= H*W */
  int64_t in_batch_stride;
  void* out_hi;
  void* out_lo;
  int64_t out_plane_stride;    /* 16-byte units, >= out_H*out_W */
  int64_t out_batch_stride;
} rsa_plane_window_params;
int rsa_plane_window(const rsa_plane_window_params* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RESSELT_AMD_GFISR1_H */
