/*
 * resselt_amd.h — C-ABI of the MI355X (gfx950) super-resolution forward-pass engine.
 *
 * The reference (rewaifu/resselt) has NO FFI: its hot path is `model.forward(x)` of
 * nn.Modules that delegate every operation to PyTorch ATen.  Each entry point below
 * names the reference ATen op sequence (file:line under /root/reference) that it
 * replaces.  The library is loaded with ctypes by `resselt_amd/engine/lib.py`; the
 * binding a maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  All data pointers are DEVICE pointers
 *     owned by the caller (PyTorch caching allocator); the library never allocates,
 *     never synchronises and keeps no global state besides a thread-local error string.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *   - return value: 0 = ok, < 0 = argument error (RSA_E_*), > 0 = hipError_t from a launch.
 *
 * Activation storage ("split planes", the engine's internal HBM layout)
 *   A C-channel feature map of H x W pixels is stored channel-blocked by 8 ("NCHW8c"):
 *       hi[n][plane = c/8][y][x][c%8]   bf16   (round-to-nearest-even of the f32 value)
 *       lo[n][plane = c/8][y][x][c%8]   bf16   (bf16 of the rounding residual v - hi)
 *   One (plane,y,x) cell is a 16-byte "unit": 8 channels of one pixel = one MFMA
 *   k-group operand (v_mfma_f32_16x16x32_bf16 B fragment) and one coalesced 16 B lane load.
 *   Dense concatenation (reference torch.cat along dim 1) is a plane offset into a shared
 *   buffer, never a copy.  Residual streams are additionally kept in f32 as
 *       f32[n][plane4 = c/4][y][x][c%4]          ("NCHW4c")
 *   which is exactly the accumulator fragment of the MFMA (4 consecutive channels / lane).
 */
#ifndef RESSELT_AMD_H
#define RESSELT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSA_VERSION 400 /* 0.4.0: rsa_conv2d_pair (cross-layer fusion of residual dense block convolutions), fp16 saturation + overflow status */

/* error codes (negative = argument errors) */
#define RSA_OK 0
#define RSA_E_ARG (-1)       /* null / out-of-range argument */
#define RSA_E_UNSUPPORTED (-2) /* combination not compiled in */
#define RSA_E_ALIGN (-3)     /* pointer not 16-byte aligned */
#define RSA_E_FP16_RANGE (-5) /* rsa_check_status only: rsa_check_finite has seen an infinity or a NaN since the last call (an activation of a
                                one-product fp16 layer left the format's range, or the input was not finite): rerun with three bf16 products */
#define RSA_E_INTERNAL (-4)  /* a kernel reported a protocol failure (ring schedule hand-off timed out): results of the launches since the
                                last rsa_check_status() == RSA_OK are not to be trusted */

/* activation selector of the fused epilogue */
enum rsa_act {
  RSA_ACT_NONE = 0,
  RSA_ACT_LRELU = 1, /* act_param = negative slope; reference utilities/block.py:17-30 */
  RSA_ACT_MISH = 2,  /* reference archs/spanplus/arch.py:121 (nn.Mish)                  */
  RSA_ACT_SILU = 3,  /* reference archs/span/arch.py:164 (nn.SiLU)                      */
  RSA_ACT_GELU = 4,  /* erf GELU, reference archs/swinir/arch.py:34-40 (nn.GELU)        */
  RSA_ACT_SPAB_GATE = 5, /* y = (acc + res1) * (sigmoid(acc) - 0.5); spanplus/arch.py:126-127 */
  RSA_ACT_PRELU = 6      /* per-channel slopes act_vec[cout]; nn.PReLU(num_parameters=C), compact/arch.py:42-52 */
};

/* dtype of plain tensors crossing the boundary.  F32 / F16 / BF16: NCHW float tensors.  RSA_U8: an 8-bit IMAGE, channel-interleaved
 * [N][H][W][C] as image decoders deliver it (the reference leaves both conversions to its callers):
 *   read  (rsa_nchw_to_planes):           v = byte / 255   (a true division: bit-identical to torch's img.float() / 255)
 *   write (rsa_conv2d final store):       byte = round-half-even(clamp(v, 0, 1) * 255)   (torch: (y.clamp(0, 1) * 255).round()) */
enum rsa_dtype { RSA_F32 = 0, RSA_F16 = 1, RSA_BF16 = 2, RSA_U8 = 3 };

/* 16-bit element format of split planes and packed weights.  A plane buffer has ONE format; `hi` is the round-to-nearest-even of the f32
 * value in that format and `lo` (optional) the same rounding of the residual v - hi:
 *   RSA_PF_BF16: 8 + 8 significant bits with both halves, f32 range                       -> v_mfma_f32_16x16x32_bf16
 *   RSA_PF_F16 : 11 significant bits with hi alone, 22 with both, |v| < 65504             -> v_mfma_f32_16x16x32_f16
 * The one-product fp16 mode (products == 1, in_fmt == RSA_PF_F16) reads hi only: a third of the matrix instructions and half the
 * activation bytes of products == 3; the engine's `precision = 'auto'` uses it where the error budget allows. */
enum rsa_plane_fmt { RSA_PF_BF16 = 0, RSA_PF_F16 = 1 };

/*
 * One fused convolution launch.
 *
 * Replaces, in one kernel, the reference sequence
 *   [torch.cat of earlier outputs] -> [nn.Upsample(x2, nearest)] -> nn.Conv2d(k=1|3, s=1, zero pad k/2, bias)
 *   -> [activation] -> [* alpha + residual] -> [* beta + residual2] -> [nn.PixelShuffle]
 * i.e. utilities/block.py:148-200 (conv_block), :454-465 (ResidualDenseBlock_5C.forward),
 * :340-344 (RRDB.forward), :83-91 (ShortcutBlock), :510-537 (upconv_block), :477-507
 * (pixelshuffle_block); archs/spanplus/arch.py:94-130; archs/swinir/arch.py:34-40 (Linear = k1 conv).
 *
 * Arithmetic: implicit GEMM on v_mfma_f32_16x16x32_bf16 / _f16 (in_fmt), f32 accumulate.
 *   products == 1 : acc += hi(a)*hi(w)                                 ("bf16" / "fp16")
 *   products == 3 : acc += hi(a)*hi(w) + lo(a)*hi(w) + hi(a)*lo(w)     ("bf16x3": ~16-bit operands; "fp16x3": ~22-bit)
 */
typedef struct rsa_conv_params {
  /* geometry */
  int32_t batch;        /* N */
  int32_t H, W;         /* OUTPUT height/width in pixels (before pixel_shuffle) */
  int32_t ksize;        /* 1 or 3 */
  int32_t upsample2x;   /* 1: input map is (H/2 x W/2), nearest-upsampled on read */
  int32_t cin_planes;   /* input planes (of 8 channels) consumed, starting at in_hi/in_lo */
  int32_t cout;         /* real output channels */
  int32_t products;     /* 1 or 3 */

  /* input, split planes; strides in 16-byte units */
  const void* in_hi;
  const void* in_lo;        /* may be NULL when products == 1 */
  int64_t in_plane_stride;  /* units between planes  (= Hin*Win for a dense tensor) */
  int64_t in_batch_stride;  /* units between images  */

  /* weights in the packed layout described below (resselt_amd/engine/pack.py), bias f32[round_up(cout,16)] */
  const void* w_packed;
  const float* bias; /* may be NULL */

  /* epilogue */
  int32_t act;      /* enum rsa_act */
  float act_param;  /* LeakyReLU slope */
  float alpha;      /* used when res1 != NULL (or act == SPAB gate) */
  const float* res1; /* f32 NCHW4c [N][ceil(cout/4)][H][W][4] */
  float beta;
  const float* res2;

  /* outputs; each may be NULL */
  void* out_hi;             /* split planes, written at plane offset out_plane_off */
  void* out_lo;             /* NULL allowed (bf16 single-plane consumers) */
  int32_t out_plane_off;    /* first plane written (cout/8 planes follow; tail channels zeroed) */
  int64_t out_plane_stride; /* units */
  int64_t out_batch_stride; /* units */
  float* out_f32;           /* f32 NCHW4c residual stream */

  void* out_nchw;           /* final plain tensor [N][cout/r^2][H*r][W*r], dtype out_dtype -- or, for RSA_U8, the 8-bit image
                               [N][H*r][W*r][cout/r^2]; exclusive with out_hi/out_f32/res1/res2 (separate kernel instantiation) */
  int32_t out_dtype;        /* enum rsa_dtype */
  int32_t pixel_shuffle;    /* r >= 1 (depth-to-space factor applied while storing out_nchw; r > 1: out_nchw 16-byte aligned) */
  float out_scale;          /* out_nchw value = v * out_scale + out_shift[oc]  (SwinIR x/img_range + mean, */
  const float* out_shift;   /*   archs/swinir/arch.py:1013); NULL = none */
  const float* act_vec;     /* RSA_ACT_PRELU: negative slopes, f32[round_up(cout,16)], 16-byte aligned */
  const void* out_base;     /* optional with out_nchw: plain [N][cout/r^2][H][W] tensor of dtype out_dtype whose pixel (y,x) is
                               ADDED to all r x r output pixels it covers (nearest-upsampled base image, compact/arch.py:61-64) */
  int32_t out_base_div;     /* 0: the base image is H x W as described above.  > 0: the base image is out_base_h x out_base_w and output pixel
                               (Y, X) receives base pixel (min(Y / div, h-1), min(X / div, w-1)) -- F.interpolate(x, scale_factor=div) of the
                               UNPADDED input under a padded / unshuffled convolution grid (rtmosr/arch.py:383-387) */
  int32_t out_base_h, out_base_w;
  int32_t w_layout;         /* layout of w_packed: must equal rsa_conv_weight_layout(this descriptor); see rsa_pack_weights */
  /* Residual operands as SPLIT PLANES instead of f32 maps (value = hi + lo, ~16 bits): the residual stream of a residual dense block
   * is then stored once (the planes the next convolution reads) instead of twice.  res1_hi excludes res1, res2_hi excludes res2;
   * the planes start at the residual's channel 0; strides in 16-byte units, shared by both; lo pointers may be NULL (hi only). */
  const void* res1_hi;
  const void* res1_lo;
  const void* res2_hi;
  const void* res2_lo;
  int64_t res_plane_stride;
  int64_t res_batch_stride;
  /* enum rsa_plane_fmt of the three plane operands (0 = bf16, the default of a zeroed descriptor) */
  int32_t in_fmt;   /* in_hi / in_lo AND w_packed: selects the matrix instruction */
  int32_t out_fmt;  /* out_hi / out_lo */
  int32_t res_fmt;  /* res1_hi / res1_lo / res2_hi / res2_lo */
  int32_t tile_order; /* ring schedule only: 0 = output tiles in band order from the top of the map, 1 = the same order reversed (bottom first).
                         Alternating it between consecutive layers makes a layer start on the rows its producer wrote last, which are still in
                         the 256 MB Infinity Cache (a 1080p layer moves 0.4-0.9 GB); other schedules ignore it.  Any other value: RSA_E_ARG */
  /* Round 4: the lo halves of an fp16 residual stream as 8-bit codes.  A residual dense block's `x5 * 0.2 + x` (reference
   * utilities/block.py:463-465) carries its stream as hi (fp16) + lo; |lo| is at most half an ulp of hi = 2^12 f32 ulps, so a signed byte
   * codes it as the distance from f32(hi) to the value in steps of 32 f32 ulps, counted along the f32 bit patterns:
   *   code = min((sat16(bits(v) - bits(f32(hi))) + 16) >> 5, 127) & 0xff,   value = as_float(bits(f32(hi)) + (code << 5)).
   * hi + code keep 19 significant bits (fp16 hi + fp16 lo: 22) and the stream is 3 bytes per channel instead of 4; with hi = 0 or subnormal
   * any code decodes to within 2^-24 of the value, a non-finite hi keeps the stream's hi non-finite.  An lo8 plane holds 8-byte units
   * [n][plane][y][x][8 codes]: the plane stride is that of the hi planes (in units), the batch stride is lo8_batch_stride (8-byte units).
   * Bits of lo8_flags: RSA_LO8_RES1 (res1_lo), RSA_LO8_RES2 (res2_lo), RSA_LO8_OUT (out_lo); only with fp16 planes (res_fmt / out_fmt =
   * RSA_PF_F16) and plane residuals / outputs that have hi + lo. */
  int32_t lo8_flags;
  int32_t reserved_lo8;     /* must be 0 */
  int64_t lo8_batch_stride; /* 8-byte units between images of an lo8 buffer (shared by the flagged operands) */
  /* Channel pooling in the epilogue (RCAN's channel attention, csrc/rcan.hip): NULL, the value of a zeroed descriptor, = off.  When set, the
   * launch also writes per-output-channel partial sums of its f32 epilogue values (after bias and activation, before they are rounded to
   * planes; pixels outside the map excluded) as f32 [batch][slots][16 * ceil(cout / 16)], slots = rsa_conv_pool_slots(p): every entry is
   * written by exactly one wave, no atomics, a fixed reduction order -- two runs give the same bits, and the planes are the bits of the
   * same launch without pooling.  Compiled for the ring schedule's 3x3 layers with 48 or 64 output channels, bias + LeakyReLU / linear,
   * plane output (optionally the f32 map), no residual, in three bf16 products and in one fp16 product; anything else: RSA_E_UNSUPPORTED. */
  float* pool_sums;
} rsa_conv_params;
#define RSA_LO8_RES1 1
#define RSA_LO8_RES2 2
#define RSA_LO8_OUT 4

/* Launch `n` fused convolutions in order on `stream` (one host call per forward pass).  Both return RSA_E_INTERNAL, without launching,
 * when a kernel of an EARLIER call has reported a protocol failure that rsa_check_status has not yet been asked about. */
int rsa_conv2d(const rsa_conv_params* p, void* stream);
int rsa_conv2d_list(const rsa_conv_params* list, int32_t n, void* stream);

/* Cross-layer fusion of a residual dense block (SURVEY.md 8b `sr_rdb_fused`; reference utilities/block.py:454-465): descriptors `a` and `b`
 * are a FUSABLE PAIR when b is the growth convolution that follows a in the block -- both 3x3, one fp16 product, 32 output channels, bias +
 * LeakyReLU / linear into hi-only fp16 planes, a writing the four planes right behind its own input planes and b reading a's input planes
 * plus those four (conv1 -> conv2, conv3 -> conv4).  rsa_conv2d_pair runs both in one launch that streams the common input through LDS once
 * (b's last 32 input channels never leave the chip before b has used them; a's output is still written for the later layers); the result
 * is bit-identical to rsa_conv2d(a) followed by rsa_conv2d(b).  rsa_conv2d_list fuses such neighbours by itself unless RSA_CONV_PAIR=0
 * is set in the environment.  rsa_conv_pair_fusable: 1 when the list would fuse (a, b), else 0.  rsa_conv2d_pair on anything else:
 * RSA_E_UNSUPPORTED.  Both descriptors carry their own packed weights (layout 1), exactly as for separate launches.
 * A fused launch is ONE sweep over the map: it walks its tiles in the direction of its FIRST descriptor (a.tile_order; b.tile_order is not
 * looked at).  A caller that alternates tile_order alternates it per launch, giving both halves of a fusable pair the same value. */
int rsa_conv2d_pair(const rsa_conv_params* a, const rsa_conv_params* b, void* stream);
int rsa_conv_pair_fusable(const rsa_conv_params* a, const rsa_conv_params* b);

/* Failure word of the ring schedule (csrc/conv_ring.h: a hand-off between the loader wave and the compute waves that timed out makes the
 * kernel drain with wrong pixels).  The kernels report into host-visible memory, so this call never synchronises: it sees the failures of
 * every launch that has COMPLETED.  Call it after the stream (or an event behind the forward) has been synchronised to judge that forward.
 * Returns RSA_OK, or RSA_E_INTERNAL once (the word is cleared; rsa_last_error_string says how many hand-offs failed). */
int rsa_check_status(void);

/* Range guard of the fp16 plane format.  The fp16 epilogues convert with v_cvt_pk_f16_f32, which turns a value beyond +-65504 into an
 * infinity; the infinity (or the NaN that inf - inf / inf * 0 make of it) then travels with the residual stream of the network to its end --
 * the reference's `x5 * 0.2 + x` (utilities/block.py:463-465) carries it -- where ONE pass over a small tensor finds it.  This call scans
 * `count` elements of a plain array (`dtype`: RSA_F32 / RSA_F16 / RSA_BF16; a split-plane buffer is such an array of its 16-bit format) on
 * `stream` and adds to a host-visible word when it meets a non-finite value; it never synchronises.  rsa_check_status() then returns
 * RSA_E_FP16_RANGE once (after RSA_E_INTERNAL, which has priority).  The engine runs it behind every forward of a model whose precision
 * policy has fp16 layers (0.06 % of an RRDBNet 1080p frame) and `precision = 'auto'` answers a hit by re-running in three bf16 products.
 * (A saturating convert was rejected: it would turn an out-of-range activation into a finite wrong value that no later check can see.) */
int rsa_check_finite(const void* data, int32_t dtype, int64_t count, void* stream);

/* Bytes of the packed weight blob for a (cout, cin_planes, ksize, products) convolution. */
int64_t rsa_packed_weight_bytes(int32_t cout, int32_t cin_planes, int32_t ksize, int32_t products);
/* the same for a given layout (layouts 0..2 have the size above; layout 3 is 32 K steps of 4 cout tiles = 256 KiB) */
int64_t rsa_packed_weight_bytes_layout(int32_t cout, int32_t cin_planes, int32_t ksize, int32_t products, int32_t layout);

/* Number of 16-channel cout tiles one workgroup computes for `cout` output channels (1..4); the grid has
 * ceil(ceil(cout/16) / tiles) slabs in y.  Exposed so host code and tests can reason about launch geometry. */
int rsa_conv_cout_tiles(int32_t cout);

/* Slots per image of rsa_conv_params.pool_sums for this descriptor (its pool_sums field itself is not looked at): 16 x 32 pixel tiles of
 * the map times the row groups of waves that own a tile.  RSA_E_UNSUPPORTED when the pooling epilogue is not compiled for the descriptor. */
int rsa_conv_pool_slots(const rsa_conv_params* p);

/*
 * Weight packing: OIHW f32 weights (device pointer, contiguous [cout][cin][k][k]) -> the MFMA A-fragment blob of
 * rsa_packed_weight_bytes(cout, cin_planes, ksize, products) bytes that rsa_conv2d streams.  Replaces what
 * nn.Module.load_state_dict does with an nn.Conv2d / nn.Linear weight (reference registry.py:113).  Two K orders exist and the
 * schedule a descriptor dispatches to fixes which one it reads; ask with rsa_conv_weight_layout(descriptor) (every field except
 * w_packed / w_layout filled in) and pass the answer as `layout` here and as rsa_conv_params.w_layout:
 *   0  blob[chunk q][tap t][cout_tile][hi|lo][lane 0..63][8] bf16, lane l: cout = 16*tile + (l & 15), cin = 32*q + 8*(l >> 4) + j
 *   1  tap-pair order of the ring schedule (3x3, three products, whole 32-channel chunks): resselt_amd/csrc/pack.hip
 *   2  the same per 16-channel half chunk, five K steps each (an odd number of half chunks, e.g. 48 input channels)
 *   3  nearest x2 upsampling + 3x3 as four 2x2 phase convolutions on the source map, taps pre-summed (64 -> 64 channels;
 *      resselt_amd/csrc/conv_ring_up.h)
 * (hi = RNE of w in `fmt` (enum rsa_plane_fmt), lo = the same rounding of w - hi; only hi when products == 1).
 */
int rsa_conv_weight_layout(const rsa_conv_params* p);
int rsa_pack_weights(const float* w_oihw, int32_t cout, int32_t cin, int32_t cin_planes, int32_t ksize, int32_t products, int32_t layout,
                     int32_t fmt, void* out, void* stream);

/* Name of the kernel a descriptor dispatches to (matches the rocprofv3 kernel names; bench.py groups its rooflines by it). */
const char* rsa_conv_kernel_name(const rsa_conv_params* p);

/* Debug: hand-offs of the ring schedule that ran into their spin bound since the last call (always 0 in a correct build; tests assert it).
 * Synchronises the device (unlike rsa_check_status, which is the product's way to learn of the same event). */
int rsa_debug_ring_aborts(void);
/* Debug: polls a hand-off of the ring schedule may spend before it gives up (default 2^18; 1 forces the failure path: tests). */
int rsa_debug_set_ring_spin_limit(int32_t polls);
/* Debug: force the ring schedule on (1) / off (0) for descriptors built afterwards, or follow RSA_CONV_RING again (-1).  Descriptors carry
 * the layout they were built for, so change it only between building descriptor sets (in-process A/B timing). */
int rsa_debug_set_ring(int32_t mode);
/* Debug: pair fusion inside rsa_conv2d_list on (1) / off (0), or follow RSA_CONV_PAIR again (-1): in-process A/B timing. */
int rsa_debug_set_pair(int32_t mode);

/*
 * Plain NCHW tensor [N][C][src_h][src_w] -> split planes of size H x W, with per-channel affine v = (x - mean[c]) * scale.
 * Replaces the implicit NCHW read of the first conv, `(x - mean) * img_range` (archs/span/arch.py:232-234,
 * archs/swinir/arch.py:966-967) and, when H > src_h or W > src_w, the right/bottom REFLECT padding of
 * pad_to_multiple (utilities/padding.py:24-29; SwinIR.check_image_size).  Channels padded to 8 with zeros.
 * unshuffle = r > 1 additionally fuses torch.pixel_unshuffle(x, r) (RRDBNet x2plus/x1 front end, archs/esrgan/arch.py:130-137):
 * the planes then hold C*r*r channels of an (H x W) grid covering H*r x W*r source pixels.
 */
int rsa_nchw_to_planes(const void* x, int32_t dtype, int32_t batch, int32_t C, int32_t H, int32_t W, int32_t src_h, int32_t src_w,
                       int32_t unshuffle, const float* mean, float scale, void* out_hi, void* out_lo, int64_t out_plane_stride,
                       int64_t out_batch_stride, int32_t out_fmt, void* stream);

/* split planes / f32 NCHW4c -> plain NCHW (debug + parity of intermediates) */
int rsa_planes_to_nchw(const void* hi, const void* lo, int64_t plane_stride, int64_t batch_stride, int32_t batch,
                       int32_t C, int32_t H, int32_t W, int32_t fmt, float* out, void* stream);

/*
 * DySample upsampler head: sigmoid-gated learned offsets -> bilinear border gather over channel groups -> 1x1 conv.
 * Replaces resselt/utilities/dysample.py:47-83 after the two 1x1 offset/scope convs (run as ONE rsa_conv2d whose
 * f32 NCHW4c output holds offset channels [0, oc) and scope channels [oc, 2*oc), oc = 2*groups*scale^2).
 */
typedef struct rsa_dysample_params {
  int32_t batch;
  int32_t H, W;          /* low-resolution size */
  int32_t C;             /* feature channels, multiple of 4*groups */
  int32_t groups;        /* 4 in the reference */
  int32_t scale;
  int32_t out_ch;        /* 1..8 */
  const float* x_f32;    /* features, f32 NCHW4c [N][C/4][H][W][4] */
  const float* offscope; /* f32 NCHW4c [N][2*oc/4][H][W][4] */
  const float* init_pos; /* [oc] (registered buffer of the reference module, dysample.py:43-45) */
  const float* end_w;    /* [out_ch][C]; NULL = x_f32 is PRE-PROJECTED: C == 4*groups, channel 4g+o = sum over the channels c of group g of
                            W_end[o][c] * x[c] (the 1x1 end conv applied per group at low resolution; sampling is linear), out_ch <= 4 */
  const float* end_b;    /* [out_ch] or NULL */
  void* out_nchw;        /* [N][out_ch][H*scale][W*scale] */
  int32_t out_dtype;     /* enum rsa_dtype */
} rsa_dysample_params;

int rsa_dysample(const rsa_dysample_params* p, void* stream);

/*
 * nn.LayerNorm over the channel axis of a token map (tokens = pixels).
 * Replaces norm1 / norm2 / patch_embed.norm / norm of resselt/archs/swinir/arch.py:306,333,640,959 together with the
 * flatten/transpose/view round trips of PatchEmbed / PatchUnEmbed (:638-642,679-682): the map never changes layout.
 */
typedef struct rsa_layernorm_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;               /* channels normalised over */
  float eps;
  const float* x_f32;      /* f32 NCHW4c [N][ceil(C/4)][H][W][4] */
  const float* gamma;      /* [C] */
  const float* beta;       /* [C] */
  void* out_hi;            /* split planes [N][ceil(C/8)][H][W][8], tail channels zeroed; may be NULL */
  void* out_lo;            /* may be NULL */
  int64_t out_plane_stride; /* 16-byte units; with out_hi set, at least H*W (RSA_E_ARG otherwise) */
  int64_t out_batch_stride;
  float* out_f32;          /* optional f32 NCHW4c copy of the result */
  int32_t out_fmt;         /* enum rsa_plane_fmt of out_hi / out_lo */
  int32_t reserved0;       /* must be 0 */
} rsa_layernorm_params;

int rsa_layernorm(const rsa_layernorm_params* p, void* stream);

/*
 * (Shifted-)window multi-head self-attention core: softmax(q k^T + B[idx] (+ mask)) v for every window and head.
 * Replaces, between the qkv and proj Linear layers, resselt/archs/swinir/arch.py:141-170 (WindowAttention.forward) and the
 * torch.roll / window_partition / window_reverse / calculate_mask data movement of SwinTransformerBlock.forward (:295-335).
 * Input planes: [(which*heads + head)*4, +4) hold 32 channels (head_dim zero-padded) of q (pre-scaled), k, v.
 * bias_frag: relative_position_bias_table gathered by relative_position_index and laid out in accumulator-fragment order
 *            [head][query tile 2][key tile 2][lane 64][16] f32 (resselt_amd/archs/swinir/arch.py::bias_fragments);
 *            key slots beyond window^2 carry -1e30.
 */
typedef struct rsa_window_attn_params {
  int32_t batch;
  int32_t H, W;            /* multiples of `window` */
  int32_t heads;
  int32_t window;          /* <= 8 */
  int32_t shift;           /* 0 or window/2 */
  int32_t products;        /* 1 or 3 */
  const void* qkv_hi;
  const void* qkv_lo;      /* may be NULL when products == 1 */
  int64_t qkv_plane_stride; /* 16-byte units */
  int64_t qkv_batch_stride;
  const float* bias_frag;
  void* out_hi;            /* planes [head*4, +4) : attention output, head_dim padded to 32 */
  void* out_lo;
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_window_attn_params;

int rsa_window_attention(const rsa_window_attn_params* p, void* stream);

/* ------------------------------------------------------------------------------------------- fused Swin block halves
 * The two halves of SwinTransformerBlock.forward (resselt/archs/swinir/arch.py:295-335), each as ONE launch that reads the f32
 * residual stream once and writes it once; everything between (LayerNorm output, q / k / v, attention output, the MLP's hidden map)
 * stays in LDS and registers.  One workgroup = 64 tokens (a window, or 64 consecutive tokens for the MLP).
 *
 * rsa_swin_attn_block:  out = x + proj(window_attention(qkv(norm1(x))))      (:295-330 with WindowAttention.forward :133-173,
 *                       torch.roll / window_partition / window_reverse / calculate_mask as index arithmetic)
 * rsa_swin_mlp_block :  out = x + fc2(GELU(fc1(norm2(x))))                   (:331-335 with Mlp.forward :34-40)
 *
 * Weights are rsa_pack_weights blobs in layout 0 (ksize 1): wqkv over rows regrouped per head (row (which, head, d) with head_dim
 * zero-padded to 32 and the q rows pre-scaled; cin_planes = ceil(C/8)), wproj over columns padded the same way (cin_planes =
 * 4*heads), w1 [hidden][C] (cin_planes = ceil(C/8)), w2 [C][hidden] (cin_planes = ceil(hidden/8)).  Biases are f32 vectors padded
 * with zeros to a multiple of 16.  bias_frag16: relative_position_bias_table[relative_position_index] in the accumulator order of
 * 16x16 tiles, [head][key tile 4][query tile 4][lane 64][4] f32: lane l, element r <-> key 16*kt + 4*(l >> 4) + r, query
 * 16*qt + (l & 15), every value multiplied by log2(e) (the kernel's softmax runs in base 2); key slots beyond window^2 carry -1e30.  Limits: C <= 256 (a multiple of 4), heads <= 8, head_dim <= 32,
 * window <= 8, hidden <= 512; `out` may be `x` (in place). */
typedef struct rsa_swin_attn_block_params {
  int32_t batch;
  int32_t H, W;            /* multiples of `window` */
  int32_t C;               /* embedding width */
  int32_t heads;
  int32_t window;          /* <= 8 */
  int32_t shift;           /* 0 or window/2 */
  int32_t products;        /* 1 or 3 */
  float eps;               /* LayerNorm epsilon */
  const float* x;          /* f32 NCHW4c [N][ceil(C/4)][H][W][4] */
  const float* gamma;      /* norm1 weight / bias, [C] */
  const float* beta;
  const void* wqkv;        /* packed, cout = 3*heads*32 */
  const float* bqkv;       /* [3*heads*32] */
  const float* bias_frag16;
  const void* wproj;       /* packed, cout = C, cin_planes = 4*heads */
  const float* bproj;      /* [C] padded to 16 */
  float* out;              /* f32 NCHW4c, same shape as x */
} rsa_swin_attn_block_params;

int rsa_swin_attn_block(const rsa_swin_attn_block_params* p, void* stream);

typedef struct rsa_swin_mlp_block_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;
  int32_t hidden;
  int32_t products;        /* 1 or 3 */
  float eps;
  const float* x;          /* f32 NCHW4c */
  const float* gamma;      /* norm2 weight / bias, [C] */
  const float* beta;
  const void* w1;          /* packed, cout = hidden, cin_planes = ceil(C/8) */
  const float* b1;         /* [hidden] padded to 16 */
  const void* w2;          /* packed, cout = C, cin_planes = ceil(hidden/8) */
  const float* b2;         /* [C] padded to 16 */
  float* out;              /* f32 NCHW4c */
  void* out_hi;            /* optional split-plane copy of the result (the input of the convolution that follows a block group) */
  void* out_lo;
  int64_t out_plane_stride; /* 16-byte units */
  int64_t out_batch_stride;
  int32_t fmt;             /* enum rsa_plane_fmt of w1 / w2 and of the kernel's internal images (selects the matrix instruction): RSA_PF_F16 with
                              products == 1 is the one-product fp16 form; out_hi / out_lo are bf16 planes in every form */
  int32_t reserved0;       /* must be 0 */
} rsa_swin_mlp_block_params;

int rsa_swin_mlp_block(const rsa_swin_mlp_block_params* p, void* stream);

/* rsa_swin_block: both halves in one launch -- out = x1 + fc2(GELU(fc1(norm2(x1)))), x1 = x + proj(window_attention(qkv(norm1(x))))
 * (SwinTransformerBlock.forward, resselt/archs/swinir/arch.py:295-335).  x1 stays in registers: the residual stream is read once and
 * written once per block.  Operands and limits as for the two half launches above (resselt_amd/csrc/swin_block_full.hip). */
typedef struct rsa_swin_block_params {
  int32_t batch;
  int32_t H, W;            /* multiples of `window` */
  int32_t C;
  int32_t heads;
  int32_t window;          /* <= 8 */
  int32_t shift;           /* 0 or window/2 */
  int32_t hidden;
  int32_t products;        /* 1 or 3 */
  float eps;
  const float* x;          /* f32 NCHW4c */
  const float* gamma1;     /* norm1 */
  const float* beta1;
  const void* wqkv;
  const float* bqkv;
  const float* bias_frag16;
  const void* wproj;
  const float* bproj;
  const float* gamma2;     /* norm2 */
  const float* beta2;
  const void* w1;
  const float* b1;
  const void* w2;
  const float* b2;
  float* out;              /* f32 NCHW4c; may be x */
  void* out_hi;            /* optional split-plane copy of the result */
  void* out_lo;
  int64_t out_plane_stride; /* 16-byte units */
  int64_t out_batch_stride;
  int32_t fmt;             /* enum rsa_plane_fmt of the packed weights, of the on-chip operand images and of out_hi / out_lo.  fp16 is compiled
                              for products == 1: that instantiation keeps no lo images, its LDS array is 64 KB and two windows share a CU */
  int32_t reserved0;       /* must be 0 */
} rsa_swin_block_params;

int rsa_swin_block(const rsa_swin_block_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- DAT ops
 * Building blocks of the Dual Aggregation Transformer path (reference archs/dat/arch.py).  Tokens are pixels; every map is in
 * the split-plane layout [N][planes][H][W][8] (bf16 hi, optional lo).  Attention maps use the head-padded channel layout of
 * rsa_window_attention: head h owns channels [32h, 32h+32), head_dim <= 32, pad channels are zero. */

/* Rectangular (shifted) window attention core of Spatial_Attention.forward (arch.py:224-267) together with the zero padding,
 * torch.roll, img2windows / windows2img and calculate_mask of Adaptive_Spatial_Attention.forward (arch.py:336-411, 446-492).
 * One call = one branch (one window orientation) over `heads` consecutive head slots starting at `head0`. */
typedef struct rsa_rect_attn_params {
  int32_t batch;
  int32_t H, W;             /* token map size; tokens outside it (padding up to Hp x Wp) have q = k = v = 0 */
  int32_t Hp, Wp;           /* padded grid: multiples of win_h / win_w, >= H / W */
  int32_t win_h, win_w;     /* win_h * win_w <= 256 */
  int32_t shift_h, shift_w; /* 0 (no mask) or the cyclic shift; 0 <= shift < win */
  int32_t heads;            /* head slots this call processes */
  int32_t head0;            /* first of them */
  int32_t heads_total;      /* head slots per q / k / v group: q planes [0, 4*heads_total), then k, then v */
  int32_t products;         /* 1 or 3 */
  const void* qkv_hi;
  const void* qkv_lo;       /* may be NULL when products == 1 */
  int64_t qkv_plane_stride; /* 16-byte units */
  int64_t qkv_batch_stride;
  const float* bias_frag;   /* [heads][T][T][64][16] f32, T = tiles of 32 tokens (1, 2, 4 or 8): S^T accumulator order, -1e30 on padded keys */
  void* out_hi;             /* planes [(head0 + h)*4, +4) */
  void* out_lo;
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  /* Cross-window mode (0 = off): keys / values come from the kwin_h x kwin_w window that starts kpad pixels up-left of the query
   * window, zeros outside the map -- OCAB of HAT (reference archs/hat/arch.py:403-470: nn.Unfold with padding).  bias_frag is then
   * [heads][QT][KT][64][16] with QT = ceil(win_h*win_w / 32), KT = ceil(kwin_h*kwin_w / 32).  No shift, Hp == H, Wp == W. */
  int32_t kwin_h, kwin_w;
  int32_t kpad_h, kpad_w;
  /* Wide heads: a head slot is head_chunks x 4 planes (head_dim <= 32*head_chunks, zero-padded), 0 or 1 = the 32-channel slots above;
   * 2..4 (self-attention only): DRCT's dense groups run heads of 46..122 channels (reference archs/drct/arch.py:204-329).  q planes
   * [0, 4*head_chunks*heads_total), then k, then v; out planes [(head0 + h)*4*head_chunks, +4*head_chunks). */
  int32_t head_chunks;
  int32_t fmt;              /* enum rsa_plane_fmt of the q / k / v planes AND of the output planes (0 = bf16).  RSA_PF_F16 with products == 1: the
                               one-product fp16 form (v_mfma_f32_32x32x16_f16; probabilities rounded to fp16) */
  int32_t reserved0;        /* must be 0 */
} rsa_rect_attn_params;
int rsa_rect_attention(const rsa_rect_attn_params* p, void* stream);

/* Channel ("transposed") attention weights of Adaptive_Channel_Attention.forward (arch.py:577-585):
 *   attn[b][h] = softmax_j( normalize(q)[i] . normalize(k)[j] * temperature[h] )   over ALL tokens of image b,
 * written as the packed bf16 hi/lo weights of a block-diagonal 1x1 convolution (rsa_conv2d, cin = cout = 32*heads) so that
 * `attn @ v` is one more launch of the convolution kernel.  Two deterministic stages (per-chunk partial Gram matrices in
 * `workspace`, then one workgroup per (image, head)); no atomics. */
typedef struct rsa_channel_attn_params {
  int32_t batch;
  int32_t H, W;
  int32_t heads;
  int32_t head_dim;          /* <= 32 */
  int32_t products;          /* layout of w_packed: 3 = hi+lo, 1 = hi only */
  const void* q_hi;          /* planes [4h, 4h+4) = head h */
  const void* q_lo;          /* may be NULL */
  const void* k_hi;
  const void* k_lo;
  int64_t plane_stride;      /* 16-byte units (same for q and k) */
  int64_t batch_stride;
  const float* temperature;  /* [heads] */
  float* workspace;          /* >= rsa_channel_attn_workspace_bytes() */
  void* w_packed;            /* [batch] blobs of rsa_packed_weight_bytes(32*heads, 4*heads, 1, products); off-diagonal blocks must be zero */
  int32_t fmt;               /* enum rsa_plane_fmt of q / k AND of the packed weights written (0 = bf16, the default of a zeroed descriptor; round 4: fp16 planes) */
  int32_t reserved1;         /* must be 0 */
} rsa_channel_attn_params;
int64_t rsa_channel_attn_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t heads);
int rsa_channel_attention_weights(const rsa_channel_attn_params* p, void* stream);

/* Depthwise 3x3 convolution, zero padding 1 (arch.py:52, 322, 540):  out = act(dw(x') + bias) [* mul]
 * with x' = x, or x' = (x - mean_p) * rstd_p * gamma_c + beta_c when `stats` is given (the LayerNorm of SpatialGate, arch.py:55-59,
 * applied on the fly from per-pixel statistics; padding stays zero AFTER the normalisation).  BatchNorm(eval) is folded by the host. */
typedef struct rsa_dwconv_params {
  int32_t batch;
  int32_t H, W;
  int32_t planes;            /* 8 channels each */
  int32_t act;               /* RSA_ACT_NONE or RSA_ACT_GELU */
  const void* in_hi;
  const void* in_lo;         /* may be NULL */
  int64_t in_plane_stride;
  int64_t in_batch_stride;
  const float* weight;       /* [planes*8][9] */
  const float* bias;         /* [planes*8] */
  const float* stats;        /* optional [batch][H*W][2] = (mean, rstd) */
  const float* gamma;        /* [planes*8], with stats */
  const float* beta;
  const void* mul_hi;        /* optional elementwise multiplier map */
  const void* mul_lo;
  int64_t mul_plane_stride;
  int64_t mul_batch_stride;
  void* out_hi;
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  int32_t fmt;               /* enum rsa_plane_fmt of every plane operand of this call (0 = bf16, the default of a zeroed descriptor; round 4: fp16 planes) */
  int32_t reserved1;         /* must be 0 */
} rsa_dwconv_params;
int rsa_dwconv3x3(const rsa_dwconv_params* p, void* stream);
/* Depthwise 5x5, zero padding 2, weight [planes*8][25]: OmniShift of RTMoSR re-parameterised to one kernel (archs/rtmosr/arch.py:253-289).
 * act must be RSA_ACT_NONE and stats NULL; the optional multiplier map is supported. */
int rsa_dwconv5x5(const rsa_dwconv_params* p, void* stream);

/* Per-pixel LayerNorm statistics over channels [0, C) of a plane range: stats[b][pixel] = (mean, 1/sqrt(var + eps)). */
int rsa_plane_stats(const void* in_hi, const void* in_lo, int64_t plane_stride, int64_t batch_stride, int32_t batch, int32_t H, int32_t W,
                    int32_t C, float eps, float* stats, void* stream);
/* the same over planes of format `fmt` (enum rsa_plane_fmt; rsa_plane_stats = bf16 planes) */
int rsa_plane_stats_fmt(const void* in_hi, const void* in_lo, int64_t plane_stride, int64_t batch_stride, int32_t batch, int32_t H, int32_t W,
                        int32_t C, float eps, int32_t fmt, float* stats, void* stream);

/* channel_interaction of the AIM (arch.py:326-332): gate[b][c] = sigmoid( W2 . gelu(W1 . mean_pixels(x[b]) + b1) + b2 ).
 * BatchNorm(eval) folded into W1/b1 by the host.  Deterministic two-stage mean; `workspace` >= rsa_channel_gate_workspace_bytes(). */
typedef struct rsa_channel_gate_params {
  int32_t batch;
  int32_t H, W;
  int32_t planes;            /* C = 8*planes (pad channels carry zero weights) */
  int32_t hidden;            /* <= 128 */
  const void* in_hi;
  const void* in_lo;         /* may be NULL */
  int64_t in_plane_stride;
  int64_t in_batch_stride;
  const float* w1;           /* [hidden][C] */
  const float* b1;           /* [hidden] */
  const float* w2;           /* [C][hidden] */
  const float* b2;           /* [C] */
  float* workspace;
  float* gate;               /* [batch][C] */
  int32_t relu;              /* 0 = GELU hidden, sigmoid gate (DAT); 1 = ReLU, sigmoid (the RCAN-style channel attention of HAT's CAB,
                                archs/hat/arch.py:28-35); 2 = ReLU, Hardsigmoid (RTMoSR's CSELayer, archs/rtmosr/arch.py:7-22);
                                3 = SiLU, sigmoid (OmniSR's MBConv squeeze-excitation, archs/omni/arch.py:446-461).  Any other value is
                                RSA_E_ARG (before OmniSR, every non-zero value ran as mode 1) */
  int32_t fmt;               /* enum rsa_plane_fmt of every plane operand of this call (0 = bf16, the default of a zeroed descriptor; round 4: fp16 planes) */
} rsa_channel_gate_params;
int64_t rsa_channel_gate_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t planes);
int rsa_channel_gate(const rsa_channel_gate_params* p, void* stream);

/* Adaptive Interaction Module combine (arch.py:494-508 and 595-607):  s = w2 . gelu(W1 . src[p] + b1) + b2  (spatial_interaction, BN folded)
 *   mode 0 (spatial block): src = att,  out = att * gate[c] + sigmoid(s) * conv
 *   mode 1 (channel block): src = conv, out = att * sigmoid(s) + conv * gate[c] */
typedef struct rsa_aim_params {
  int32_t batch;
  int32_t H, W;
  int32_t planes;
  int32_t hidden;            /* <= 16 */
  int32_t mode;
  const void* att_hi;
  const void* att_lo;
  int64_t att_plane_stride;
  int64_t att_batch_stride;
  const void* conv_hi;
  const void* conv_lo;
  int64_t conv_plane_stride;
  int64_t conv_batch_stride;
  const float* gate;         /* [batch][8*planes] */
  const float* w1;           /* [hidden][8*planes] */
  const float* b1;           /* [hidden] */
  const float* w2;           /* [hidden] */
  float b2;
  void* out_hi;
  void* out_lo;
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  int32_t fmt;               /* enum rsa_plane_fmt of every plane operand of this call (0 = bf16, the default of a zeroed descriptor; round 4: fp16 planes) */
  int32_t reserved1;         /* must be 0 */
} rsa_aim_params;
int rsa_aim_combine(const rsa_aim_params* p, void* stream);

/* out = base + x * gate[b][c] * scale on f32 maps [N][ceil(C/4)][H][W][4], x in split planes; gate rows have 8*ceil(C/8) entries.
 * HAT's `shortcut + conv_x * conv_scale` with the CAB's channel attention as the gate (reference archs/hat/arch.py:37-39, 345). */
int rsa_gated_add(const void* x_hi, const void* x_lo, int64_t plane_stride, int64_t batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C,
                  const float* gate, float scale, const float* base_f32, float* out_f32, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- RTMoSR ops
 * (reference archs/rtmosr/arch.py; every RepConv / OmniShift is re-parameterised to one kernel by the host) */

/* RMSNorm over channels (arch.py:32-37): out = scale[c] * x / (||x||_2 / sqrt(C) + eps) + offset[c];  f32 map in, split planes out. */
int rsa_rmsnorm(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, float eps, const float* scale, const float* offset, void* out_hi,
                void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride, void* stream);

/* ParPixelUnshuffle's two reads of its input (arch.py:292-299), `planes` planes of H x W (both even):
 *   unshuffled_f32: PixelUnshuffle(2) as an f32 map [N][planes*8][H/2][W/2][4] (f32 group c holds the 2x2 block of channel c) -- the
 *                   residual operand of the RepConv that follows;  pool: MaxPool2d(2) as split planes [N][planes][H/2][W/2][8]. */
int rsa_unshuffle_pool(const void* in_hi, const void* in_lo, int64_t in_plane_stride, int64_t in_batch_stride, int32_t batch, int32_t H, int32_t W,
                       int32_t planes, float* unshuffled_f32, void* pool_hi, void* pool_lo, int64_t pool_plane_stride, int64_t pool_batch_stride,
                       void* stream);

/* The gate of GatedCNNBlock.forward (arch.py:334-336):  out = mish(g) * cat(i, PixelShuffle(2)(c * gate)).
 * g = planes [0, g_planes) and i = planes [g_planes, g_planes + i_planes) of the fc1 output `f` (H x W); c = (g_planes - i_planes)*4
 * planes at H/2 x W/2 (the OmniShift output); gate = the SE layer's per-channel factors of c, or NULL. */
typedef struct rsa_gated_shuffle_params {
  int32_t batch;
  int32_t H, W;              /* both even */
  int32_t g_planes;          /* planes of g = planes of the output */
  int32_t i_planes;          /* planes of i */
  const void* f_hi;
  const void* f_lo;          /* may be NULL */
  int64_t f_plane_stride;
  int64_t f_batch_stride;
  const void* c_hi;
  const void* c_lo;
  int64_t c_plane_stride;
  int64_t c_batch_stride;
  const float* gate;         /* [batch][gate_stride] or NULL */
  int64_t gate_stride;
  void* out_hi;
  void* out_lo;
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_gated_shuffle_params;
int rsa_gated_shuffle_mul(const rsa_gated_shuffle_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- PLKSR ops
 * (reference archs/plksr/plksr.py and rplksr.py; resselt_amd/csrc/plksr.hip) */

/* Partial large-kernel convolution (PLKConv2d, rplksr.py:22-37, plksr.py:54-93): a dense K x K convolution, zero padding K/2, of
 * pdim = 8*planes input channels to pdim output channels + bias.  Input: `planes` planes at in_hi / in_lo.  Output: planes
 * [out_plane_off, out_plane_off + planes) of another buffer; no other plane is touched.  Arithmetic as rsa_conv2d: fmt RSA_PF_BF16 with
 * products == 3 (hi + lo) or RSA_PF_F16 with products == 1 (hi only), v_mfma_f32_16x16x32_{bf16,f16}, f32 accumulate.
 * w_packed: rsa_plk_packed_weight_bytes bytes, [plane p][K step s][cout tile ct][hi|lo][lane 64][8] where lane l of step s holds
 * W[16 ct + (l & 15)][8 p + j][tap 4 s + (l >> 4)] (taps row-major, zero past K*K and past pdim; resselt_amd/engine/plk.py).
 * bias: f32[16 * ceil(planes / 2)].  3 <= K <= 31 odd, planes <= 8. */
typedef struct rsa_plk_conv_params {
  int32_t batch;
  int32_t H, W;
  int32_t ksize;
  int32_t planes;           /* pdim / 8 */
  int32_t products;         /* 1 or 3 */
  const void* in_hi;
  const void* in_lo;        /* products == 3 only */
  int64_t in_plane_stride;  /* 16-byte units */
  int64_t in_batch_stride;
  const void* w_packed;
  const float* bias;
  void* out_hi;
  void* out_lo;             /* may be NULL */
  int64_t out_plane_stride; /* 16-byte units */
  int64_t out_batch_stride;
  int32_t out_plane_off;
  int32_t fmt;              /* enum rsa_plane_fmt of every plane operand and of w_packed */
  int32_t reserved0;        /* must be 0 */
  int32_t reserved1;
} rsa_plk_conv_params;
int64_t rsa_plk_packed_weight_bytes(int32_t ksize, int32_t planes, int32_t products);
int rsa_plk_conv(const rsa_plk_conv_params* p, void* stream);

/* nn.GroupNorm statistics over whole images (rplksr.py:94, 103): stats[n][g] = (mean, 1 / sqrt(var + eps)) of channels
 * [g*C/groups, (g+1)*C/groups) x every pixel of an f32 map [N][C/4][H][W][4] (biased variance, as torch).  Two deterministic stages: partial
 * (count, mean, M2) per chunk of pixels, computed around a per-group shift, into `workspace` (rsa_group_norm_workspace_bytes), then Chan's
 * pairwise combination per (image, group).  Stays on the device: rsa_group_norm_apply reads `stats` in stream order.  groups <= 8. */
int64_t rsa_group_norm_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t groups);
int rsa_group_norm_stats(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t groups, float eps, float* workspace,
                         float* stats, void* stream);

/* out = (x - mean_g) * rstd_g * gamma[c] + beta[c] + skip  (PLKBlock.forward of RealPLKSR, rplksr.py:98-105) -> split planes and/or an
 * f32 map (the next block's input and residual stream).  C a multiple of 8. */
typedef struct rsa_group_norm_apply_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;
  int32_t groups;
  int32_t out_fmt;          /* enum rsa_plane_fmt of out_hi / out_lo */
  const float* x_f32;       /* f32 [N][C/4][H][W][4] */
  const float* stats;       /* [N][groups][2] from rsa_group_norm_stats */
  const float* gamma;       /* [C] */
  const float* beta;        /* [C] */
  const float* skip_f32;    /* f32 map like x, or NULL */
  void* out_hi;             /* planes [N][C/8][H][W][8], or NULL */
  void* out_lo;             /* may be NULL */
  int64_t out_plane_stride; /* 16-byte units */
  int64_t out_batch_stride;
  float* out_f32;           /* may be NULL; may not alias x_f32 / skip_f32 of other pixels (same pixel is fine) */
  int32_t reserved0;        /* must be 0 */
  int32_t reserved1;
} rsa_group_norm_apply_params;
int rsa_group_norm_apply(const rsa_group_norm_apply_params* p, void* stream);

/* Element-wise attention gate (EA.forward, rplksr.py:40-49, plksr.py:247-256): out = x * sigmoid(g), g = the f32 output (bias included) of
 * EA's 3x3 convolution of x, x read from split planes (hi + lo), out written as split planes.  A streaming kernel rather than an epilogue of
 * rsa_conv2d: every compiled convolution schedule keeps its code unchanged.  C a multiple of 8. */
typedef struct rsa_ea_gate_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;
  const float* g_f32;       /* f32 [N][C/4][H][W][4] */
  const void* x_hi;
  const void* x_lo;         /* may be NULL */
  int64_t x_plane_stride;   /* 16-byte units */
  int64_t x_batch_stride;
  void* out_hi;
  void* out_lo;             /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  int32_t fmt;              /* enum rsa_plane_fmt of x and out */
  int32_t reserved0;        /* must be 0 */
} rsa_ea_gate_params;
int rsa_ea_gate(const rsa_ea_gate_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- Real-CUGAN ops
 * (reference archs/cugan/arch.py; resselt_amd/csrc/cugan.hip)
 *
 * The U-Nets of Real-CUGAN crop their maps (valid 3x3 convolutions, F.pad with negative pads).  The engine keeps each U-Net stage on one
 * "grid" (a plane buffer of fixed size) and every tensor of the reference as a WINDOW of a grid: origin (y0, x0) and size (h, w) in pixels.
 * The 3x3 convolutions run as zero-padded rsa_conv2d on the whole grid; the kernels below take windows for their operands. */

/* Transposed convolution (nn.ConvTranspose2d, weights [cin][cout][k][k]; arch.py:126, 130, 181, 185, 213-214) and, through
 * rsa_conv_s2, the stride-2 2x2 convolution (nn.Conv2d(c, c, 2, 2, 0), arch.py:124, 204-206).  Both are implicit GEMMs on
 * v_mfma_f32_16x16x32_{bf16,f16} over phases: rsa_deconv splits the output into stride x stride phases, each a dense convolution of the
 * input with ceil((k - r) / stride) taps per axis (r = the phase's index in o + pad); rsa_conv_s2 has one phase of 2 x 2 taps that reads
 * the pixel pairs (2i, 2i+1) counted from the input window's origin, whatever its parity.
 *   input   window (in_y0, in_x0, in_h, in_w) of planes with row length in_W; pixels outside the window read as zero
 *   output  rsa_deconv: out_h = (in_h - 1) * stride - 2 pad + ksize (likewise out_w); rsa_conv_s2: out_h = in_h / 2 (floor)
 *           written at (out_y0 + y, out_x0 + x) of a grid with row length out_W: split planes (out_hi, optional out_lo) and / or an f32 map
 *           out_f32 [N][ceil(cout/4)][out_H][out_W][4] of the same grid; channels past cout are written as zero
 *   epilogue v = acc + bias[c]; act (RSA_ACT_NONE, RSA_ACT_LRELU with slope act_param, or for rsa_deconv RSA_ACT_GELU); + the residual window (res_hi / res_lo at
 *           (res_y0 + y, res_x0 + x), row length res_W) when res_hi != NULL
 *   w_packed rsa_resample_packed_weight_bytes bytes: [phase][K step][cout tile][hi|lo][lane 64][8]; see resselt_amd/engine/cugan.py.
 * fmt RSA_PF_BF16 with products == 3 or RSA_PF_F16 with products == 1, like rsa_plk_conv.  cin_planes <= 32, cout <= 128. */
typedef struct rsa_resample_conv_params {
  int32_t batch;
  int32_t ksize, stride, pad; /* rsa_deconv: (2, 2, 0), (4, 2, 3), (5, 3, 2) or any k <= 6, stride <= 3, pad < k; rsa_conv_s2: (2, 2, 0) */
  int32_t cin_planes;
  int32_t cout;
  int32_t products;
  int32_t fmt;              /* enum rsa_plane_fmt of every plane operand and of w_packed */
  const void* in_hi;
  const void* in_lo;        /* products == 3 only */
  int64_t in_plane_stride;  /* 16-byte units */
  int64_t in_batch_stride;
  int32_t in_W;             /* row length of the input grid */
  int32_t in_y0, in_x0, in_h, in_w;
  int32_t act;              /* RSA_ACT_NONE or RSA_ACT_LRELU; rsa_deconv also RSA_ACT_GELU (erf GELU, FDAT's x4 transpose+conv head) */
  float act_param;
  int32_t reserved0;        /* must be 0 */
  const void* w_packed;
  const float* bias;        /* f32[16 * ceil(cout / 16)] */
  const void* res_hi;       /* residual planes (cout % 8 == 0 not required: channels past cout are ignored), or NULL */
  const void* res_lo;       /* may be NULL */
  int64_t res_plane_stride;
  int64_t res_batch_stride;
  int32_t res_W, res_y0, res_x0;
  int32_t out_H, out_W, out_y0, out_x0;
  void* out_hi;             /* may be NULL when out_f32 is given */
  void* out_lo;             /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  float* out_f32;           /* may be NULL */
  int32_t reserved1;        /* must be 0 */
} rsa_resample_conv_params;
int64_t rsa_resample_packed_weight_bytes(int32_t ksize, int32_t stride, int32_t transposed, int32_t cin_planes, int32_t cout, int32_t products);
int rsa_deconv(const rsa_resample_conv_params* p, void* stream);
int rsa_conv_s2(const rsa_resample_conv_params* p, void* stream);

/* Squeeze-excitation over a window (SEBlock.forward, arch.py:58-69, bias=True, reduction 8), applied IN PLACE to that window:
 *   m[n][c] = mean of x over the window;  g = sigmoid(W2 . relu(W1 . m + b1) + b2);  x[window] *= g.
 * The same math as rsa_channel_gate with relu = 1, but the mean covers a window of a larger map and the gate is applied.  Three kernels:
 * per-row-chunk channel sums into `workspace` (rsa_region_se_workspace_bytes), one workgroup per image for the ordered f64 reduction and the
 * two 1x1 convolutions (gate f32[batch][C]), and the in-place scale of the window.  Deterministic.  C = 8 * planes <= 256, hidden <= 64. */
typedef struct rsa_region_se_params {
  int32_t batch;
  int32_t planes;
  int32_t hidden;
  int32_t fmt;              /* enum rsa_plane_fmt of x */
  void* x_hi;
  void* x_lo;               /* may be NULL */
  int64_t x_plane_stride;   /* 16-byte units */
  int64_t x_batch_stride;
  int32_t W;                /* row length of the grid */
  int32_t y0, x0, h, w;     /* the window */
  int32_t reserved0;        /* must be 0 */
  const float* w1;          /* [hidden][C] */
  const float* b1;          /* [hidden] */
  const float* w2;          /* [C][hidden] */
  const float* b2;          /* [C] */
  float* workspace;
  float* gate;              /* [batch][C] */
} rsa_region_se_params;
int64_t rsa_region_se_workspace_bytes(int32_t batch, int32_t h, int32_t planes);
int rsa_region_se(const rsa_region_se_params* p, void* stream);

/* Input stage of Real-CUGAN (UpCunet*.forward, arch.py:300-306, 342-349, 386-394, 426-431): an image [N][C][h][w] of `dtype` (or RSA_U8
 * [N][h][w][C], v = byte / 255) -> v * in_scale + in_shift (the `pro` affine x * 0.7 + 0.15, or 1 / 0) -> reflect pad (pad_top, pad_left; the
 * padded map is unshuffle * out_H x unshuffle * out_W, every pad < h resp. w) -> pixel_unshuffle(unshuffle) -> split planes of the
 * out_H x out_W grid (C * unshuffle^2 channels, tail channels zero). */
typedef struct rsa_cugan_input_params {
  const void* x;
  int32_t dtype;
  int32_t batch, C, h, w;
  int32_t pad_top, pad_left;
  int32_t unshuffle;        /* 1 or 2 */
  float in_scale, in_shift;
  int32_t out_H, out_W;
  int32_t fmt;              /* enum rsa_plane_fmt of out */
  void* out_hi;
  void* out_lo;             /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
  int32_t reserved0;        /* must be 0 */
} rsa_cugan_input_params;
int rsa_cugan_input(const rsa_cugan_input_params* p, void* stream);

/* Output stage of Real-CUGAN (arch.py:307-315, 350-358, 395-410, 432-442): from an f32 map [N][ceil(C r^2 / 4)][map_H][map_W][4], with r
 * = pixel_shuffle, the output pixel (c, Y, X), Y < out_h, X < out_w, is
 *   v = map[c r^2 + (Y % r) r + X % r][y0 + Y / r][x0 + X / r]   (the final crop and nn.PixelShuffle(r))
 *   v += base[c][Y / base_div][X / base_div] * base_scale + base_shift   when base != NULL (F.interpolate(x00, nearest) of the input image,
 *        of dtype `dtype`; for RSA_U8 an [N][h][w][C] image read as byte / 255)
 *   v = (v - out_shift) / out_div                                        (the `pro` inverse; 0 and 1 otherwise)
 * stored as `dtype` [N][C][out_h][out_w] or, for RSA_U8, [N][out_h][out_w][C] = round-half-even(clamp(v, 0, 1) * 255). */
typedef struct rsa_cugan_output_params {
  const float* map;
  int32_t batch, C;
  int32_t map_H, map_W, y0, x0;
  int32_t pixel_shuffle;    /* 1 or 2 */
  int32_t out_h, out_w;
  int32_t dtype;            /* of out and of base */
  void* out;
  const void* base;         /* may be NULL */
  int32_t base_h, base_w, base_div;
  float base_scale, base_shift;
  float out_shift, out_div;
  int32_t reserved0;        /* must be 0 */
} rsa_cugan_output_params;
int rsa_cugan_output(const rsa_cugan_output_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- MoSR ops
 * (reference archs/mosr/arch.py and archs/mosrv2/arch.py; resselt_amd/csrc/mosr.hip) */

/* The middle step of the MoSR / MoSRv2 gated block (mosr/arch.py:99-105, mosrv2/arch.py:174-210, 272-278):
 *   out = mish(g) * cat(x[0 : i_planes), seg_0(x), seg_1(x), ...)
 * on split planes.  Output plane p multiplies plane p of g with plane p of the concatenation; the concatenation's planes are read from x in
 * the same order (passthrough planes first, then each segment's planes), so out, g and x each have i_planes + sum(seg[s].planes) planes.
 * A segment is a depthwise convolution of its own planes, zero padding (kh/2, kw/2) as nn.Conv2d(..., groups=C): 1 x 1 = identity (no
 * weights; weight / bias ignored), k x k for k in {3, 5, 7, 9, 11}, and the bands 1 x k and k x 1 for the same k.  Any other shape:
 * RSA_E_UNSUPPORTED.  weight f32 [planes*8][kh*kw] (row-major taps), bias f32 [planes*8].  fmt: enum rsa_plane_fmt of every plane operand. */
typedef struct rsa_gated_dwconv_segment {
  int32_t planes;            /* 8 channels each, >= 1 */
  int32_t kh, kw;
  int32_t reserved0;         /* must be 0 */
  const float* weight;
  const float* bias;
} rsa_gated_dwconv_segment;

typedef struct rsa_gated_dwconv_params {
  int32_t batch;
  int32_t H, W;
  int32_t fmt;
  int32_t i_planes;          /* passthrough planes, >= 0 */
  int32_t n_segments;        /* 0..4 */
  rsa_gated_dwconv_segment seg[4];
  const void* g_hi;
  const void* g_lo;          /* may be NULL */
  int64_t g_plane_stride;    /* 16-byte units */
  int64_t g_batch_stride;
  const void* x_hi;
  const void* x_lo;          /* may be NULL */
  int64_t x_plane_stride;
  int64_t x_batch_stride;
  void* out_hi;
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_gated_dwconv_params;
int rsa_gated_dwconv(const rsa_gated_dwconv_params* p, void* stream);

/* The image shortcut of MoSRv2 (mosrv2/arch.py:297, 328-337):  out[n][c][Y][X] += bilinear(xp, scale)[n][c][Y][X]  (align_corners=False)
 * for Y < out_h, X < out_w, where xp is the input x [N][C][h][w] reflect-padded at the bottom / right to pad_h x pad_w (pad_h < 2h,
 * pad_w < 2w; the pad is applied on the fly) and bilinear samples xp at ((Y + 0.5) / scale - 0.5, (X + 0.5) / scale - 0.5), clamped to
 * [0, pad - 1].  out is [N][C][out_H][out_W] with out_h <= out_H, out_w <= out_W; x and out share `dtype` (RSA_F32 / RSA_F16 / RSA_BF16). */
typedef struct rsa_bilinear_add_params {
  int32_t batch, C;
  int32_t h, w;              /* input */
  int32_t pad_h, pad_w;      /* reflect-padded input size */
  int32_t scale;             /* 1..8 */
  int32_t dtype;
  int32_t out_H, out_W;      /* output tensor */
  int32_t out_h, out_w;      /* region written */
  const void* x;
  void* out;
} rsa_bilinear_add_params;
int rsa_bilinear_add(const rsa_bilinear_add_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- RGT ops
 * (reference archs/rgt/arch.py, RG_SA :500-544 and Block :608-619; resselt_amd/csrc/rgt.hip) */

/* Cross-attention of every token of a full-resolution map against a small per-image key / value set (RG_SA :534-542):
 *   out[n][head][i] = softmax_j( q[n][head][i] . k[n][head][j] ) v[n][head][j]     over ALL j < nkeys, no mask, no bias
 * The scale is folded into the q weights by the host.  Maps use the head-padded layout: head h owns planes [4h, 4h+4) (32 channels) of
 * q, k, v and out; channels past dim_qk (q, k) and dim_v (v) must be zero.  Key / value token j is unit j of its planes (a row-major
 * h' x w' map).  products 3: bf16 hi+lo, three products per contraction; products 1: hi only, fmt = RSA_PF_BF16 or RSA_PF_F16 (the
 * one-product fp16 form, v_mfma_f32_32x32x16_f16, probabilities rounded to fp16).  q, k, v and out share the format. */
#define RSA_RG_MAX_KEYS 3969 /* 63 x 63: the eval recursion count of RG_SA keeps H / 4^t and W / 4^t below 64 */
typedef struct rsa_rg_attn_params {
  int32_t batch;
  int32_t H, W;              /* query / output map */
  int32_t heads;
  int32_t nkeys;             /* 1..RSA_RG_MAX_KEYS tokens per image */
  int32_t dim_qk, dim_v;     /* per-head widths, 1..32 (RSA_E_UNSUPPORTED otherwise) */
  int32_t products;          /* 1 or 3 */
  int32_t fmt;               /* enum rsa_plane_fmt */
  int32_t reserved0;         /* must be 0 */
  const void* q_hi;
  const void* q_lo;          /* NULL allowed with products == 1 (also k_lo, v_lo) */
  int64_t q_plane_stride;    /* 16-byte units, >= H*W */
  int64_t q_batch_stride;
  const void* k_hi;
  const void* k_lo;
  int64_t k_plane_stride;    /* >= nkeys */
  int64_t k_batch_stride;
  const void* v_hi;
  const void* v_lo;
  int64_t v_plane_stride;    /* >= nkeys */
  int64_t v_batch_stride;
  void* out_hi;
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;  /* >= H*W */
  int64_t out_batch_stride;
} rsa_rg_attn_params;
int rsa_rg_attention(const rsa_rg_attn_params* p, void* stream);

/* RG_SA's recursion (:512-523): the depthwise 4x4 stride-4 convolution `reduction1` (weights and bias) applied `times` times, each step
 * with its own bias as in the reference, in one launch.  The output is (H >> 2t) x (W >> 2t): every step floors, so rows / columns past
 * 4^t * (H >> 2t) are never read.  weight f32 [planes*8][16] (row-major taps), bias f32 [planes*8].  Input and output planes share fmt;
 * lo pointers may be NULL.  RSA_E_ARG when the map reduces to nothing. */
typedef struct rsa_rg_reduce_params {
  int32_t batch;
  int32_t H, W;              /* input map */
  int32_t planes;            /* 8 channels each */
  int32_t times;             /* 1..6 */
  int32_t fmt;               /* enum rsa_plane_fmt */
  const void* in_hi;
  const void* in_lo;
  int64_t in_plane_stride;
  int64_t in_batch_stride;
  const float* weight;
  const float* bias;
  void* out_hi;
  void* out_lo;
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_rg_reduce_params;
int rsa_rg_reduce(const rsa_rg_reduce_params* p, void* stream);

/* GELU(LayerNorm(x)) over the C channels of an f32 NCHW4c map into split planes (RG_SA's norm_act, :494).  Same descriptor as
 * rsa_layernorm; out_hi is required, out_f32 must be NULL.  One thread per pixel: meant for the pooled map of RG_SA. */
int rsa_layernorm_gelu(const rsa_layernorm_params* p, void* stream);

/* out += gamma[c] * res over f32 NCHW4c maps [N][ceil(C/4)][H][W][4] (the HAI term of RGT's Block, :619).  gamma f32[round_up(C, 4)],
 * zero-padded; all pointers 16-byte aligned. */
int rsa_scale_add(const float* res, const float* gamma, float* out, int32_t batch, int32_t H, int32_t W, int32_t C, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- FDAT ops
 * (reference archs/fdat/arch.py, SimplifiedAIM :521-548, SimplifiedDATBlock :574-607, LDA_AQU :135-279, PA :282-288; csrc/fdat.hip) */

/* The AIM interaction of an FDAT block, the residual add and norm2, in one pass over the C-wide stream:
 *   mode 0 (spatial block):  f = a * cm[n][ch] + c                       (channel_modulates_spatial, cm = the channel gate of c)
 *   mode 1 (channel block):  f = a + c * sigmoid(sum_ch w[ch] * a[ch])   (spatial_modulates_channel)
 *   x_out = x + f  (f32 NCHW4c; x_out may equal x);  out = LayerNorm(x + f) with gamma, beta, eps (centred form) as split planes.
 * a (the attention's proj output) and c (GELU(dwconv(n1))) are split planes [N][ceil(C/8)][H][W][8] of format fmt; lo pointers may be
 * NULL.  out_hi NULL: only x_out is written.  x NULL (out_hi NULL too): x_out = f, the interaction alone -- the unfused path's first
 * pass, followed by rsa_scale_add (x += f) and rsa_layernorm.  Tail channels of out are written as zero.
 * C 1..256.  A pixel's channels belong to one workgroup (mode 1's dot product needs all of them before the gate). */
typedef struct rsa_fdat_interact_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                 /* 1..256 */
  int32_t mode;              /* 0 or 1 */
  int32_t fmt;               /* enum rsa_plane_fmt of a, c and out */
  const void* a_hi;
  const void* a_lo;
  int64_t a_plane_stride;    /* 16-byte units, >= H*W */
  int64_t a_batch_stride;
  const void* c_hi;
  const void* c_lo;
  int64_t c_plane_stride;
  int64_t c_batch_stride;
  const float* cm;           /* mode 0: [batch][8 * ceil(C/8)] (the layout of rsa_channel_gate's gate) */
  const float* w;            /* mode 1: [C] */
  const float* x;            /* f32 NCHW4c [N][ceil(C/4)][H][W][4]; NULL: x_out = f */
  float* x_out;              /* may equal x */
  const float* gamma;        /* [C], with out_hi */
  const float* beta;
  float eps;
  int32_t reserved0;         /* must be 0 */
  void* out_hi;              /* may be NULL */
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_fdat_interact_params;
int rsa_fdat_interact(const rsa_fdat_interact_params* p, void* stream);

/* PA of FDAT's pa_up head followed by its LeakyReLU:  out = lrelu(x * sigmoid(logit), slope), unit by unit over `planes` planes.
 * logit is the 1x1 convolution PA.conv (bias included) written as planes.  x, logit and out share strides and the plane format; lo
 * pointers may be NULL; out may equal x. */
int rsa_pa_gate(const void* x_hi, const void* x_lo, const void* logit_hi, const void* logit_lo, int64_t plane_stride, int64_t batch_stride,
                int32_t batch, int32_t H, int32_t W, int32_t planes, float slope, int32_t fmt, void* out_hi, void* out_lo, void* stream);

/* LDA_AQU (reference :135-279) at the output resolution Hout x Wout, in two kernels around one rsa_conv2d:
 *   rsa_lda_offsets    per output pixel: q_hr = bilinear(q, align_corners=True) of the H x W map q (`hidden` channels), its depthwise
 *                      3x3 (zero padding at Hout x Wout, no bias; weight [gc][9] shared by the groups), LayerNorm over each group's gc =
 *                      hidden / groups channels (gamma, beta [gc], eps) and SiLU, as split planes of `hidden` channels
 *   (rsa_conv2d)       the offset convolution gc -> 2 * 9 per group as one 3x3 launch with block-diagonal weights, into an f32 map
 *   rsa_lda_attention  per output pixel and group g: nine sample points (i, j) + tanh(o) * range + base (channel order (kh kw d), d = 0
 *                      = y), mapped to the H x W maps as the reference does: y_lr = (i + dy) * (H - 1) / (Hout - 1), likewise x; bilinear
 *                      gathers with zeros outside of group g's channels of k (+ rpb[tap][ch]) and of v; scores scale * q_hr . k summed over
 *                      ALL groups (one head), a softmax over the nine taps, and out[g * C/groups + c] = sum_tap p_tap * v_g,tap[c].
 * groups must be 2; hidden 2..64 and even; C (v and out channels) a multiple of 16 up to 256; Hout, Wout >= 2. */
typedef struct rsa_lda_offsets_params {
  int32_t batch;
  int32_t H, W;              /* q map */
  int32_t Hout, Wout;
  int32_t hidden;
  int32_t groups;            /* 2 */
  int32_t fmt;               /* enum rsa_plane_fmt of q and out */
  const void* q_hi;
  const void* q_lo;          /* may be NULL */
  int64_t q_plane_stride;
  int64_t q_batch_stride;
  const float* dw_weight;    /* [hidden / groups][9] */
  const float* gamma;        /* [hidden / groups] */
  const float* beta;
  float eps;
  int32_t reserved0;         /* must be 0 */
  void* out_hi;              /* Hout x Wout planes of `hidden` channels */
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_lda_offsets_params;
int rsa_lda_offsets(const rsa_lda_offsets_params* p, void* stream);

typedef struct rsa_lda_attn_params {
  int32_t batch;
  int32_t H, W;              /* q, k, v maps */
  int32_t Hout, Wout;
  int32_t hidden;            /* q / k channels */
  int32_t C;                 /* v / out channels */
  int32_t groups;            /* 2 */
  int32_t fmt;               /* enum rsa_plane_fmt of q, k, v and out */
  float range;               /* offset range factor (11) */
  float scale;               /* hidden ** -0.5 */
  int32_t reserved0;         /* must be 0 */
  const void* q_hi;
  const void* q_lo;
  int64_t q_plane_stride;
  int64_t q_batch_stride;
  const void* k_hi;
  const void* k_lo;
  int64_t k_plane_stride;
  int64_t k_batch_stride;
  const void* v_hi;
  const void* v_lo;
  int64_t v_plane_stride;
  int64_t v_batch_stride;
  const float* offset;       /* f32 NCHW4c [N][ceil(18 * groups / 4)][Hout][Wout][4]: group g = channels [18 g, 18 g + 18) */
  const float* rpb;          /* [9][hidden] relative_position_bias_table */
  void* out_hi;              /* Hout x Wout planes of C channels */
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_lda_attn_params;
int rsa_lda_attention(const rsa_lda_attn_params* p, void* stream);

/* ---- OmniSR (csrc/omnisr.hip; reference resselt/archs/omni/arch.py) ----
 * Heads sit on whole 8-channel planes: head h of a width-d head owns planes [h*hp, h*hp + hp), hp = ceil(d / 8), its channels >= d are zero.
 * The qkv planes hold q at planes [0, heads*hp), k at [heads*hp, 2*heads*hp) and v at [2*heads*hp, 3*heads*hp).  H and W are the padded
 * map, multiples of ws.  Token sets:
 *   block (grid = 0): window (wy, wx) holds pixels (wy*ws + r, wx*ws + c), r, c < ws                          (:824, :521-596)
 *   grid  (grid = 1): rsa_omni_window_attention: window (wy, wx) holds pixels (r*H/ws + wy, c*W/ws + wx)       (:842)
 *                     rsa_omni_channel_attention: residue class (r0, c0) holds pixels (i*ws + r0, j*ws + c0)   (:742-799)
 * rsa_omni_window_attention: out = softmax(q k^T + B[rel(i, j)][h]) v per window and head (q pre-scaled by the host); bias_table is
 *   nn.Embedding((2ws-1)^2, heads).weight or NULL; ws in 2..8, head_dim <= 32, heads <= 8.
 * rsa_omni_channel_attention: per token set and head, A = softmax_row(T[h] * q^ k^T) over the d channels with q^, k^ the L2-normalised
 *   (eps 1e-12) channel rows over the set, out = A v.  Window mode with ws^2 <= 64: one launch, everything in LDS, no workspace (may
 *   be NULL).  Otherwise three kernels, no atomics: partial Gram matrices and squared norms per 64-token chunk into `workspace`, one
 *   ordered finish per (image, set, head), then the apply pass.  ws >= 1, head_dim <= 32, heads <= 8. */
typedef struct rsa_omni_attn_params {
  int32_t batch;
  int32_t H, W;
  int32_t ws;
  int32_t heads;
  int32_t head_dim;
  int32_t grid;              /* 0 = block token sets, 1 = grid token sets (see above) */
  int32_t fmt;               /* enum rsa_plane_fmt of the qkv and out planes */
  const void* qkv_hi;
  const void* qkv_lo;        /* may be NULL */
  int64_t qkv_plane_stride;
  int64_t qkv_batch_stride;
  const float* bias_table;   /* window attention: optional [(2ws-1)^2][heads]; channel attention: must be NULL */
  const float* temperature;  /* channel attention: [heads]; window attention: must be NULL */
  float* workspace;          /* channel attention: rsa_omni_channel_attn_workspace_bytes() (0 in the one-launch window mode); window attention: must be NULL */
  void* out_hi;              /* heads*hp planes */
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_omni_attn_params;
int rsa_omni_window_attention(const rsa_omni_attn_params* p, void* stream);
int64_t rsa_omni_channel_attn_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t ws, int32_t heads, int32_t head_dim, int32_t grid);
int rsa_omni_channel_attention(const rsa_omni_attn_params* p, void* stream);

/* Gated_Conv_FeedForward's middle (:436-439): out = GELU(dw3x3(x1)) * dw3x3(x2), zero padding 1, no bias, exact (erf) GELU.  x1 is planes
 * [0, planes) and x2 planes [planes, 2*planes) of the input; weight [2*planes*8][9] in the same channel order. */
typedef struct rsa_gelu_gate_dwconv_params {
  int32_t batch;
  int32_t H, W;
  int32_t planes;            /* output planes */
  int32_t fmt;               /* enum rsa_plane_fmt of every plane operand */
  int32_t reserved0;         /* must be 0 */
  const void* in_hi;
  const void* in_lo;         /* may be NULL */
  int64_t in_plane_stride;
  int64_t in_batch_stride;
  const float* weight;
  void* out_hi;
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_gelu_gate_dwconv_params;
int rsa_gelu_gate_dwconv(const rsa_gelu_gate_dwconv_params* p, void* stream);

/* MBConv's squeeze-excitation applied (:460): out[b][c][p] = in[b][c][p] * gate[b][c] with gate [batch][8*planes] from rsa_channel_gate
 * (relu = 3); in place allowed (out = in). */
int rsa_omni_gate_scale(const void* in_hi, const void* in_lo, int64_t plane_stride, int64_t batch_stride, int32_t batch, int32_t H, int32_t W,
                        int32_t planes, const float* gate, int32_t fmt, void* out_hi, void* out_lo, void* stream);

/* ESA (:18-46) on f32 NCHW4c maps [N][ceil(C/4)][H][W][4]:
 *   rsa_esa_conv3x3   3x3 convolution with bias, stride 1 or 2, zero padding 0 or 1 (conv2: stride 2 pad 0; conv3: stride 1 pad 1);
 *                     Hout = (H + 2 pad - 3) / stride + 1; cin, cout <= 64
 *   rsa_esa_maxpool   max_pool2d(7, stride 3): Hout = (H - 7) / 3 + 1 (H, W >= 7)
 *   rsa_esa_apply     out = x * sigmoid(W4 (bilinear(c3) + Wf c1 + bf) + b4), bilinear with align_corners = False from Hc x Wc to H x W;
 *                     out (f32 map, may be x) and optionally split planes of out; f <= 32, C <= 128 */
typedef struct rsa_esa_conv_params {
  int32_t batch;
  int32_t H, W;
  int32_t Hout, Wout;
  int32_t cin, cout;
  int32_t stride, pad;
  int32_t reserved0;         /* must be 0 */
  const float* in;
  const float* weight;       /* [cout][cin][3][3] */
  const float* bias;         /* [cout] */
  float* out;
} rsa_esa_conv_params;
int rsa_esa_conv3x3(const rsa_esa_conv_params* p, void* stream);
int rsa_esa_maxpool(const float* in, int32_t batch, int32_t C, int32_t H, int32_t W, float* out, void* stream);

typedef struct rsa_esa_apply_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                 /* channels of x */
  int32_t f;                 /* ESA channels */
  int32_t Hc, Wc;            /* c3 map */
  int32_t fmt;               /* enum rsa_plane_fmt of out_hi / out_lo */
  const float* x;            /* f32 map, C channels */
  const float* c1;           /* f32 map, f channels, H x W (conv1's output) */
  const float* c3;           /* f32 map, f channels, Hc x Wc */
  const float* wf;           /* [f][f] conv_f */
  const float* bf;           /* [f] */
  const float* w4;           /* [C][f] conv4 */
  const float* b4;           /* [C] */
  float* out;                /* f32 map, C channels (may equal x) */
  void* out_hi;              /* optional split planes of out */
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_esa_apply_params;
int rsa_esa_apply(const rsa_esa_apply_params* p, void* stream);

/* ---- ATD (csrc/atd.hip; reference resselt/archs/atd/arch.py) ----
 * Tokens are the pixels of the padded H x W map, token index = y*W + x.  The similarity path (wq, wk, L2 normalisation, logits, softmax,
 * argmax) is f32 whatever `products` says.  Nothing here uses atomics whose order could change a result: every reduction has a fixed order.
 *
 * rsa_atd_dict      per image, from the dictionary td [batch][m][C] (f32): kn[batch][m][16] = normalize(wk td + bk) (eps 1e-12, columns >= rc
 *                   zero) and V^T = (wv td + bv)^T as bf16 hi / lo [batch][32*ceil(C/32)][128] (rows >= C and columns >= m zero).    (:236-241)
 * rsa_atd_ca        per pixel: q = normalize(wq xn + bq); sim = softmax_m(q . kn * scale[m]); id = first maximum of sim; out = sim V
 *                   (v_mfma_f32_32x32x16_bf16, three products or one) as an f32 NCHW4c map.  scale[m] = 1 + clamp(s, 0, 1) ln m.   (:234-249)
 * rsa_atd_sort      stable counting sort of ids [batch][n] (values < m <= 128): perm[b][pos] = token, inv[b][token] = pos, tokens of one
 *                   category in ascending token index.  Three kernels; workspace of rsa_atd_sort_workspace_bytes().                 (:304-307)
 * rsa_atd_attention softmax(scale * q k^T (+ bias) (+ mask)) v over token groups of at most 256 tokens, flash-style on
 *                   v_mfma_f32_32x32x16_bf16.  The qkv planes hold q at planes [0, heads*hp), k at [heads*hp, 2*heads*hp), v behind them;
 *                   head h owns planes [h*hp, h*hp + hp), hp = ceil(head_dim / 8), channels >= head_dim zero.
 *                     mode 0 (window, :446-472): group = a ws x ws window of the map rolled by -shift; bias_table [heads][(2ws-1)^2];
 *                       the shift mask (-100 across the regions of :1057-1082) is derived from the geometry.  H, W multiples of ws.
 *                     mode 1 (category, :297-331): group g = sorted positions [g*gs, g*gs + gs) through perm; positions >= n of the last
 *                       group are the flipped tail of the sorted sequence (keys only).  gs = min(n, category_size) <= 256.
 *                   The output of a token lands on that token's pixel in both modes.
 * rsa_atd_dwconv    out = x + GELU(dw5x5(x) + bias) on split planes (ConvFFN's middle, :81-85); weight f32 [planes*8][25].
 * rsa_atd_refine    td <- sigmoid(sigma) td + (1 - sigmoid(sigma)) softmax_n(InstanceNorm(sim^T)) x  (:483-487): column statistics in f64
 *                   partial sums, a softmax over all pixels and the weighted sum of x (f32 NCHW4c map), four kernels, fixed reduction
 *                   trees; workspace of rsa_atd_refine_workspace_bytes(). */
typedef struct rsa_atd_dict_params {
  int32_t batch;
  int32_t C;                 /* 1..256 */
  int32_t m;                 /* dictionary tokens, 1..128 */
  int32_t rc;                /* reduced width, 1..16 */
  const float* td;           /* [batch][m][C] */
  const float* wk;           /* [rc][C] */
  const float* bk;           /* [rc] or NULL */
  const float* wv;           /* [C][C] */
  const float* bv;           /* [C] or NULL */
  float* kn;                 /* [batch][m][16] */
  void* vt_hi;               /* bf16 [batch][32*ceil(C/32)][128] */
  void* vt_lo;               /* same shape */
} rsa_atd_dict_params;
int rsa_atd_dict(const rsa_atd_dict_params* p, void* stream);

typedef struct rsa_atd_ca_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                 /* 1..256 */
  int32_t m;                 /* 1..128 */
  int32_t rc;                /* 1..16 */
  int32_t products;          /* 3 or 1: bf16 products of sim V */
  int32_t reserved0;         /* must be 0 */
  const float* xn;           /* f32 NCHW4c map of norm1(x) */
  const float* wq;           /* [rc][C] */
  const float* bq;           /* [rc] or NULL */
  const float* kn;           /* rsa_atd_dict */
  const float* scale;        /* [m] */
  const void* vt_hi;
  const void* vt_lo;
  float* sim;                /* [batch][H*W][m] or NULL */
  int32_t* ids;              /* [batch][H*W] or NULL */
  float* out;                /* f32 NCHW4c map */
} rsa_atd_ca_params;
int rsa_atd_ca(const rsa_atd_ca_params* p, void* stream);

int64_t rsa_atd_sort_workspace_bytes(int32_t batch, int64_t n);
int rsa_atd_sort(const int32_t* ids, int32_t batch, int64_t n, int32_t m, int32_t* perm, int32_t* inv, void* workspace, void* stream);

typedef struct rsa_atd_attn_params {
  int32_t batch;
  int32_t H, W;
  int32_t heads;
  int32_t head_dim;          /* 1..64 */
  int32_t mode;              /* 0 = window, 1 = category */
  int32_t ws;                /* window mode: 2..16 */
  int32_t shift;             /* window mode: 0 <= shift < ws */
  int32_t gs;                /* category mode: group size, 1..256 */
  int32_t products;          /* 3 or 1 */
  float scale;               /* multiplies q k^T */
  int32_t reserved0;         /* must be 0 */
  const void* qkv_hi;
  const void* qkv_lo;        /* products == 3 */
  int64_t qkv_plane_stride;
  int64_t qkv_batch_stride;
  const float* bias_table;   /* window mode: [heads][(2ws-1)^2] or NULL */
  const int32_t* perm;       /* category mode: [batch][H*W], values < H*W */
  void* out_hi;              /* heads*hp planes */
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_atd_attn_params;
int rsa_atd_attention(const rsa_atd_attn_params* p, void* stream);

typedef struct rsa_atd_dwconv_params {
  int32_t batch;
  int32_t H, W;
  int32_t planes;
  const void* in_hi;
  const void* in_lo;         /* may be NULL */
  int64_t in_plane_stride;
  int64_t in_batch_stride;
  const float* weight;       /* [planes*8][25] */
  const float* bias;         /* [planes*8] */
  void* out_hi;
  void* out_lo;              /* may be NULL */
  int64_t out_plane_stride;
  int64_t out_batch_stride;
} rsa_atd_dwconv_params;
int rsa_atd_dwconv(const rsa_atd_dwconv_params* p, void* stream);

typedef struct rsa_atd_refine_params {
  int32_t batch;
  int32_t H, W;
  int32_t C;                 /* 1..256 */
  int32_t m;                 /* 1..128 */
  float eps;                 /* InstanceNorm1d eps */
  const float* sim;          /* [batch][H*W][m] */
  const float* x;            /* f32 NCHW4c map (the layer's output) */
  const float* gamma;        /* norm3.weight [m] */
  const float* beta;         /* norm3.bias [m] */
  const float* sigma;        /* [m], before the sigmoid */
  float* td;                 /* [batch][m][C], updated in place */
  void* workspace;
} rsa_atd_refine_params;
int64_t rsa_atd_refine_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t C, int32_t m);
int rsa_atd_refine(const rsa_atd_refine_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- RCAN ops
 * (reference archs/rcan/arch.py, CALayer :148-164, RCAB :168-196, RCAN.forward :320-332; csrc/rcan.hip) */

/* The tail of a residual channel attention block: out = x + gate[n][c] * y on split planes of format fmt, two kernels on `stream`.
 *   1. pool_sums != NULL: one workgroup per image adds the `slots` partial sums per channel that the block's second convolution left
 *      (rsa_conv_params.pool_sums, f32 [batch][slots][16 * ceil(C / 16)]) in f64 in a fixed order (strided partials in ascending slot
 *      order, then the partials in order: the same bits on every run), divides by H * W and writes
 *      gate[n][c] = sigmoid(W2 . relu(W1 . mean + b1) + b2), f32 [batch][C] (the matrix products in f64 too).
 *      pool_sums == NULL: `gate` is an input (for instance from rsa_channel_gate with relu = 1), w1 .. b2 are not read.
 *   2. one pass over the map: reads y (the convolution's planes) and x (the block's input), writes the planes the next convolution reads;
 *      out may be x or y.  Every lo pointer may be NULL (the value is then hi alone / lo is not written).
 * w1 [hidden][C], b1 [hidden], w2 [C][hidden], b2 [C], f32.  C % 8 == 0, C <= 512, hidden 1..128; strides in 16-byte units; plane pointers
 * 16-byte aligned; H, W arbitrary. */
int rsa_rcab_tail(const float* pool_sums, int32_t slots, const float* w1, const float* b1, const float* w2, const float* b2, int32_t hidden,
                  float* gate, const void* y_hi, const void* y_lo, int64_t y_plane_stride, int64_t y_batch_stride, const void* x_hi,
                  const void* x_lo, int64_t x_plane_stride, int64_t x_batch_stride, void* out_hi, void* out_lo, int64_t out_plane_stride,
                  int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t fmt, void* stream);

/* RCAN's input stage (forward :323-324): out[n][o][p] = bias[o] + sum_c weight[o][c] * (x[n][c][p] * scale), f32 [N][C][H][W], C <= 4 -- the
 * `x * rgb_range` and the sub_mean 1x1 convolution as one pointwise step.  x is [N][C][H][W] of `dtype`, or RSA_U8 [N][H][W][C] (v = byte / 255).
 * weight f32 [C][C], bias f32 [C]. */
int rsa_rcan_input(const void* x, int32_t dtype, int32_t batch, int32_t C, int32_t H, int32_t W, float scale, const float* weight,
                   const float* bias, float* out, void* stream);

/* 8-bit images either side of the path (the reference leaves both steps to its callers):
 *   rsa_image_u8_to_nchw   uint8 [N][H][W][C] (interleaved, as image decoders deliver it) -> float [N][C][H][W], v / 255
 *   rsa_nchw_to_image_u8   float [N][C][H][W] -> uint8 [N][H][W][C], round-half-even(clamp(v, 0, 1) * 255)  (torch: (y.clamp(0,1)*255).round())
 * dtype = rsa_dtype of the float tensor. */
int rsa_image_u8_to_nchw(const uint8_t* img, int32_t batch, int32_t H, int32_t W, int32_t C, void* out, int32_t dtype, void* stream);
int rsa_nchw_to_image_u8(const void* x, int32_t dtype, int32_t batch, int32_t C, int32_t H, int32_t W, uint8_t* img, void* stream);

/* ---- GateR (reference archs/gater/arch.py) ----
 * nn.RMSNorm over the channels of an f32 stream map [N][ceil(C/4)][H][W][4]:  out = x * rsqrt(mean_c(x^2) + eps) * weight[c], written as split
 * planes of `fmt` (out_lo may be NULL).  NOT rsa_rmsnorm, which is RTMoSR's  x / (rms + eps) * scale + offset.  A pixel of zeros gives zeros. */
int rsa_rmsnorm_torch(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, float eps, const float* weight, void* out_hi, void* out_lo,
                      int64_t out_plane_stride, int64_t out_batch_stride, int32_t fmt, void* stream);

/* PixelUnshuffle(2) of an f32 map: x_f32 [N][C/4][H][W][4] -> out_f32 [N][C][H/2][W/2][4] with output channel 4c + 2i + j at (y, x) = input
 * channel c at (2y + i, 2x + j).  A permutation (bit-exact).  H, W even, C % 4 == 0, not in place. */
int rsa_pixel_unshuffle2(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, float* out_f32, void* stream);

/* cat(a, b) over channels as one f32 map: a_nchw is a plain f32 [N][Ca][H][W] tensor (e.g. a depth-to-space store), b_map an f32 map
 * [N][Cb/4][H][W][4]; out_map [N][(Ca+Cb)/4][H][W][4].  Ca, Cb multiples of 4. */
int rsa_f32map_concat(const float* a_nchw, int32_t Ca, const float* b_map, int32_t Cb, int32_t batch, int32_t H, int32_t W, float* out_map, void* stream);

/* Focused linear attention (FLPVT2, eight heads of head_dim = C / 8 channels, head_dim 24 or 48) over the H x W tokens of each image.
 * qkv: split planes of one 3C-wide linear layer, [q | k | v] with C / 8 planes each (qkv_lo may be NULL).  For t in q, k (whole tokens,
 * before the head split):  t = (relu(t) + 1e-6) / softplus(scale[c]);  n0 = ||t||_2 over C;  t = t^factor[c];  t = t / ||t||_2 * n0.
 *   rsa_fla_reduce  per image and head:  KV = k^T v / n  and  mean_n(k)  into the first batch * (8 d d + 8 d) floats of `workspace`.
 *                   Two kernels, no atomics: partial sums per chunk of 128 consecutive tokens, added in ascending chunk order -- the
 *                   result is bit-identical from run to run and does not depend on the launch geometry.
 *   rsa_fla_apply   out = (q KV) / (q . mean(k) + 1e-6) + dwc(v): the 5x5 depthwise convolution (zero padding) whose head_dim filters
 *                   dwc_weight [d][25], dwc_bias [d] are shared by all heads (channel c uses filter c % d).  out: C / 8 split planes.
 * All arithmetic is f32.  workspace: rsa_fla_workspace_bytes(batch, H * W, head_dim) bytes, 16-byte aligned, the same for both calls. */
int64_t rsa_fla_workspace_bytes(int32_t batch, int32_t tokens, int32_t head_dim);
int rsa_fla_reduce(const void* qkv_hi, const void* qkv_lo, int64_t qkv_plane_stride, int64_t qkv_batch_stride, int32_t batch, int32_t H, int32_t W,
                   int32_t head_dim, int32_t fmt, const float* scale, const float* factor, void* workspace, int64_t workspace_bytes, void* stream);
int rsa_fla_apply(const void* qkv_hi, const void* qkv_lo, int64_t qkv_plane_stride, int64_t qkv_batch_stride, int32_t batch, int32_t H, int32_t W,
                  int32_t head_dim, int32_t fmt, const float* scale, const float* factor, const void* workspace, int64_t workspace_bytes,
                  const float* dwc_weight, const float* dwc_bias, void* out_hi, void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride,
                  void* stream);

/* ---------------------------------------------------------------------------------------------------------------- EIMN ops
 * (reference archs/eimn/arch.py, DFFM :65-92, SADFFM :38-62, MOLRCM :103-146, EIMNBlock :149-171; csrc/eimn.hip)
 * Plane operands are split planes of format fmt (every lo pointer may be NULL), strides in 16-byte units (a plane stride
 * is at least H * W and, with batch > 1, a batch stride at least the operand's planes times its plane stride), pointers 16-byte aligned. */

/* MOLRCM's depthwise chain in one launch: out = cat(spatial_1(r[a]), r[b], spatial_2(r[c])) with r = region(q): a 5x5 depthwise convolution
 * with bias and zero padding 2 on every plane, then per plane group a 5x5 with dilation 2 and padding 4 (the first planes_a planes), nothing
 * (the next planes_b) or a 7x7 with dilation 3 and padding 9 (the last planes_c), each with its bias.  The second stage zero-pads r: outside
 * the map its input is 0.  gelu_in != 0 applies the exact (erf) GELU to q as it is read (proj_query's activation; GELU(0) = 0, so the zero
 * padding is unaffected).  With P = planes_a + planes_b + planes_c, all f32 and 16-byte aligned, per half plane of four channels:
 *   w1 [2P][25][4], b1 [2P][4], w2 [2P][49][4] (row-major taps; a 5x5 uses the first 25 rows, an identity plane none), b2 [2P][4].
 * Not in place.  1 <= P <= 32767. */
int rsa_eimn_query_chain(const void* q_hi, const void* q_lo, int64_t q_plane_stride, int64_t q_batch_stride, void* out_hi, void* out_lo,
                         int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t planes_a, int32_t planes_b,
                         int32_t planes_c, int32_t gelu_in, int32_t fmt, const float* w1, const float* b1, const float* w2, const float* b2,
                         void* stream);

/* SADFFM's middle (:58-59): out = GELU(dw3x3(x1) + b1) * (dw3x3(x2) + b2), zero padding 1, exact GELU: rsa_gelu_gate_dwconv with the
 * biases of SAL.  x1 is planes [0, planes) and x2 planes [planes, 2 * planes) of the input; weight [2 * planes * 8][9] and
 * bias [2 * planes * 8] in the same channel order.  Not in place. */
int rsa_eimn_sal(const void* in_hi, const void* in_lo, int64_t in_plane_stride, int64_t in_batch_stride, void* out_hi, void* out_lo,
                 int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t planes, int32_t fmt,
                 const float* weight, const float* bias, void* stream);

/* out = silu(f) * v = f * sigmoid(f) * v over `planes` planes (:145-146); out may be f or v. */
int rsa_eimn_silu_mul(const void* f_hi, const void* f_lo, int64_t f_plane_stride, int64_t f_batch_stride, const void* v_hi, const void* v_lo,
                      int64_t v_plane_stride, int64_t v_batch_stride, void* out_hi, void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride,
                      int32_t batch, int32_t H, int32_t W, int32_t planes, int32_t fmt, void* stream);

/* DFFM behind linear_out, with the block's second residual and the stage's LayerNorm, on f32 maps [N][C/4][H][W][4]; C % 8 == 0,
 * 8 <= C <= 128, reduced width rc in 1..32.  With n = gamma * (z - mean_c z) / sqrt(var_c z + eps) + beta per pixel (channels-first LayerNorm):
 *   rsa_eimn_dffm_reduce  workspace[n][slot][c] = sum of n over the 256 pixels of the slot, slots = ceil(H * W / 256): the norm in f64, every
 *                         value rounded to f32 once and added in a fixed f32 tree of depth RSA_EIMN_DFFM_DEPTH (that rounding included).
 *                         Every entry is written; no atomics; the same bits on every run.
 *   rsa_eimn_dffm_gates   one workgroup per image, f64: mean = ordered sum of the slots / (H * W), g = GELU(wg . mean + bg) [rc],
 *                         gates[n][c] = sigmoid(wc . g + bc) for c < C and gates[n][C] = ws[rc:] . g + bs; gates is f32 [batch][C + 4].
 *   rsa_eimn_dffm_apply   per pixel: l = GELU(wl . n + bl), s = sigmoid(ws[:rc] . l + gates[n][C]),
 *                         v = x + scale[c] * z * gates[n][c] * s;  norm_gamma != NULL: v = LayerNorm_c(v) with norm_eps, norm_gamma, norm_beta;
 *                         add != NULL: v += add.  Writes v to out_f32 (may be x) and as split planes.
 * wg, wl [rc][C]; wc [C][rc]; ws [2 rc]; bs [1]; gamma, beta, scale, norm_gamma, norm_beta [C]; all f32.
 * workspace: rsa_eimn_dffm_workspace_bytes(batch, H, W, C) bytes, 16-byte aligned. */
#define RSA_EIMN_DFFM_DEPTH 10
int64_t rsa_eimn_dffm_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t C);
int rsa_eimn_dffm_reduce(const float* z, int32_t batch, int32_t H, int32_t W, int32_t C, const float* gamma, const float* beta, float eps,
                         void* workspace, int64_t workspace_bytes, void* stream);
int rsa_eimn_dffm_gates(const void* workspace, int64_t workspace_bytes, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t rc, const float* wg,
                        const float* bg, const float* wc, const float* bc, const float* ws, const float* bs, float* gates, void* stream);
int rsa_eimn_dffm_apply(const float* z, const float* x, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t rc, const float* gamma,
                        const float* beta, float eps, const float* wl, const float* bl, const float* ws, const float* gates, const float* scale,
                        const float* norm_gamma, const float* norm_beta, float norm_eps, const float* add, float* out_f32, void* out_hi,
                        void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride, int32_t fmt, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- RHA ops
 * (reference archs/rha/arch.py, FocusedLinearAttention :188-302, HybridAttention :398-415, GatedCNNBlock :418-450; csrc/rha.hip)
 * Plane operands are split planes of format fmt (every lo pointer may be NULL), strides in 16-byte units (a plane stride is at least
 * H * W and, with batch > 1, a batch stride at least the operand's planes times its plane stride), pointers 16-byte aligned.  A plane
 * operand may start at a plane offset inside a wider buffer: pass the pointer of its first plane and the wider buffer's strides. */

/* MaxPool(down) -> roll(-shift) -> FocusedLinearAttention on every window x window window -> roll(+shift) in one launch, one workgroup
 * per (image, window) of the pooled map [H / down][W / down].  x: C2 / 8 planes at FULL resolution H x W (multiples of down * window);
 * the maximum of a down x down cell is taken over hi + lo and starts from the cell's first element.  A token at window-local row r of
 * window row wy is pooled row (wy * window + r + shift) mod (H / down), likewise for columns: the roll is cyclic and there is no mask.
 * Per window, with N = window^2 tokens, 8 heads of d = C2 / 8 channels, all in f32:
 *   q | k | v = token Wqkv^T + bqkv;  k += pos;  q, k = (relu(.) + 1e-6) * inv_scale[c];  u <- u^3 / ||u^3|| * ||u|| over all C2 channels
 *   (evaluated on u / max(u), so that no intermediate leaves the f32 normal range);  per head kv = k^T v / N, z = 1 / (q . mean(k) + 1e-6);
 *   out = (q kv) z + dwc(v) (5x5 depthwise, filter c % d, zero padding at the WINDOW border);  proj.
 * out: f32 map [batch][C2 / 4][H / down][W / down][4] at the un-rolled pooled coordinates.
 * wqkv_t [C2][3 C2] and wproj_t [C2][C2] are the TRANSPOSED Linear weights (input-major), pos_t [C2][N] the transposed positional
 * encoding, inv_scale [C2] = 1 / softplus(scale), dwc_w [d][25], dwc_b [d], bqkv [3 C2], bproj [C2]; all f32.
 * C2 in {8, 16, 24, 32}, down in {1, 2, 4, 8}, window in {4, 8}, 0 <= shift < window.  rsa_rha_window_attn_lds_bytes: the dynamic LDS of
 * a workgroup, 4 * (4 C2 N + 4 C2^2 + C2 d + 6 C2 + 26 d) bytes (50,848 at C2 = 32, window 8), or RSA_E_ARG. */
int64_t rsa_rha_window_attn_lds_bytes(int32_t C2, int32_t window);
int rsa_rha_window_attn(const void* x_hi, const void* x_lo, int64_t x_plane_stride, int64_t x_batch_stride, int32_t batch, int32_t H, int32_t W,
                        int32_t C2, int32_t down, int32_t window, int32_t shift, int32_t fmt, const float* wqkv_t, const float* bqkv,
                        const float* pos_t, const float* inv_scale, const float* dwc_w, const float* dwc_b, const float* wproj_t, const float* bproj,
                        float* out, void* stream);

/* out = cat(dw5x5(x1) + bias, bilinear_up(att, down)): 2 * C2 / 8 planes.  x1: C2 / 8 planes, 5x5 depthwise with weight [C2][25], bias [C2]
 * and zero padding 2 at the image border.  att: f32 map [batch][C2 / 4][H / down][W / down][4], sampled as
 * F.interpolate(mode='bilinear', align_corners=False): src = (dst + 0.5) / down - 0.5 clamped at 0, the upper neighbour clamped to the edge;
 * down = 1 is a copy.  down in {1, 2, 4, 8}; H and W multiples of down.  Not in place. */
int rsa_rha_mix(const void* x_hi, const void* x_lo, int64_t x_plane_stride, int64_t x_batch_stride, const float* att, void* out_hi, void* out_lo,
                int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C2, int32_t down, int32_t fmt,
                const float* weight, const float* bias, void* stream);

/* out = mish(g) * cat(i, a * c) over hidden_planes planes: f holds [g | i | c] = hidden_planes + i_planes + (hidden_planes - i_planes)
 * planes, a the hidden_planes - i_planes planes that multiply c.  0 <= i_planes < hidden_planes.  Not in place. */
int rsa_rha_gate(const void* f_hi, const void* f_lo, int64_t f_plane_stride, int64_t f_batch_stride, const void* a_hi, const void* a_lo,
                 int64_t a_plane_stride, int64_t a_batch_stride, void* out_hi, void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride,
                 int32_t batch, int32_t H, int32_t W, int32_t hidden_planes, int32_t i_planes, int32_t fmt, void* stream);

/* ---------------------------------------------------------------------------------------------------------------- FlexNet ops
 * (reference archs/flexnet/arch.py, OmniShift :65-125, LMLTVIT :137-229, ChannelMix :232-263, TransformerBlock :266-281; csrc/flexnet.hip)
 * Plane operands are split planes of format fmt (every lo pointer may be NULL unless said otherwise), strides in 16-byte units (a plane
 * stride is at least H * W and, with batch > 1, a batch stride at least the operand's planes times its plane stride), pointers 16-byte
 * aligned.  A plane operand may start at a plane offset inside a wider buffer: pass the pointer of its first plane and the wider
 * buffer's strides.  f32 maps are [batch][C / 4][H][W][4]. */

/* out = dw5x5(rmsnorm(x)): y = x * (1 / sqrt(mean_c(x^2) + eps)) * norm_weight[c] over the C channels of a pixel (nn.RMSNorm), then the
 * bias-free 5x5 depthwise filter weight [C][25] over the NORMALISED map with zero padding 2 at the image border (a position outside the
 * image contributes 0).  x_f32: f32 map; out: C / 8 planes.  One launch; the normalised map never reaches memory.  A pixel of zeros
 * normalises to zeros.  C a multiple of 8, eps >= 0. */
int rsa_flex_norm_shift(const float* x_f32, int32_t batch, int32_t H, int32_t W, int32_t C, float eps, const float* norm_weight, const float* weight,
                        void* out_hi, void* out_lo, int64_t out_plane_stride, int64_t out_batch_stride, int32_t fmt, void* stream);

/* out = softmax(q k^T) v + lepe(v) on every 8 x 8 window of the map (windows anchored at the origin; H and W multiples of 8), ONE head of
 * C channels; q is expected pre-scaled.  qkv: [q | k | v] = 3 C / 8 planes; out: C / 8 planes, not the qkv buffer.  Both products run on
 * v_mfma_f32_16x16x32_{bf16,f16}: products == 3 multiplies hi and lo of q, k, v and of the probabilities (hi hi + lo hi + hi lo; qkv_lo
 * required), products == 1 the hi planes only (qkv_lo is ignored, by lepe too).  The softmax is f32 with the row maximum subtracted.
 * lepe: 3x3 depthwise convolution of v with bias and zero padding at the WINDOW border, lepe_w [9][C] (tap-major), lepe_b [C], f32.
 * C a multiple of 16 from 16 to 128; nothing is padded to 32 channels in memory.  rsa_flex_window_attn_lds_bytes: the dynamic LDS of a
 * workgroup, (products == 3 ? 2 : 1) * C * 144 bytes, or RSA_E_ARG. */
int64_t rsa_flex_window_attn_lds_bytes(int32_t C, int32_t products);
int rsa_flex_window_attn(const void* qkv_hi, const void* qkv_lo, int64_t qkv_plane_stride, int64_t qkv_batch_stride, void* out_hi, void* out_lo,
                         int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t products,
                         int32_t fmt, const float* lepe_w, const float* lepe_b, void* stream);

/* out = relu(in)^2 over hidden / 8 planes; with norm != 0 followed by k * (1 / sqrt(mean(k^2) + eps)) over the hidden channels of a pixel
 * (nn.RMSNorm without its weight).  A pixel without a positive value gives zeros.  In place is allowed (out_hi == in_hi, same strides).
 * hidden a multiple of 8. */
int rsa_flex_sqrelu(const void* in_hi, const void* in_lo, int64_t in_plane_stride, int64_t in_batch_stride, void* out_hi, void* out_lo,
                    int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t hidden, int32_t norm, float eps,
                    int32_t fmt, void* stream);

/* v = base + sigmoid(r) * kv over C channels: r and kv are C / 8 planes, base an f32 map.  v goes to the f32 map out_f32 (may be base
 * itself, may be NULL) and / or to the C / 8 planes out_hi (may be NULL; out_lo optional); at least one of the two. */
int rsa_flex_gate_add(const void* r_hi, const void* r_lo, int64_t r_plane_stride, int64_t r_batch_stride, const void* kv_hi, const void* kv_lo,
                      int64_t kv_plane_stride, int64_t kv_batch_stride, const float* base_f32, float* out_f32, void* out_hi, void* out_lo,
                      int64_t out_plane_stride, int64_t out_batch_stride, int32_t batch, int32_t H, int32_t W, int32_t C, int32_t fmt, void* stream);

/* version / errors */
int rsa_version(void);
const char* rsa_last_error_string(void);

#ifdef __cplusplus
}
#endif
#endif /* RESSELT_AMD_H */
