// conv_inst_ringpool.hip — conv_ring<..., XRES = 7>: the one-stream shapes of the ring schedule with the channel-pooling epilogue
// (rsa_conv_params.pool_sums; conv_common.h EM 5).  The second convolution of RCAN's residual channel attention block (archs/rcan/arch.py:168-196
// of the reference): 64 -> 64 over whole chunks (SHAPE 1) and 48 -> 48 in half mode (SHAPE 3), three bf16 products or one fp16 product.
#include "conv_ring.h"

namespace rsa {
int conv_launch_pool(const rsa_conv_params& p, hipStream_t stream) {  // the caller has checked conv_pool_eligible
  const bool f16 = p.in_fmt == RSA_PF_F16;
  if (p.cout == 48) return f16 ? launch_ring<3, 0, 0, 1, RSA_PF_F16, 1, 7>(p, stream) : launch_ring<3, 0, 0, 1, RSA_PF_BF16, 3, 7>(p, stream);
  return f16 ? launch_ring<1, 0, 0, 0, RSA_PF_F16, 1, 7>(p, stream) : launch_ring<1, 0, 0, 0, RSA_PF_BF16, 3, 7>(p, stream);
}
unsigned int conv_ringpool_aborts() { return ring_aborts_this_unit(); }
#ifdef RSA_RING_DEBUG
int conv_ringpool_set_dbg(unsigned v) { return hipMemcpyToSymbol(HIP_SYMBOL(g_ring_dbg), &v, sizeof(v)) == hipSuccess ? 0 : -1; }
#endif
}  // namespace rsa
