// folded deconv + 3x3 kernels, bf16 storage (upconv_impl.h).
#include "upconv_impl.h"
extern "C" int ccvpe_upconv3x3_bf16(const ccvpe_upconv_desc* d, void* stream) { return ccvpe::upconv_run<ccvpe::bf16_t>(d, stream); }
// (the route is host arithmetic: answering for fp32 here instantiates none of its kernels)
extern "C" int ccvpe_upconv3x3_route(const ccvpe_upconv_desc* d, int is_bf16) {
  return is_bf16 ? ccvpe::upconv_route<ccvpe::bf16_t>(d) : ccvpe::upconv_route<float>(d);
}
