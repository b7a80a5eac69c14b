// gemm_kernel<float, ...> (gemm128.h): the fp32 (parity) instantiations of the 128 x 128 register-staged kernel
#include "gemm128.h"

void gemm_units::launch_gemm128_f32(const GemmP& p, bool vec, int ta, int tb, int batch, hipStream_t st) { launch128<float>(p, vec, ta, tb, batch, st); }
