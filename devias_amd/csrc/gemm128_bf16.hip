// gemm_kernel<bf16, ...> (gemm128.h): the bf16 instantiations of the 128 x 128 register-staged kernel
#include "gemm128.h"

void gemm_units::launch_gemm128_bf16(const GemmP& p, bool vec, int ta, int tb, int batch, hipStream_t st) { launch128<bf16>(p, vec, ta, tb, batch, st); }
