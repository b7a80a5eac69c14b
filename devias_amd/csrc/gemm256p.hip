// the static-list instantiations of gemm256p_kernel (gemm256p.h): what the step runs by default
#include "gemm256p.h"

void gemm_units::launch_gemm256p(const GemmP& p, bool tb, int side, int epi, int cus, hipStream_t st) { pers_launch<false>(tb, side, epi, dim3(cus), st, p); }
