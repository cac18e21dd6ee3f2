// The Sobol sampler's forms of K1 / K3 / the AOV kernel and the sampler probe: pt_kernels.hip compiled a second time
// with PT_QMC_TU, which leaves out its non-template kernels and its launchers and adds the QMC ones (the end of that file). A
// translation unit of its own so that the sixteen extra k_shade forms compile next to the existing ones, not after them.
#define PT_QMC_TU 1
#include "pt_kernels.hip"
