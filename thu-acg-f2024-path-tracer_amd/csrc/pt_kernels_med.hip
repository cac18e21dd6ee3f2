// The participating-media forms of K1 / K3 and the medium probe: pt_kernels.hip compiled once more with PT_MED_TU,
// which leaves out its non-template kernels and its launchers and adds the MED ones (the end of that file). A translation unit of
// its own, like pt_kernels_qmc.hip, so that the sixteen extra k_shade forms compile next to the existing ones, not after them.
#define PT_MED_TU 1
#include "pt_kernels.hip"
