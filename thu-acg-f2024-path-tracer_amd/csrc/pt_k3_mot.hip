// The MOT forms of K1 / K3 (unit_forms<UNIT_MOT>: motion in effect — moving instances and the shutter; plain mode, the default
// variant's shapes x LIGHTS x LIST x QMC) and of the AOV walk.
#include "pt_forms.h"
#include "pt_k_trace.h"

namespace pt {

__global__ __launch_bounds__(BLOCK) void k_aov_mot(SceneD sc, CamD cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov, uint32_t overwrite) {
    aov_pixels<false, true>(sc, cam, seed, spp_begin, spp_end, aov, overwrite);
}
__global__ __launch_bounds__(BLOCK) void k_aov_mot_qmc(SceneD sc, CamD cam, uint64_t seed, uint32_t spp_begin, uint32_t spp_end, double* aov, uint32_t overwrite) {
    aov_pixels<true, true>(sc, cam, seed, spp_begin, spp_end, aov, overwrite);
}

FormKernels forms_mot(const ShadeForm& f) { return unit_forms<UNIT_MOT>(f, f.qmc ? k_aov_mot_qmc : k_aov_mot); }

}  // namespace pt
