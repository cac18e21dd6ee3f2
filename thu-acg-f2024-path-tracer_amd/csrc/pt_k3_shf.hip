// The light-shaft forms of K3 (unit_forms<UNIT_SHF>: punctual lights and participating media in effect together, pt_scene_set_punctual_media,
// DESIGN.md §22; the modes MED and HET x the default variant's shapes x LIGHTS x LIST x QMC). K1 has none: a camera ray's bounce word is the MED forms'.
#include "pt_forms.h"

namespace pt {

FormKernels forms_shf(const ShadeForm& f) { return unit_forms<UNIT_SHF>(f, nullptr); }

}  // namespace pt
