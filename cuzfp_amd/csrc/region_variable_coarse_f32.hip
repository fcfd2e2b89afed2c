// cuzfp_amd/csrc/region_variable_coarse_f32.hip -- float instantiations of the
// sub-box decoder of variable-rate streams at a coarser target mode.
#include "region_variable_coarse_kernels.hpp"

namespace cuzfp {
template int launch_decode_region_variable_coarse_type<float>(const Problem&, const Region&, const uint64_t*, size_t,
                                                              const uint16_t*, const uint64_t*, uint32_t, int, bool,
                                                              void*, hipStream_t);
}  // namespace cuzfp
