// cuzfp_amd/csrc/region_variable_f32.hip -- float instantiations of the sub-box
// decoder of variable-rate streams, and the type-independent index builder.
#define CUZFP_VARIABLE_INDEX_UNIT 1
#include "region_variable_kernels.hpp"

namespace cuzfp {
template int launch_decode_region_variable_type<float>(const Problem&, const Region&, const uint64_t*, size_t,
                                                       const uint16_t*, const uint64_t*, bool, void*, hipStream_t);
}  // namespace cuzfp
