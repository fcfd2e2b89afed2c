// cuzfp_amd/csrc/region_variable_f64.hip -- double instantiations of the sub-box
// decoder of variable-rate streams.
#include "region_variable_kernels.hpp"

namespace cuzfp {
template int launch_decode_region_variable_type<double>(const Problem&, const Region&, const uint64_t*, size_t,
                                                        const uint16_t*, const uint64_t*, bool, void*, hipStream_t);
}  // namespace cuzfp
