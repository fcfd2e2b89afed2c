// cuzfp_amd/csrc/region_variable_update_f64.hip -- double instantiations of the
// sub-box encoder of variable-rate streams.
#include "region_variable_update_kernels.hpp"

namespace cuzfp {
template int launch_encode_region_variable_type<double>(const Problem&, const Region&, const void*, bool, bool, uint32_t,
                                                    int, const uint64_t*, size_t, const uint16_t*, const uint64_t*,
                                                    uint64_t*, uint64_t, uint16_t*, uint64_t*, uint64_t*, uint64_t*,
                                                    uint64_t*, hipStream_t);
}  // namespace cuzfp
