// cuzfp_amd/csrc/region_variable_crop_f32.hip -- float instantiations of the
// crop and paste of variable-rate streams.
#include "region_variable_crop_kernels.hpp"

namespace cuzfp {
template int launch_extract_region_variable_type<float>(unsigned, const Region&, const uint64_t*, size_t,
                                                        const uint16_t*, const uint64_t*, uint64_t*, uint64_t,
                                                        uint16_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*,
                                                        hipStream_t);
template int launch_insert_region_variable_type<float>(const Problem&, const Region&, const uint64_t*, size_t,
                                                       const uint16_t*, const uint64_t*, const uint64_t*, size_t,
                                                       const uint16_t*, const uint64_t*, uint64_t*, uint64_t,
                                                       uint16_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*,
                                                       hipStream_t);
}  // namespace cuzfp
