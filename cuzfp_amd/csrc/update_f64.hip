// cuzfp_amd/csrc/update_f64.hip -- double instantiations of the sub-box encoder.
#include "region_update_kernels.hpp"

namespace cuzfp {
template int launch_encode_region_type<double>(const Problem&, const Region&, const void*, bool, bool, uint64_t*,
                                            hipStream_t);
}  // namespace cuzfp
