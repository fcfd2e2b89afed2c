// cuzfp_amd/csrc/update_i32.hip -- int32 instantiations of the sub-box encoder.
#include "region_update_kernels.hpp"

namespace cuzfp {
template int launch_encode_region_type<int32_t>(const Problem&, const Region&, const void*, bool, bool, uint64_t*,
                                            hipStream_t);
}  // namespace cuzfp
