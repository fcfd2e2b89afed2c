// cuzfp_amd/csrc/update_i64.hip -- int64 instantiations of the sub-box encoder.
#include "region_update_kernels.hpp"

namespace cuzfp {
template int launch_encode_region_type<int64_t>(const Problem&, const Region&, const void*, bool, bool, uint64_t*,
                                            hipStream_t);
}  // namespace cuzfp
