// cuzfp_amd/csrc/region_f64.hip -- double instantiations of the sub-box decoder.
#include "region_kernels.hpp"

namespace cuzfp {
template int launch_decode_region_type<double>(const Problem&, const Region&, const uint64_t*, bool, uint32_t, void*,
                                              hipStream_t);
}  // namespace cuzfp
