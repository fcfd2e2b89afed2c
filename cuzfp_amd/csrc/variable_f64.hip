// cuzfp_amd/csrc/variable_f64.hip -- double instantiations of the variable-rate kernels.
#include "variable_kernels.hpp"

namespace cuzfp {
template int launch_encode_variable_type<double>(const Problem&, const void*, bool, uint32_t, int, uint64_t*, uint64_t,
                                                 uint16_t*, uint64_t*, uint64_t*, uint64_t*, hipStream_t);
template int launch_decode_variable_type<double>(const Problem&, const uint64_t*, size_t, const uint16_t*, bool, void*,
                                                 uint64_t*, uint64_t*, hipStream_t);
}  // namespace cuzfp
