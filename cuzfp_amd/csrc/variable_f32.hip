// cuzfp_amd/csrc/variable_f32.hip -- float instantiations of the variable-rate
// kernels, and the type-independent scan and zero-fill kernels.
#define CUZFP_VARIABLE_SHARED_UNIT 1
#include "variable_kernels.hpp"

namespace cuzfp {
template int launch_encode_variable_type<float>(const Problem&, const void*, bool, uint32_t, int, uint64_t*, uint64_t,
                                                uint16_t*, uint64_t*, uint64_t*, uint64_t*, hipStream_t);
template int launch_decode_variable_type<float>(const Problem&, const uint64_t*, size_t, const uint16_t*, bool, void*,
                                                uint64_t*, uint64_t*, hipStream_t);
}  // namespace cuzfp
