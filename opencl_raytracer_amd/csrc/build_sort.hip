// build_sort.hip -- the sort of a device-side scene build (include/rt_hip_build.h; lbvh.h): (key, face id) pairs by the 30 bits
// of the key, stable, so that equal keys stay in rising face id.  rocPRIM's radix sort; a translation unit of its own, so
// that kernels.hip and its flags stay what they are.
#include <cstring>  // (rocPRIM's texture_cache_iterator.hpp calls memset without it)

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "device_internal.h"

namespace ocrt {

constexpr unsigned BUILD_KEY_BITS = 30u;

// The temporary storage the sort of `pairs` pairs asks for.
size_t build_sort_bytes(uint32_t pairs) {
	size_t bytes = 0;
	OCRT_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t *) nullptr, (uint32_t *) nullptr, (const uint32_t *) nullptr,
	                                   (uint32_t *) nullptr, (size_t) pairs, 0u, BUILD_KEY_BITS, (hipStream_t) nullptr));
	return bytes;
}

void launch_build_sort(void *temporary, size_t temporary_bytes, const void *keys_in, void *keys_out, const void *ids_in, void *ids_out,
                       uint32_t pairs, void *stream) {
	OCRT_HIP(rocprim::radix_sort_pairs(temporary, temporary_bytes, (const uint32_t *) keys_in, (uint32_t *) keys_out, (const uint32_t *) ids_in,
	                                   (uint32_t *) ids_out, (size_t) pairs, 0u, BUILD_KEY_BITS, (hipStream_t) stream));
}

}  // namespace ocrt
