// sign_sort.hip -- the two sorts of a sign table's incidence (include/rt_hip_signed.h; kernels/signed.hip.h): the 3 F corners
// by vertex id (32 bits), and by the edge's (min, max) vertex pair (64 bits), each with the value 3 leaf + corner, stable, so
// that equal keys stay in rising value.  rocPRIM's radix sort; a translation unit of its own beside build_sort.hip, so that
// kernels.hip and its flags stay what they are.
#include <cstring>  // (rocPRIM's texture_cache_iterator.hpp calls memset without it)

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "device_internal.h"

namespace ocrt {

// The temporary storage the larger of the two sorts of `pairs` pairs asks for.
size_t sign_sort_bytes(uint32_t pairs) {
	size_t narrow = 0, wide = 0;
	OCRT_HIP(rocprim::radix_sort_pairs(nullptr, narrow, (const uint32_t *) nullptr, (uint32_t *) nullptr, (const uint32_t *) nullptr,
	                                   (uint32_t *) nullptr, (size_t) pairs, 0u, 32u, (hipStream_t) nullptr));
	OCRT_HIP(rocprim::radix_sort_pairs(nullptr, wide, (const unsigned long long *) nullptr, (unsigned long long *) nullptr,
	                                   (const uint32_t *) nullptr, (uint32_t *) nullptr, (size_t) pairs, 0u, 64u, (hipStream_t) nullptr));
	return narrow > wide ? narrow : wide;
}

// `wide`: 64-bit keys (the edges'), else 32-bit keys (the vertices').
void launch_sign_sort(bool wide, void *temporary, size_t temporary_bytes, const void *keys_in, void *keys_out, const void *values_in,
                      void *values_out, uint32_t pairs, void *stream) {
	if (wide)
		OCRT_HIP(rocprim::radix_sort_pairs(temporary, temporary_bytes, (const unsigned long long *) keys_in, (unsigned long long *) keys_out,
		                                   (const uint32_t *) values_in, (uint32_t *) values_out, (size_t) pairs, 0u, 64u, (hipStream_t) stream));
	else
		OCRT_HIP(rocprim::radix_sort_pairs(temporary, temporary_bytes, (const uint32_t *) keys_in, (uint32_t *) keys_out,
		                                   (const uint32_t *) values_in, (uint32_t *) values_out, (size_t) pairs, 0u, 32u, (hipStream_t) stream));
}

}  // namespace ocrt
