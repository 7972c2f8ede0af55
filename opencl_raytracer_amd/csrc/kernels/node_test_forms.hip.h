// kernels/node_test_forms.hip.h -- a test kernel: the any-hit walk's node test (walk.hip.h, OCRT_TEST_CE_SCALED) against the
// form it replaced, on caller-supplied records and walk rays (include/rt_hip_debug.h, rt_debug_node_test_forms)
// (part of the one translation unit kernels.hip)
#pragma once

namespace ocrt {

// The twelve-instruction form the loop ran before near and far of an axis came from one packed fma: every value by a
// v_fma_f32 of its own, |inv| by source modifiers.  It lives on HERE only, as the reference of the packed form: near in v59,
// far in v56.
#define OCRT_TEST_CE_TWELVE(CX, CY, CZ, EX, EY, EZ)      \
	"\tv_fma_f32 v56, " CX ", %[ix], %[oix]\n"           \
	"\tv_fma_f32 v57, " CY ", %[iy], %[oiy]\n"           \
	"\tv_fma_f32 v58, " CZ ", %[iz], %[oiz]\n"           \
	"\tv_fma_f32 v59, -" EX ", |%[ix]|, v56\n"           \
	"\tv_fma_f32 v56, " EX ", |%[ix]|, v56\n"            \
	"\tv_fma_f32 v60, -" EY ", |%[iy]|, v57\n"           \
	"\tv_fma_f32 v57, " EY ", |%[iy]|, v57\n"            \
	"\tv_fma_f32 v61, -" EZ ", |%[iz]|, v58 clamp\n"     \
	"\tv_fma_f32 v58, " EZ ", |%[iz]|, v58 clamp\n"      \
	"\tv_max3_f32 v59, v59, v60, v61\n"                  \
	"\tv_min3_f32 v56, v56, v57, v58\n"                  \
	"\tv_cmp_lt_f32 vcc, v59, v56\n"

// One form on the record at byte offset `at`, fetched into the registers the loop holds it in (LOAD: node `a` in s[48:55],
// node `b` in s[56:63]); NEAR / FAR: where the form leaves the two values.
#define OCRT_NODE_TEST_FORM(LOAD, TEST, NEAR, FAR)                                                                             \
	asm volatile("\ts_load_dwordx8 " LOAD ", %[base], %[at]\n"                                                                 \
	             "\ts_waitcnt lgkmcnt(0)\n" TEST "\tv_mov_b32 %[near], " NEAR "\n"                                             \
	             "\tv_mov_b32 %[far], " FAR "\n"                                                                               \
	             "\tv_cndmask_b32 %[hit], 0, 1, vcc\n"                                                                         \
	             : [near] "=&v"(near), [far] "=&v"(far), [hit] "=&v"(hit)                                                      \
	             : [base] "s"(records), [at] "s"(at), [ix] "v"(ix), [iy] "v"(iy), [iz] "v"(iz), [oix] "v"(oix), [oiy] "v"(oiy), \
	               [oiz] "v"(oiz), [axy] "v"(abs_xy), [azw] "v"(abs_zw)                                                        \
	             : "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", \
	               "v56", "v57", "v58", "v59", "v60", "v61", "vcc", "memory")

// A lane per ray, a wave per 64 rays (`rays` is a multiple of 64), every ray against every record.  rays6: a WalkRay each
// (ix, iy, iz, oix, oiy, oiz), as make_walk_ray leaves them.  out: nine words per (ray, record) -- near, far and the decision
// (0 / 1) of the twelve-instruction form, of the packed form on node `a`'s registers, and of the packed form on node `b`'s.
__global__ __launch_bounds__(64) void node_test_forms_kernel(const float4 *records, uint32_t boxes, const float *rays6, uint32_t *out) {
	const uint32_t ray = blockIdx.x * 64u + threadIdx.x;
	const float *r = rays6 + 6u * (size_t) ray;
	const float ix = r[0], iy = r[1], iz = r[2], oix = r[3], oiy = r[4], oiz = r[5];
	const f32x2 abs_xy = { __builtin_fabsf(ix), __builtin_fabsf(iy) };
	const f32x2 abs_zw = { __builtin_fabsf(iz), __builtin_fabsf(iz) };
	for (uint32_t box = 0u; box < boxes; ++box) {
		const uint32_t at = (uint32_t) __builtin_amdgcn_readfirstlane((int) (box * 32u));
		uint32_t *o = out + ((size_t) ray * boxes + box) * 9u;
		uint32_t near, far, hit;
		OCRT_NODE_TEST_FORM("s[48:55]", OCRT_TEST_CE_TWELVE("s48", "s49", "s50", "s52", "s53", "s54"), "v59", "v56");
		o[0] = near; o[1] = far; o[2] = hit;
		OCRT_NODE_TEST_FORM("s[48:55]", OCRT_TEST_CE_SCALED("s48", "s49", "s50", "s[52:53]", "s[54:55]"), "v56", "v57");
		o[3] = near; o[4] = far; o[5] = hit;
		OCRT_NODE_TEST_FORM("s[56:63]", OCRT_TEST_CE_SCALED("s56", "s57", "s58", "s[60:61]", "s[62:63]"), "v56", "v57");
		o[6] = near; o[7] = far; o[8] = hit;
	}
}

}  // namespace ocrt
