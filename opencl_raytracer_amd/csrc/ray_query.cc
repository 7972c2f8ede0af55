// ray_query.cc -- ray queries, multi-hit queries and ambient-occlusion queries on a render host's uploaded scene (ray_query.h).
#include "ray_query.h"

#include <cmath>
#include <stdexcept>

#include "device_internal.h"

namespace ocrt {

namespace {
constexpr size_t QUERY_COUNT_BYTES = (size_t) 1 << 18;  // kernels/query.hip.h: QUERY_BUCKETS words
constexpr uint32_t QUERY_NO_SORT = 1u, QUERY_SORT_MIN = 16384u;  // include/rt_hip_query.h
constexpr uint32_t MULTIHIT_MAX_SLOTS = 16u;                     // include/rt_hip_multihit.h, kernels/multihit.hip.h
size_t round16(size_t bytes) { return (bytes + 15u) & ~(size_t) 15u; }
}  // namespace

RayQueries::RayQueries(DeviceRenderer &renderer) : dev(renderer) {
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	OCRT_HIP(hipEventCreate((hipEvent_t *) &ev_start));
	OCRT_HIP(hipEventCreate((hipEvent_t *) &ev_stop));
}

RayQueries::~RayQueries() {
	if (hipSetDevice(dev.deviceIndex()) != hipSuccess)
		return;
	if (timed)
		(void) hipEventSynchronize((hipEvent_t) ev_stop);
	device_free(d_count);
	device_free(d_order);
	device_free(d_stage);
	device_free(d_ao_hits);
	device_free(d_list);
	(void) hipEventDestroy((hipEvent_t) ev_start);
	(void) hipEventDestroy((hipEvent_t) ev_stop);
}

// (hipFree waits for the device: a query still running on the old buffer finishes first)
void RayQueries::grow(void *&buffer, size_t &capacity, size_t bytes) {
	if (bytes <= capacity && buffer)
		return;
	device_free(buffer);
	capacity = 0;
	buffer = device_alloc(bytes);
	capacity = bytes;
}

// The sort key's origin cells: 8 per axis over the root's box (exact records, read once per uploaded scene).  A box that
// is no box (damaged arrays) gives [-1, 1]: the key then sorts worse, the results are the same.
void RayQueries::sceneBox(const DeviceScene &scene, float lo[3], float scale[3]) {
	const std::shared_ptr<const DeviceScene> current = dev.deviceScene();
	if (boxed.lock() != current) {
		NodeRec root{};
		if (scene.nodeCount() > 0)
			OCRT_HIP(hipMemcpy(&root, scene.buffers().nodes, sizeof root, hipMemcpyDeviceToHost));
		for (int k = 0; k < 3; ++k) {
			const float extent = root.hi[k] - root.lo[k];
			const bool usable = std::isfinite(root.lo[k]) && std::isfinite(extent) && extent > 0.0f;
			box_lo[k] = usable ? root.lo[k] : -1.0f;
			box_scale[k] = usable ? 8.0f / extent : 4.0f;
			if (!std::isfinite(box_scale[k]))
				box_scale[k] = 4.0f, box_lo[k] = -1.0f;
		}
		boxed = current;
	}
	for (int k = 0; k < 3; ++k) {
		lo[k] = box_lo[k];
		scale[k] = box_scale[k];
	}
}

void RayQueries::traceDevice(bool closest, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                             uint32_t flags, const QueryOutputs &out, void *stream) {
	if (!dev.sceneReady() || !dev.deviceScene())
		throw std::logic_error("ray query before a scene was uploaded");
	if (n == 0)
		return;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	hipStream_t s = (hipStream_t) (stream ? stream : dev.streamHandle());
	const DeviceScene &scene = *dev.deviceScene();
	// one set of scratch per host: a query on another stream waits for the one before it
	if (timed)
		OCRT_HIP(hipStreamWaitEvent(s, (hipEvent_t) ev_stop, 0));
	const bool sort = !(flags & QUERY_NO_SORT) && n >= QUERY_SORT_MIN;
	if (sort) {
		size_t count_bytes = d_count ? QUERY_COUNT_BYTES : 0;
		grow(d_count, count_bytes, QUERY_COUNT_BYTES);
		grow(d_order, order_bytes, (size_t) n * sizeof(uint32_t));
	}
	float lo[3], scale[3];
	if (sort)
		sceneBox(scene, lo, scale);
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_start, s));
	if (sort)
		launch_query_sort(origins4, directions4, n, lo, scale, d_count, d_order, s);
	launch_query(scene.buffers(), dev.params().node_count, closest, origins4, directions4, sort ? d_order : nullptr, n, max_distance,
	             out.hit, out.distance, out.leaf, out.barycentric, out.position, out.normal, s);
	OCRT_HIP(hipGetLastError());
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_stop, s));
	timed = true;
	have_ms = false;
}

void RayQueries::traceHost(bool closest, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                           uint32_t flags, unsigned char *hit, float *distance, uint32_t *leaf, float *barycentric, float *position,
                           float *normal) {
	if (!dev.sceneReady() || !dev.deviceScene())
		throw std::logic_error("ray query before a scene was uploaded");
	if (n == 0)
		return;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	hipStream_t s = (hipStream_t) dev.streamHandle();
	// staging: origins, directions, then the outputs asked for
	const size_t ray_bytes = (size_t) n * 16u, word_bytes = round16((size_t) n * 4u), vec_bytes = round16((size_t) n * 12u);
	size_t at = 2 * ray_bytes;
	QueryOutputs out;
	auto place = [&](bool wanted, size_t bytes) -> size_t {
		if (!wanted)
			return (size_t) -1;
		const size_t here = at;
		at += bytes;
		return here;
	};
	const size_t o_hit = place(hit != nullptr, round16(n)), o_dist = place(closest && distance, word_bytes);
	const size_t o_leaf = place(closest && leaf, word_bytes), o_bary = place(closest && barycentric, vec_bytes);
	const size_t o_pos = place(closest && position, vec_bytes), o_norm = place(closest && normal, vec_bytes);
	grow(d_stage, stage_bytes, at);
	char *base = (char *) d_stage;
	auto dptr = [&](size_t offset) -> void * { return offset == (size_t) -1 ? nullptr : base + offset; };
	out.hit = (unsigned char *) dptr(o_hit);
	out.distance = (float *) dptr(o_dist);
	out.leaf = (uint32_t *) dptr(o_leaf);
	out.barycentric = (float *) dptr(o_bary);
	out.position = (float *) dptr(o_pos);
	out.normal = (float *) dptr(o_norm);
	OCRT_HIP(hipMemcpyAsync(base, origins4, ray_bytes, hipMemcpyHostToDevice, s));
	OCRT_HIP(hipMemcpyAsync(base + ray_bytes, directions4, ray_bytes, hipMemcpyHostToDevice, s));
	traceDevice(closest, (const float *) base, (const float *) (base + ray_bytes), n, max_distance, flags, out, s);
	auto back = [&](void *host, const void *device, size_t bytes) {
		if (host && device)
			OCRT_HIP(hipMemcpyAsync(host, device, bytes, hipMemcpyDeviceToHost, s));
	};
	back(hit, out.hit, n);
	back(distance, out.distance, (size_t) n * 4u);
	back(leaf, out.leaf, (size_t) n * 4u);
	back(barycentric, out.barycentric, (size_t) n * 12u);
	back(position, out.position, (size_t) n * 12u);
	back(normal, out.normal, (size_t) n * 12u);
	OCRT_HIP(hipStreamSynchronize(s));
}

void RayQueries::multihitDevice(const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k,
                                uint32_t flags, const MultiHitOutputs &out, void *stream) {
	if (!dev.sceneReady() || !dev.deviceScene())
		throw std::logic_error("multi-hit query before a scene was uploaded");
	if (k > MULTIHIT_MAX_SLOTS)
		throw std::invalid_argument("more slots per ray than RT_MULTIHIT_MAX_K");
	// without a slot array the lists are not wanted: the count-only walk
	const uint32_t slots = out.anySlot() ? k : 0u;
	if (n == 0 || (slots == 0 && !out.count))
		return;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	hipStream_t s = (hipStream_t) (stream ? stream : dev.streamHandle());
	const DeviceScene &scene = *dev.deviceScene();
	// one set of scratch per host: a query on another stream waits for the one before it
	if (timed)
		OCRT_HIP(hipStreamWaitEvent(s, (hipEvent_t) ev_stop, 0));
	const bool sort = !(flags & QUERY_NO_SORT) && n >= QUERY_SORT_MIN;
	if (sort) {
		size_t count_bytes = d_count ? QUERY_COUNT_BYTES : 0;
		grow(d_count, count_bytes, QUERY_COUNT_BYTES);
		grow(d_order, order_bytes, (size_t) n * sizeof(uint32_t));
	}
	if (slots)
		grow(d_list, list_bytes, (size_t) n * slots * 8u);
	float lo[3], scale[3];
	if (sort)
		sceneBox(scene, lo, scale);
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_start, s));
	if (sort)
		launch_query_sort(origins4, directions4, n, lo, scale, d_count, d_order, s);
	launch_multihit(scene.buffers(), dev.params().node_count, origins4, directions4, sort ? d_order : nullptr, n, max_distance, slots,
	                d_list, out.count, out.distance, out.leaf, out.barycentric, out.position, out.normal, s);
	OCRT_HIP(hipGetLastError());
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_stop, s));
	timed = true;
	have_ms = false;
}

void RayQueries::multihitHost(const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k, uint32_t flags,
                              const MultiHitOutputs &host) {
	if (!dev.sceneReady() || !dev.deviceScene())
		throw std::logic_error("multi-hit query before a scene was uploaded");
	if (k > MULTIHIT_MAX_SLOTS)
		throw std::invalid_argument("more slots per ray than RT_MULTIHIT_MAX_K");
	if (n == 0 || (!host.count && !host.anySlot()))
		return;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	hipStream_t s = (hipStream_t) dev.streamHandle();
	// staging: origins, directions, then the outputs asked for
	const size_t ray_bytes = (size_t) n * 16u, slots = (size_t) n * k;
	size_t at = 2 * ray_bytes;
	auto place = [&](const void *wanted, size_t bytes) -> size_t {
		if (!wanted)
			return (size_t) -1;
		const size_t here = at;
		at += round16(bytes);
		return here;
	};
	const size_t o_count = place(host.count, (size_t) n * 4u), o_dist = place(host.distance, slots * 4u);
	const size_t o_leaf = place(host.leaf, slots * 4u), o_bary = place(host.barycentric, slots * 12u);
	const size_t o_pos = place(host.position, slots * 12u), o_norm = place(host.normal, slots * 12u);
	grow(d_stage, stage_bytes, at);
	char *base = (char *) d_stage;
	auto dptr = [&](size_t offset) -> void * { return offset == (size_t) -1 ? nullptr : base + offset; };
	MultiHitOutputs out;
	out.count = (uint32_t *) dptr(o_count);
	out.distance = (float *) dptr(o_dist);
	out.leaf = (uint32_t *) dptr(o_leaf);
	out.barycentric = (float *) dptr(o_bary);
	out.position = (float *) dptr(o_pos);
	out.normal = (float *) dptr(o_norm);
	OCRT_HIP(hipMemcpyAsync(base, origins4, ray_bytes, hipMemcpyHostToDevice, s));
	OCRT_HIP(hipMemcpyAsync(base + ray_bytes, directions4, ray_bytes, hipMemcpyHostToDevice, s));
	multihitDevice((const float *) base, (const float *) (base + ray_bytes), n, max_distance, k, flags, out, s);
	auto back = [&](void *to, const void *device, size_t bytes) {
		if (to && device && bytes)
			OCRT_HIP(hipMemcpyAsync(to, device, bytes, hipMemcpyDeviceToHost, s));
	};
	back(host.count, out.count, (size_t) n * 4u);
	back(host.distance, out.distance, slots * 4u);
	back(host.leaf, out.leaf, slots * 4u);
	back(host.barycentric, out.barycentric, slots * 12u);
	back(host.position, out.position, slots * 12u);
	back(host.normal, out.normal, slots * 12u);
	OCRT_HIP(hipStreamSynchronize(s));
}

uint32_t RayQueries::aoRaysPerPoint(const DeviceRenderer &renderer) {
	const KernelParams &kp = renderer.params();
	const bool available = renderer.sceneReady() && renderer.deviceScene() && kp.ao_mode != AO_NONE && kp.ao_dirs > 0 &&
	                       renderer.deviceScene()->aoDirs() == kp.ao_dirs;
	return available ? kp.ao_dirs : 0u;
}
uint32_t RayQueries::aoDivisor(const DeviceRenderer &renderer) { return aoRaysPerPoint(renderer) ? renderer.params().ao_divisor : 0u; }

void RayQueries::aoDevice(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags, float *ao,
                          uint32_t *occluded, void *stream) {
	if (!dev.sceneReady() || !dev.deviceScene())
		throw std::logic_error("ambient-occlusion query before a scene was uploaded");
	if (aoRaysPerPoint(dev) == 0)
		throw std::logic_error("ambient-occlusion query on a host whose options have ambient occlusion off");
	if (n == 0 || (!ao && !occluded))
		return;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	hipStream_t s = (hipStream_t) (stream ? stream : dev.streamHandle());
	const DeviceScene &scene = *dev.deviceScene();
	const KernelParams &kp = dev.params();
	// one set of scratch per host: a query on another stream waits for the one before it
	if (timed)
		OCRT_HIP(hipStreamWaitEvent(s, (hipEvent_t) ev_stop, 0));
	// the POINTS are ordered (key: point and normal) from as many on as make RT_QUERY_SORT_MIN rays
	const bool sort = !(flags & QUERY_NO_SORT) && (uint64_t) n * kp.ao_dirs >= QUERY_SORT_MIN;
	if (sort) {
		size_t count_bytes = d_count ? QUERY_COUNT_BYTES : 0;
		grow(d_count, count_bytes, QUERY_COUNT_BYTES);
		grow(d_order, order_bytes, (size_t) n * sizeof(uint32_t));
	}
	if (!occluded)
		grow(d_ao_hits, ao_hits_bytes, (size_t) n * sizeof(uint32_t));
	float lo[3], scale[3];
	if (sort)
		sceneBox(scene, lo, scale);
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_start, s));
	if (sort)
		launch_query_sort(points4, normals4, n, lo, scale, d_count, d_order, s);
	launch_ao_query(scene.buffers(), kp.node_count, kp.ao_mode, kp.ao_dirs, kp.ao_divisor, kp.ao_max_distance, points4, normals4, seeds,
	                sort ? d_order : nullptr, n, occluded ? occluded : (uint32_t *) d_ao_hits, ao, s);
	OCRT_HIP(hipGetLastError());
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_stop, s));
	timed = true;
	have_ms = false;
}

void RayQueries::aoHost(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags, float *ao,
                        uint32_t *occluded) {
	if (!dev.sceneReady() || !dev.deviceScene())
		throw std::logic_error("ambient-occlusion query before a scene was uploaded");
	if (aoRaysPerPoint(dev) == 0)
		throw std::logic_error("ambient-occlusion query on a host whose options have ambient occlusion off");
	if (n == 0 || (!ao && !occluded))
		return;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	hipStream_t s = (hipStream_t) dev.streamHandle();
	// staging: points, normals, the counts, then the seeds and the values if there are any
	const size_t vec_bytes = (size_t) n * 16u, word_bytes = round16((size_t) n * 4u);
	const size_t o_count = 2 * vec_bytes, o_seeds = o_count + word_bytes, o_ao = o_seeds + (seeds ? word_bytes : 0);
	grow(d_stage, stage_bytes, o_ao + (ao ? word_bytes : 0));
	char *base = (char *) d_stage;
	uint32_t *d_occluded = (uint32_t *) (base + o_count), *d_seeds = seeds ? (uint32_t *) (base + o_seeds) : nullptr;
	float *d_value = ao ? (float *) (base + o_ao) : nullptr;
	OCRT_HIP(hipMemcpyAsync(base, points4, vec_bytes, hipMemcpyHostToDevice, s));
	OCRT_HIP(hipMemcpyAsync(base + vec_bytes, normals4, vec_bytes, hipMemcpyHostToDevice, s));
	if (seeds)
		OCRT_HIP(hipMemcpyAsync(d_seeds, seeds, (size_t) n * 4u, hipMemcpyHostToDevice, s));
	aoDevice((const float *) base, (const float *) (base + vec_bytes), d_seeds, n, flags, d_value, d_occluded, s);
	if (ao)
		OCRT_HIP(hipMemcpyAsync(ao, d_value, (size_t) n * 4u, hipMemcpyDeviceToHost, s));
	if (occluded)
		OCRT_HIP(hipMemcpyAsync(occluded, d_occluded, (size_t) n * 4u, hipMemcpyDeviceToHost, s));
	OCRT_HIP(hipStreamSynchronize(s));
}

float RayQueries::lastMs() {
	if (!timed)
		return 0.0f;
	if (!have_ms) {
		OCRT_HIP(hipSetDevice(dev.deviceIndex()));
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
		OCRT_HIP(hipEventElapsedTime(&last_ms, (hipEvent_t) ev_start, (hipEvent_t) ev_stop));
		have_ms = true;
	}
	return last_ms;
}

}  // namespace ocrt
