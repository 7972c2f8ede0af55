// ray_query.h -- ray queries, multi-hit queries and ambient-occlusion queries on a render host's uploaded scene
// (include/rt_hip_query.h, include/rt_hip_multihit.h, include/rt_hip_ao.h; kernels/query.hip.h, kernels/multihit.hip.h,
// kernels/ao_query.hip.h).
#pragma once
#include <cstdint>
#include <memory>

#include "device_renderer.h"

namespace ocrt {

// Outputs of a closest-hit query by ray index, device pointers; null: not written.
struct QueryOutputs {
	unsigned char *hit = nullptr;
	float *distance = nullptr;
	uint32_t *leaf = nullptr;
	float *barycentric = nullptr, *position = nullptr, *normal = nullptr;
};

// Outputs of a multi-hit query, device pointers; null: not written.  `count` by ray index, the others by ray and slot
// (slot j of ray i at i * k + j).
struct MultiHitOutputs {
	uint32_t *count = nullptr;
	float *distance = nullptr;
	uint32_t *leaf = nullptr;
	float *barycentric = nullptr, *position = nullptr, *normal = nullptr;
	bool anySlot() const { return distance || leaf || barycentric || position || normal; }
};

// What one render host needs beyond its renderer to answer queries: scratch of its own (the sort's counts and order,
// the staging buffers of the host-memory form), grown on demand and never shared with the frame's buffers, and the
// events that time the last query.  Reads the renderer's scene and stream, changes nothing of it.
class RayQueries {
	public:
		explicit RayQueries(DeviceRenderer &renderer);
		~RayQueries();
		RayQueries(const RayQueries &) = delete;
		RayQueries &operator=(const RayQueries &) = delete;

		// Device memory, enqueued on `stream` (null: the renderer's); `closest` false: occlusion into out.hit alone.
		void traceDevice(bool closest, const float *origins4, const float *directions4, uint32_t n, float max_distance,
		                 uint32_t flags, const QueryOutputs &out, void *stream);
		// Host memory, blocking: the rays go through the staging buffers on the renderer's stream.
		void traceHost(bool closest, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t flags,
		               unsigned char *hit, float *distance, uint32_t *leaf, float *barycentric, float *position, float *normal);
		// Multi-hit queries (include/rt_hip_multihit.h): the count of accepted triangles per ray and the first k of them.
		// Device memory, enqueued on `stream` (null: the renderer's); k <= RT_MULTIHIT_MAX_K, 0 = the count alone.
		void multihitDevice(const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k, uint32_t flags,
		                    const MultiHitOutputs &out, void *stream);
		// Host memory, blocking.
		void multihitHost(const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k, uint32_t flags,
		                  const MultiHitOutputs &out);
		// Ambient-occlusion queries (include/rt_hip_ao.h): the reference's ambient_occlusion() of n points with the options
		// the scene was uploaded for -- table, mode, rays per point, divisor and reach come from the renderer's launch
		// constants and its DeviceScene.  std::logic_error where those options have ambient occlusion off.
		// (static: what a renderer's uploaded scene answers, before any query has made scratch for it)
		static uint32_t aoRaysPerPoint(const DeviceRenderer &renderer);  // 0: not available
		static uint32_t aoDivisor(const DeviceRenderer &renderer);
		// Device memory, enqueued on `stream` (null: the renderer's); `seeds`, `ao`, `occluded` may be null.
		void aoDevice(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags, float *ao,
		              uint32_t *occluded, void *stream);
		// Host memory, blocking.
		void aoHost(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags, float *ao,
		            uint32_t *occluded);
		float lastMs();  // the last query of any kind

	private:
		void grow(void *&buffer, size_t &capacity, size_t bytes);
		void sceneBox(const DeviceScene &scene, float lo[3], float scale[3]);

		DeviceRenderer &dev;
		void *d_count = nullptr, *d_order = nullptr, *d_stage = nullptr;
		void *d_ao_hits = nullptr;  // aoDevice without an `occluded` array: the points' counts
		void *d_list = nullptr;  // multihitDevice: the rays' key lists, n * k * 8 bytes
		size_t order_bytes = 0, stage_bytes = 0, ao_hits_bytes = 0, list_bytes = 0;
		void *ev_start = nullptr, *ev_stop = nullptr;
		bool timed = false, have_ms = false;
		float last_ms = 0.0f;
		std::weak_ptr<const DeviceScene> boxed;  // the scene box_lo / box_scale were read from
		float box_lo[3] = { 0, 0, 0 }, box_scale[3] = { 0, 0, 0 };
};

// kernels.hip
void launch_query_sort(const void *origins, const void *directions, uint32_t n, const float lo[3], const float scale[3], void *count,
                       void *order, void *stream);
void launch_query(const SceneBuffers &scene, uint32_t node_count, bool closest, const void *origins, const void *directions,
                  const void *order, uint32_t n, float max_distance, unsigned char *hit, float *distance, uint32_t *leaf,
                  float *barycentric, float *position, float *normal, void *stream);
void launch_multihit(const SceneBuffers &scene, uint32_t node_count, const void *origins, const void *directions, const void *order,
                     uint32_t n, float max_distance, uint32_t k, void *list, uint32_t *count, float *distance, uint32_t *leaf,
                     float *barycentric, float *position, float *normal, void *stream);
void launch_ao_query(const SceneBuffers &scene, uint32_t node_count, int ao_mode, uint32_t rays_per_point, uint32_t divisor,
                     float max_distance, const void *points, const void *normals, const uint32_t *seeds, const void *order, uint32_t n,
                     uint32_t *count, float *ao, void *stream);

}  // namespace ocrt
