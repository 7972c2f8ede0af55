// ray_query.h -- ray queries on a render host's uploaded scene (include/rt_hip_query.h; kernels/query.hip.h).
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
		float lastMs();

	private:
		void grow(void *&buffer, size_t &capacity, size_t bytes);
		void sceneBox(const DeviceScene &scene, float lo[3], float scale[3]);

		DeviceRenderer &dev;
		void *d_count = nullptr, *d_order = nullptr, *d_stage = nullptr;
		size_t order_bytes = 0, stage_bytes = 0;
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

}  // namespace ocrt
