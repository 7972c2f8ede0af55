// ray_query.cc -- ray queries, segment queries, multi-hit queries, ambient-occlusion queries, frame layers and multi-view rendering on a render
// host's uploaded scene (ray_query.h).
#include "ray_query.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../include/rt_hip_instances.h"
#include "device_internal.h"

namespace ocrt {

namespace {
constexpr size_t QUERY_COUNT_BYTES = (size_t) 1 << 18;  // kernels/query.hip.h: QUERY_BUCKETS words
constexpr uint32_t QUERY_NO_SORT = 1u, QUERY_SORT_MIN = 16384u;  // include/rt_hip_query.h
constexpr uint32_t MULTIHIT_MAX_SLOTS = 16u;                     // include/rt_hip_multihit.h, kernels/multihit.hip.h
size_t round16(size_t bytes) { return (bytes + 15u) & ~(size_t) 15u; }
constexpr uint32_t QUERY_MAX_RAYS = 1u << 27;  // include/rt_hip_query.h
constexpr uint32_t VIEWS_MAX_CHUNK = 65535u;   // layers_kernel, views_resize_kernel: a grid's second and third dimension
constexpr size_t PINNED_HEAD = 16u;            // viewsDevice: the read-back word in front of the poses
}  // namespace

RayQueries::RayQueries(DeviceRenderer &renderer) : dev(renderer) {
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	OCRT_HIP(hipEventCreate((hipEvent_t *) &ev_start));
	OCRT_HIP(hipEventCreate((hipEvent_t *) &ev_stop));
	OCRT_HIP(hipEventCreate((hipEvent_t *) &ev_update_start));
	OCRT_HIP(hipEventCreate((hipEvent_t *) &ev_update_stop));
	OCRT_HIP(hipEventCreateWithFlags((hipEvent_t *) &ev_frames, hipEventDisableTiming));
	for (void *&ev : ev_build)
		OCRT_HIP(hipEventCreate((hipEvent_t *) &ev));
	for (void *&ev : ev_sign)
		OCRT_HIP(hipEventCreate((hipEvent_t *) &ev));
}

RayQueries::~RayQueries() {
	if (hipSetDevice(dev.deviceIndex()) != hipSuccess)
		return;
	if (timed)
		(void) hipEventSynchronize((hipEvent_t) ev_stop);
	for (Scratch *scratch : { &count, &order, &stage, &ao_hits, &ao_rows, &vis_rows, &list, &views, &build, &coords_flag, &nearest_counts, &inst_device,
		                         &inst_spare, &inst_plan, &sign_table, &sign_vertices, &sign_edges })
		device_free(scratch->ptr);
	for (void *ev : ev_sign)
		if (ev)
			(void) hipEventDestroy((hipEvent_t) ev);
	for (void *ev : ev_build)
		if (ev)
			(void) hipEventDestroy((hipEvent_t) ev);
	for (void *ev : ev_inst)
		if (ev)
			(void) hipEventDestroy((hipEvent_t) ev);
	if (pinned)
		(void) hipHostFree(pinned);
	(void) hipEventDestroy((hipEvent_t) ev_start);
	(void) hipEventDestroy((hipEvent_t) ev_stop);
	(void) hipEventDestroy((hipEvent_t) ev_update_start);
	(void) hipEventDestroy((hipEvent_t) ev_update_stop);
	(void) hipEventDestroy((hipEvent_t) ev_frames);
}

// (hipFree waits for the device: a query still running on the old buffer finishes first)
void RayQueries::grow(Scratch &scratch, size_t bytes) {
	if (bytes <= scratch.bytes && scratch.ptr)
		return;
	device_free(scratch.ptr);
	scratch.bytes = 0;
	scratch.ptr = device_alloc(bytes);
	scratch.bytes = bytes;
}

void RayQueries::requireScene(const char *query) const {
	if (!dev.sceneReady() || !dev.deviceScene())
		throw std::logic_error(std::string(query) + " before a scene was uploaded");
}

void RayQueries::requireSlots(uint32_t k) const {
	requireScene("multi-hit query");
	if (k > MULTIHIT_MAX_SLOTS)
		throw std::invalid_argument("more slots per ray than RT_MULTIHIT_MAX_K");
}

void RayQueries::requireAo() const {
	requireScene("ambient-occlusion query");
	if (aoRaysPerPoint(dev) == 0)
		throw std::logic_error("ambient-occlusion query on a host whose options have ambient occlusion off");
}

// The sort key's origin cells: 8 per axis over the root's box (exact records, read once per uploaded scene).  A box that
// is no box (damaged arrays) gives [-1, 1]: the key then sorts worse, the results are the same.
void RayQueries::sceneBox(const DeviceScene &scene, float lo[3], float scale[3]) {
	const std::shared_ptr<const DeviceScene> current = dev.deviceScene();
	if (boxed.lock() != current) {
		NodeRec root{};
		// (the copy below is ordered against no stream: an update still on its way to the root is waited for first)
		if (timed)
			OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
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

// The way into everything enqueued here, up to its own launches.  enter(): the stream (null: the renderer's) and the wait
// for the query before -- one set of scratch per host, so a query on another stream waits before any scratch is touched.
// begin(), on the stream entered: the scratch (the sort's, and what the family needs of its own, `needs`: every grow comes
// before ev_start, because hipFree synchronises), ev_start, and the sort of the n items keyed by (keys_a4, keys_b4) where
// the call allows it and makes RT_QUERY_SORT_MIN `rays` or more.
void *RayQueries::enter(void *stream) {
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	hipStream_t s = (hipStream_t) (stream ? stream : dev.streamHandle());
	if (timed)
		OCRT_HIP(hipStreamWaitEvent(s, (hipEvent_t) ev_stop, 0));
	return s;
}

RayQueries::Enqueue RayQueries::begin(void *entered, const float *keys_a4, const float *keys_b4, uint32_t n, uint64_t rays, uint32_t flags,
                                      std::initializer_list<Need> needs, bool segments, const float *box) {
	hipStream_t s = (hipStream_t) entered;
	const bool sort = !(flags & QUERY_NO_SORT) && rays >= QUERY_SORT_MIN;
	if (sort) {
		grow(count, QUERY_COUNT_BYTES);
		grow(order, (size_t) n * sizeof(uint32_t));
	}
	for (const Need &need : needs)
		if (need.scratch)
			grow(*need.scratch, need.bytes);
	float lo[3], scale[3];
	if (sort && box) {
		std::copy(box, box + 3, lo);
		std::copy(box + 3, box + 6, scale);
	} else if (sort) {
		sceneBox(*dev.deviceScene(), lo, scale);
	}
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_start, s));
	if (sort && keys_b4)
		launch_query_sort(keys_a4, keys_b4, n, lo, scale, count.ptr, order.ptr, s, segments);
	else if (sort)  // (points without a direction: the key of the position alone)
		launch_nearest_sort(keys_a4, n, lo, scale, count.ptr, order.ptr, s);
	return Enqueue{ s, sort ? order.ptr : nullptr };
}

// ... and the way out, after them.
void RayQueries::end(const Enqueue &q) {
	OCRT_HIP(hipGetLastError());
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_stop, (hipStream_t) q.stream));
	timed = true;
	have_ms = false;
}

// ---- arrays in host memory: one staging buffer, one path (ray_query.h: Arrays, staged) ----
// (the pointer variables are of many types: their values are read and written as bytes, never through a void **)
RayQueries::Arrays &RayQueries::Arrays::add(void *variable, size_t bytes, bool wanted, bool input) {
	if (!wanted)
		return *this;
	if (count == sizeof piece / sizeof piece[0])
		throw std::logic_error("more arrays in one call than RayQueries::Arrays holds");
	Piece &p = piece[count++];
	p.variable = variable;
	p.bytes = bytes;
	p.input = input;
	std::memcpy(&p.host, variable, sizeof p.host);
	return *this;
}

RayQueries::Arrays &RayQueries::Arrays::records(RecordOutputs &r, size_t records) {
	return out(r.distance, records * 4u).out(r.leaf, records * 4u).out(r.barycentric, records * 12u).out(r.position, records * 12u).out(
	    r.normal, records * 12u);
}

RayQueries::Arrays &RayQueries::Arrays::layers(LayerOutputs &l, size_t records) {
	out(l.hit, records).records(l, records);
	return out(l.direction, records * 12u).out(l.shade, records * 4u).out(l.ao, records * 4u).out(l.value, records * 4u);
}

void *RayQueries::stageIn(Arrays &arrays) {
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	hipStream_t s = (hipStream_t) dev.streamHandle();
	size_t total = 0;
	for (size_t i = 0; i < arrays.count; ++i)
		total += round16(arrays.piece[i].bytes);
	grow(stage, total);
	char *at = (char *) stage.ptr;
	for (size_t i = 0; i < arrays.count; ++i) {
		Arrays::Piece &p = arrays.piece[i];
		p.device = at;
		at += round16(p.bytes);
		std::memcpy(p.variable, &p.device, sizeof p.device);
		if (p.input)
			OCRT_HIP(hipMemcpyAsync(p.device, p.host, p.bytes, hipMemcpyHostToDevice, s));
	}
	return s;
}

void RayQueries::stageOut(const Arrays &arrays, void *stream) {
	for (size_t i = 0; i < arrays.count; ++i) {
		const Arrays::Piece &p = arrays.piece[i];
		if (!p.input && p.host && p.bytes)
			OCRT_HIP(hipMemcpyAsync(p.host, p.device, p.bytes, hipMemcpyDeviceToHost, (hipStream_t) stream));
	}
	OCRT_HIP(hipStreamSynchronize((hipStream_t) stream));
}

template <class Body> void RayQueries::staged(Where where, Arrays &arrays, Body &&body) {
	if (!where.host) {
		body(where.stream);
		return;
	}
	void *s = stageIn(arrays);
	body(s);
	stageOut(arrays, s);
}

void RayQueries::requireQuery(bool instanced, const char *query) const {
	if (instanced)
		requireInstances(("instanced " + std::string(query)).c_str());
	else
		requireScene(query);
}

RayQueries::Target RayQueries::target(bool instanced) {
	if (!instanced)
		return Target{ nullptr, nullptr };
	refreshInstances();  // (an update, a build or a new upload is picked up before the launch)
	return Target{ &inst_set, inst_box };
}

void RayQueries::trace(bool closest, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t flags,
                       QueryOutputs out, Where where, bool instanced, uint32_t *instance) {
	requireQuery(instanced, "ray query");
	if (n == 0)
		return;
	if (!closest) {  // (occlusion: the flags alone)
		static_cast<RecordOutputs &>(out) = RecordOutputs();
		instance = nullptr;
	}
	Arrays arrays;
	arrays.in(origins4, (size_t) n * 16u).in(directions4, (size_t) n * 16u).out(out.hit, n).records(out, n).out(instance, (size_t) n * 4u);
	staged(where, arrays, [&](void *stream) {
		const Target to = target(instanced);
		const Enqueue q = begin(enter(stream), origins4, directions4, n, n, flags, {}, false, to.box);
		launch_query(dev.deviceScene()->buffers(), dev.params().node_count, to.set, closest, origins4, directions4, q.order, n, max_distance, out,
		             instance, q.stream);
		end(q);
	});
}

// ---- the instance set (include/rt_hip_instances.h) ----
void RayQueries::setInstances(const float *world_from_object, uint32_t n) {
	if (n > RT_INSTANCES_MAX)
		throw std::invalid_argument("more instances than RT_INSTANCES_MAX");
	if (n > 0 && !world_from_object)
		throw std::invalid_argument("null transform array");
	std::vector<float> inverses;
	if (n > 0 && !instance_inverses(world_from_object, n, inverses))  // (every transform or none: the set stays on a refusal)
		throw std::invalid_argument("instance transform refused: an entry that is not finite, a zero determinant, or an inverse that is not finite");
	inst_inverse.swap(inverses);
	inst_built = false;  // (a device-built set ends here: include/rt_hip_instance_build.h)
	inst_built_n = 0;
	if (n == 0) {
		inst_inverse.clear();
		inst_world.clear();
	} else {
		inst_world.assign(world_from_object, world_from_object + (size_t) n * 12u);
	}
	inst_nodes.clear();
	inst_current = false;
	if (n > 0 && dev.sceneReady() && dev.deviceScene())
		refreshInstances();
}

void RayQueries::requireInstances(const char *what) const {
	requireScene(what);
	if (instanceCount() == 0)
		throw std::logic_error(std::string(what) + " without an instance set (rt_set_instances)");
}

void RayQueries::setInstanceBox(const float lo[3], const float hi[3]) {
	for (int k = 0; k < 3; ++k) {  // (sceneBox's rule, on the top-level root)
		const float extent = hi[k] - lo[k];
		const bool usable = std::isfinite(lo[k]) && std::isfinite(extent) && extent > 0.0f && std::isfinite(8.0f / extent);
		inst_box[k] = usable ? lo[k] : -1.0f;
		inst_box[3 + k] = usable ? 8.0f / extent : 4.0f;
	}
}

// The tree from the root box as it is on the device now, and the set's three arrays into inst_device.  Waits for this
// host's queries (an update on its way to the root, a query still reading the old arrays) before it reads or writes.
void RayQueries::refreshInstances() {
	const std::shared_ptr<const DeviceScene> current = dev.deviceScene();
	if (inst_current && inst_scene.lock() == current)
		return;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	if (inst_built) {  // (on the device, from the transforms that lie there and node 0 as it lies there: nothing to refuse)
		if (!planInstancesOnDevice((const float *) inst_set.world, inst_built_n, dev.streamHandle()))
			throw std::logic_error("a device-built instance set was refused when planned again (its transforms were accepted before)");
		return;
	}
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	NodeRec root{};
	if (current->nodeCount() > 0)
		OCRT_HIP(hipMemcpy(&root, current->buffers().nodes, sizeof root, hipMemcpyDeviceToHost));
	const uint32_t n = instanceCount();
	instance_tree(root.lo, root.hi, inst_world.data(), inst_inverse.data(), n, inst_nodes);
	std::vector<float> bounds;  // (the closest-point walk's: instance_nearest.h)
	instance_bounds(root.lo, root.hi, inst_world.data(), inst_inverse.data(), n, bounds);
	const size_t rows = (size_t) n * 12u * sizeof(float), tree = inst_nodes.size() * sizeof(InstanceNode);
	const size_t bound_bytes = bounds.size() * sizeof(float);
	grow(inst_device, 2u * rows + tree + bound_bytes);
	char *at = (char *) inst_device.ptr;
	OCRT_HIP(hipMemcpy(at, inst_world.data(), rows, hipMemcpyHostToDevice));
	OCRT_HIP(hipMemcpy(at + rows, inst_inverse.data(), rows, hipMemcpyHostToDevice));
	OCRT_HIP(hipMemcpy(at + 2u * rows, inst_nodes.data(), tree, hipMemcpyHostToDevice));
	OCRT_HIP(hipMemcpy(at + 2u * rows + tree, bounds.data(), bound_bytes, hipMemcpyHostToDevice));
	inst_set = InstanceBuffers{ at + 2u * rows, at + rows, (uint32_t) inst_nodes.size(), at, at + 2u * rows + tree };
	setInstanceBox(inst_nodes[0].lo, inst_nodes[0].hi);
	inst_scene = current;
	inst_current = true;
}

void RayQueries::instanceNodes(void *out) {
	requireInstances("instance tree");
	refreshInstances();
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	if (out)
		OCRT_HIP(hipMemcpy(out, inst_set.top, (size_t) inst_set.top_count * sizeof(InstanceNode), hipMemcpyDeviceToHost));
}

// ---- device-side instance sets (include/rt_hip_instance_build.h) ----
namespace {
size_t round256(size_t bytes) { return (bytes + 255u) & ~(size_t) 255u; }

// Where a plan's temporaries lie in inst_plan (kernels/instance_build.hip.h, InstanceBuildArgs, has every array's size).
struct InstancePlanScratch {
	size_t reach_partials, reach, leaves, box_partials, box, keys, ids, sorted_keys, sorted_ids, ranges, inner_links, leaf_links, counters, inner_at,
	    leaf_at, sort, sort_bytes, bytes;
};
InstancePlanScratch instance_plan_scratch(uint32_t n) {
	InstancePlanScratch at{};
	size_t end = 0;
	auto take = [&](size_t bytes) {
		const size_t p = end;
		end += round256(bytes ? bytes : 1);
		return p;
	};
	const size_t groups = build_partials(n), count = n;
	at.reach_partials = take(groups * 8);
	at.reach = take(8);
	at.leaves = take(count * 32);
	at.box_partials = take(groups * 32);
	at.box = take(32);
	at.keys = take(count * 4);
	at.ids = take(count * 4);
	at.sorted_keys = take(count * 4);
	at.sorted_ids = take(count * 4);
	at.ranges = take(count * 8);
	at.inner_links = take(count * 4);
	at.leaf_links = take(count * 4);
	at.counters = take(count * 4);
	at.inner_at = take(count * 4);
	at.leaf_at = take(count * 4);
	at.sort_bytes = n >= 2u ? build_sort_bytes(n) : 0;
	at.sort = take(at.sort_bytes);
	at.bytes = end;
	return at;
}
}  // namespace

RayQueries::InstanceSetLayout RayQueries::instanceSetLayout(uint32_t n) {
	InstanceSetLayout at{};
	const size_t rows = (size_t) n * 12u * sizeof(float), tree = (2u * (size_t) n - 1u) * sizeof(InstanceNode);
	at.inverse = rows;
	at.tree = 2u * rows + 16u;  // (16-byte aligned; the flag's word in the four bytes in front: one read brings both)
	at.flag = at.tree - sizeof(uint32_t);
	at.bounds = at.tree + tree + sizeof(InstanceNode);  // (a zero record behind the tree, as behind a scene's nodes)
	at.bytes = at.bounds + (size_t) n * 16u;
	return at;
}

void RayQueries::clearInstances() {
	inst_world.clear();
	inst_inverse.clear();
	inst_nodes.clear();
	inst_built = false;
	inst_built_n = 0;
	inst_current = false;
}

bool RayQueries::planInstancesOnDevice(const float *world_device, uint32_t n, void *stream) {
	// (behind the queries before it: one of them may still read the allocation the plan before last left as the spare one; an
	// update on its way to node 0 is waited for too)
	hipStream_t s = (hipStream_t) enter(stream);
	const std::shared_ptr<const DeviceScene> scene = dev.sceneReady() ? dev.deviceScene() : nullptr;
	const bool rooted = scene && scene->nodeCount() > 0;
	if (rooted && s != (hipStream_t) dev.streamHandle()) {  // (node 0 is read: behind whatever the renderer's stream still does to it)
		OCRT_HIP(hipEventRecord((hipEvent_t) ev_frames, (hipStream_t) dev.streamHandle()));
		OCRT_HIP(hipStreamWaitEvent(s, (hipEvent_t) ev_frames, 0));
	}
	const InstanceSetLayout set = instanceSetLayout(n);
	const InstancePlanScratch where = instance_plan_scratch(n);
	grow(inst_spare, set.bytes);
	grow(inst_plan, where.bytes);
	for (void *&ev : ev_inst)
		if (!ev)
			OCRT_HIP(hipEventCreate((hipEvent_t *) &ev));
	char *const made = (char *) inst_spare.ptr, *const base = (char *) inst_plan.ptr;
	const size_t rows = (size_t) n * 12u * sizeof(float), tree = (2u * (size_t) n - 1u) * sizeof(InstanceNode);
	OCRT_HIP(hipMemcpyAsync(made, world_device, rows, hipMemcpyDeviceToDevice, s));
	OCRT_HIP(hipMemsetAsync(made + set.tree - 16u, 0, 16u, s));
	OCRT_HIP(hipMemsetAsync(made + set.tree + tree, 0, sizeof(InstanceNode), s));
	InstancePlanBuffers b{};
	b.world = made;
	b.scene_root = rooted ? scene->buffers().nodes : nullptr;
	b.n = n;
	b.inverse = made + set.inverse;
	b.flag = made + set.flag;
	b.reach_partials = base + where.reach_partials;
	b.reach = base + where.reach;
	b.leaves = base + where.leaves;
	b.bounds = made + set.bounds;
	b.box_partials = base + where.box_partials;
	b.box = base + where.box;
	b.keys = base + where.keys;
	b.ids = base + where.ids;
	b.sorted_keys = base + where.sorted_keys;
	b.sorted_ids = base + where.sorted_ids;
	b.ranges = base + where.ranges;
	b.inner_links = base + where.inner_links;
	b.leaf_links = base + where.leaf_links;
	b.counters = base + where.counters;
	b.inner_at = base + where.inner_at;
	b.leaf_at = base + where.leaf_at;
	b.nodes = made + set.tree;
	inst_timed = false;
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_inst[0], s));
	launch_instance_keys(b, s);
	if (n >= 2u) {
		launch_build_sort(base + where.sort, where.sort_bytes, b.keys, b.sorted_keys, b.ids, b.sorted_ids, n, s);
		launch_instance_tree(b, s);
	}
	OCRT_HIP(hipGetLastError());
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_inst[1], s));
	inst_timed = true;
	have_inst_ms = false;
	// the one wait: the flag and the root record
	struct {
		uint32_t flag;
		InstanceNode root;
	} head{};
	static_assert(sizeof head == 36, "the flag's word lies directly in front of the root record");
	OCRT_HIP(hipMemcpyAsync(&head, made + set.flag, sizeof head, hipMemcpyDeviceToHost, s));
	OCRT_HIP(hipStreamSynchronize(s));
	if (head.flag)
		return false;  // (the launches wrote the spare allocation and the temporaries alone)
	std::swap(inst_device, inst_spare);
	inst_set = InstanceBuffers{ made + set.tree, made + set.inverse, 2u * n - 1u, made, made + set.bounds };
	setInstanceBox(head.root.lo, head.root.hi);
	inst_world.clear();
	inst_inverse.clear();
	inst_nodes.clear();
	inst_built = true;
	inst_built_n = n;
	inst_scene = scene;
	inst_current = rooted;
	return true;
}

void RayQueries::buildInstancesDevice(const float *world_from_object, uint32_t n, void *stream) {
	if (n > RT_INSTANCES_MAX)
		throw std::invalid_argument("more instances than RT_INSTANCES_MAX");
	if (n == 0) {
		clearInstances();
		return;
	}
	if (!world_from_object)
		throw std::invalid_argument("null transform array");
	if (!planInstancesOnDevice(world_from_object, n, stream))
		throw std::invalid_argument("instance transform refused: an entry that is not finite, a zero determinant, or an inverse that is not finite");
}

void RayQueries::buildInstancesHost(const float *world_from_object, uint32_t n) {
	if (n > RT_INSTANCES_MAX)
		throw std::invalid_argument("more instances than RT_INSTANCES_MAX");
	if (n > 0 && !world_from_object)
		throw std::invalid_argument("null transform array");
	if (n == 0) {
		clearInstances();
		return;
	}
	Arrays arrays;
	arrays.in(world_from_object, (size_t) n * 12u * sizeof(float));
	staged(Where::hostMemory(), arrays, [&](void *s) { buildInstancesDevice(world_from_object, n, s); });
}

void RayQueries::instanceWorld(float *out) {
	if (!out || instanceCount() == 0)
		return;
	if (!inst_built) {
		std::copy(inst_world.begin(), inst_world.end(), out);
		return;
	}
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	OCRT_HIP(hipMemcpy(out, inst_set.world, (size_t) inst_built_n * 12u * sizeof(float), hipMemcpyDeviceToHost));
}

void RayQueries::instanceInverses(float *out) {
	if (!out || instanceCount() == 0)
		return;
	if (!inst_built) {
		std::copy(inst_inverse.begin(), inst_inverse.end(), out);
		return;
	}
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	OCRT_HIP(hipMemcpy(out, inst_set.inverses, (size_t) inst_built_n * 12u * sizeof(float), hipMemcpyDeviceToHost));
}

void RayQueries::instanceBounds(float *out) {
	requireInstances("instance bounds");
	refreshInstances();
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	if (out)
		OCRT_HIP(hipMemcpy(out, inst_set.bounds, (size_t) instanceCount() * 4u * sizeof(float), hipMemcpyDeviceToHost));
}

float RayQueries::lastInstanceBuildMs() {
	if (!inst_timed)
		return 0.0f;
	if (!have_inst_ms) {
		OCRT_HIP(hipSetDevice(dev.deviceIndex()));
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_inst[1]));
		OCRT_HIP(hipEventElapsedTime(&last_inst_ms, (hipEvent_t) ev_inst[0], (hipEvent_t) ev_inst[1]));
		have_inst_ms = true;
	}
	return last_inst_ms;
}

void RayQueries::segments(bool closest, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                          QueryOutputs out, Where where, bool instanced, uint32_t *instance) {
	requireQuery(instanced, "segment query");
	if (n == 0)
		return;
	if (!closest) {  // (occlusion: the flags alone)
		static_cast<RecordOutputs &>(out) = RecordOutputs();
		instance = nullptr;
	}
	Arrays arrays;
	arrays.in(from4, (size_t) n * 16u).in(to4, (size_t) n * 16u).out(out.hit, n).records(out, n).out(instance, (size_t) n * 4u);
	staged(where, arrays, [&](void *stream) {
		const Target to = target(instanced);
		const Enqueue q = begin(enter(stream), from4, to4, n, n, flags, {}, true, to.box);
		launch_segments(dev.deviceScene()->buffers(), dev.params().node_count, to.set, closest, from4, to4, q.order, n, t_lo, t_hi, out, instance,
		                q.stream);
		end(q);
	});
}

void RayQueries::visibility(const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo, float t_hi, uint32_t flags,
                            VisibilityOutputs out, Where where, bool instanced) {
	requireQuery(instanced, "visibility query");
	if (np == 0 || nt == 0 || !out.any())
		return;
	const size_t row_bytes = (size_t) visibilityWords(nt) * sizeof(uint32_t);
	Arrays arrays;  // (host memory: the rows are staged whether they are copied back or not)
	arrays.in(points4, (size_t) np * 16u).in(targets4, (size_t) nt * 16u).scratch(out.mask, (size_t) np * row_bytes).out(out.count, (size_t) np * 4u);
	staged(where, arrays, [&](void *stream) {
		const Target to = target(instanced);
		// the POINTS are ordered, by position alone, from RT_QUERY_SORT_MIN of them on; the rows are the caller's, or scratch where
		// only the counts are wanted
		const Enqueue q = begin(enter(stream), points4, nullptr, np, np, flags, { Need{ out.mask ? nullptr : &vis_rows, (size_t) np * row_bytes } },
		                        false, to.box);
		launch_visibility(dev.deviceScene()->buffers(), dev.params().node_count, to.set, points4, np, targets4, nt, q.order, t_lo, t_hi,
		                  out.mask ? out.mask : (uint32_t *) vis_rows.ptr, out.count, q.stream);
		end(q);
	});
}

// What the closest-point walk may do follows from the scene: where every box holds the triangles beneath it -- an upload the
// packer found so, the refit rule's boxes after an update or a build -- each lane descends for a starting bound and boxes are
// passed by (kernels/nearest.hip.h); otherwise (damaged arrays) every leaf is tested.  After an update or a build whose
// coordinates only the device has seen, the word they left (checkCoordinates) decides it once more, in the kernel.
// `instanced` (include/rt_hip_instance_nearest.h): the same rules decide what the nested walk may do in both of its trees --
// the top-level boxes are made from the scene's root box and promise what it promises (kernels/instance_nearest.hip.h).
void RayQueries::nearest(const float *points4, uint32_t n, float max_distance, uint32_t flags, QueryOutputs out, Where where, bool instanced,
                         uint32_t *instance) {
	requireQuery(instanced, "closest-point query");
	if (n == 0)
		return;
	Arrays arrays;
	arrays.in(points4, (size_t) n * 16u).out(out.hit, n).records(out, n).out(instance, (size_t) n * 4u);
	staged(where, arrays, [&](void *stream) {
		const Target to = target(instanced);
		const std::shared_ptr<const DeviceScene> scene = dev.deviceScene();
		const bool counting = (nearest_debug & 4u) != 0u;
		const Enqueue q = begin(enter(stream), points4, nullptr, n, n, flags,
		                        { Need{ counting ? &nearest_counts : nullptr, 2u * sizeof(uint64_t) } }, false, to.box);
		launch_nearest(scene->buffers(), scene->nodeCount(), scene->triCount(), to.set, points4, q.order, n, max_distance, nearestWalk(*scene), out,
		               instance, flagged.lock() == scene ? coords_flag.ptr : nullptr, counting ? nearest_counts.ptr : nullptr, q.stream);
		nearest_counted = counting;
		end(q);
	});
}

// ---- signed distance queries (include/rt_hip_signed.h) ----
namespace {
constexpr size_t SIGN_REC_BYTES = 96u;                    // signed_point.h: SP_REC_FLOATS floats
constexpr uint64_t SIGNED_GRID_CHUNK = (uint64_t) 1 << 24;  // voxels per slab of the host form, as far as whole slices allow
}  // namespace

uint32_t RayQueries::nearestWalk(const DeviceScene &scene) const {
	uint32_t walk = scene.boxesEnclose() ? 3u : 0u;  // NEAREST_START | NEAREST_PRUNE
	if (nearest_debug & 1u)
		walk &= ~1u;
	if (nearest_debug & 2u)
		walk = 0u;
	return walk;
}

// The table of the current scene on `stream`, which has waited for the host's last query already: made in full where the
// topology is new -- the two sorts of the corners, the kept incidence, the sums; blocking: the sorts' scratch is let go
// before the call returns --, its sums redone where only the positions are.
const void *RayQueries::ensureSignTable(void *stream) {
	hipStream_t s = (hipStream_t) stream;
	const std::shared_ptr<const DeviceScene> scene = dev.deviceScene();
	const uint32_t leaves = scene->triCount();
	const size_t corners = (size_t) leaves * 3u;
	const bool topology = signed_scene.lock() != scene;
	if (!topology && sign_fresh)
		return sign_table.ptr;
	if (!topology) {
		OCRT_HIP(hipEventRecord((hipEvent_t) ev_sign[0], s));
		launch_sign_sums(sign_vertices.ptr, sign_edges.ptr, scene->buffers(), leaves, sign_table.ptr, s);
		OCRT_HIP(hipEventRecord((hipEvent_t) ev_sign[1], s));
		OCRT_HIP(hipGetLastError());
		sign_fresh = sign_timed = true;
		return sign_table.ptr;
	}
	const std::vector<uint32_t> *host_faces = scene->hostFaces();
	if (!scene->deviceFaces() && (!host_faces || host_faces->size() != corners))
		throw std::logic_error("signed distance query: the scene was uploaded without its faces");
	signed_scene.reset();
	grow(sign_table, (size_t) leaves * SIGN_REC_BYTES);
	grow(sign_vertices, corners * sizeof(uint32_t));
	grow(sign_edges, corners * sizeof(uint32_t));
	// the sorts' scratch: the faces (where only the host has them), keys and values in and out, rocPRIM's own
	const size_t words = round256(corners * 4u), wide = round256(corners * 8u), sort_bytes = sign_sort_bytes((uint32_t) corners);
	void *scratch = device_alloc(5u * words + 2u * wide + round256(sort_bytes));
	try {
		char *at = (char *) scratch;
		auto take = [&](size_t bytes) {
			void *p = at;
			at += bytes;
			return p;
		};
		void *faces = take(words), *vertex_keys = take(words), *vertex_sorted = take(words), *values = take(words), *values_sorted = take(words);
		void *edge_keys = take(wide), *edge_sorted = take(wide), *temporary = take(round256(sort_bytes));
		OCRT_HIP(hipEventRecord((hipEvent_t) ev_sign[0], s));
		const void *leaf_faces = scene->deviceFaces();
		if (!leaf_faces) {
			OCRT_HIP(hipMemcpyAsync(faces, host_faces->data(), corners * sizeof(uint32_t), hipMemcpyHostToDevice, s));
			leaf_faces = faces;
		}
		launch_sign_keys(leaf_faces, leaves, vertex_keys, edge_keys, values, s);
		launch_sign_sort(false, temporary, sort_bytes, vertex_keys, vertex_sorted, values, values_sorted, (uint32_t) corners, s);
		launch_sign_heads(false, vertex_sorted, values_sorted, leaves, sign_vertices.ptr, s);
		launch_sign_sort(true, temporary, sort_bytes, edge_keys, edge_sorted, values, values_sorted, (uint32_t) corners, s);
		launch_sign_heads(true, edge_sorted, values_sorted, leaves, sign_edges.ptr, s);
		launch_sign_sums(sign_vertices.ptr, sign_edges.ptr, scene->buffers(), leaves, sign_table.ptr, s);
		OCRT_HIP(hipEventRecord((hipEvent_t) ev_sign[1], s));
		OCRT_HIP(hipGetLastError());
		OCRT_HIP(hipStreamSynchronize(s));
	} catch (...) {
		device_free(scratch);
		throw;
	}
	device_free(scratch);
	signed_scene = scene;
	sign_fresh = sign_timed = true;
	return sign_table.ptr;
}

void RayQueries::prepareSigned(void *stream) {
	requireScene("signed distance query");
	hipStream_t s = (hipStream_t) enter(stream);
	(void) ensureSignTable(s);
	OCRT_HIP(hipStreamSynchronize(s));
}

float RayQueries::lastSignBuildMs() {
	if (!sign_timed)
		return 0.0f;
	float ms = 0.0f;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_sign[1]));
	OCRT_HIP(hipEventElapsedTime(&ms, (hipEvent_t) ev_sign[0], (hipEvent_t) ev_sign[1]));
	return ms;
}

void RayQueries::downloadSignTable(void *out) {
	prepareSigned(nullptr);
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	const size_t bytes = (size_t) dev.deviceScene()->triCount() * SIGN_REC_BYTES;
	if (out && bytes)
		OCRT_HIP(hipMemcpy(out, sign_table.ptr, bytes, hipMemcpyDeviceToHost));
}

void RayQueries::signedDistance(const float *points4, uint32_t n, float max_distance, uint32_t flags, QueryOutputs out, uint8_t *feature,
                                float *pseudonormal4, Where where) {
	requireScene("signed distance query");
	if (n == 0)
		return;
	Arrays arrays;
	arrays.in(points4, (size_t) n * 16u).out(out.hit, n).records(out, n).out(feature, n).out(pseudonormal4, (size_t) n * 16u);
	staged(where, arrays, [&](void *stream) {
		void *s = enter(stream);
		const void *table = ensureSignTable(s);  // (made here unless prepareSigned has been called: ahead of begin() either way)
		const std::shared_ptr<const DeviceScene> scene = dev.deviceScene();
		const Enqueue q = begin(s, points4, nullptr, n, n, flags, {}, false, nullptr);
		launch_signed(scene->buffers(), scene->nodeCount(), scene->triCount(), points4, q.order, n, max_distance, nearestWalk(*scene), out, feature,
		              pseudonormal4, table, flagged.lock() == scene ? coords_flag.ptr : nullptr, q.stream);
		end(q);
	});
}

void RayQueries::signedGridDevice(const float origin[3], const float spacing[3], const uint32_t dims[3], float max_distance, float *distance,
                                  uint32_t *leaf, void *stream, uint32_t z_first) {
	requireScene("signed distance query");
	if ((uint64_t) dims[0] * dims[1] * dims[2] == 0u)
		return;
	void *s = enter(stream);
	const void *table = ensureSignTable(s);
	const std::shared_ptr<const DeviceScene> scene = dev.deviceScene();
	const Enqueue q = begin(s, nullptr, nullptr, 0u, 0u, QUERY_NO_SORT, {}, false, nullptr);  // (no points, no order, no sort)
	launch_signed_grid(scene->buffers(), scene->nodeCount(), scene->triCount(), origin, spacing, dims[0], dims[1], dims[2], z_first, max_distance,
	                   nearestWalk(*scene), distance, leaf, table, flagged.lock() == scene ? coords_flag.ptr : nullptr, q.stream);
	end(q);
}

void RayQueries::signedGridHost(const float origin[3], const float spacing[3], const uint32_t dims[3], float max_distance, float *distance,
                                uint32_t *leaf) {
	requireScene("signed distance query");
	const uint64_t slice = (uint64_t) dims[0] * dims[1];
	if (slice * dims[2] == 0u)
		return;
	// slab by slab through the staging buffer, so that it holds one slab's voxels, not the grid's
	const uint32_t per_slab = (uint32_t) std::min<uint64_t>(dims[2], std::max<uint64_t>(1u, SIGNED_GRID_CHUNK / slice));
	float ms = 0.0f;
	for (uint32_t first = 0; first < dims[2]; first += per_slab) {
		const uint32_t slab[3] = { dims[0], dims[1], std::min(per_slab, dims[2] - first) };
		const size_t voxels = (size_t) (slice * slab[2]), offset = (size_t) (slice * first);
		float *slab_distance = distance ? distance + offset : nullptr;
		uint32_t *slab_leaf = leaf ? leaf + offset : nullptr;
		Arrays arrays;
		arrays.out(slab_distance, voxels * 4u).out(slab_leaf, voxels * 4u);
		staged(Where::hostMemory(), arrays,
		       [&](void *s) { signedGridDevice(origin, spacing, slab, max_distance, slab_distance, slab_leaf, s, first); });
		ms += lastMs();
	}
	last_ms = ms;  // (every slab's events have been read: the call's time is their sum)
	have_ms = true;
}

void RayQueries::setNearestWalk(uint32_t debug_flags) {
#ifndef OCRT_DEBUG_KNOBS
	if (debug_flags != 0u)
		throw std::logic_error("the closest-point walk's switches and counters are the A/B build's (-DOCRT_DEBUG_KNOBS)");
#endif
	nearest_debug = debug_flags & 7u;
}

void RayQueries::lastNearestCounts(uint64_t counts[2]) {
	counts[0] = counts[1] = 0u;
	if (!nearest_counted || !nearest_counts.ptr)
		return;
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	OCRT_HIP(hipMemcpy(counts, nearest_counts.ptr, 2u * sizeof(uint64_t), hipMemcpyDeviceToHost));
}

// Behind an update's or a build's own launches, on their stream: the word the closest-point queries of `scene` read.
void RayQueries::checkCoordinates(const std::shared_ptr<const DeviceScene> &scene, const float *vertices4, uint32_t num_vertices, void *stream) {
	launch_nearest_coordinates(vertices4, num_vertices, coords_flag.ptr, stream);
	flagged = scene;
}

void RayQueries::multihit(const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k, uint32_t flags,
                          MultiHitOutputs out, Where where, bool instanced, uint32_t *instance) {
	if (instanced)
		requireInstances("instanced multi-hit query");
	requireSlots(k);
	if (!instanced)
		instance = nullptr;
	// without a slot array the lists are not wanted: the count-only walk
	const uint32_t slots = out.anySlot() || instance ? k : 0u;
	if (n == 0 || (slots == 0 && !out.count))
		return;
	Arrays arrays;
	arrays.in(origins4, (size_t) n * 16u).in(directions4, (size_t) n * 16u).out(out.count, (size_t) n * 4u).records(out, (size_t) n * k);
	arrays.out(instance, (size_t) n * k * 4u);
	staged(where, arrays, [&](void *stream) {
		const Target to = target(instanced);
		const Enqueue q = begin(enter(stream), origins4, directions4, n, n, flags,
		                        { Need{ slots ? &list : nullptr, (size_t) n * slots * (instanced ? 12u : 8u) } }, false, to.box);
		launch_multihit(dev.deviceScene()->buffers(), dev.params().node_count, to.set, origins4, directions4, q.order, n, max_distance, slots,
		                list.ptr, out, instance, q.stream);
		end(q);
	});
}

uint32_t RayQueries::aoRaysPerPoint(const DeviceRenderer &renderer) {
	const KernelParams &kp = renderer.params();
	const bool available = renderer.sceneReady() && renderer.deviceScene() && kp.ao_mode != AO_NONE && kp.ao_dirs > 0 &&
	                       renderer.deviceScene()->aoDirs() == kp.ao_dirs;
	return available ? kp.ao_dirs : 0u;
}
uint32_t RayQueries::aoDivisor(const DeviceRenderer &renderer) { return aoRaysPerPoint(renderer) ? renderer.params().ao_divisor : 0u; }

void RayQueries::ao(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags, float *ao,
                    uint32_t *occluded, Where where, bool instanced) {
	if (instanced)
		requireInstances("instanced ambient-occlusion query");
	requireAo();
	if (n == 0 || (!ao && !occluded))
		return;
	Arrays arrays;  // (host memory: the counts are staged whether they are copied back or not: the kernel counts into them)
	arrays.in(points4, (size_t) n * 16u).in(normals4, (size_t) n * 16u).scratch(occluded, (size_t) n * 4u).in(seeds, (size_t) n * 4u);
	arrays.out(ao, (size_t) n * 4u);
	staged(where, arrays, [&](void *stream) {
		const Target to = target(instanced);
		// the POINTS are ordered (key: point and normal) from as many on as make RT_QUERY_SORT_MIN rays
		const Enqueue q = begin(enter(stream), points4, normals4, n, (uint64_t) n * dev.params().ao_dirs, flags,
		                        { Need{ occluded ? nullptr : &ao_hits, (size_t) n * sizeof(uint32_t) } }, false, to.box);
		aoEnqueue(q, points4, normals4, seeds, q.order, n, occluded ? occluded : (uint32_t *) ao_hits.ptr, ao, instanced);
		end(q);
	});
}

void RayQueries::aoEnqueue(const Enqueue &q, const float *points4, const float *normals4, const uint32_t *seeds, const void *order,
                           uint32_t n, uint32_t *count, float *ao, bool instanced) {
	const KernelParams &kp = dev.params();
	launch_ao_query(dev.deviceScene()->buffers(), kp.node_count, instanced ? &inst_set : nullptr, kp.ao_mode, kp.ao_dirs, kp.ao_divisor,
	                kp.ao_max_distance, points4, normals4, seeds, order, n, count, ao, q.stream);
}

void RayQueries::directional(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags,
                             DirectionalOutputs out, Where where, bool instanced) {
	if (instanced)
		requireInstances("instanced directional occlusion query");
	requireAo();
	if (n == 0 || !out.any())
		return;
	const size_t row_bytes = (size_t) aoMaskWords(dev) * sizeof(uint32_t);
	Arrays arrays;  // (host memory: the rows are staged whether they are copied back or not)
	arrays.in(points4, (size_t) n * 16u).in(normals4, (size_t) n * 16u).in(seeds, (size_t) n * 4u).scratch(out.mask, (size_t) n * row_bytes);
	arrays.out(out.occluded, (size_t) n * 4u).out(out.ao, (size_t) n * 4u).out(out.bent, (size_t) n * 12u);
	staged(where, arrays, [&](void *stream) {
		const Target to = target(instanced);
		const KernelParams &kp = dev.params();
		// the POINTS are ordered as for ao; the rows are the caller's, or scratch where only what is made of them is wanted
		const Enqueue q = begin(enter(stream), points4, normals4, n, (uint64_t) n * kp.ao_dirs, flags,
		                        { Need{ out.mask ? nullptr : &ao_rows, (size_t) n * row_bytes } }, false, to.box);
		launch_ao_directional(dev.deviceScene()->buffers(), kp.node_count, to.set, kp.ao_mode, kp.ao_dirs, kp.ao_divisor, kp.ao_max_distance, points4,
		                      normals4, seeds, q.order, n, out.mask ? out.mask : (uint32_t *) ao_rows.ptr, out.occluded, out.ao, out.bent,
		                      q.stream);
		end(q);
	});
}

void RayQueries::aoRays(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, float *origins4, float *directions4,
                        Where where) {
	requireAo();
	if (n == 0 || (!origins4 && !directions4))
		return;
	const KernelParams &kp = dev.params();
	Arrays arrays;
	arrays.in(points4, (size_t) n * 16u).in(normals4, (size_t) n * 16u).in(seeds, (size_t) n * 4u).out(origins4, (size_t) n * 16u);
	arrays.out(directions4, (size_t) n * kp.ao_dirs * 16u);
	staged(where, arrays, [&](void *stream) {
		const Enqueue q = begin(enter(stream), nullptr, nullptr, n, (uint64_t) n * kp.ao_dirs, QUERY_NO_SORT);  // (nothing is walked: no order)
		launch_ao_rays(dev.deviceScene()->buffers(), kp.ao_mode, kp.ao_dirs, points4, normals4, seeds, n, origins4, directions4, q.stream);
		end(q);
	});
}

// What a layers call may ask of this host; returns whether it needs the ambient-occlusion step (`ao`, or `value` on a host
// whose options have ambient occlusion on).
bool RayQueries::requireLayers(const LayerOutputs &out) const { return requireFrameRays(out.ao != nullptr, out.ao || out.value); }

// ... `ao`: that layer is asked for; `product`: something made of it -- or, without it, of the head-light term alone -- is.
bool RayQueries::requireFrameRays(bool ao, bool product) const {
	requireScene("frame layers");
	const KernelParams &kp = dev.params();
	if (kp.part.nranks > 1)
		throw std::logic_error("frame layers on a band-partitioned host: it renders a part of the image only");
	const uint32_t per_point = aoRaysPerPoint(dev);
	if (ao && per_point == 0)
		throw std::logic_error("the ao layer on a host whose options have ambient occlusion off");
	const bool with_ao = per_point != 0 && product;
	const uint64_t n = (uint64_t) kp.width * kp.height;
	if (n > QUERY_MAX_RAYS || (with_ao && n > QUERY_MAX_RAYS / per_point))
		throw std::invalid_argument(with_ao ? "more sub-pixels than RT_QUERY_MAX_RAYS / rays per point: ask for neither ao nor value"
		                                    : "more sub-pixels than RT_QUERY_MAX_RAYS");
	return with_ao;
}

// (a piece that is not needed has no bytes; with nothing needed, `bytes` is 0)
RayQueries::ChunkScratch RayQueries::chunkScratch(size_t poses, size_t entries, bool listing, size_t products) {
	ChunkScratch c{};
	auto piece = [&c](size_t bytes) {
		const size_t here = c.bytes;
		c.bytes += round16(bytes);
		return here;
	};
	const size_t listable = listing ? entries : 0u;
	c.poses = piece(poses * sizeof(CameraPose));
	c.listed = piece(listing ? sizeof(uint32_t) : 0u);
	c.points = piece(entries * 16u);
	c.normals = piece(entries * 16u);
	c.seeds = piece(listable * 4u);
	c.order = piece(listable * 4u);
	c.flags = piece(listable);
	c.sums = piece((listable + 1023u) / 1024u * 4u);
	c.product = piece(products * 4u);
	return c;
}

uint32_t RayQueries::castChunk(const Enqueue &q, const ChunkScratch &at, bool listing, const void *poses, uint32_t views,
                               const LayerOutputs &to, float *product, bool with_ao, bool instanced, uint32_t *instance) {
	const KernelParams &kp = dev.params();
	hipStream_t s = (hipStream_t) q.stream;
	char *const base = (char *) this->views.ptr;
	ViewList list{};
	if (with_ao) {
		list.points = base + at.points;
		list.normals = base + at.normals;
	}
	if (with_ao && listing) {
		list.flags = (unsigned char *) (base + at.flags);
		list.seeds = (uint32_t *) (base + at.seeds);
		list.sums = (uint32_t *) (base + at.sums);
		list.order = (uint32_t *) (base + at.order);
		list.listed = (uint32_t *) (base + at.listed);
	}
	// (without the ambient-occlusion step `value` is the head-light term itself)
	launch_layers(dev.deviceScene()->buffers(), kp, instanced ? &inst_set : nullptr, poses, dev.camera(), dev.cameraIsSet(), views, to, instance,
	              with_ao ? nullptr : product, to.ao, product, with_ao ? &list : nullptr, s);
	if (!with_ao)
		return 0u;
	// the reference's ambient_occlusion(position, normal, index) in index order: of every sub-pixel -- seed i for point i --
	// or of the hit ones alone, whose number then sizes the launch
	uint32_t *const count = (uint32_t *) ao_hits.ptr;
	uint32_t entries = views * kp.width * kp.height;
	if (listing) {
		// (the step's counts go by sub-pixel: all the chunk's are cleared -- while the host waits --, the hit ones are
		// counted into)
		uint32_t *const listed_host = (uint32_t *) pinned;
		OCRT_HIP(hipMemsetAsync(count, 0, (size_t) entries * sizeof(uint32_t), s));
		OCRT_HIP(hipMemcpyAsync(listed_host, list.listed, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		OCRT_HIP(hipStreamSynchronize(s));
		if (*listed_host > entries)
			throw DeviceError("multi-view rendering: more sub-pixels listed than the chunk holds");
		entries = *listed_host;
	}
	aoEnqueue(q, (const float *) list.points, (const float *) list.normals, list.seeds, list.order, entries, count, nullptr, instanced);
	launch_views_scatter(list, count, kp.ao_divisor, to.ao, product, entries, s);
	return entries;
}

void RayQueries::layers(LayerOutputs out, Where where) {
	const bool with_ao = requireLayers(out);
	const KernelParams &kp = dev.params();
	const uint32_t n = kp.width * kp.height;
	if (n == 0 || !out.any())
		return;
	Arrays arrays;
	arrays.layers(out, n);
	staged(where, arrays, [&](void *stream) {
		// one view, the host's own pose: with the ambient-occlusion step every sub-pixel is an entry of it -- nothing is
		// listed, nothing read back, the call only enqueues
		const ChunkScratch at = chunkScratch(0u, with_ao ? n : 0u, false, 0u);
		const Enqueue q =
		    begin(enter(stream), nullptr, nullptr, n, n, QUERY_NO_SORT,
		          { Need{ with_ao ? &views : nullptr, at.bytes }, Need{ with_ao ? &ao_hits : nullptr, (size_t) n * sizeof(uint32_t) } });
		(void) castChunk(q, at, false, nullptr, 1u, out, out.value, with_ao);
		end(q);
	});
}

// What a views call may ask of this host: what a layers call may, with the image counted among the layers made of `value`.
bool RayQueries::requireViews(const ViewOutputs &out) const { return requireFrameRays(out.ao != nullptr, out.ao || out.value || out.image); }

// Views per chunk: as many as keep a chunk's sub-pixels -- with the ambient-occlusion step: their rays, were all of them
// hit -- within what one query takes (requireViews: one view does), or the debug limit.
uint32_t RayQueries::viewsPerChunk(bool with_ao) const {
	const KernelParams &kp = dev.params();
	const uint64_t n = (uint64_t) kp.width * kp.height, most = with_ao ? QUERY_MAX_RAYS / aoRaysPerPoint(dev) : QUERY_MAX_RAYS;
	const uint32_t fit = (uint32_t) std::min<uint64_t>(std::max<uint64_t>(most / (n ? n : 1u), 1u), VIEWS_MAX_CHUNK);
	return views_chunk ? std::min(views_chunk, fit) : fit;
}

// `out` from view `view` on.
ViewOutputs RayQueries::viewsFrom(const ViewOutputs &out, size_t view, const KernelParams &kp, size_t image_bytes) {
	const size_t first = view * (size_t) kp.width * kp.height;
	ViewOutputs at = out;
	auto advance = [](auto *&p, size_t by) {
		if (p)
			p += by;
	};
	advance(at.hit, first);
	advance(at.distance, first);
	advance(at.leaf, first);
	advance(at.barycentric, 3u * first);
	advance(at.position, 3u * first);
	advance(at.normal, 3u * first);
	advance(at.direction, 3u * first);
	advance(at.shade, first);
	advance(at.ao, first);
	advance(at.value, first);
	advance(at.image, view * image_bytes);
	return at;
}

void RayQueries::viewsDevice(const CameraPose *cameras, uint32_t views, const ViewOutputs &out, void *stream) {
	viewsCall(false, cameras, views, out, nullptr, stream);
}

void RayQueries::viewsHost(const CameraPose *cameras, uint32_t views, const ViewOutputs &host) { viewsStaged(false, cameras, views, host, nullptr); }

// ---- instanced views (include/rt_hip_instance_views.h) ----
void RayQueries::instanceViewsDevice(const CameraPose *cameras, uint32_t views, const ViewOutputs &out, uint32_t *instance, void *stream) {
	viewsCall(true, cameras, views, out, instance, stream);
}

void RayQueries::instanceViewsHost(const CameraPose *cameras, uint32_t views, const ViewOutputs &host, uint32_t *instance) {
	viewsStaged(true, cameras, views, host, instance);
}

void RayQueries::viewsCall(bool instanced, const CameraPose *cameras, uint32_t views, const ViewOutputs &out, uint32_t *instance,
                           void *stream) {
	if (instanced)
		requireInstances("instanced views");
	const bool with_ao = requireViews(out);
	const KernelParams &kp = dev.params();
	const RayTracer &rt = dev.rayTracer();
	const uint32_t n = kp.width * kp.height, grid = RayTracer::gridSize(rt.options.nSuperSamples);
	if (views == 0 || n == 0 || !(out.any() || instance))
		return;
	if (instanced)
		refreshInstances();
	const uint32_t per_chunk = std::min(viewsPerChunk(with_ao), views);
	const size_t most = (size_t) per_chunk * n, image_bytes = (size_t) rt.options.width * rt.options.height;
	// the poses: into host memory of this host's own that the copies may read after the call has returned -- once the
	// call before, which may still be reading it, is over
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	const size_t pose_bytes = (size_t) views * sizeof(CameraPose);
	if (PINNED_HEAD + pose_bytes > pinned_bytes) {
		if (pinned)
			(void) hipHostFree(pinned);
		pinned = nullptr;
		pinned_bytes = 0;
		OCRT_HIP(hipHostMalloc(&pinned, PINNED_HEAD + pose_bytes, hipHostMallocDefault));
		pinned_bytes = PINNED_HEAD + pose_bytes;
	}
	const CameraPose *const poses_host = (const CameraPose *) ((char *) pinned + PINNED_HEAD);
	std::memcpy((char *) pinned + PINNED_HEAD, cameras, pose_bytes);
	// a chunk's scratch: its poses, then -- as far as the call needs them -- the list of its hit sub-pixels and the chunk's
	// float images where the caller has no `value` array for them
	const bool own_product = out.image && !out.value;
	const ChunkScratch at = chunkScratch(per_chunk, with_ao ? most : 0u, true, own_product ? most : 0u);
	const Enqueue q = begin(enter(stream), nullptr, nullptr, n, n, QUERY_NO_SORT,
	                        { Need{ &this->views, at.bytes }, Need{ with_ao ? &ao_hits : nullptr, most * sizeof(uint32_t) } });
	char *const base = (char *) this->views.ptr;
	hipStream_t s = (hipStream_t) q.stream;
	ViewsDone done;
	done.views = views;
	for (uint32_t first = 0; first < views; first += per_chunk, ++done.chunks) {
		const uint32_t chunk = std::min(per_chunk, views - first);
		const ViewOutputs to = viewsFrom(out, first, kp, image_bytes);
		// (`product`: the chunk's float images -- the caller's `value`, or scratch for the 8-bit images alone)
		float *const product = own_product ? (float *) (base + at.product) : to.value;
		OCRT_HIP(hipMemcpyAsync(base + at.poses, poses_host + first, (size_t) chunk * sizeof(CameraPose), hipMemcpyHostToDevice, s));
		done.ao_points += castChunk(q, at, true, base + at.poses, chunk, to, product, with_ao, instanced,
		                            instance ? instance + (size_t) first * n : nullptr);
		if (to.image)
			launch_views_resize(product, to.image, kp, rt.options.width, rt.options.height, grid, chunk, s);
	}
	end(q);
	last_views = done;
}

void RayQueries::viewsStaged(bool instanced, const CameraPose *cameras, uint32_t views, const ViewOutputs &host, uint32_t *instance) {
	if (instanced)
		requireInstances("instanced views");
	const bool with_ao = requireViews(host);
	const KernelParams &kp = dev.params();
	const RayTracer &rt = dev.rayTracer();
	const size_t n = (size_t) kp.width * kp.height, image_bytes = (size_t) rt.options.width * rt.options.height;
	if (views == 0 || n == 0 || !(host.any() || instance))
		return;
	// chunk by chunk through the staging buffer, so that it holds one chunk's outputs, not the call's
	const uint32_t per_chunk = std::min(viewsPerChunk(with_ao), views);
	ViewsDone done;
	float ms = 0.0f;
	for (uint32_t first = 0; first < views; first += per_chunk) {
		const size_t chunk = std::min(per_chunk, views - first), m = chunk * n;
		ViewOutputs to = viewsFrom(host, first, kp, image_bytes);
		uint32_t *to_instance = instance ? instance + (size_t) first * n : nullptr;  // (the instanced form's alone)
		Arrays arrays;
		arrays.layers(to, m).out(to.image, chunk * image_bytes).out(to_instance, m * 4u);
		staged(Where::hostMemory(), arrays, [&](void *s) { viewsCall(instanced, cameras + first, (uint32_t) chunk, to, to_instance, s); });
		ms += lastMs();
		done.views += last_views.views;
		done.chunks += last_views.chunks;
		done.ao_points += last_views.ao_points;
	}
	last_views = done;
	last_ms = ms;  // (every chunk's events have been read: the call's time is their sum)
	have_ms = true;
}

// The update is a query as far as ordering goes: it waits for the one before it by ev_stop and leaves ev_stop behind for the
// one after it -- whatever streams they run on.  The frames of the renderer's own stream read the records too: the update
// waits for that stream's tail on the device (an event of its own; nothing blocks the host).
void RayQueries::updateDevice(const float *vertices4, const float *vnormals4, uint32_t num_vertices, void *stream) {
	const char *why = "";
	DeviceScene *const scene = dev.updatableScene(&why);
	if (!scene)
		throw std::logic_error(why);
	if (num_vertices != scene->vertexCount())
		throw std::invalid_argument("vertex update: the number of vertices differs from the upload's (the topology stays: every position is replaced)");
	if (!vertices4)
		throw std::invalid_argument("vertex update: null vertex array");
	hipStream_t s = (hipStream_t) enter(stream);
	if (s != (hipStream_t) dev.streamHandle()) {
		OCRT_HIP(hipEventRecord((hipEvent_t) ev_frames, (hipStream_t) dev.streamHandle()));
		OCRT_HIP(hipStreamWaitEvent(s, (hipEvent_t) ev_frames, 0));
	}
	// (from here on the records are the new positions' as far as the host is concerned, whether the launches below succeed
	// or not: no frame may lean on the old walk array again, and the sort's box is read afresh)
	dev.markSceneUpdated();
	boxed.reset();
	inst_current = false;
	sign_fresh = false;  // (the sign table's sums are the old positions': redone by the next signed query, from the kept incidence)
	grow(coords_flag, sizeof(uint32_t));
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_start, s));
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_update_start, s));
	scene->updateVertices(vertices4, vnormals4, dev.refitGroup(), s);
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_update_stop, s));
	checkCoordinates(dev.deviceScene(), vertices4, num_vertices, s);  // (for the closest-point queries; not part of the update's own time)
	update_timed = true;
	have_update_ms = false;
	end(Enqueue{ s, nullptr });
}

void RayQueries::updateHost(const float *vertices4, const float *vnormals4, uint32_t num_vertices) {
	const char *why = "";
	DeviceScene *const scene = dev.updatableScene(&why);
	if (!scene)
		throw std::logic_error(why);
	if (num_vertices != scene->vertexCount())
		throw std::invalid_argument("vertex update: the number of vertices differs from the upload's (the topology stays: every position is replaced)");
	if (!vertices4)
		throw std::invalid_argument("vertex update: null vertex array");
	for (size_t i = 0; i < (size_t) num_vertices; ++i)
		for (unsigned k = 0; k < 3; ++k)
			if (!(std::fabs(vertices4[4 * i + k]) <= 1.0e37f))  // (false for a NaN too)
				throw std::invalid_argument("vertex update: a coordinate is not finite or exceeds 1e37 (nothing was written)");
	if (num_vertices == 0)
		return;
	Arrays arrays;
	arrays.in(vertices4, (size_t) num_vertices * 16u).in(vnormals4, (size_t) num_vertices * 16u);
	staged(Where::hostMemory(), arrays, [&](void *s) { updateDevice(vertices4, vnormals4, num_vertices, s); });
}

float RayQueries::lastUpdateMs() {
	if (!update_timed)
		return 0.0f;
	if (!have_update_ms) {
		OCRT_HIP(hipSetDevice(dev.deviceIndex()));
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_update_stop));
		OCRT_HIP(hipEventElapsedTime(&last_update_ms, (hipEvent_t) ev_update_start, (hipEvent_t) ev_update_stop));
		have_update_ms = true;
	}
	return last_update_ms;
}

// A build orders itself as an update does.  Its launches leave the renderer's scene alone -- they write scratch and the new
// scene's own allocations --, so a refused build changes nothing; an accepted one replaces the scene once its records are
// enqueued, and the queries after it wait for them by ev_stop.
void RayQueries::buildDevice(const float *vertices4, const float *vnormals4, uint32_t num_vertices, const uint32_t *faces, uint32_t num_faces,
                             void *stream) {
	if (dev.sceneIsShared())
		throw std::logic_error("build on a host whose scene on the device is shared with other hosts (one copy, many readers: upload a scene of the host's own)");
	if (!vertices4 || !vnormals4 || !faces)
		throw std::invalid_argument("build: null vertex, normal or face array (the device does not compute vertex normals)");
	if (num_faces == 0 || num_vertices == 0)
		throw std::invalid_argument("build: no faces, or no vertices");
	if (num_faces >= (1u << 25))
		throw std::invalid_argument("build: scene too large for 32-bit device offsets");
	hipStream_t s = (hipStream_t) enter(stream);
	if (s != (hipStream_t) dev.streamHandle()) {
		OCRT_HIP(hipEventRecord((hipEvent_t) ev_frames, (hipStream_t) dev.streamHandle()));
		OCRT_HIP(hipStreamWaitEvent(s, (hipEvent_t) ev_frames, 0));
	}
	grow(build, DeviceScene::buildScratchBytes(num_faces));
	grow(coords_flag, sizeof(uint32_t));
	build_timed = false;
	std::shared_ptr<DeviceScene> made = DeviceScene::build(dev.deviceIndex(), dev.options(), vertices4, vnormals4, num_vertices, faces, num_faces,
	                                                       dev.refitGroup(), build.ptr, s, ev_build, &last_build_ms[2]);
	build_timed = true;
	have_build_ms = false;
	dev.adoptBuilt(std::move(made));  // (waits for the renderer's own stream and lets the old scene go)
	boxed.reset();
	inst_current = false;
	checkCoordinates(dev.deviceScene(), vertices4, num_vertices, s);
	OCRT_HIP(hipEventRecord((hipEvent_t) ev_start, s));
	end(Enqueue{ s, nullptr });
}

void RayQueries::buildHost(const float *vertices4, const float *vnormals4, uint32_t num_vertices, const uint32_t *faces, uint32_t num_faces) {
	if (dev.sceneIsShared())
		throw std::logic_error("build on a host whose scene on the device is shared with other hosts (one copy, many readers: upload a scene of the host's own)");
	if (!vertices4 || !vnormals4 || !faces)
		throw std::invalid_argument("build: null vertex, normal or face array");
	if (num_faces == 0 || num_vertices == 0)
		throw std::invalid_argument("build: no faces, or no vertices");
	if (num_faces >= (1u << 25))
		throw std::invalid_argument("build: scene too large for 32-bit device offsets");
	for (size_t i = 0; i < (size_t) num_faces * 3; ++i)
		if (faces[i] >= num_vertices)
			throw std::invalid_argument("build: face references a vertex out of range (nothing was written)");
	for (size_t i = 0; i < (size_t) num_vertices; ++i)
		for (unsigned k = 0; k < 3; ++k)
			if (!(std::fabs(vertices4[4 * i + k]) <= 1.0e37f))  // (false for a NaN too)
				throw std::invalid_argument("build: a coordinate is not finite or exceeds 1e37 (nothing was written)");
	Arrays arrays;
	arrays.in(vertices4, (size_t) num_vertices * 16u).in(vnormals4, (size_t) num_vertices * 16u).in(faces, (size_t) num_faces * 12u);
	staged(Where::hostMemory(), arrays, [&](void *s) { buildDevice(vertices4, vnormals4, num_vertices, faces, num_faces, s); });
}

void RayQueries::lastBuildTimes(float ms[3]) {
	ms[0] = ms[1] = ms[2] = 0.0f;
	if (!build_timed)
		return;
	if (!have_build_ms) {
		OCRT_HIP(hipSetDevice(dev.deviceIndex()));
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_build[3]));
		OCRT_HIP(hipEventElapsedTime(&last_build_ms[0], (hipEvent_t) ev_build[0], (hipEvent_t) ev_build[1]));
		OCRT_HIP(hipEventElapsedTime(&last_build_ms[1], (hipEvent_t) ev_build[2], (hipEvent_t) ev_build[3]));
		have_build_ms = true;
	}
	for (int k = 0; k < 3; ++k)
		ms[k] = last_build_ms[k];
}

float RayQueries::lastBuildMs() {
	float ms[3];
	lastBuildTimes(ms);
	return ms[0] + ms[1];
}

void RayQueries::downloadRecords(void *nodes_out, void *tris_out, void *shade_out) {
	requireScene("record download");
	OCRT_HIP(hipSetDevice(dev.deviceIndex()));
	if (timed)
		OCRT_HIP(hipEventSynchronize((hipEvent_t) ev_stop));
	OCRT_HIP(hipStreamSynchronize((hipStream_t) dev.streamHandle()));
	const DeviceScene &scene = *dev.deviceScene();
	const SceneBuffers b = scene.buffers();
	if (nodes_out && scene.nodeCount())
		OCRT_HIP(hipMemcpy(nodes_out, b.nodes, (size_t) scene.nodeCount() * sizeof(NodeRec), hipMemcpyDeviceToHost));
	if (tris_out && scene.triCount())
		OCRT_HIP(hipMemcpy(tris_out, b.tris, (size_t) scene.triCount() * sizeof(TriRec), hipMemcpyDeviceToHost));
	if (shade_out && scene.triCount())
		OCRT_HIP(hipMemcpy(shade_out, b.shade, (size_t) scene.triCount() * sizeof(ShadeRec), hipMemcpyDeviceToHost));
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
