// device_scene.cc -- ocrt::DeviceScene (device_renderer.h): one uploaded scene on one GPU, shared by every render host of
// that GPU.
#include <limits>
#include <mutex>

#include "device_internal.h"
#include "refit.h"

namespace ocrt {

namespace {
// the allocation made ahead of time by DeviceScene::reserve, waiting for the scene it was made for
std::mutex reserved_mutex;
void *reserved_arena = nullptr;
size_t reserved_bytes = 0;
int reserved_device = -1;

size_t round_up(size_t bytes) { return (bytes + 255) & ~(size_t) 255; }
}  // namespace

std::vector<float> DeviceScene::takeOptions(const RayTracer::Options &opts) {
	std::vector<float> table;
	ao_on = opts.enableAO && opts.aoNumSamples > 0;
	ao_method = (int) opts.aoMethod;
	ao_samples = opts.aoNumSamples;
	ao_alpha_min = opts.aoAlphaMin;
	ao_alpha_max = opts.aoAlphaMax;
	if (ao_on) {
		if (opts.aoMethod == RayTracer::AmbientOcclusionMethod::UNIFORM) {
			// The reference's order, ring by ring.  (The occlusion count of a hit is a sum over the directions, so the order is
			// free: while a workgroup's four waves took FIXED quarters of a tile's directions the table was dealt round-robin
			// to the quarters so that they cost about the same; with the claim's cursor -- kernels.hip, ao_kernel -- the waves
			// balance themselves, and neighbouring directions cast at the same time are worth 0.5-2 %.)
			table = uniform_ao_table(opts.aoNumSamples, opts.aoAlphaMin, opts.aoAlphaMax);
			ao_dirs = (uint32_t) (table.size() / 4);
		} else {
			// RANDOM casts the normal ray plus AO_NUM_SAMPLES + 1 random ones (reference :260-275)
			ao_dirs = opts.aoNumSamples + 2;
		}
	}
	walk_distance = ao_on ? kernel_float(opts.aoMaxDistance) : 0.0f;
	return table;
}

void DeviceScene::finishTable(const RayTracer::Options &opts, size_t table_bytes) {
#ifdef OCRT_OCML_BUILTINS
	// (test-only build: the table as the reference kernel's own float trigonometry makes it on this device, kernels.hip)
	if (table_bytes && opts.aoMethod == RayTracer::AmbientOcclusionMethod::UNIFORM &&
	    ocml_ao_table(d_ao, opts.aoNumSamples, opts.aoAlphaMin, opts.aoAlphaMax, ao_dirs) != ao_dirs)
		throw DeviceError("the device's trigonometry counts another number of ambient-occlusion directions than the host's");
#else
	(void) opts;
	(void) table_bytes;
#endif
}

std::shared_ptr<DeviceScene> DeviceScene::create(int device, const PackedScene &scene, const RayTracer::Options &opts, bool for_a_stream,
                                                 const float *eye) {
	UploadClock clock;
	OCRT_HIP(hipSetDevice(device));
	std::shared_ptr<DeviceScene> out(new DeviceScene());
	out->device_index = device;
	const std::vector<float> table = out->takeOptions(opts);
	if (eye)
		for (unsigned k = 0; k < 3; ++k)
			out->walk_eye[k] = eye[k];
	// (a prepared array is taken if it was made for this distance, for this eye and for at least as much as is wanted now)
	const std::shared_ptr<const WalkArray> made = (scene.walk && scene.walk_max_distance == out->walk_distance && same_eye(scene.walk->eye, eye) &&
	                                               (scene.walk_for_a_stream || !for_a_stream))
	                                                  ? scene.walk
	                                                  : std::make_shared<const WalkArray>(make_walk_array(scene, out->walk_distance, for_a_stream, eye));
	const WalkArray &walk = *made;
	clock.mark("direction table + walk array (made here unless prepared)");
	out->scene_facts_ = scene_facts(scene, walk);
	out->node_count = (uint32_t) scene.nodes.size();
	out->tri_count = (uint32_t) scene.tris.size();
	const size_t nodes_bytes = scene.nodes.size() * sizeof(NodeRec);
	const size_t tris_bytes = scene.tris.size() * sizeof(TriRec);
	const size_t shade_bytes = scene.shade.size() * sizeof(ShadeRec);
	const size_t ao_bytes = table.size() * sizeof(float);
	// One allocation for the five arrays (each starts on a 256-byte boundary) -- the one made ahead of time if there is
	// one and it is large enough.  One node of zero padding behind the exact nodes: the shared walk fetches a node
	// together with its successor.
	const size_t walk_bytes = walk.nodes.size() * sizeof(NodeRec);
	const size_t need = round_up(nodes_bytes + sizeof(NodeRec)) + round_up(walk_bytes) + round_up(tris_bytes) + round_up(shade_bytes) +
	                    round_up(ao_bytes) + 256;
	{
		std::lock_guard<std::mutex> lock(reserved_mutex);
		if (reserved_arena && reserved_device == device && reserved_bytes >= need) {
			out->arena = reserved_arena;
		} else if (reserved_arena && reserved_device == device) {
			(void) hipFree(reserved_arena);  // (too small after all)
		}
		if (reserved_device == device) {
			reserved_arena = nullptr;
			reserved_bytes = 0;
			reserved_device = -1;
		}
	}
	if (!out->arena)
		out->arena = device_alloc(need);
	char *at = (char *) out->arena;
	auto take = [&](size_t bytes) {
		void *p = at;
		at += round_up(bytes);
		return p;
	};
	out->d_nodes = take(nodes_bytes + sizeof(NodeRec));
	out->d_walk = walk_bytes ? take(walk_bytes) : nullptr;
	out->d_tris = take(tris_bytes);
	out->d_shade = take(shade_bytes);
	out->d_ao = take(ao_bytes ? ao_bytes : 1);
	clock.mark("allocation");
	const NodeRec zero{};
	OCRT_HIP(hipMemcpy((char *) out->d_nodes + nodes_bytes, &zero, sizeof zero, hipMemcpyHostToDevice));
	if (walk_bytes)
		OCRT_HIP(hipMemcpy(out->d_walk, walk.nodes.data(), walk_bytes, hipMemcpyHostToDevice));
	OCRT_HIP(hipMemcpy(out->d_nodes, scene.nodes.data(), nodes_bytes, hipMemcpyHostToDevice));
	OCRT_HIP(hipMemcpy(out->d_tris, scene.tris.data(), tris_bytes, hipMemcpyHostToDevice));
	OCRT_HIP(hipMemcpy(out->d_shade, scene.shade.data(), shade_bytes, hipMemcpyHostToDevice));
	if (ao_bytes)
		OCRT_HIP(hipMemcpy(out->d_ao, table.data(), ao_bytes, hipMemcpyHostToDevice));
	OCRT_HIP(hipDeviceSynchronize());
	out->finishTable(opts, ao_bytes);
	clock.mark("copies of walk array, nodes, leaf records, normals, table");
	out->device_bytes = nodes_bytes + walk_bytes + tris_bytes + shade_bytes + ao_bytes;
	// What a vertex update will need, kept on the host (one sweep over the node records; the faces are shared, not copied):
	// nothing of it goes to the device before the first update.
	out->leaf_faces = scene.leaf_faces;
	out->vertex_count = scene.vertex_count;
	out->node_skips.resize(scene.nodes.size());
	out->leaf_nodes.assign(scene.tris.size(), 0u);
	for (size_t i = 0; i < scene.nodes.size(); ++i) {
		out->node_skips[i] = scene.nodes[i].skip;
		if (scene.nodes[i].skip == 1 && scene.nodes[i].leaf < out->leaf_nodes.size())
			out->leaf_nodes[scene.nodes[i].leaf] = (uint32_t) i;
	}
	clock.mark("tree shape kept for vertex updates");
	return out;
}

DeviceScene::~DeviceScene() {
	if (hipSetDevice(device_index) != hipSuccess)
		return;
	device_free(arena);
	device_free(refit_arena);
	device_free(d_schedule);
}

// The first update's uploads (faces, leaf -> node map) and the schedule for `group_nodes`, blocking: they are made once.
void DeviceScene::prepareRefit(uint32_t group_nodes) {
	// (a scene built on the device has faces and map there from the start, and nothing of them on the host)
	if (node_skips.size() != node_count ||
	    (!refit_arena && (!leaf_faces || leaf_faces->size() != (size_t) tri_count * 3 || leaf_nodes.size() != tri_count)))
		throw std::logic_error("vertex update: the scene was uploaded without its faces");
	const uint32_t wanted = group_nodes == 0 ? REFIT_DEFAULT_GROUP : group_nodes < REFIT_MAX_GROUP ? group_nodes : REFIT_MAX_GROUP;
	if (!refit_arena) {
		const size_t faces_bytes = leaf_faces->size() * sizeof(uint32_t), map_bytes = leaf_nodes.size() * sizeof(uint32_t);
		refit_arena = device_alloc(round_up(faces_bytes) + round_up(map_bytes));
		d_faces = refit_arena;
		d_leaf_nodes = (char *) refit_arena + round_up(faces_bytes);
		OCRT_HIP(hipMemcpy(d_faces, leaf_faces->data(), faces_bytes, hipMemcpyHostToDevice));
		OCRT_HIP(hipMemcpy(d_leaf_nodes, leaf_nodes.data(), map_bytes, hipMemcpyHostToDevice));
		refit_bytes = faces_bytes + map_bytes;
	}
	if (refit_group_nodes == wanted)
		return;
	uploadSchedule(wanted);
}

// The schedule for groups of `wanted` nodes, made of node_skips and copied to the device (blocking).
void DeviceScene::uploadSchedule(uint32_t wanted) {
	const RefitSchedule schedule = make_refit_schedule(node_skips, wanted);
	const size_t entries_bytes = schedule.entries.size() * sizeof(uint32_t), children_bytes = schedule.children.size() * sizeof(uint32_t),
	             groups_bytes = schedule.groups.size() * sizeof(uint32_t);
	const size_t need = round_up(entries_bytes) + round_up(children_bytes) + round_up(groups_bytes);
	OCRT_HIP(hipDeviceSynchronize());  // (an update by the old schedule may still be running)
	if (need > schedule_capacity || !d_schedule) {
		device_free(d_schedule);
		schedule_capacity = 0;
		d_schedule = device_alloc(need);
		schedule_capacity = need;
	}
	d_entries = d_schedule;
	d_children = (char *) d_schedule + round_up(entries_bytes);
	d_groups = (char *) d_children + round_up(children_bytes);
	if (entries_bytes)
		OCRT_HIP(hipMemcpy(d_entries, schedule.entries.data(), entries_bytes, hipMemcpyHostToDevice));
	if (children_bytes)
		OCRT_HIP(hipMemcpy(d_children, schedule.children.data(), children_bytes, hipMemcpyHostToDevice));
	if (groups_bytes)
		OCRT_HIP(hipMemcpy(d_groups, schedule.groups.data(), groups_bytes, hipMemcpyHostToDevice));
	refit_pass_first = schedule.pass_first;
	refit_group_nodes = wanted;
}

namespace {
// Where the pieces of a build's scratch lie (each on a 256-byte boundary).
struct BuildScratch {
	size_t centres, partials, root, flag, keys, ids, sorted_keys, sorted_ids, ranges, inner_links, leaf_links, skips, sort, sort_bytes, bytes;
};
BuildScratch build_scratch(uint32_t faces) {
	BuildScratch at{};
	size_t end = 0;
	auto take = [&](size_t bytes) {
		const size_t p = end;
		end += round_up(bytes ? bytes : 1);
		return p;
	};
	const size_t n = faces;
	at.centres = take(n * 16);
	at.partials = take((size_t) build_partials(faces) * 32);
	at.root = take(32);
	at.flag = take(4);
	at.keys = take(n * 4);
	at.ids = take(n * 4);
	at.sorted_keys = take(n * 4);
	at.sorted_ids = take(n * 4);
	at.ranges = take(n * 8);
	at.inner_links = take(n * 4);
	at.leaf_links = take(n * 4);
	at.skips = take(n * 8);
	at.sort_bytes = build_sort_bytes(faces);
	at.sort = take(at.sort_bytes);
	at.bytes = end;
	return at;
}
}  // namespace

size_t DeviceScene::buildScratchBytes(uint32_t num_faces) { return build_scratch(num_faces).bytes; }

std::shared_ptr<DeviceScene> DeviceScene::build(int device, const RayTracer::Options &opts, const float *vertices4, const float *vnormals4,
                                                uint32_t num_vertices, const uint32_t *faces, uint32_t num_faces, uint32_t group_nodes, void *scratch,
                                                void *stream, void *const events[4], float *host_ms) {
	if (!vertices4 || !vnormals4 || !faces || !scratch)
		throw std::invalid_argument("build: null vertex, normal or face array");
	if (num_faces == 0 || num_vertices == 0)
		throw std::invalid_argument("build: no faces, or no vertices");
	if (num_faces >= (1u << 25))  // (pack_scene's bound: the kernels address leaf records with 32-bit byte offsets)
		throw std::invalid_argument("build: scene too large for 32-bit device offsets");
	OCRT_HIP(hipSetDevice(device));
	hipStream_t s = (hipStream_t) stream;
	std::shared_ptr<DeviceScene> out(new DeviceScene());
	out->device_index = device;
	const std::vector<float> table = out->takeOptions(opts);
	out->scene_facts_ = SceneFacts{};  // (no padded walk array: every walk takes the exact form)
	out->scene_facts_.prune_margin = std::numeric_limits<float>::infinity();
	out->scene_facts_.boxes_enclose = true;  // (the refit rule's boxes)
	out->node_count = 2u * num_faces - 1u;
	out->tri_count = num_faces;
	out->vertex_count = num_vertices;
	const size_t nodes_bytes = (size_t) out->node_count * sizeof(NodeRec), tris_bytes = (size_t) num_faces * sizeof(TriRec),
	             shade_bytes = (size_t) num_faces * sizeof(ShadeRec), ao_bytes = table.size() * sizeof(float);
	// one allocation for the four arrays, as an upload's (a zero record behind the nodes: the shared walk fetches a node with
	// its successor), one for the leaf-ordered faces and the leaf -> node map, as a first update's
	out->arena = device_alloc(round_up(nodes_bytes + sizeof(NodeRec)) + round_up(tris_bytes) + round_up(shade_bytes) + round_up(ao_bytes) + 256);
	char *at = (char *) out->arena;
	auto take = [&](size_t bytes) {
		void *p = at;
		at += round_up(bytes);
		return p;
	};
	out->d_nodes = take(nodes_bytes + sizeof(NodeRec));
	out->d_tris = take(tris_bytes);
	out->d_shade = take(shade_bytes);
	out->d_ao = take(ao_bytes ? ao_bytes : 1);
	out->device_bytes = nodes_bytes + tris_bytes + shade_bytes + ao_bytes;
	const size_t faces_bytes = (size_t) num_faces * 3 * sizeof(uint32_t), map_bytes = (size_t) num_faces * sizeof(uint32_t);
	out->refit_arena = device_alloc(round_up(faces_bytes) + round_up(map_bytes));
	out->d_faces = out->refit_arena;
	out->d_leaf_nodes = (char *) out->refit_arena + round_up(faces_bytes);
	out->refit_bytes = faces_bytes + map_bytes;

	const BuildScratch where = build_scratch(num_faces);
	char *const base = (char *) scratch;
	BuildBuffers b{};
	b.faces = faces;
	b.vertices = vertices4;
	b.num_faces = num_faces;
	b.num_vertices = num_vertices;
	b.centres = base + where.centres;
	b.partials = base + where.partials;
	b.root = base + where.root;
	b.flag = base + where.flag;
	b.keys = base + where.keys;
	b.ids = base + where.ids;
	b.sorted_keys = base + where.sorted_keys;
	b.sorted_ids = base + where.sorted_ids;
	b.leaf_faces = out->d_faces;
	b.ranges = base + where.ranges;
	b.inner_links = base + where.inner_links;
	b.leaf_links = base + where.leaf_links;
	b.nodes = out->d_nodes;
	b.skips = base + where.skips;
	b.leaf_node = out->d_leaf_nodes;
	// the topology: keys, the sort, shape and layout
	OCRT_HIP(hipEventRecord((hipEvent_t) events[0], s));
	OCRT_HIP(hipMemsetAsync(b.flag, 0, sizeof(uint32_t), s));
	OCRT_HIP(hipMemsetAsync(b.skips, 0, (size_t) out->node_count * sizeof(uint32_t), s));
	OCRT_HIP(hipMemsetAsync((char *) out->d_nodes + nodes_bytes, 0, sizeof(NodeRec), s));
	OCRT_HIP(hipMemsetAsync(out->d_leaf_nodes, 0, map_bytes, s));  // (every entry is written by the layout; no launch ever reads an unwritten one)
	launch_build_keys(b, s);
	launch_build_sort(base + where.sort, where.sort_bytes, b.keys, b.sorted_keys, b.ids, b.sorted_ids, num_faces, s);
	launch_build_tree(b, s);
	OCRT_HIP(hipGetLastError());
	OCRT_HIP(hipEventRecord((hipEvent_t) events[1], s));
	// the one wait: the skips for the schedule, the flag, the face of every leaf
	uint32_t flag = 0;
	out->node_skips.resize(out->node_count);
	out->built_faces.resize(num_faces);
	OCRT_HIP(hipMemcpyAsync(&flag, b.flag, sizeof flag, hipMemcpyDeviceToHost, s));
	OCRT_HIP(hipMemcpyAsync(out->node_skips.data(), b.skips, (size_t) out->node_count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	OCRT_HIP(hipMemcpyAsync(out->built_faces.data(), b.sorted_ids, (size_t) num_faces * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	if (ao_bytes)
		OCRT_HIP(hipMemcpyAsync(out->d_ao, table.data(), ao_bytes, hipMemcpyHostToDevice, s));
	OCRT_HIP(hipStreamSynchronize(s));
	if (flag)
		throw std::invalid_argument("build: a face references a vertex out of range (nothing was read through it; the host's scene stays as it was)");
	const auto before = std::chrono::steady_clock::now();
	out->uploadSchedule(group_nodes == 0 ? REFIT_DEFAULT_GROUP : group_nodes < REFIT_MAX_GROUP ? group_nodes : REFIT_MAX_GROUP);
	if (host_ms)
		*host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - before).count();
	out->finishTable(opts, ao_bytes);
	// the records and the boxes, as an update makes them
	OCRT_HIP(hipEventRecord((hipEvent_t) events[2], s));
	out->updateVertices(vertices4, vnormals4, group_nodes, s);
	OCRT_HIP(hipEventRecord((hipEvent_t) events[3], s));
	return out;
}

void DeviceScene::updateVertices(const float *vertices4, const float *vnormals4, uint32_t group_nodes, void *stream) {
	OCRT_HIP(hipSetDevice(device_index));
	prepareRefit(group_nodes);
	launch_refit_leaves(d_faces, d_leaf_nodes, vertices4, vnormals4, d_tris, d_shade, d_nodes, tri_count, stream);
	for (size_t p = 0; p + 1 < refit_pass_first.size(); ++p)
		launch_refit_inner(d_entries, d_children, d_groups, d_nodes, refit_pass_first[p], refit_pass_first[p + 1] - refit_pass_first[p], stream);
	OCRT_HIP(hipGetLastError());
	// (every box is the refit rule's now, whatever was uploaded: they hold their triangles wherever the coordinates are numbers)
	scene_facts_.boxes_enclose = true;
}

void DeviceScene::reserve(int device, size_t bytes) {
	if (bytes == 0 || hipSetDevice(device) != hipSuccess)
		return;
	void *p = nullptr;
	if (hipMalloc(&p, bytes) != hipSuccess) {
		(void) hipGetLastError();
		return;  // (create() allocates for itself)
	}
	std::lock_guard<std::mutex> lock(reserved_mutex);
	if (reserved_arena) {
		(void) hipSetDevice(reserved_device);
		(void) hipFree(reserved_arena);
		(void) hipSetDevice(device);
	}
	reserved_arena = p;
	reserved_bytes = bytes;
	reserved_device = device;
}

size_t DeviceScene::bytesFor(size_t triangles, size_t ao_directions) {
	const size_t nodes = triangles ? 2 * triangles - 1 : 0;
	// exact nodes + padding, two copies of the walk records with their END records and slack, leaf records, normals, table
	return round_up((nodes + 1) * sizeof(NodeRec)) + round_up((2 * (nodes + 2) + 2) * sizeof(NodeRec)) + round_up(triangles * sizeof(TriRec)) +
	       round_up(triangles * sizeof(ShadeRec)) + round_up(ao_directions * 4 * sizeof(float) + 1) + 256;
}

bool DeviceScene::servesOptions(const RayTracer::Options &opts) const {
	const bool on = opts.enableAO && opts.aoNumSamples > 0;
	if (on != ao_on)
		return false;
	if (!on)
		return true;
	return (int) opts.aoMethod == ao_method && opts.aoNumSamples == ao_samples && opts.aoAlphaMin == ao_alpha_min &&
	       opts.aoAlphaMax == ao_alpha_max && kernel_float(opts.aoMaxDistance) == walk_distance;
}

}  // namespace ocrt
