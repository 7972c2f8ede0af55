// c_api.cc -- the extern "C" boundary declared in include/rt_hip.h (the seam), rt_hip_ring.h (streams of frames, several GPUs), rt_hip_debug.h,
// rt_hip_query.h, rt_hip_multihit.h, rt_hip_ao.h, rt_hip_directional.h, rt_hip_layers.h, rt_hip_views.h, rt_hip_update.h, rt_hip_build.h and
// rt_hip_camera.h.
#include "../../include/rt_hip.h"
#include "../../include/rt_hip_ao.h"
#include "../../include/rt_hip_camera.h"
#include "../../include/rt_hip_directional.h"
#include "../../include/rt_hip_layers.h"
#include "../../include/rt_hip_debug.h"
#include "../../include/rt_hip_multihit.h"
#include "../../include/rt_hip_nearest.h"
#include "../../include/rt_hip_signed.h"
#include "../../include/rt_hip_query.h"
#include "../../include/rt_hip_segment.h"
#include "../../include/rt_hip_instance_build.h"
#include "../../include/rt_hip_instance_directional.h"
#include "../../include/rt_hip_instance_multihit.h"
#include "../../include/rt_hip_instance_nearest.h"
#include "../../include/rt_hip_instance_segments.h"
#include "../../include/rt_hip_instance_views.h"
#include "../../include/rt_hip_instances.h"
#include "../../include/rt_hip_views.h"
#include "../../include/rt_hip_update.h"
#include "../../include/rt_hip_build.h"

#include <algorithm>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>

#include "bvh.h"
#include "band_gather.h"
#include "camera.h"
#include "device_internal.h"
#include "device_renderer.h"
#include "frame_ring.h"
#include "hip_host.h"
#include "lbvh.h"
#include "mesh.h"
#include "ray_query.h"
#include "ray_tracer.h"
#include "refit.h"
#include "scene_pack.h"

struct rt_scene {
	Mesh mesh;
	BVH bvh;
	std::vector<uint32_t> sorted_faces;
	bool built = false;
};

struct rt_host {
	std::unique_ptr<ocrt::DeviceRenderer> owned;  // empty for a view of a ring's renderer (rt_ring_host)
	ocrt::DeviceRenderer *dev = nullptr;
	std::unique_ptr<ocrt::RayQueries> queries;  // rt_hip_query.h: made at the first query (destroyed before `owned`)
};

struct rt_ring {
	std::unique_ptr<ocrt::FrameRing> ring;
	std::vector<rt_host> views;  // rt_ring_host: the ring's renderers as borrowed rt_host handles
};

namespace {

thread_local std::string g_error;
thread_local int g_error_code = RT_OK;

int fail(int code, const std::string &message) {
	g_error = message;
	g_error_code = code;
	return code;
}

// What the entry points of a host's own state check first -- they work before an upload too, but not on the hosts of a
// frame ring --; `family` names the queries in the message ("ray", "closest-point").
int owned_precheck(const rt_host *h, const char *family) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	if (!h->owned)
		return fail(RT_E_STATE, std::string(family) + " queries are not available on the hosts of a frame ring");
	return RT_OK;
}

// ... and what every query entry point does.
int host_precheck(const rt_host *h, const char *family) {
	const int rc = owned_precheck(h, family);
	if (rc != RT_OK)
		return rc;
	if (!h->dev->sceneReady())
		return fail(RT_E_STATE, std::string(family) + " query before a scene was uploaded");
	return RT_OK;
}

int instance_set_required(const rt_host *h, const char *what) {
	if (!h->queries || h->queries->instanceCount() == 0)
		return fail(RT_E_STATE, std::string(what) + " without an instance set (rt_set_instances)");
	return RT_OK;
}

bool aligned(std::initializer_list<const void *> pointers, uintptr_t bytes) {
	uintptr_t all = 0;
	for (const void *p : pointers)
		all |= (uintptr_t) p;
	return (all & (bytes - 1u)) == 0;
}

// A family of queries over `items` read from one or two float4 arrays, as its messages name it.
struct Family {
	const char *name;         // "<name> queries are not available ...", "<name> query before ...", "<name> query without an instance set"
	const char *items;        // "more <items> than RT_QUERY_MAX_RAYS in one call"
	const char *null_arrays;  // the message for a null array
	const char *unaligned;    // the message for a device array that is not 16-byte aligned
	bool instanced;           // the host's instance set is asked for
};
constexpr Family RAYS = { "ray", "rays", "null ray arrays", "device ray arrays must be 16-byte aligned", false };
constexpr Family INSTANCED_RAYS = { "instanced ray", "rays", "null ray arrays", "device ray arrays must be 16-byte aligned", true };
constexpr Family SEGMENTS = { "segment", "segments", "null point arrays", "device point arrays must be 16-byte aligned", false };
constexpr Family INSTANCED_SEGMENTS = { "instanced segment", "segments", "null point arrays", "device point arrays must be 16-byte aligned",
	                                    true };
constexpr Family POINTS = { "closest-point", "points", "null point array", "the device point array must be 16-byte aligned", false };
constexpr Family SIGNED_POINTS = { "signed distance", "points", "null point array", "the device point array must be 16-byte aligned", false };
constexpr Family INSTANCED_POINTS = { "instanced closest-point", "points", "null point array",
	                                  "the device point array must be 16-byte aligned", true };

// What these families check before they touch the device ("Errors" of include/rt_hip_query.h, rt_hip_segment.h,
// rt_hip_nearest.h, rt_hip_instances.h, rt_hip_instance_segments.h), in this order: the host, the set, the count -- `items`
// rays, segments, pairs of a mask or points --, the arrays (`b4`: `a4` once more for a family with one).
int query_precheck(const rt_host *h, const Family &f, const float *a4, const float *b4, uint64_t items, bool device) {
	int rc = host_precheck(h, f.name);
	if (rc == RT_OK && f.instanced)
		rc = instance_set_required(h, (std::string(f.name) + " query").c_str());
	if (rc != RT_OK)
		return rc;
	if (items > RT_QUERY_MAX_RAYS)
		return fail(RT_E_INVALID, "more " + std::string(f.items) + " than RT_QUERY_MAX_RAYS in one call");
	if (items > 0 && (!a4 || !b4))
		return fail(RT_E_INVALID, f.null_arrays);
	if (device && items > 0 && !aligned({ a4, b4 }, 16))
		return fail(RT_E_INVALID, f.unaligned);
	return RT_OK;
}

ocrt::RayQueries &queries_of(rt_host *h) {
	if (!h->queries)
		h->queries.reset(new ocrt::RayQueries(*h->dev));
	return *h->queries;
}

// ... and every ambient-occlusion query (include/rt_hip_ao.h, "Errors"); `rays`: the rays per point, for the caller.
int ao_precheck(const rt_host *h, const float *points4, const float *normals4, uint32_t n, bool device, uint32_t *rays) {
	const int rc = host_precheck(h, "ambient-occlusion");
	if (rc != RT_OK)
		return rc;
	const uint32_t per_point = ocrt::RayQueries::aoRaysPerPoint(*h->dev);
	if (per_point == 0)
		return fail(RT_E_STATE, "ambient-occlusion query on a host whose options have ambient occlusion off");
	if (n > RT_QUERY_MAX_RAYS / per_point)
		return fail(RT_E_INVALID, "more points than RT_QUERY_MAX_RAYS / rays per point in one call");
	if (n > 0 && (!points4 || !normals4))
		return fail(RT_E_INVALID, "null point or normal arrays");
	if (device && n > 0 && !aligned({ points4, normals4 }, 16))
		return fail(RT_E_INVALID, "device point and normal arrays must be 16-byte aligned");
	if (rays)
		*rays = per_point;
	return RT_OK;
}

// rt_hit_arrays / rt_multihit_arrays as the query code takes them; null: no output at all.
template <class Arrays> void record_outputs(const Arrays *from, ocrt::RecordOutputs &to) {
	if (!from)
		return;
	to.distance = from->distance;
	to.leaf = from->leaf;
	to.barycentric = from->barycentric;
	to.position = from->position;
	to.normal = from->normal;
}
// The occlusion forms' output: the flags alone.
ocrt::QueryOutputs occlusion_outputs(uint8_t *occluded) {
	ocrt::QueryOutputs q;
	q.hit = occluded;
	return q;
}
ocrt::QueryOutputs hit_outputs(const rt_hit_arrays *from) {
	ocrt::QueryOutputs q;
	q.hit = from ? from->hit : nullptr;
	record_outputs(from, q);
	return q;
}
ocrt::MultiHitOutputs multihit_outputs(const rt_multihit_arrays *from) {
	ocrt::MultiHitOutputs q;
	q.count = from ? from->count : nullptr;
	record_outputs(from, q);
	return q;
}
bool records_aligned(const ocrt::RecordOutputs &q) { return aligned({ q.distance, q.leaf, q.barycentric, q.position, q.normal }, 4); }
// ... and the instanced families' arrays apart: the record or the slots, and the instance indices beside them.
ocrt::QueryOutputs hit_outputs(const rt_instance_hit_arrays *from) { return hit_outputs(from ? &from->record : nullptr); }
ocrt::MultiHitOutputs multihit_outputs(const rt_instance_multihit_arrays *from) { return multihit_outputs(from ? &from->slots : nullptr); }
template <class Arrays> uint32_t *instance_of(const Arrays *from) { return from ? from->instance : nullptr; }

// Where a call's arrays live (ray_query.h): host memory for the blocking entry points, device memory and the caller's
// stream for the *_device ones.  Every family below is written once, as <family>_call(h, ..., where): its checks in the
// header's order -- the alignment of device arrays among them --, then the one RayQueries method; the exported functions
// forward to it.
using Where = ocrt::RayQueries::Where;
const Where HOST = Where::hostMemory();
Where on(void *hip_stream) { return Where::deviceMemory(hip_stream); }

// Maps the exception in flight to an RT_E_* code.
int fail_from_exception() {
	try {
		throw;
	} catch (const ocrt::DeviceError &e) {
		return fail(RT_E_DEVICE, e.what());
	} catch (const std::invalid_argument &e) {
		return fail(RT_E_INVALID, e.what());
	} catch (const std::logic_error &e) {
		return fail(RT_E_STATE, e.what());
	} catch (const std::runtime_error &e) {
		const bool no_device = std::strcmp(e.what(), "No device found") == 0;
		return fail(no_device ? RT_E_NO_DEVICE : RT_E_IO, e.what());
	} catch (const std::exception &e) {
		return fail(RT_E_INVALID, e.what());
	} catch (...) {
		return fail(RT_E_INVALID, "unknown error");
	}
}

RayTracer::Options to_options(const rt_options &o) {
	RayTracer::Options r;
	r.width = o.width;
	r.height = o.height;
	r.focalLength = o.focal_length;
	r.nSuperSamples = o.n_super_samples;
	r.enableShading = o.enable_shading != 0;
	r.enableAO = o.enable_ao != 0;
	r.aoMaxDistance = o.ao_max_distance;
	r.aoNumSamples = o.ao_num_samples;
	r.aoMethod = o.ao_method == 0 ? RayTracer::AmbientOcclusionMethod::UNIFORM : RayTracer::AmbientOcclusionMethod::RANDOM;
	r.aoAlphaMin = o.ao_alpha_min;
	r.aoAlphaMax = o.ao_alpha_max;
	r.bvhMethod = o.bvh_method == 0 ? BVH::Method::CUT_LONGEST_AXIS : BVH::Method::SURFACE_AREA_HEURISTIC;
	return r;
}

static_assert(sizeof(rt_camera) == sizeof(ocrt::CameraPose), "rt_camera is CameraPose");
ocrt::CameraPose to_pose(const rt_camera &c) {
	ocrt::CameraPose p;
	std::memcpy(&p, &c, sizeof p);
	return p;
}
void from_pose(const ocrt::CameraPose &p, rt_camera *out) { std::memcpy(out, &p, sizeof p); }

template <class F> int guarded(F &&body) {
	try {
		body();
		return RT_OK;
	} catch (...) {
		return fail_from_exception();
	}
}

// rt_upload / rt_ring_upload: the caller's arrays (four floats per box corner, vertex and normal), validated and packed,
// into `target` (a renderer or a ring).
template <class Target>
int upload_arrays(Target *target, const uint32_t *faces, uint32_t num_faces, const uint32_t *nodes, uint32_t num_nodes, const float *aabbs,
                  const float *vertices, uint32_t num_vertices, const float *vnormals) {
	if (!target || !faces || !nodes || !aabbs || !vertices || !vnormals)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		auto as_vec3 = [](const float *p, size_t n) {
			std::vector<Vec3f> v(n);
			for (size_t i = 0; i < n; ++i)
				v[i] = Vec3f(p[4 * i], p[4 * i + 1], p[4 * i + 2]);
			return v;
		};
		const std::vector<uint32_t> f(faces, faces + 3 * (size_t) num_faces);
		const std::vector<uint32_t> n(nodes, nodes + num_nodes);
		target->upload(ocrt::pack_scene(f, n, as_vec3(aabbs, 2 * (size_t) num_nodes), as_vec3(vertices, num_vertices),
		                                as_vec3(vnormals, num_vertices)));
	});
}

}  // namespace

extern "C" {

const char *rt_last_error(void) { return g_error.c_str(); }
int rt_last_error_code(void) { return g_error_code; }

void rt_options_default(rt_options *out) {
	const RayTracer::Options d = RayTracer::defaults();
	out->width = d.width;
	out->height = d.height;
	out->focal_length = d.focalLength;
	out->n_super_samples = d.nSuperSamples;
	out->enable_shading = d.enableShading;
	out->enable_ao = d.enableAO;
	out->ao_max_distance = d.aoMaxDistance;
	out->ao_num_samples = d.aoNumSamples;
	out->ao_method = 0;
	out->ao_alpha_min = d.aoAlphaMin;
	out->ao_alpha_max = d.aoAlphaMax;
	out->bvh_method = 0;
}

uint32_t rt_total_width(const rt_options *o) { return RayTracer(to_options(*o)).totalWidth; }
uint32_t rt_total_height(const rt_options *o) { return RayTracer(to_options(*o)).totalHeight; }

int rt_resize_cpu(const rt_options *o, const float *tmp, uint8_t *image) {
	if (!o || !tmp || !image)
		return fail(RT_E_INVALID, "null argument");
	if (RayTracer::gridSize(o->n_super_samples) == 0)
		return fail(RT_E_INVALID, "supersample count must be positive");
	RayTracer(to_options(*o)).resize(tmp, image);
	return RT_OK;
}

rt_scene *rt_scene_load_off(const char *path) {
	std::unique_ptr<rt_scene> s(new (std::nothrow) rt_scene);
	if (!s || !path) {
		fail(RT_E_INVALID, "null argument");
		return nullptr;
	}
	const int rc = guarded([&] {
		load_off_mesh(path, &s->mesh);
		compute_vertex_normals(&s->mesh);
	});
	return rc == RT_OK ? s.release() : nullptr;
}

rt_scene *rt_scene_from_arrays(const float *vertices4, uint32_t num_vertices, const uint32_t *faces, uint32_t num_faces) {
	if ((!vertices4 && num_vertices) || (!faces && num_faces)) {
		fail(RT_E_INVALID, "null argument");
		return nullptr;
	}
	std::unique_ptr<rt_scene> s(new (std::nothrow) rt_scene);
	if (!s)
		return nullptr;
	for (uint32_t i = 0; i < 3 * num_faces; ++i)
		if (faces[i] >= num_vertices) {
			fail(RT_E_INVALID, "face references a vertex out of range");
			return nullptr;
		}
	s->mesh.vertices.resize(num_vertices);
	for (uint32_t i = 0; i < num_vertices; ++i)
		s->mesh.vertices[i] = Vec3f(vertices4[4 * i], vertices4[4 * i + 1], vertices4[4 * i + 2]);
	s->mesh.faces.assign(faces, faces + 3 * (size_t) num_faces);
	compute_vertex_normals(&s->mesh);
	return s.release();
}

void rt_scene_free(rt_scene *s) { delete s; }
uint32_t rt_scene_num_vertices(const rt_scene *s) { return (uint32_t) s->mesh.vertices.size(); }
uint32_t rt_scene_num_faces(const rt_scene *s) { return (uint32_t) (s->mesh.faces.size() / 3); }

int rt_scene_build_bvh(rt_scene *s, int method) {
	if (!s)
		return fail(RT_E_INVALID, "null scene");
	return guarded([&] {
		s->built = false;
		s->bvh = BVH(method == 0 ? BVH::Method::CUT_LONGEST_AXIS : BVH::Method::SURFACE_AREA_HEURISTIC);
		s->bvh.buildBVH(s->mesh);
		s->sorted_faces = sort_faces_by_leaf_order(s->mesh, s->bvh);
		s->built = true;
	});
}

uint32_t rt_scene_num_nodes(const rt_scene *s) { return s->built ? (uint32_t) s->bvh.nodes.size() : 0; }
const float *rt_scene_vertices(const rt_scene *s) { return &s->mesh.vertices.data()->x; }
const float *rt_scene_vnormals(const rt_scene *s) { return &s->mesh.vnormals.data()->x; }
const uint32_t *rt_scene_faces(const rt_scene *s) { return s->mesh.faces.data(); }
const uint32_t *rt_scene_nodes(const rt_scene *s) { return s->bvh.nodes.data(); }
const float *rt_scene_aabbs(const rt_scene *s) { return &s->bvh.aabbs.data()->x; }
const uint32_t *rt_scene_triangles(const rt_scene *s) { return s->bvh.triangles.data(); }
const uint32_t *rt_scene_sorted_faces(const rt_scene *s) { return s->sorted_faces.data(); }

rt_host *rt_create_on(const rt_options *o, int device, uint32_t rank, uint32_t nranks) {
	if (!o) {
		fail(RT_E_INVALID, "null options");
		return nullptr;
	}
	std::unique_ptr<rt_host> h(new (std::nothrow) rt_host);
	if (!h)
		return nullptr;
	const int rc = guarded([&] {
		h->owned.reset(new ocrt::DeviceRenderer(to_options(*o), device, rank, nranks));
		h->dev = h->owned.get();
	});
	return rc == RT_OK ? h.release() : nullptr;
}

rt_host *rt_create(const rt_options *o) { return rt_create_on(o, -1, 0, 1); }

void rt_destroy(rt_host *h) {
	if (h && h->owned)  // (a view handed out by rt_ring_host belongs to its ring)
		delete h;
}

int rt_upload(rt_host *h, const uint32_t *faces, uint32_t num_faces, const uint32_t *nodes, uint32_t num_nodes,
              const float *aabbs, const float *vertices, uint32_t num_vertices, const float *vnormals) {
	return upload_arrays(h ? h->dev : nullptr, faces, num_faces, nodes, num_nodes, aabbs, vertices, num_vertices, vnormals);
}

int rt_upload_scene(rt_host *h, const rt_scene *s) {
	if (!h || !s)
		return fail(RT_E_INVALID, "null argument");
	if (!s->built)
		return fail(RT_E_STATE, "scene has no BVH yet (call rt_scene_build_bvh)");
	return guarded([&] {
		h->dev->upload(ocrt::pack_scene(s->sorted_faces, s->bvh.nodes, s->bvh.aabbs, s->mesh.vertices, s->mesh.vnormals));
	});
}

int rt_render(rt_host *h) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	return guarded([&] {
		h->dev->enqueueRender();
		h->dev->synchronize();
	});
}

int rt_render_async(rt_host *h) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	return guarded([&] { h->dev->enqueueRender(); });
}

int rt_sync(rt_host *h) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	return guarded([&] { h->dev->synchronize(); });
}

int rt_download(rt_host *h, float *image) {
	if (!h || !image)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->downloadFloat(image); });
}

int rt_download_u8(rt_host *h, uint8_t *image) {
	if (!h || !image)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->downloadResizedFull(image); });
}

uint32_t rt_local_rows(const rt_host *h) { return h ? h->dev->localRows() : 0; }

int rt_download_u8_local(rt_host *h, uint8_t *rows) {
	if (!h || !rows)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->downloadResizedLocal(rows); });
}

uint32_t rt_partition_local_rows(const rt_options *o, uint32_t rank, uint32_t nranks) {
	const uint32_t n = RayTracer::gridSize(o->n_super_samples);
	if (n == 0 || nranks == 0 || rank >= nranks)
		return 0;
	const ocrt::Partition part{ rank, nranks, ocrt::band_tile_rows_for(n) };
	return ocrt::local_tile_rows_for(o->height * n, part) * ocrt::TILE_H / n;
}

uint32_t rt_partition_global_row(const rt_options *o, uint32_t rank, uint32_t nranks, uint32_t local_row) {
	const uint32_t n = RayTracer::gridSize(o->n_super_samples);
	if (n == 0 || nranks == 0)
		return 0xFFFFFFFFu;
	const uint32_t rows_per_band = ocrt::band_tile_rows_for(n) * ocrt::TILE_H / n;
	const uint32_t band_local = local_row / rows_per_band;
	return (band_local * nranks + rank) * rows_per_band + local_row % rows_per_band;
}

uint32_t rt_local_to_global_row(const rt_host *h, uint32_t local_row) {
	if (!h)
		return 0xFFFFFFFFu;
	const ocrt::KernelParams &p = h->dev->params();
	const RayTracer::Options &ro = h->dev->rayTracer().options;
	rt_options o{};
	o.n_super_samples = ro.nSuperSamples;
	return rt_partition_global_row(&o, p.part.rank, p.part.nranks, local_row);
}

int rt_resize_into_device(rt_host *h, void *device_u8) {
	if (!h || !device_u8)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->enqueueResizeInto(device_u8); });
}

int rt_set_stream(rt_host *h, void *hip_stream) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	return guarded([&] { h->dev->setStream(hip_stream); });
}

int rt_get_stream(rt_host *h, void **hip_stream) {
	if (!h || !hip_stream)
		return fail(RT_E_INVALID, "null argument");
	*hip_stream = h->dev->streamHandle();
	return RT_OK;
}

int rt_set_device_share(rt_host *h, unsigned int hosts) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	h->dev->setDeviceShare(hosts);
	return RT_OK;
}

int rt_expect_frames(rt_host *h, uint64_t frames) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	return guarded([&] { h->dev->expectFrames(frames); });
}

int rt_use_private_stream(rt_host *h) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	return guarded([&] { h->dev->usePrivateStream(); });
}

int rt_get_stats(rt_host *h, rt_stats *out) {
	if (!h || !out)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		const ocrt::RenderStats s = h->dev->stats();
		out->primary_rays = s.primary_rays;
		out->primary_hits = s.primary_hits;
		out->ao_rays = s.ao_rays;
		out->ao_occluded = s.ao_occluded;
	});
}

float rt_last_kernel_ms(const rt_host *h) { return h ? h->dev->lastKernelMs() : 0.0f; }
double rt_total_kernel_ms(const rt_host *h) { return h ? h->dev->totalKernelMs() : 0.0; }
float rt_last_ao_ms(const rt_host *h) { return h ? h->dev->lastAoMs() : 0.0f; }
double rt_total_ao_ms(const rt_host *h) { return h ? h->dev->totalAoMs() : 0.0; }
uint64_t rt_kernel_launches(const rt_host *h) { return h ? h->dev->kernelLaunches() : 0; }
void rt_reset_timers(rt_host *h) {
	if (h)
		h->dev->resetTimers();
}

/* ---- frame ring ------------------------------------------------------------------------------------------------ */
rt_ring *rt_ring_create(const rt_options *o, int device, uint32_t rank, uint32_t nranks, uint32_t hosts) {
	if (!o) {
		fail(RT_E_INVALID, "null options");
		return nullptr;
	}
	std::unique_ptr<rt_ring> r(new (std::nothrow) rt_ring);
	if (!r)
		return nullptr;
	const int rc = guarded([&] {
		r->ring.reset(new ocrt::FrameRing(to_options(*o), device, rank, nranks, hosts));
		r->views.resize(r->ring->size());
		for (uint32_t k = 0; k < r->ring->size(); ++k)
			r->views[k].dev = &r->ring->host(k);
	});
	return rc == RT_OK ? r.release() : nullptr;
}

void rt_ring_destroy(rt_ring *r) { delete r; }

int rt_ring_upload(rt_ring *r, const uint32_t *faces, uint32_t num_faces, const uint32_t *nodes, uint32_t num_nodes,
                   const float *aabbs, const float *vertices, uint32_t num_vertices, const float *vnormals) {
	return upload_arrays(r ? r->ring.get() : nullptr, faces, num_faces, nodes, num_nodes, aabbs, vertices, num_vertices, vnormals);
}

int rt_ring_upload_scene(rt_ring *r, const rt_scene *s) {
	if (!r || !s)
		return fail(RT_E_INVALID, "null argument");
	if (!s->built)
		return fail(RT_E_STATE, "scene has no BVH yet (call rt_scene_build_bvh)");
	return guarded([&] {
		r->ring->upload(ocrt::pack_scene(s->sorted_faces, s->bvh.nodes, s->bvh.aabbs, s->mesh.vertices, s->mesh.vnormals));
	});
}

int rt_ring_device_bytes(const rt_ring *r, uint64_t *scene_bytes, uint32_t *scene_copies, uint64_t *total_bytes) {
	if (!r)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		std::vector<const ocrt::DeviceScene *> seen;
		for (uint32_t k = 0; k < r->ring->size(); ++k) {
			const ocrt::DeviceScene *s = r->ring->host(k).deviceScene().get();
			if (s && std::find(seen.begin(), seen.end(), s) == seen.end())
				seen.push_back(s);
		}
		if (scene_bytes)
			*scene_bytes = seen.empty() ? 0 : seen.front()->bytes();
		if (scene_copies)
			*scene_copies = (uint32_t) seen.size();
		if (total_bytes)
			*total_bytes = r->ring->uploadedBytes();
	});
}

int rt_ring_set_calibration(rt_ring *r, int on) {
	if (!r)
		return fail(RT_E_INVALID, "null argument");
	r->ring->setCalibration(on != 0);
	return RT_OK;
}

int rt_ring_calibration(const rt_ring *r, float *ms_without, float *ms_with, int *prefetch_in_use) {
	if (!r)
		return fail(RT_E_INVALID, "null argument");
	if (ms_without)
		*ms_without = r->ring->calibrationMs()[0];
	if (ms_with)
		*ms_with = r->ring->calibrationMs()[1];
	if (prefetch_in_use)
		*prefetch_in_use = r->ring->aoPrefetch() ? 1 : 0;
	return RT_OK;
}

int rt_walk_entries(rt_host *h, uint32_t *tiles_hit, uint32_t *tiles_narrowed, double *mean_share, double *mean_packet_share) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		const ocrt::DeviceRenderer::WalkEntries e = h->dev->walkEntries();
		if (tiles_hit)
			*tiles_hit = e.tiles_hit;
		if (tiles_narrowed)
			*tiles_narrowed = e.tiles_narrowed;
		if (mean_share)
			*mean_share = e.mean_share;
		if (mean_packet_share)
			*mean_packet_share = e.mean_packet_share;
	});
}

int rt_debug_walk_interval_ends(rt_host *h, uint32_t out[6]) {
	if (!h || !out)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		const ocrt::DeviceRenderer::IntervalEnds e = h->dev->walkIntervalEnds();
		out[0] = e.intervals;
		out[1] = e.whole_array;
		out[2] = e.after_leaf;
		out[3] = e.after_inner;
		out[4] = e.last_is_leaf;
		out[5] = e.last_is_inner;
	});
}

int rt_set_ao_prefetch(rt_host *h, int on) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->setAoPrefetch(on != 0); });
}

// ---- include/rt_hip_debug.h ----
int rt_debug_measure_tile_costs(rt_host *h, uint32_t frames, int reorder) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		// (without `reorder` the list in place stays, and its split prefix and cheap suffix with it)
		h->dev->measureTileCosts(frames, reorder != 0);
	});
}

int rt_debug_set_primary_split(rt_host *h, uint32_t above) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->setPrimarySplit(above); });
}

int rt_debug_set_order_policy(rt_host *h, float heavy, float runway, float split_above) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->setOrderPolicy(heavy, runway, split_above); });
}

uint32_t rt_debug_tile_order_slots(rt_host *h) {
	if (!h)
		return 0;
	std::vector<uint32_t> order, constants, words;
	std::vector<float> cost;
	h->dev->tileOrder(order, constants, words, cost);
	return (uint32_t) order.size();
}

uint32_t rt_debug_tiles(rt_host *h) {
	if (!h)
		return 0;
	const ocrt::KernelParams &kp = h->dev->params();
	return kp.tiles_x * kp.local_tile_rows;
}

int rt_debug_tile_order(rt_host *h, uint32_t *order_out, uint32_t *constants24, uint32_t *tile_words, float *tile_costs) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		std::vector<uint32_t> order, constants, words;
		std::vector<float> cost;
		h->dev->tileOrder(order, constants, words, cost);
		if (order_out)
			std::copy(order.begin(), order.end(), order_out);
		if (constants24)
			std::copy(constants.begin(), constants.end(), constants24);
		const uint32_t tiles = rt_debug_tiles(h);
		if (tile_words)
			for (uint32_t t = 0; t < tiles; ++t)
				tile_words[t] = t < words.size() ? words[t] : 0u;
		if (tile_costs)
			for (uint32_t t = 0; t < tiles; ++t)
				tile_costs[t] = t < cost.size() ? cost[t] : 0.0f;
	});
}

int rt_debug_set_tile_order(rt_host *h, const uint32_t *order, uint32_t slots, const uint32_t *constants24) {
	if (!h || !order || !constants24)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		h->dev->setTileOrder(std::vector<uint32_t>(order, order + slots), std::vector<uint32_t>(constants24, constants24 + 24));
	});
}

int rt_debug_split_tiles(rt_host *h, uint32_t out[8]) {
	if (!h || !out)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		const auto &splits = h->dev->splitTiles();
		std::copy(splits.begin(), splits.end(), out);
	});
}

int rt_debug_set_cheap_claims(rt_host *h, float cheap_below) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->setCheapClaims(cheap_below); });
}

int rt_debug_cheap_tiles(rt_host *h, uint32_t out[8]) {
	if (!h || !out)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		const auto &cheap = h->dev->cheapTiles();
		std::copy(cheap.begin(), cheap.end(), out);
	});
}

int rt_debug_prune_facts(rt_host *h, float *prune_margin, uint32_t *unpruned_bytes, uint32_t *primary_bytes) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	if (!h->dev->deviceScene())
		return fail(RT_E_STATE, "no scene on the device");
	const ocrt::KernelParams &kp = h->dev->params();  // (as the launches get them)
	if (prune_margin)
		*prune_margin = kp.prune_margin;
	if (unpruned_bytes)
		*unpruned_bytes = kp.unpruned_bytes;
	if (primary_bytes)
		*primary_bytes = kp.primary_walk_bytes;
	return RT_OK;
}

int rt_debug_poison_hit_list(rt_host *h) {
	if (!h)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { h->dev->poisonHitList(); });
}

int rt_debug_node_test_forms(int device, const float *records8, uint32_t boxes, const float *rays6, uint32_t rays, uint32_t *out9) {
	if (!records8 || !rays6 || !out9)
		return fail(RT_E_INVALID, "null argument");
	if (boxes == 0 || boxes > 65536u || rays == 0 || rays > 65536u || rays % 64u != 0)
		return fail(RT_E_INVALID, "1 ... 65536 records and a multiple of 64 rays, 65536 at the most");
	const size_t record_bytes = (size_t) boxes * 32u, ray_bytes = (size_t) rays * 24u, out_bytes = (size_t) rays * boxes * 36u;
	return guarded([&] {
		OCRT_HIP(hipSetDevice(device));
		void *d_records = nullptr, *d_rays = nullptr, *d_out = nullptr;
		try {
			d_records = ocrt::device_alloc(record_bytes);
			d_rays = ocrt::device_alloc(ray_bytes);
			d_out = ocrt::device_alloc(out_bytes);
			OCRT_HIP(hipMemcpy(d_records, records8, record_bytes, hipMemcpyHostToDevice));
			OCRT_HIP(hipMemcpy(d_rays, rays6, ray_bytes, hipMemcpyHostToDevice));
			ocrt::launch_node_test_forms(d_records, boxes, d_rays, rays, d_out, nullptr);
			OCRT_HIP(hipGetLastError());
			OCRT_HIP(hipMemcpy(out9, d_out, out_bytes, hipMemcpyDeviceToHost));
		} catch (...) {
			ocrt::device_free(d_records);
			ocrt::device_free(d_rays);
			ocrt::device_free(d_out);
			throw;
		}
		ocrt::device_free(d_records);
		ocrt::device_free(d_rays);
		ocrt::device_free(d_out);
	});
}

uint32_t rt_ring_size(const rt_ring *r) { return r ? r->ring->size() : 0; }
uint32_t rt_ring_slots(const rt_ring *r) { return r ? r->ring->slots() : 0; }
uint32_t rt_ring_local_rows(const rt_ring *r) { return r ? r->ring->localRows() : 0; }
uint32_t rt_ring_in_flight(const rt_ring *r) { return r ? r->ring->inFlight() : 0; }
rt_host *rt_ring_host(rt_ring *r, uint32_t slot) { return (r && slot < r->views.size()) ? &r->views[slot] : nullptr; }

int rt_ring_set_graph_mode(rt_ring *r, int on) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] { r->ring->setGraphMode(on != 0); });
}

int rt_ring_set_pacing(rt_ring *r, float beta) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	r->ring->setPacing(beta);
	return RT_OK;
}

int rt_ring_bind_output(rt_ring *r, uint32_t slot, void *device_u8) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] { r->ring->bindOutput(slot, device_u8); });
}

int rt_ring_submit(rt_ring *r, uint64_t *frame) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] {
		const uint64_t f = r->ring->submit();
		if (frame)
			*frame = f;
	});
}

int rt_ring_collect(rt_ring *r, uint64_t *frame, uint32_t *slot, const void **device_bands) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] {
		const ocrt::FrameRing::Collected c = r->ring->collect();
		if (frame)
			*frame = c.frame;
		if (slot)
			*slot = c.slot;
		if (device_bands)
			*device_bands = c.device_bands;
	});
}

int rt_ring_collect_into_device(rt_ring *r, void *device_u8) {
	if (!r || !device_u8)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		const ocrt::FrameRing::Collected c = r->ring->collect();
		ocrt::DeviceRenderer &h = r->ring->host((uint32_t) (c.frame % r->ring->size()));
		if (hipSetDevice(h.deviceIndex()) != hipSuccess ||
		    hipMemcpyAsync(device_u8, c.device_bands, (size_t) h.localRows() * h.width(), hipMemcpyDeviceToDevice,
		                   (hipStream_t) h.streamHandle()) != hipSuccess ||
		    hipStreamSynchronize((hipStream_t) h.streamHandle()) != hipSuccess)
			throw ocrt::DeviceError("copying a collected frame's bands failed");
	});
}

int rt_ring_step(rt_ring *r) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] { r->ring->step(); });
}

int rt_ring_run(rt_ring *r, uint32_t frames) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] {
		for (uint32_t k = 0; k < frames; ++k)
			r->ring->step();
	});
}

int rt_ring_drain(rt_ring *r) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] { r->ring->drain(); });
}

int rt_ring_last_image_device(rt_ring *r, const void **device_u8) {
	if (!r || !device_u8)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { *device_u8 = r->ring->lastImageDevice(); });
}

int rt_ring_download_last(rt_ring *r, uint8_t *image) {
	if (!r || !image)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { r->ring->downloadLast(image); });
}

int rt_ring_reset_clock(rt_ring *r) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] { r->ring->resetClock(); });
}

int rt_ring_keep_frame_times(rt_ring *r, int on) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] { r->ring->keepFrameTimes(on != 0); });
}

int rt_ring_frame_times(const rt_ring *r, uint64_t frame, float ms[4]) {
	if (!r || !ms)
		return fail(RT_E_INVALID, "null argument");
	return r->ring->frameTimes(frame, ms) ? RT_OK : fail(RT_E_STATE, "no time stamps kept for that frame");
}

int rt_ring_timers(rt_ring *r, double *kernel_ms, uint64_t *frames, double *ao_ms, uint64_t *ao_frames) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	double k = 0, a = 0;
	uint64_t nk = 0, na = 0;
	for (uint32_t s = 0; s < r->ring->size(); ++s) {
		const ocrt::DeviceRenderer &h = r->ring->host(s);
		k += h.totalKernelMs();
		a += h.totalAoMs();
		nk += h.kernelLaunches();
		na += h.aoLaunches();
	}
	if (kernel_ms)
		*kernel_ms = k;
	if (frames)
		*frames = nk;
	if (ao_ms)
		*ao_ms = a;
	if (ao_frames)
		*ao_frames = na;
	return RT_OK;
}

int rt_ring_cpu_times(const rt_ring *r, double *submit_s, double *wait_s, double *collect_s, uint64_t *frames) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	const ocrt::FrameRing::CpuTimes &t = r->ring->cpuTimes();
	if (submit_s)
		*submit_s = t.submit_s;
	if (wait_s)
		*wait_s = t.wait_s;
	if (collect_s)
		*collect_s = t.collect_s;
	if (frames)
		*frames = t.frames;
	return RT_OK;
}

void rt_ring_reset_timers(rt_ring *r) {
	if (r)
		for (uint32_t s = 0; s < r->ring->size(); ++s)
			r->ring->host(s).resetTimers();
}

int rt_rccl_available(void) { return ocrt::rccl_available() ? 1 : 0; }

int rt_rccl_unique_id(void *out128) {
	if (!out128)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] { ocrt::rccl_unique_id(out128); });
}

int rt_ring_attach_rccl(rt_ring *r, const void *unique_id128) {
	if (!r || !unique_id128)
		return fail(RT_E_INVALID, "null argument");
	return guarded([&] {
		ocrt::DeviceRenderer &h = r->ring->host(0);
		const ocrt::Partition &part = h.params().part;
		r->ring->attachGather(std::unique_ptr<ocrt::BandGather>(new ocrt::BandGather(
		    h.rayTracer().options, part.rank, part.nranks, h.deviceIndex(), unique_id128, r->ring->slots())));
	});
}

int rt_ring_set_gather_timeout(rt_ring *r, double seconds) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] {
		if (!r->ring->hasGather())
			throw std::logic_error("no communicator attached (rt_ring_attach_rccl)");
		r->ring->gatherOrNull()->setTimeout(seconds);
	});
}

int rt_ring_rccl_info(rt_ring *r, int *comm_ranks, int *rccl_version) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] {
		if (!r->ring->hasGather())
			throw std::logic_error("no communicator attached (rt_ring_attach_rccl)");
		r->ring->gatherOrNull()->describe(comm_ranks, rccl_version);
	});
}

int rt_ring_rccl_self_test(rt_ring *r) {
	if (!r)
		return fail(RT_E_INVALID, "null ring");
	return guarded([&] {
		if (!r->ring->hasGather())
			throw std::logic_error("no communicator attached (rt_ring_attach_rccl)");
		r->ring->gatherSelfTest();
	});
}

void rt_print_info(void) { HipHost::printInfo(); }
// ---- rt_hip_query.h ----
namespace {

// (`f`: RAYS or INSTANCED_RAYS; `instance`: the instanced closest form's indices, or null)
int rays_call(rt_host *h, const Family &f, bool closest, const float *origins4, const float *directions4, uint32_t n, float max_distance,
              uint32_t flags, const ocrt::QueryOutputs &q, uint32_t *instance, Where where) {
	const int rc = query_precheck(h, f, origins4, directions4, n, !where.host);
	if (rc != RT_OK || n == 0)
		return rc;
	if (!where.host && !(records_aligned(q) && aligned({ instance }, 4)))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).trace(closest, origins4, directions4, n, max_distance, flags, q, where, f.instanced, instance); });
}

}  // namespace

int rt_trace_closest(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t flags,
                     const rt_hit_arrays *out) {
	return rays_call(h, RAYS, true, origins4, directions4, n, max_distance, flags, hit_outputs(out), nullptr, HOST);
}

int rt_trace_occluded(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t flags,
                      uint8_t *occluded) {
	return rays_call(h, RAYS, false, origins4, directions4, n, max_distance, flags, occlusion_outputs(occluded), nullptr, HOST);
}

int rt_trace_closest_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                            uint32_t flags, const rt_hit_arrays *out, void *hip_stream) {
	return rays_call(h, RAYS, true, origins4, directions4, n, max_distance, flags, hit_outputs(out), nullptr, on(hip_stream));
}

int rt_trace_occluded_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                             uint32_t flags, uint8_t *occluded, void *hip_stream) {
	return rays_call(h, RAYS, false, origins4, directions4, n, max_distance, flags, occlusion_outputs(occluded), nullptr, on(hip_stream));
}

// ---- rt_hip_segment.h ----
namespace {

ocrt::RayQueries::VisibilityOutputs visibility_outputs(const rt_visibility_arrays *from) {
	ocrt::RayQueries::VisibilityOutputs q;
	if (!from)
		return q;
	q.mask = from->mask;
	q.count = from->count;
	return q;
}

// (`f`: SEGMENTS or INSTANCED_SEGMENTS)
int segments_call(rt_host *h, const Family &f, bool closest, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi,
                  uint32_t flags, const ocrt::QueryOutputs &q, uint32_t *instance, Where where) {
	const int rc = query_precheck(h, f, from4, to4, n, !where.host);
	if (rc != RT_OK || n == 0)
		return rc;
	if (!where.host && !(records_aligned(q) && aligned({ instance }, 4)))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).segments(closest, from4, to4, n, t_lo, t_hi, flags, q, where, f.instanced, instance); });
}

int visibility_call(rt_host *h, const Family &f, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo, float t_hi,
                    uint32_t flags, const rt_visibility_arrays *out, Where where) {
	const uint64_t pairs = (uint64_t) np * nt;
	const int rc = query_precheck(h, f, points4, targets4, pairs, !where.host);
	if (rc != RT_OK || pairs == 0)
		return rc;
	const ocrt::RayQueries::VisibilityOutputs q = visibility_outputs(out);
	if (!where.host && !aligned({ q.mask, q.count }, 4))
		return fail(RT_E_INVALID, "device uint32 outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).visibility(points4, np, targets4, nt, t_lo, t_hi, flags, q, where, f.instanced); });
}

}  // namespace

int rt_segments_closest(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                        const rt_hit_arrays *out) {
	return segments_call(h, SEGMENTS, true, from4, to4, n, t_lo, t_hi, flags, hit_outputs(out), nullptr, HOST);
}

int rt_segments_occluded(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                         uint8_t *occluded) {
	return segments_call(h, SEGMENTS, false, from4, to4, n, t_lo, t_hi, flags, occlusion_outputs(occluded), nullptr, HOST);
}

int rt_segments_closest_device(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                               const rt_hit_arrays *out, void *hip_stream) {
	return segments_call(h, SEGMENTS, true, from4, to4, n, t_lo, t_hi, flags, hit_outputs(out), nullptr, on(hip_stream));
}

int rt_segments_occluded_device(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                                uint8_t *occluded, void *hip_stream) {
	return segments_call(h, SEGMENTS, false, from4, to4, n, t_lo, t_hi, flags, occlusion_outputs(occluded), nullptr, on(hip_stream));
}

int rt_visibility_masks(rt_host *h, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo, float t_hi,
                        uint32_t flags, const rt_visibility_arrays *out) {
	return visibility_call(h, SEGMENTS, points4, np, targets4, nt, t_lo, t_hi, flags, out, HOST);
}

int rt_visibility_masks_device(rt_host *h, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo,
                               float t_hi, uint32_t flags, const rt_visibility_arrays *out, void *hip_stream) {
	return visibility_call(h, SEGMENTS, points4, np, targets4, nt, t_lo, t_hi, flags, out, on(hip_stream));
}

// ---- rt_hip_instances.h ----
// (the set's own entry points work before an upload too: owned_precheck)
int rt_set_instances(rt_host *h, const float *world_from_object, uint32_t n) {
	const int rc = owned_precheck(h, "instanced ray");
	if (rc != RT_OK)
		return rc;
	if (n > RT_INSTANCES_MAX)
		return fail(RT_E_INVALID, "more instances than RT_INSTANCES_MAX");
	if (n > 0 && !world_from_object)
		return fail(RT_E_INVALID, "null transform array");
	if (n == 0 && !h->queries)
		return RT_OK;
	return guarded([&] { queries_of(h).setInstances(world_from_object, n); });
}

uint32_t rt_instance_count(const rt_host *h) { return h && h->queries ? h->queries->instanceCount() : 0u; }

uint32_t rt_instance_node_count(const rt_host *h) {
	const uint32_t n = rt_instance_count(h);
	return n ? 2u * n - 1u : 0u;
}

int rt_instances_object_from_world(rt_host *h, float *out) {
	const int rc = owned_precheck(h, "instanced ray");
	if (rc != RT_OK)
		return rc;
	if (!out || !h->queries)
		return RT_OK;
	return guarded([&] { h->queries->instanceInverses(out); });
}

// ---- rt_hip_instance_build.h ----
int rt_build_instances_device(rt_host *h, const float *world_from_object, uint32_t n, void *hip_stream) {
	const int rc = owned_precheck(h, "instanced ray");
	if (rc != RT_OK)
		return rc;
	if (n > RT_INSTANCES_MAX)
		return fail(RT_E_INVALID, "more instances than RT_INSTANCES_MAX");
	if (n > 0 && !world_from_object)
		return fail(RT_E_INVALID, "null transform array");
	if (n > 0 && !aligned({ world_from_object }, 16))
		return fail(RT_E_INVALID, "the device transform array must be 16-byte aligned");
	if (n == 0 && !h->queries)
		return RT_OK;
	return guarded([&] { queries_of(h).buildInstancesDevice(world_from_object, n, hip_stream); });
}

int rt_build_instances(rt_host *h, const float *world_from_object, uint32_t n) {
	const int rc = owned_precheck(h, "instanced ray");
	if (rc != RT_OK)
		return rc;
	if (n > RT_INSTANCES_MAX)
		return fail(RT_E_INVALID, "more instances than RT_INSTANCES_MAX");
	if (n > 0 && !world_from_object)
		return fail(RT_E_INVALID, "null transform array");
	if (n == 0 && !h->queries)
		return RT_OK;
	return guarded([&] { queries_of(h).buildInstancesHost(world_from_object, n); });
}

int rt_instances_world_from_object(rt_host *h, float *out) {
	const int rc = owned_precheck(h, "instanced ray");
	if (rc != RT_OK)
		return rc;
	if (!out || !h->queries)
		return RT_OK;
	return guarded([&] { h->queries->instanceWorld(out); });
}

int rt_instance_bounds(rt_host *h, float *out) {
	const int rc = host_precheck(h, "instanced ray");
	if (rc != RT_OK)
		return rc;
	if (!h->queries || h->queries->instanceCount() == 0)
		return fail(RT_E_STATE, "instance bounds without an instance set (rt_set_instances, rt_build_instances)");
	return guarded([&] { h->queries->instanceBounds(out); });
}

float rt_last_instance_build_ms(rt_host *h) {
	if (!h || !h->queries)
		return 0.0f;
	float ms = 0.0f;
	guarded([&] { ms = h->queries->lastInstanceBuildMs(); });
	return ms;
}

int rt_instance_nodes(rt_host *h, void *out) {
	const int rc = host_precheck(h, "instanced ray");
	if (rc != RT_OK)
		return rc;
	if (!h->queries || h->queries->instanceCount() == 0)
		return fail(RT_E_STATE, "instance tree without an instance set (rt_set_instances)");
	return guarded([&] { h->queries->instanceNodes(out); });
}

int rt_trace_instances_closest(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t flags,
                               const rt_instance_hit_arrays *out) {
	return rays_call(h, INSTANCED_RAYS, true, origins4, directions4, n, max_distance, flags, hit_outputs(out), instance_of(out), HOST);
}

int rt_trace_instances_occluded(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t flags,
                                uint8_t *occluded) {
	return rays_call(h, INSTANCED_RAYS, false, origins4, directions4, n, max_distance, flags, occlusion_outputs(occluded), nullptr, HOST);
}

int rt_trace_instances_closest_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                                      uint32_t flags, const rt_instance_hit_arrays *out, void *hip_stream) {
	return rays_call(h, INSTANCED_RAYS, true, origins4, directions4, n, max_distance, flags, hit_outputs(out), instance_of(out), on(hip_stream));
}

int rt_trace_instances_occluded_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                                       uint32_t flags, uint8_t *occluded, void *hip_stream) {
	return rays_call(h, INSTANCED_RAYS, false, origins4, directions4, n, max_distance, flags, occlusion_outputs(occluded), nullptr,
	                 on(hip_stream));
}

// ---- rt_hip_instance_segments.h ----
int rt_instances_segments_closest(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                                  const rt_instance_hit_arrays *out) {
	return segments_call(h, INSTANCED_SEGMENTS, true, from4, to4, n, t_lo, t_hi, flags, hit_outputs(out), instance_of(out), HOST);
}

int rt_instances_segments_occluded(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                                   uint8_t *occluded) {
	return segments_call(h, INSTANCED_SEGMENTS, false, from4, to4, n, t_lo, t_hi, flags, occlusion_outputs(occluded), nullptr, HOST);
}

int rt_instances_segments_closest_device(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi,
                                         uint32_t flags, const rt_instance_hit_arrays *out, void *hip_stream) {
	return segments_call(h, INSTANCED_SEGMENTS, true, from4, to4, n, t_lo, t_hi, flags, hit_outputs(out), instance_of(out), on(hip_stream));
}

int rt_instances_segments_occluded_device(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi,
                                          uint32_t flags, uint8_t *occluded, void *hip_stream) {
	return segments_call(h, INSTANCED_SEGMENTS, false, from4, to4, n, t_lo, t_hi, flags, occlusion_outputs(occluded), nullptr, on(hip_stream));
}

int rt_instances_visibility_masks(rt_host *h, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo, float t_hi,
                                  uint32_t flags, const rt_visibility_arrays *out) {
	return visibility_call(h, INSTANCED_SEGMENTS, points4, np, targets4, nt, t_lo, t_hi, flags, out, HOST);
}

int rt_instances_visibility_masks_device(rt_host *h, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo,
                                         float t_hi, uint32_t flags, const rt_visibility_arrays *out, void *hip_stream) {
	return visibility_call(h, INSTANCED_SEGMENTS, points4, np, targets4, nt, t_lo, t_hi, flags, out, on(hip_stream));
}

// ---- rt_hip_nearest.h ----
namespace {

// (`f`: POINTS or INSTANCED_POINTS)
int points_call(rt_host *h, const Family &f, const float *points4, uint32_t n, float max_distance, uint32_t flags, const ocrt::QueryOutputs &q,
                uint32_t *instance, Where where) {
	const int rc = query_precheck(h, f, points4, points4, n, !where.host);
	if (rc != RT_OK || n == 0)
		return rc;
	if (!where.host && !(records_aligned(q) && aligned({ instance }, 4)))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).nearest(points4, n, max_distance, flags, q, where, f.instanced, instance); });
}

int signed_call(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags, const rt_signed_arrays *out, Where where) {
	const int rc = query_precheck(h, SIGNED_POINTS, points4, points4, n, !where.host);
	if (rc != RT_OK || n == 0)
		return rc;
	const ocrt::QueryOutputs q = hit_outputs(out ? &out->hit : nullptr);
	if (!where.host && !records_aligned(q))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	if (!where.host && out && !aligned({ out->pseudonormal4 }, 16))
		return fail(RT_E_INVALID, "the device pseudonormal array must be 16-byte aligned");
	return guarded([&] {
		queries_of(h).signedDistance(points4, n, max_distance, flags, q, out ? out->feature : nullptr, out ? out->pseudonormal4 : nullptr, where);
	});
}

}  // namespace

int rt_closest_points(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags, const rt_hit_arrays *out) {
	return points_call(h, POINTS, points4, n, max_distance, flags, hit_outputs(out), nullptr, HOST);
}

int rt_closest_points_device(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags, const rt_hit_arrays *out,
                             void *hip_stream) {
	return points_call(h, POINTS, points4, n, max_distance, flags, hit_outputs(out), nullptr, on(hip_stream));
}

// ---- rt_hip_signed.h ----
int rt_signed_distance(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags, const rt_signed_arrays *out) {
	return signed_call(h, points4, n, max_distance, flags, out, HOST);
}

int rt_signed_distance_device(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags, const rt_signed_arrays *out,
                              void *hip_stream) {
	return signed_call(h, points4, n, max_distance, flags, out, on(hip_stream));
}

namespace {
// What both grid forms check before they touch the device (include/rt_hip_signed.h, "Errors").
int grid_precheck(const rt_host *h, const float *origin, const float *spacing, const uint32_t *dims) {
	const int rc = host_precheck(h, "signed distance");
	if (rc != RT_OK)
		return rc;
	if (!origin || !spacing || !dims)
		return fail(RT_E_INVALID, "null origin, spacing or dims");
	for (int k = 0; k < 3; ++k) {
		if (!(spacing[k] > 0.0f) || !std::isfinite(spacing[k]))
			return fail(RT_E_INVALID, "the grid's spacing must be positive and finite");
		if (dims[k] == 0)
			return fail(RT_E_INVALID, "a grid dimension of 0");
	}
	// (each factor below 2^32: the first product cannot wrap, the second is checked before it is made)
	const uint64_t slice = (uint64_t) dims[0] * dims[1], limit = (uint64_t) 1 << 31;
	if (slice > limit || slice * dims[2] > limit)
		return fail(RT_E_INVALID, "more than 2^31 voxels in one grid");
	return RT_OK;
}
}  // namespace

int rt_signed_distance_grid(rt_host *h, const float *origin, const float *spacing, const uint32_t *dims, float max_distance, float *distance,
                            uint32_t *leaf) {
	if (const int rc = grid_precheck(h, origin, spacing, dims); rc != RT_OK)
		return rc;
	return guarded([&] { queries_of(h).signedGridHost(origin, spacing, dims, max_distance, distance, leaf); });
}

int rt_signed_distance_grid_device(rt_host *h, const float *origin, const float *spacing, const uint32_t *dims, float max_distance,
                                   float *distance, uint32_t *leaf, void *hip_stream) {
	if (const int rc = grid_precheck(h, origin, spacing, dims); rc != RT_OK)
		return rc;
	if (!aligned({ distance, leaf }, 4))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).signedGridDevice(origin, spacing, dims, max_distance, distance, leaf, hip_stream); });
}

int rt_prepare_signed_distance(rt_host *h) {
	if (const int rc = host_precheck(h, "signed distance"); rc != RT_OK)
		return rc;
	return guarded([&] { queries_of(h).prepareSigned(nullptr); });
}

float rt_last_sign_build_ms(rt_host *h) {
	if (!h || !h->queries)
		return 0.0f;
	try {
		return h->queries->lastSignBuildMs();
	} catch (...) {
		fail_from_exception();
		return 0.0f;
	}
}

int rt_debug_sign_table(rt_host *h, float *table) {
	if (const int rc = host_precheck(h, "signed distance"); rc != RT_OK)
		return rc;
	if (!table)
		return fail(RT_E_INVALID, "null table");
	return guarded([&] { queries_of(h).downloadSignTable(table); });
}

// ---- rt_hip_instance_nearest.h ----
int rt_instances_closest_points(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags,
                                const rt_instance_hit_arrays *out) {
	return points_call(h, INSTANCED_POINTS, points4, n, max_distance, flags, hit_outputs(out), instance_of(out), HOST);
}

int rt_instances_closest_points_device(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags,
                                       const rt_instance_hit_arrays *out, void *hip_stream) {
	return points_call(h, INSTANCED_POINTS, points4, n, max_distance, flags, hit_outputs(out), instance_of(out), on(hip_stream));
}

int rt_debug_set_nearest_walk(rt_host *h, uint32_t flags) {
	if (const int rc = owned_precheck(h, "closest-point"); rc != RT_OK)
		return rc;
	return guarded([&] { queries_of(h).setNearestWalk(flags); });
}

int rt_debug_last_nearest_counts(rt_host *h, uint64_t *node_tests, uint64_t *triangle_tests) {
	if (const int rc = owned_precheck(h, "closest-point"); rc != RT_OK)
		return rc;
	uint64_t counts[2] = { 0u, 0u };
	const int rc = h->queries ? guarded([&] { h->queries->lastNearestCounts(counts); }) : RT_OK;
	if (node_tests)
		*node_tests = counts[0];
	if (triangle_tests)
		*triangle_tests = counts[1];
	return rc;
}

// ---- rt_hip_multihit.h ----
namespace {

// The checks of include/rt_hip_multihit.h ("Errors") beyond query_precheck's; `q`: the outputs asked for.
// (`f`: RAYS, or INSTANCED_RAYS with the slots' `instance` array beside them -- include/rt_hip_instance_multihit.h)
int multihit_call(rt_host *h, const Family &f, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k,
                  uint32_t flags, const ocrt::MultiHitOutputs &q, uint32_t *instance, Where where) {
	const int rc = query_precheck(h, f, origins4, directions4, n, !where.host);
	if (rc != RT_OK)
		return rc;
	if (k > RT_MULTIHIT_MAX_K)
		return fail(RT_E_INVALID, "more slots per ray than RT_MULTIHIT_MAX_K");
	if (k == 0 && (q.anySlot() || instance))
		return fail(RT_E_INVALID, "k == 0 asks for the count alone: the slot arrays must be null");
	if ((uint64_t) n * (k ? k : 1u) > RT_QUERY_MAX_RAYS)
		return fail(RT_E_INVALID, "more than RT_QUERY_MAX_RAYS slots (n * k) in one call");
	if (!where.host && !(aligned({ q.count, instance }, 4) && records_aligned(q)))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	if (n == 0)
		return RT_OK;
	return guarded([&] { queries_of(h).multihit(origins4, directions4, n, max_distance, k, flags, q, where, f.instanced, instance); });
}

}  // namespace

int rt_trace_multihit(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k,
                      uint32_t flags, const rt_multihit_arrays *out) {
	return multihit_call(h, RAYS, origins4, directions4, n, max_distance, k, flags, multihit_outputs(out), nullptr, HOST);
}

int rt_trace_multihit_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k,
                             uint32_t flags, const rt_multihit_arrays *out, void *hip_stream) {
	return multihit_call(h, RAYS, origins4, directions4, n, max_distance, k, flags, multihit_outputs(out), nullptr, on(hip_stream));
}

// ---- rt_hip_instance_multihit.h ----
int rt_trace_instances_multihit(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k,
                                uint32_t flags, const rt_instance_multihit_arrays *out) {
	return multihit_call(h, INSTANCED_RAYS, origins4, directions4, n, max_distance, k, flags, multihit_outputs(out), instance_of(out), HOST);
}

int rt_trace_instances_multihit_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                                       uint32_t k, uint32_t flags, const rt_instance_multihit_arrays *out, void *hip_stream) {
	return multihit_call(h, INSTANCED_RAYS, origins4, directions4, n, max_distance, k, flags, multihit_outputs(out), instance_of(out),
	                     on(hip_stream));
}

// ---- rt_hip_ao.h ----
int rt_ao_rays_per_point(const rt_host *h, uint32_t *rays, uint32_t *divisor) {
	uint32_t per_point = 0;
	const int rc = ao_precheck(h, nullptr, nullptr, 0, false, &per_point);
	if (rc != RT_OK)
		return rc;
	if (rays)
		*rays = per_point;
	if (divisor)
		*divisor = ocrt::RayQueries::aoDivisor(*h->dev);
	return RT_OK;
}

namespace {

// ao_precheck; `instanced` (include/rt_hip_instance_views.h, "Errors"): behind the instanced families' own two checks.
int ao_query_precheck(const rt_host *h, bool instanced, const float *points4, const float *normals4, uint32_t n, Where where) {
	int rc = instanced ? host_precheck(h, "instanced ambient-occlusion") : RT_OK;
	if (rc == RT_OK && instanced)
		rc = instance_set_required(h, "instanced ambient-occlusion query");
	return rc != RT_OK ? rc : ao_precheck(h, points4, normals4, n, !where.host, nullptr);
}

int ao_call(rt_host *h, bool instanced, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags,
            float *ao, uint32_t *occluded, Where where) {
	const int rc = ao_query_precheck(h, instanced, points4, normals4, n, where);
	if (rc != RT_OK || n == 0)
		return rc;
	if (!where.host && !aligned({ seeds, ao, occluded }, 4))
		return fail(RT_E_INVALID, "device seeds and outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).ao(points4, normals4, seeds, n, flags, ao, occluded, where, instanced); });
}

}  // namespace

int rt_trace_ao(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags, float *ao,
                uint32_t *occluded) {
	return ao_call(h, false, points4, normals4, seeds, n, flags, ao, occluded, HOST);
}

int rt_trace_ao_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags,
                       float *ao, uint32_t *occluded, void *hip_stream) {
	return ao_call(h, false, points4, normals4, seeds, n, flags, ao, occluded, on(hip_stream));
}

// ---- rt_hip_directional.h ----
namespace {

ocrt::RayQueries::DirectionalOutputs directional_outputs(const rt_ao_directional_arrays *from) {
	ocrt::RayQueries::DirectionalOutputs q;
	if (!from)
		return q;
	q.ao = from->ao;
	q.occluded = from->occluded;
	q.mask = from->mask;
	q.bent = from->bent;
	return q;
}

}  // namespace

int rt_ao_mask_words(const rt_host *h, uint32_t *words) {
	uint32_t per_point = 0;
	const int rc = ao_precheck(h, nullptr, nullptr, 0, false, &per_point);
	if (rc != RT_OK)
		return rc;
	if (words)
		*words = (per_point + 31u) / 32u;
	return RT_OK;
}

namespace {

int directional_call(rt_host *h, bool instanced, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                     uint32_t flags, const rt_ao_directional_arrays *out, Where where) {
	const int rc = ao_query_precheck(h, instanced, points4, normals4, n, where);
	if (rc != RT_OK || n == 0)
		return rc;
	const ocrt::RayQueries::DirectionalOutputs q = directional_outputs(out);
	if (!where.host && !aligned({ seeds, q.ao, q.occluded, q.mask, q.bent }, 4))
		return fail(RT_E_INVALID, "device seeds and outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).directional(points4, normals4, seeds, n, flags, q, where, instanced); });
}

int ao_rays_call(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, float *origins4,
                 float *directions4, Where where) {
	const int rc = ao_query_precheck(h, false, points4, normals4, n, where);
	if (rc != RT_OK || n == 0)
		return rc;
	if (!where.host && !aligned({ origins4, directions4 }, 16))
		return fail(RT_E_INVALID, "device origin and direction arrays must be 16-byte aligned");
	if (!where.host && !aligned({ seeds }, 4))
		return fail(RT_E_INVALID, "device seeds must be 4-byte aligned");
	return guarded([&] { queries_of(h).aoRays(points4, normals4, seeds, n, origins4, directions4, where); });
}

}  // namespace

int rt_trace_ao_directional(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags,
                            const rt_ao_directional_arrays *out) {
	return directional_call(h, false, points4, normals4, seeds, n, flags, out, HOST);
}

int rt_trace_ao_directional_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                                   uint32_t flags, const rt_ao_directional_arrays *out, void *hip_stream) {
	return directional_call(h, false, points4, normals4, seeds, n, flags, out, on(hip_stream));
}

int rt_ao_rays(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, float *origins4,
               float *directions4) {
	return ao_rays_call(h, points4, normals4, seeds, n, origins4, directions4, HOST);
}

int rt_ao_rays_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, float *origins4,
                      float *directions4, void *hip_stream) {
	return ao_rays_call(h, points4, normals4, seeds, n, origins4, directions4, on(hip_stream));
}

// ---- rt_hip_layers.h ----
namespace {

ocrt::LayerOutputs layer_outputs(const rt_layer_arrays &from) {
	ocrt::LayerOutputs q;
	q.hit = from.hit;
	record_outputs(&from, q);
	q.direction = from.direction;
	q.shade = from.shade;
	q.ao = from.ao;
	q.value = from.value;
	return q;
}

// What both layers entry points check before they touch the device (include/rt_hip_layers.h, "Errors"); the limits that
// depend on the host's options are RayQueries::requireLayers'.
int layers_precheck(const rt_host *h, const rt_layer_arrays *out) {
	const int rc = host_precheck(h, "frame-layer");
	if (rc != RT_OK)
		return rc;
	if (!out)
		return fail(RT_E_INVALID, "null layer arrays");
	return RT_OK;
}

int layers_call(rt_host *h, const rt_layer_arrays *out, Where where) {
	const int rc = layers_precheck(h, out);
	if (rc != RT_OK)
		return rc;
	const ocrt::LayerOutputs q = layer_outputs(*out);
	if (!where.host && !(records_aligned(q) && aligned({ q.direction, q.shade, q.ao, q.value }, 4)))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).layers(q, where); });
}

}  // namespace

int rt_render_layers(rt_host *h, const rt_layer_arrays *out) { return layers_call(h, out, HOST); }

int rt_render_layers_device(rt_host *h, const rt_layer_arrays *out, void *hip_stream) { return layers_call(h, out, on(hip_stream)); }

// ---- rt_hip_views.h ----
namespace {

// What both views entry points check before they touch the device (include/rt_hip_views.h, "Errors"); the limits that
// depend on the host's options are RayQueries::requireViews'.
int views_precheck(const rt_host *h, const rt_camera *cameras, uint32_t views, const rt_view_arrays *out) {
	const int rc = host_precheck(h, "multi-view");
	if (rc != RT_OK)
		return rc;
	if (!out)
		return fail(RT_E_INVALID, "null view arrays");
	if (views > 0 && !cameras)
		return fail(RT_E_INVALID, "null cameras");
	return RT_OK;
}

ocrt::ViewOutputs view_outputs(const rt_view_arrays &from) {
	ocrt::ViewOutputs q;
	static_cast<ocrt::LayerOutputs &>(q) = layer_outputs(from.layers);
	q.image = from.image;
	return q;
}

}  // namespace

int rt_render_views(rt_host *h, const rt_camera *cameras, uint32_t views, const rt_view_arrays *out) {
	const int rc = views_precheck(h, cameras, views, out);
	if (rc != RT_OK)
		return rc;
	return guarded([&] { queries_of(h).viewsHost(reinterpret_cast<const ocrt::CameraPose *>(cameras), views, view_outputs(*out)); });
}

int rt_render_views_device(rt_host *h, const rt_camera *cameras, uint32_t views, const rt_view_arrays *out, void *hip_stream) {
	const int rc = views_precheck(h, cameras, views, out);
	if (rc != RT_OK)
		return rc;
	const ocrt::ViewOutputs q = view_outputs(*out);
	if (!(records_aligned(q) && aligned({ q.direction, q.shade, q.ao, q.value }, 4)))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	return guarded([&] { queries_of(h).viewsDevice(reinterpret_cast<const ocrt::CameraPose *>(cameras), views, q, hip_stream); });
}

// ---- rt_hip_instance_views.h ----
namespace {

int instance_views_precheck(const rt_host *h, const rt_camera *cameras, uint32_t views, const rt_instance_view_arrays *out) {
	int rc = host_precheck(h, "instanced multi-view");
	if (rc == RT_OK)
		rc = instance_set_required(h, "instanced views");
	return rc != RT_OK ? rc : views_precheck(h, cameras, views, out ? &out->views : nullptr);
}

}  // namespace

int rt_trace_instances_ao(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags,
                          float *ao, uint32_t *occluded) {
	return ao_call(h, true, points4, normals4, seeds, n, flags, ao, occluded, HOST);
}

int rt_trace_instances_ao_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                                 uint32_t flags, float *ao, uint32_t *occluded, void *hip_stream) {
	return ao_call(h, true, points4, normals4, seeds, n, flags, ao, occluded, on(hip_stream));
}

// ---- rt_hip_instance_directional.h ----
int rt_trace_instances_ao_directional(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                                      uint32_t flags, const rt_ao_directional_arrays *out) {
	return directional_call(h, true, points4, normals4, seeds, n, flags, out, HOST);
}

int rt_trace_instances_ao_directional_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds,
                                             uint32_t n, uint32_t flags, const rt_ao_directional_arrays *out, void *hip_stream) {
	return directional_call(h, true, points4, normals4, seeds, n, flags, out, on(hip_stream));
}

// ---- rt_hip_instance_views.h: the views ----
int rt_render_instance_views(rt_host *h, const rt_camera *cameras, uint32_t views, const rt_instance_view_arrays *out) {
	const int rc = instance_views_precheck(h, cameras, views, out);
	if (rc != RT_OK)
		return rc;
	return guarded([&] {
		queries_of(h).instanceViewsHost(reinterpret_cast<const ocrt::CameraPose *>(cameras), views, view_outputs(out->views), out->instance);
	});
}

int rt_render_instance_views_device(rt_host *h, const rt_camera *cameras, uint32_t views, const rt_instance_view_arrays *out,
                                    void *hip_stream) {
	const int rc = instance_views_precheck(h, cameras, views, out);
	if (rc != RT_OK)
		return rc;
	const ocrt::ViewOutputs q = view_outputs(out->views);
	if (!(records_aligned(q) && aligned({ q.direction, q.shade, q.ao, q.value, out->instance }, 4)))
		return fail(RT_E_INVALID, "device float / uint32 outputs must be 4-byte aligned");
	return guarded([&] {
		queries_of(h).instanceViewsDevice(reinterpret_cast<const ocrt::CameraPose *>(cameras), views, q, out->instance, hip_stream);
	});
}

int rt_debug_set_views_chunk(rt_host *h, uint32_t max_views) {
	if (const int rc = owned_precheck(h, "multi-view"); rc != RT_OK)
		return rc;
	return guarded([&] { queries_of(h).setViewsChunk(max_views); });
}

int rt_debug_last_views(rt_host *h, uint32_t *views, uint32_t *chunks, uint64_t *ao_points) {
	if (const int rc = owned_precheck(h, "multi-view"); rc != RT_OK)
		return rc;
	const ocrt::RayQueries::ViewsDone done = h->queries ? h->queries->lastViews() : ocrt::RayQueries::ViewsDone();
	if (views)
		*views = done.views;
	if (chunks)
		*chunks = done.chunks;
	if (ao_points)
		*ao_points = done.ao_points;
	return RT_OK;
}

// ---- rt_hip_update.h ----
namespace {

int update_precheck(const rt_host *h, const float *vertices4) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	if (!h->owned)
		return fail(RT_E_STATE, "vertex updates are not available on the hosts of a frame ring: their scene on the device is shared (one copy, many readers)");
	if (!h->dev->sceneReady())
		return fail(RT_E_STATE, "vertex update before a scene was uploaded");
	if (!vertices4)
		return fail(RT_E_INVALID, "null vertex array");
	return RT_OK;
}

}  // namespace

int rt_update_vertices(rt_host *h, const float *vertices4, const float *vnormals4, uint32_t num_vertices) {
	const int rc = update_precheck(h, vertices4);
	if (rc != RT_OK)
		return rc;
	return guarded([&] { queries_of(h).updateHost(vertices4, vnormals4, num_vertices); });
}

int rt_update_vertices_device(rt_host *h, const float *vertices4, const float *vnormals4, uint32_t num_vertices, void *hip_stream) {
	const int rc = update_precheck(h, vertices4);
	if (rc != RT_OK)
		return rc;
	if (!aligned({ vertices4, vnormals4 }, 16))
		return fail(RT_E_INVALID, "device vertex and normal arrays must be 16-byte aligned");
	return guarded([&] { queries_of(h).updateDevice(vertices4, vnormals4, num_vertices, hip_stream); });
}

int rt_scene_refit(rt_scene *s, const float *vertices4, uint32_t num_vertices) {
	if (!s || !vertices4)
		return fail(RT_E_INVALID, "null argument");
	if (num_vertices != s->mesh.vertices.size())
		return fail(RT_E_INVALID, "refit: the number of vertices differs from the scene's (the topology stays: every position is replaced)");
	for (size_t i = 0; i < (size_t) num_vertices; ++i)
		for (unsigned k = 0; k < 3; ++k)
			if (!(std::fabs(vertices4[4 * i + k]) <= 1.0e37f))
				return fail(RT_E_INVALID, "refit: a coordinate is not finite or exceeds 1e37 (nothing was written)");
	return guarded([&] {
		for (uint32_t i = 0; i < num_vertices; ++i)
			s->mesh.vertices[i] = Vec3f(vertices4[4 * i], vertices4[4 * i + 1], vertices4[4 * i + 2]);
		compute_vertex_normals(&s->mesh);
		if (s->built)
			ocrt::refit_boxes(s->bvh.nodes, s->sorted_faces, s->mesh.vertices, s->bvh.aabbs);
	});
}

float rt_last_update_ms(const rt_host *h) {
	if (!h || !h->queries)
		return 0.0f;
	try {
		return h->queries->lastUpdateMs();
	} catch (...) {
		fail_from_exception();
		return 0.0f;
	}
}

// ---- rt_hip_build.h ----
namespace {

int build_precheck(const rt_host *h, const float *vertices4, const uint32_t *faces, uint32_t num_vertices, uint32_t num_faces) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	if (!h->owned)
		return fail(RT_E_STATE, "builds are not available on the hosts of a frame ring: their scene on the device is shared (one copy, many readers)");
	if (!vertices4 || !faces)
		return fail(RT_E_INVALID, "build: null vertex or face array");
	if (num_faces == 0 || num_vertices == 0)
		return fail(RT_E_INVALID, "build: no faces, or no vertices");
	if (num_faces >= (1u << 25))
		return fail(RT_E_INVALID, "build: scene too large for 32-bit device offsets");
	return RT_OK;
}

}  // namespace

int rt_build_scene(rt_host *h, const float *vertices4, const float *vnormals4, uint32_t num_vertices, const uint32_t *faces, uint32_t num_faces) {
	const int rc = build_precheck(h, vertices4, faces, num_vertices, num_faces);
	if (rc != RT_OK)
		return rc;
	return guarded([&] {
		Mesh mesh;  // (without normals: the CPU's routine over the same faces, as rt_scene_from_arrays)
		if (!vnormals4) {
			for (size_t i = 0; i < (size_t) num_faces * 3; ++i)
				if (faces[i] >= num_vertices)
					throw std::invalid_argument("build: face references a vertex out of range (nothing was written)");
			mesh.vertices.resize(num_vertices);
			for (uint32_t i = 0; i < num_vertices; ++i)
				mesh.vertices[i] = Vec3f(vertices4[4 * i], vertices4[4 * i + 1], vertices4[4 * i + 2]);
			mesh.faces.assign(faces, faces + 3 * (size_t) num_faces);
			compute_vertex_normals(&mesh);
		}
		queries_of(h).buildHost(vertices4, vnormals4 ? vnormals4 : &mesh.vnormals.data()->x, num_vertices, faces, num_faces);
	});
}

int rt_build_scene_device(rt_host *h, const float *vertices4, const float *vnormals4, uint32_t num_vertices, const uint32_t *faces,
                          uint32_t num_faces, void *hip_stream) {
	const int rc = build_precheck(h, vertices4, faces, num_vertices, num_faces);
	if (rc != RT_OK)
		return rc;
	if (!vnormals4)
		return fail(RT_E_INVALID, "build: null normal array (the device does not compute vertex normals: rt_hip_build.h)");
	if (!aligned({ vertices4, vnormals4 }, 16) || !aligned({ faces }, 4))
		return fail(RT_E_INVALID, "device vertex and normal arrays must be 16-byte aligned, the face array 4-byte aligned");
	return guarded([&] { queries_of(h).buildDevice(vertices4, vnormals4, num_vertices, faces, num_faces, hip_stream); });
}

int rt_built_faces(const rt_host *h, uint32_t *face_of_leaf) {
	if (!h || !face_of_leaf)
		return fail(RT_E_INVALID, "null argument");
	if (!h->dev->sceneReady() || !h->dev->deviceScene() || h->dev->deviceScene()->builtFaces().empty())
		return fail(RT_E_STATE, "the host's scene was not built on the device (an uploaded scene's leaf order is rt_scene_triangles)");
	const std::vector<uint32_t> &faces = h->dev->deviceScene()->builtFaces();
	std::copy(faces.begin(), faces.end(), face_of_leaf);
	return RT_OK;
}

int rt_scene_build_lbvh(rt_scene *s) {
	if (!s)
		return fail(RT_E_INVALID, "null scene");
	return guarded([&] {
		s->built = false;
		// The tree of rt_hip_build.h, steps 1-6: leaf boxes by the refit rule, the root box over them, 30-bit Morton keys of the
		// boxes' centres, the stable order by key, the binary radix tree over key << 32 | leaf, laid out in pre-order (lbvh.h) --
		// and step 8: every box by the refit rule.
		ocrt::LbvhTree tree = ocrt::lbvh_build(s->mesh.faces, s->mesh.vertices);
		s->bvh = BVH();
		s->bvh.nodes = std::move(tree.nodes);
		s->bvh.triangles = std::move(tree.triangles);
		s->bvh.aabbs.assign(2 * s->bvh.nodes.size(), Vec3f());
		s->sorted_faces = sort_faces_by_leaf_order(s->mesh, s->bvh);
		ocrt::refit_boxes(s->bvh.nodes, s->sorted_faces, s->mesh.vertices, s->bvh.aabbs);
		s->built = true;
	});
}

float rt_last_build_ms(const rt_host *h) {
	if (!h || !h->queries)
		return 0.0f;
	try {
		return h->queries->lastBuildMs();
	} catch (...) {
		fail_from_exception();
		return 0.0f;
	}
}

int rt_debug_last_build_times(rt_host *h, float ms3[3]) {
	if (!h || !ms3)
		return fail(RT_E_INVALID, "null argument");
	ms3[0] = ms3[1] = ms3[2] = 0.0f;
	if (!h->queries)
		return RT_OK;
	return guarded([&] { h->queries->lastBuildTimes(ms3); });
}

int rt_debug_set_refit_group(rt_host *h, uint32_t nodes) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	h->dev->setRefitGroup(nodes);
	return RT_OK;
}

int rt_debug_download_records(rt_host *h, void *nodes_out, void *tris_out, void *shade_out) {
	const int rc = host_precheck(h, "record");
	if (rc != RT_OK)
		return rc;
	return guarded([&] { queries_of(h).downloadRecords(nodes_out, tris_out, shade_out); });
}

int rt_debug_record_counts(const rt_host *h, uint32_t *nodes, uint32_t *leaves) {
	if (!h)
		return fail(RT_E_INVALID, "null host");
	if (!h->dev->sceneReady() || !h->dev->deviceScene())
		return fail(RT_E_STATE, "no scene on the device");
	if (nodes)
		*nodes = h->dev->deviceScene()->nodeCount();
	if (leaves)
		*leaves = h->dev->deviceScene()->triCount();
	return RT_OK;
}

int rt_debug_refit_schedule(const rt_scene *s, uint32_t group_nodes, int packed_tree, uint32_t counts6[6], uint32_t *skips_out, uint32_t *entries_out,
                            uint32_t *children_out, uint32_t *groups_out) {
	if (!s || !counts6)
		return fail(RT_E_INVALID, "null argument");
	if (!s->built)
		return fail(RT_E_STATE, "scene has no BVH yet (call rt_scene_build_bvh)");
	return guarded([&] {
		std::vector<uint32_t> skips = s->bvh.nodes;
		if (packed_tree) {  // the tree an upload puts on the device: the uploaded one, or the cheaper one pack_scene made of its leaves
			const ocrt::PackedScene packed = ocrt::pack_scene(s->sorted_faces, s->bvh.nodes, s->bvh.aabbs, s->mesh.vertices, s->mesh.vnormals);
			skips.resize(packed.nodes.size());
			for (size_t i = 0; i < packed.nodes.size(); ++i)
				skips[i] = packed.nodes[i].skip;
		}
		const ocrt::RefitSchedule schedule = ocrt::make_refit_schedule(skips, group_nodes);
		counts6[0] = (uint32_t) skips.size();
		counts6[1] = (uint32_t) (schedule.entries.size() / 4);
		counts6[2] = (uint32_t) schedule.children.size();
		counts6[3] = (uint32_t) (schedule.groups.size() / 4);
		counts6[4] = schedule.passes();
		counts6[5] = schedule.group_nodes;
		if (skips_out)
			std::copy(skips.begin(), skips.end(), skips_out);
		if (entries_out)
			std::copy(schedule.entries.begin(), schedule.entries.end(), entries_out);
		if (children_out)
			std::copy(schedule.children.begin(), schedule.children.end(), children_out);
		if (groups_out)
			std::copy(schedule.groups.begin(), schedule.groups.end(), groups_out);
	});
}

float rt_last_query_ms(const rt_host *h) {
	if (!h || !h->queries)
		return 0.0f;
	try {
		return h->queries->lastMs();
	} catch (...) {
		fail_from_exception();
		return 0.0f;
	}
}

int rt_device_count(void) { return ocrt::visible_device_count(); }

// ---- rt_hip_camera.h ----
void rt_camera_default(rt_camera *out) {
	if (out)
		from_pose(ocrt::default_camera_pose(), out);
}

int rt_camera_look_at(const float eye[3], const float target[3], const float up_hint[3], rt_camera *out) {
	if (!eye || !target || !up_hint || !out)
		return fail(RT_E_INVALID, "null argument");
	ocrt::CameraPose pose;
	if (!ocrt::camera_look_at(eye, target, up_hint, &pose))
		return fail(RT_E_INVALID, "no camera there: the eye, the target and the up hint must be finite, the eye must differ from the target, and the up hint must not lie along the view direction");
	from_pose(pose, out);
	return RT_OK;
}

int rt_set_camera(rt_host *h, const rt_camera *cam) {
	if (!h || !cam)
		return fail(RT_E_INVALID, "null argument");
	if (!h->owned)
		return fail(RT_E_STATE, "the hosts of a frame ring take the ring's camera (rt_ring_set_camera)");
	if (h->dev->sceneReady())
		return fail(RT_E_STATE, "set the camera first: rt_set_camera comes before rt_upload (an upload prepares the scene for one view)");
	return guarded([&] { h->dev->setCamera(to_pose(*cam)); });
}

int rt_get_camera(const rt_host *h, rt_camera *out, int *is_set) {
	if (!h || !out)
		return fail(RT_E_INVALID, "null argument");
	from_pose(h->dev->camera(), out);
	if (is_set)
		*is_set = h->dev->cameraIsSet() ? 1 : 0;
	return RT_OK;
}

int rt_ring_set_camera(rt_ring *r, const rt_camera *cam) {
	if (!r || !cam)
		return fail(RT_E_INVALID, "null argument");
	if (r->ring->host(0).sceneReady())
		return fail(RT_E_STATE, "set the camera first: rt_ring_set_camera comes before rt_ring_upload (an upload prepares the scene for one view)");
	return guarded([&] { r->ring->setCamera(to_pose(*cam)); });
}

}  // extern "C"
