// ray_query.h -- RayQueries: everything a render host answers about its uploaded scene beyond its own frames.  One
// method per query family (rays, segments, visibility masks, closest and signed points, multi-hit, ambient and
// directional occlusion, the rays of a point, frame layers), each for arrays in device memory or in host memory
// (Where); multi-view rendering; the instance set the `instanced` forms are cast against; vertex updates and
// device-side builds of the renderer's scene.  The C contracts are include/rt_hip_*.h, the kernels kernels/*.hip.h.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <vector>

#include "device_renderer.h"
#include "instances.h"

namespace ocrt {

// (QueryOutputs, MultiHitOutputs: device_types.h)

// What one render host needs beyond its renderer to answer queries: scratch of its own (the sort's counts and order,
// the staging buffers of the host-memory form), grown on demand and never shared with the frame's buffers, and the
// events that time the last query.  Reads the renderer's scene and stream, changes nothing of it.
class RayQueries {
	public:
		explicit RayQueries(DeviceRenderer &renderer);
		~RayQueries();
		RayQueries(const RayQueries &) = delete;
		RayQueries &operator=(const RayQueries &) = delete;

		// Where a call's arrays live: device memory, the call enqueued on `stream` (null: the renderer's) -- or host memory,
		// the call blocking: the arrays go through the staging buffer on the renderer's own stream (staged(), below).
		struct Where {
			bool host;
			void *stream;
			static Where deviceMemory(void *stream) { return Where{ false, stream }; }
			static Where hostMemory() { return Where{ true, nullptr }; }
		};
		// Rays, segments, visibility masks, points and ambient-occlusion points are cast against the uploaded scene or --
		// `instanced` -- in world space against the host's instance set (setInstances below; include/rt_hip_instances.h,
		// rt_hip_instance_segments.h, rt_hip_instance_views.h): the family's own arguments and rules, the sort keyed over the
		// top-level root box, `instance` (or null) beside a closest form's record.  std::logic_error without a set; its tree
		// is made again first if the scene changed.
		// Ray queries (include/rt_hip_query.h); `closest` false: occlusion into out.hit alone.
		void trace(bool closest, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t flags,
		           QueryOutputs out, Where where, bool instanced = false, uint32_t *instance = nullptr);
		// Multi-hit queries (include/rt_hip_multihit.h): the count of accepted triangles per ray and the first k of them;
		// k <= RT_MULTIHIT_MAX_K, 0 = the count alone.  `instanced` (include/rt_hip_instance_multihit.h): the (instance,
		// triangle) pairs among the posed copies, `instance` [n * k] (or null) beside the slot arrays; ignored on a plain call.
		void multihit(const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k, uint32_t flags,
		              MultiHitOutputs out, Where where, bool instanced = false, uint32_t *instance = nullptr);
		// Closest-point queries (include/rt_hip_nearest.h): the nearest point of the surface for each of n points, the record
		// of a closest hit (out.hit: `found`).  `instanced` (include/rt_hip_instance_nearest.h): the nearest point among the
		// posed copies, in world space.
		void nearest(const float *points4, uint32_t n, float max_distance, uint32_t flags, QueryOutputs out, Where where,
		             bool instanced = false, uint32_t *instance = nullptr);
		// Signed distance queries (include/rt_hip_signed.h): nearest's walk and rules, the distance signed by the
		// pseudonormal of the feature the nearest point lies on, out of the sign table -- made by the first of these calls
		// after an upload or a build (prepareSigned: ahead of time), its sums redone after an update.  `feature` (n bytes),
		// `pseudonormal4` (float4[n]): outputs beside the record's, either may be null.
		void signedDistance(const float *points4, uint32_t n, float max_distance, uint32_t flags, QueryOutputs out, uint8_t *feature,
		                    float *pseudonormal4, Where where);
		// The grid form: voxel (i, j, k) is origin + (i, j, k) * spacing; `distance`, `leaf`: [dims[2]][dims[1]][dims[0]], either
		// may be null.  The host form goes through the staging buffer in slabs of z-slices.
		void signedGridDevice(const float origin[3], const float spacing[3], const uint32_t dims[3], float max_distance, float *distance,
		                      uint32_t *leaf, void *stream, uint32_t z_first = 0);
		void signedGridHost(const float origin[3], const float spacing[3], const uint32_t dims[3], float max_distance, float *distance,
		                    uint32_t *leaf);
		void prepareSigned(void *stream);  // blocking
		float lastSignBuildMs();           // HIP-event time of the last build or refresh of the table (0: none yet)
		void downloadSignTable(void *out);  // triCount() records of 96 bytes (made first, if need be), once everything enqueued has finished
		// (include/rt_hip_debug.h) how the later closest-point queries walk (RT_DEBUG_NEAREST_*; the A/B build's: std::logic_error
		// for a flag in the product library), and the counts of the last counted one (waits for it)
		void setNearestWalk(uint32_t debug_flags);
		void lastNearestCounts(uint64_t counts[2]);
		// Segment queries (include/rt_hip_segment.h): segment i runs from from4[i] to to4[i]; its blockers are the triangles
		// the reference accepts for the ray (from, to - from) with a plane parameter inside (t_lo, t_hi), behind boxes that
		// pass the slab test with max_distance = t_hi.  `closest` false: occlusion into out.hit alone.
		void segments(bool closest, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
		              QueryOutputs out, Where where, bool instanced = false, uint32_t *instance = nullptr);
		// The many-to-many form: np points against nt targets, bit j of point i's row (visibilityWords(nt) words) set where
		// segment (i, j) is occluded, and the row's popcount.  Either output may be null.  No np x nt array is made.
		struct VisibilityOutputs {
			uint32_t *mask = nullptr, *count = nullptr;
			bool any() const { return mask || count; }
		};
		static uint32_t visibilityWords(uint32_t nt) { return (nt + 31u) / 32u; }
		void visibility(const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo, float t_hi, uint32_t flags,
		                VisibilityOutputs out, Where where, bool instanced = false);
		// The instance set (include/rt_hip_instances.h).  The set -- transforms, inverses and the top-level tree over the
		// scene's root box (instances.h) -- is kept here and, as float4[3n] + float4[3n] + NodeRec[2n - 1] + float4[n] (the
		// closest-point walk's bounds), in device memory of this object's own; it outlives updates, builds and uploads, after which the tree is made again before its next use.
		// std::invalid_argument for a refused transform or too many (the set stays what it was); n == 0 clears the set.
		void setInstances(const float *world_from_object, uint32_t n);
		uint32_t instanceCount() const { return inst_built ? inst_built_n : (uint32_t) (inst_world.size() / 12u); }
		// the tree as it is on the device, 2n - 1 records (waits for the queries; std::logic_error before an upload or a set)
		void instanceNodes(void *out);
		// Device-side instance sets (include/rt_hip_instance_build.h): the set made on the device from `world_from_object` in
		// device memory -- copied into memory of this object's own, then checked, inverted, boxed, keyed, sorted and laid out by
		// kernels/instance_build.hip.h into a SPARE allocation that takes the place of the set's once the flag has come back
		// clear; the host keeps the count and the root record alone.  Ordered as a build: behind this host's queries by their
		// event, enqueued on `stream` (null: the renderer's), one wait for the flag and the root record (36 bytes).
		// std::invalid_argument for a refused transform (the set stays what it was), a null array or too many; n == 0 clears
		// the set.  Before an upload the transforms are checked and kept; the tree is made at the first use.
		void buildInstancesDevice(const float *world_from_object, uint32_t n, void *stream);
		// Host memory: one upload through the staging buffer, then the same.
		void buildInstancesHost(const float *world_from_object, uint32_t n);
		// What the set holds, either kind: a built set's arrays are read from the device (waits for the queries).  The bounds
		// are made again first if the scene changed, as the tree is (std::logic_error before an upload or a set).
		void instanceWorld(float *out);
		void instanceInverses(float *out);
		void instanceBounds(float *out);
		float lastInstanceBuildMs();  // HIP-event time of the last device-side plan's launches (0: none yet)
		// Instanced views (include/rt_hip_instance_views.h): viewsDevice's arguments and rules, the rays cast against the
		// instance set; the records are the instanced ray queries', `instance` [views][N] beside the layers.
		void instanceViewsDevice(const CameraPose *cameras, uint32_t views, const ViewOutputs &out, uint32_t *instance, void *stream);
		void instanceViewsHost(const CameraPose *cameras, uint32_t views, const ViewOutputs &out, uint32_t *instance);
		// Ambient-occlusion queries (include/rt_hip_ao.h): the reference's ambient_occlusion() of n points with the options
		// the scene was uploaded for -- table, mode, rays per point, divisor and reach come from the renderer's launch
		// constants and its DeviceScene.  std::logic_error where those options have ambient occlusion off.
		// (static: what a renderer's uploaded scene answers, before any query has made scratch for it)
		static uint32_t aoRaysPerPoint(const DeviceRenderer &renderer);  // 0: not available
		static uint32_t aoDivisor(const DeviceRenderer &renderer);
		// `seeds`, `ao`, `occluded` may be null.
		void ao(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags, float *ao, uint32_t *occluded,
		        Where where, bool instanced = false);
		// Directional occlusion queries (include/rt_hip_directional.h): the same rays, their hit flags a bit each in `mask`
		// (aoMaskWords() words per point), the count and value made of a point's row, and the ordered sum of its open rays'
		// directions.  Any output may be null; errors as for ao.  `instanced` (include/rt_hip_instance_directional.h):
		// world-space points, the rays cast against the instance set.
		struct DirectionalOutputs {
			float *ao = nullptr;
			uint32_t *occluded = nullptr, *mask = nullptr;
			float *bent = nullptr;
			bool any() const { return ao || occluded || mask || bent; }
		};
		static uint32_t aoMaskWords(const DeviceRenderer &renderer) { return (aoRaysPerPoint(renderer) + 31u) / 32u; }
		void directional(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags,
		                 DirectionalOutputs out, Where where, bool instanced = false);
		// The rays themselves: origins4 float4[n], directions4 float4[n * rays per point]; either may be null; no walk is run.
		void aoRays(const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, float *origins4, float *directions4,
		            Where where);
		// Frame layers (include/rt_hip_layers.h): the closest-hit record of every sub-pixel's own ray -- the host's pose,
		// DeviceRenderer::camera() / cameraIsSet() --, its direction, head-light term, ambient-occlusion factor and their
		// product.  std::logic_error on a band-partitioned host and for out.ao where the options have ambient occlusion
		// off; std::invalid_argument where the ambient-occlusion step would exceed a query's rays.
		void layers(LayerOutputs out, Where where);
		// Multi-view rendering (include/rt_hip_views.h): the layers and the 8-bit image of `views` poses -- `cameras`, host
		// memory, copied before the call returns -- against the uploaded scene, whatever pose the host itself has; view v's
		// block of every array lies behind view v - 1's.  Worked through in chunks of viewsPerChunk() views, scratch for one
		// chunk.  Errors as for the layers; std::invalid_argument where ONE view exceeds what a layers call takes.
		// Device memory, enqueued on `stream` (null: the renderer's).  With the ambient-occlusion step the call waits, per
		// chunk, for the chunk's own rays: how many sub-pixels they hit sizes that step.
		void viewsDevice(const CameraPose *cameras, uint32_t views, const ViewOutputs &out, void *stream);
		// Host memory, blocking: staged chunk by chunk.
		void viewsHost(const CameraPose *cameras, uint32_t views, const ViewOutputs &out);
		// (include/rt_hip_debug.h) at most `max_views` views per chunk, 0: as many as fit; and what the last views call did
		void setViewsChunk(uint32_t max_views) { views_chunk = max_views; }
		struct ViewsDone {
			uint32_t views = 0, chunks = 0;
			uint64_t ao_points = 0;  // sub-pixels the ambient-occlusion step ran over: the hit ones
		};
		ViewsDone lastViews() const { return last_views; }
		float lastMs();  // the last query of any kind
		// Vertex updates (include/rt_hip_update.h): the renderer's own scene refitted on the device from `vertices4` (and
		// `vnormals4`, or null: the shading normals stay) -- serialised with this host's queries by the event they use among
		// themselves, and behind whatever the renderer's frame stream holds; a later query sees the whole update.  Closes
		// the renderer's frame path until its next upload (DeviceRenderer::markSceneUpdated) and drops the cached root box.
		// std::logic_error before an upload and on a shared scene, std::invalid_argument for another vertex count.
		// Device memory, enqueued on `stream` (null: the renderer's).
		void updateDevice(const float *vertices4, const float *vnormals4, uint32_t num_vertices, void *stream);
		// Host memory, blocking; refuses coordinates that are not finite or beyond 1e37 before anything is written.
		void updateHost(const float *vertices4, const float *vnormals4, uint32_t num_vertices);
		float lastUpdateMs();  // HIP-event time of the last update's launches (0: none yet)
		// Device-side builds (include/rt_hip_build.h): a scene made on the device from faces, vertices and normals
		// (DeviceScene::build) takes the place of the renderer's own -- or comes first.  Ordered as an update is, and the sort's
		// cached root box is dropped; the call waits once for its stream (the skips and the flag come back to the host).  Closes
		// the frame path as an update does.  std::logic_error on a shared scene; std::invalid_argument for null arrays, no
		// face, too many, and -- after the launches, the renderer's scene untouched -- for a face index out of range.
		// Device memory, enqueued on `stream` (null: the renderer's).
		void buildDevice(const float *vertices4, const float *vnormals4, uint32_t num_vertices, const uint32_t *faces, uint32_t num_faces,
		                 void *stream);
		// Host memory, blocking; refuses bad indices and what updateHost refuses of coordinates before anything is launched.
		void buildHost(const float *vertices4, const float *vnormals4, uint32_t num_vertices, const uint32_t *faces, uint32_t num_faces);
		float lastBuildMs();  // HIP-event time of the last build's launches, both runs (0: none yet)
		// (include/rt_hip_debug.h) ... apart: the topology's launches, the records' launches, the host's download-to-schedule
		// step between them (wall clock)
		void lastBuildTimes(float ms[3]);
		// (include/rt_hip_debug.h) the three record arrays as they are on the device, once everything enqueued has finished
		void downloadRecords(void *nodes_out, void *tris_out, void *shade_out);

	private:
		struct Scratch {  // device memory of this host's own, grown on demand
			void *ptr = nullptr;
			size_t bytes = 0;
		};
		// The arrays of a call, named once: the address of each pointer variable, its bytes, and whether the array is read
		// (`in`), written (`out`) or written whether the caller wants it or not (`scratch`: staged even where the pointer is
		// null, never copied back then).  A null `in` or `out` is no array at all.
		class Arrays {
			public:
				template <class T> Arrays &in(const T *&p, size_t bytes) { return add(&p, bytes, p != nullptr, true); }
				template <class T> Arrays &out(T *&p, size_t bytes) { return add(&p, bytes, p != nullptr, false); }
				template <class T> Arrays &scratch(T *&p, size_t bytes) { return add(&p, bytes, true, false); }
				Arrays &records(RecordOutputs &r, size_t records);  // the five arrays of a record, `records` records each
				Arrays &layers(LayerOutputs &l, size_t records);    // the hit flags, the record and the four layers of a frame's rays

			private:
				friend class RayQueries;
				struct Piece {
					void *variable;  // where the pointer is kept: read as the host's address, then given the staging buffer's
					size_t bytes;
					bool input;
					void *host = nullptr, *device = nullptr;
				};
				Arrays &add(void *variable, size_t bytes, bool wanted, bool input);
				Piece piece[16];
				size_t count = 0;
		};
		// What every call does with its arrays once it knows that it has work.  Device memory: body(where.stream).  Host
		// memory: the wanted arrays one behind the other in the staging buffer, each rounded up to 16 bytes, the inputs
		// uploaded, the pointer variables set to the device addresses, body(the renderer's own stream), the outputs copied back,
		// one wait.
		template <class Body> void staged(Where where, Arrays &arrays, Body &&body);
		struct Need {  // scratch of a family's own that begin() grows with the sort's
			Scratch *scratch;  // (null: none)
			size_t bytes;
		};
		struct Enqueue {
			void *stream;
			const void *order;  // the sort's order of the n items, or null: unsorted
		};

		void requireScene(const char *query) const;
		// The way into a call of `query` that may run against the instance set: the scene and -- `instanced` -- the set, or
		// std::logic_error; then, once the call knows that it has work, what it hands begin() and its launcher.
		void requireQuery(bool instanced, const char *query) const;
		struct Target {
			const InstanceBuffers *set;  // null: the uploaded scene alone
			const float *box;            // the sort's origin cells where they are not the scene's root box's, or null
		};
		Target target(bool instanced);
		void requireSlots(uint32_t k) const;
		void requireAo() const;
		bool requireLayers(const LayerOutputs &out) const;  // true: the call needs the ambient-occlusion step
		bool requireViews(const ViewOutputs &out) const;    // the same for a views call
		bool requireFrameRays(bool ao, bool product) const;
		uint32_t viewsPerChunk(bool with_ao) const;
		// Where the pieces of a chunk's scratch lie in `views`: `poses` poses, the ambient-occlusion step's `entries` points
		// and normals, with `listing` the list of the hit ones (ViewList), and `products` floats of the chunk's own.
		struct ChunkScratch {
			size_t poses, listed, points, normals, seeds, order, flags, sums, product, bytes;
		};
		static ChunkScratch chunkScratch(size_t poses, size_t entries, bool listing, size_t products);
		// A layers or views call between begin() and end(): the frame's own rays of `views` views -- `poses` on the device, or
		// null: the host's own pose, one view -- into `to`, the blocks of the first view, then where `with_ao` the
		// ambient-occlusion step and its tail into to.ao and `product`.  `listing`: the step runs over the hit sub-pixels
		// alone, and the call waits for their number, which it returns; else over all of them, enqueued like the rest.
		// `instanced`: both against the instance set (listing, poses on the device), `instance` its layer or null.
		uint32_t castChunk(const Enqueue &q, const ChunkScratch &at, bool listing, const void *poses, uint32_t views, const LayerOutputs &to,
		                   float *product, bool with_ao, bool instanced = false, uint32_t *instance = nullptr);
		// viewsDevice and instanceViewsDevice, viewsHost and instanceViewsHost: one chunk loop each
		void viewsCall(bool instanced, const CameraPose *cameras, uint32_t views, const ViewOutputs &out, uint32_t *instance, void *stream);
		void viewsStaged(bool instanced, const CameraPose *cameras, uint32_t views, const ViewOutputs &host, uint32_t *instance);
		static ViewOutputs viewsFrom(const ViewOutputs &out, size_t view, const KernelParams &kp, size_t image_bytes);
		void grow(Scratch &scratch, size_t bytes);
		void sceneBox(const DeviceScene &scene, float lo[3], float scale[3]);
		// The way into a call's launches, in two steps: enter() -- this device, the stream (null: the renderer's), behind the
		// query before -- and begin() on the stream entered.
		// (`segments`: keys_a4, keys_b4 are the two ends of segments, keyed as the rays (a, b - a); `box`: lo[3] and scale[3] of
		// the origin cells where they are not the scene's root box's)
		void *enter(void *stream);
		Enqueue begin(void *entered, const float *keys_a4, const float *keys_b4, uint32_t n, uint64_t rays, uint32_t flags,
		              std::initializer_list<Need> needs = {}, bool segments = false, const float *box = nullptr);
		void end(const Enqueue &q);
		// The ambient-occlusion step between begin() and end(): n entries -- point order[j], or j where `order` is null --,
		// counted into `count` by point index (the caller's `occluded` or ao_hits).  `instanced`: against the instance set.
		void aoEnqueue(const Enqueue &q, const float *points4, const float *normals4, const uint32_t *seeds, const void *order, uint32_t n,
		               uint32_t *count, float *ao, bool instanced = false);
		void *stageIn(Arrays &arrays);  // returns the stream
		void stageOut(const Arrays &arrays, void *stream);

		DeviceRenderer &dev;
		Scratch count, order;  // the sort's histogram and the order it makes
		Scratch stage;         // the host-memory forms' inputs and outputs
		Scratch ao_hits;       // ao without an `occluded` array: the points' counts
		Scratch ao_rows;       // directional without a `mask` array: the points' rows
		Scratch vis_rows;      // visibility without a `mask` array: the points' rows
		Scratch list;          // multihit: the rays' key lists, n * k * 8 bytes (instanced: 12)
		Scratch views;         // layers, viewsDevice (ChunkScratch): a chunk's poses, the points and normals of its
		                       // ambient-occlusion step, the list of the hit ones (ViewList), its float images where the caller
		                       // gave no `value` array
		void *pinned = nullptr;  // viewsDevice, host memory: the list's size as read back, then the call's poses
		size_t pinned_bytes = 0;
		uint32_t views_chunk = 0;
		ViewsDone last_views;
		void *ev_start = nullptr, *ev_stop = nullptr;
		bool timed = false, have_ms = false;
		float last_ms = 0.0f;
		void *ev_update_start = nullptr, *ev_update_stop = nullptr, *ev_frames = nullptr;  // an update's own times; the frame stream's tail
		bool update_timed = false, have_update_ms = false;
		float last_update_ms = 0.0f;
		Scratch build;  // buildDevice: DeviceScene::buildScratchBytes
		void *ev_build[4] = { nullptr, nullptr, nullptr, nullptr };  // around a build's two runs of launches
		bool build_timed = false, have_build_ms = false;
		float last_build_ms[3] = { 0.0f, 0.0f, 0.0f };  // topology, records, the host's step between them
		// Closest-point queries.  coords_flag: one word on the device, non-zero where the last update or build through this
		// object was given a coordinate that is no number or beyond 1e37 (checked on the device, behind the update's own
		// launches: the device-memory forms cannot look) -- the boxes of `flagged` then promise nothing and its closest-point
		// walks pass no box by.  nearest_counts: the counted form's two words.
		void checkCoordinates(const std::shared_ptr<const DeviceScene> &scene, const float *vertices4, uint32_t num_vertices, void *stream);
		Scratch coords_flag, nearest_counts;
		// Signed distance queries.  sign_table: a SignRec of 96 bytes per leaf; sign_vertices, sign_edges: the kept incidence, a
		// word per corner each (kernels/signed.hip.h).  signed_scene: the scene whose topology they were made for (an upload
		// or a build brings another); sign_fresh: the sums are the current positions' (an update ends that).
		Scratch sign_table, sign_vertices, sign_edges;
		std::weak_ptr<const DeviceScene> signed_scene;
		bool sign_fresh = false, sign_timed = false;
		void *ev_sign[2] = { nullptr, nullptr };
		const void *ensureSignTable(void *stream);
		uint32_t nearestWalk(const DeviceScene &scene) const;
		std::weak_ptr<const DeviceScene> flagged;  // the scene coords_flag speaks of
		uint32_t nearest_debug = 0;
		bool nearest_counted = false;
		std::weak_ptr<const DeviceScene> boxed;  // the scene box_lo / box_scale were read from
		float box_lo[3] = { 0, 0, 0 }, box_scale[3] = { 0, 0, 0 };
		// The instance set.  inst_device: the transforms, the inverses, the tree -- inst_set: where the last two lie in it --;
		// inst_scene / inst_current: the scene whose root box the tree was made from, and whether that box still stands (an
		// update or a build drops it, as it drops `boxed`).
		void requireInstances(const char *what) const;
		void refreshInstances();
		std::vector<float> inst_world, inst_inverse;
		std::vector<InstanceNode> inst_nodes;
		Scratch inst_device;
		InstanceBuffers inst_set = { nullptr, nullptr, 0u };
		std::weak_ptr<const DeviceScene> inst_scene;
		bool inst_current = false;
		float inst_box[6] = { 0, 0, 0, 0, 0, 0 };  // the sort's origin cells over the top-level root box: lo, scale
		void setInstanceBox(const float lo[3], const float hi[3]);
		// A device-built set (include/rt_hip_instance_build.h): inst_built, its size; the vectors above stay empty, inst_device
		// holds transforms, inverses, flag, tree and bounds (InstanceSetLayout).  inst_spare: the allocation the next plan goes
		// into; inst_plan: that plan's temporaries.
		struct InstanceSetLayout {
			size_t inverse, flag, tree, bounds, bytes;  // (the transforms lie at 0; the flag's word directly in front of the tree)
		};
		static InstanceSetLayout instanceSetLayout(uint32_t n);
		// Plans `n` transforms -- in device memory; may be the current set's own -- into inst_spare and, accepted, swaps it in.
		bool planInstancesOnDevice(const float *world_device, uint32_t n, void *stream);
		void clearInstances();
		bool inst_built = false;
		uint32_t inst_built_n = 0;
		Scratch inst_spare, inst_plan;
		void *ev_inst[2] = { nullptr, nullptr };
		bool inst_timed = false, have_inst_ms = false;
		float last_inst_ms = 0.0f;
};

// kernels.hip
void launch_query_sort(const void *origins, const void *directions, uint32_t n, const float lo[3], const float scale[3], void *count,
                       void *order, void *stream, bool segments = false);
// (`set`: null, or the instance set a family's rays are cast against; `instance`: its index beside a closest form's record)
void launch_query(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, bool closest, const void *origins,
                  const void *directions, const void *order, uint32_t n, float max_distance, const QueryOutputs &out, uint32_t *instance,
                  void *stream);
void launch_nearest_sort(const void *points, uint32_t n, const float lo[3], const float scale[3], void *count, void *order, void *stream);
void launch_nearest(const SceneBuffers &scene, uint32_t node_count, uint32_t tri_count, const InstanceBuffers *set, const void *points,
                    const void *order, uint32_t n, float max_distance, uint32_t walk, const QueryOutputs &out, uint32_t *instance,
                    const void *coords_flag, void *counts, void *stream);
void launch_nearest_coordinates(const void *vertices4, uint32_t num_vertices, void *flag, void *stream);
// signed distance queries (kernels/signed.hip.h, sign_sort.hip)
size_t sign_sort_bytes(uint32_t pairs);
void launch_sign_sort(bool wide, void *temporary, size_t temporary_bytes, const void *keys_in, void *keys_out, const void *values_in,
                      void *values_out, uint32_t pairs, void *stream);
void launch_sign_keys(const void *faces, uint32_t tri_count, void *vertex_keys, void *edge_keys, void *values, void *stream);
void launch_sign_heads(bool wide, const void *sorted_keys, const void *sorted_values, uint32_t tri_count, void *kept, void *stream);
void launch_sign_sums(const void *kept_vertices, const void *kept_edges, const SceneBuffers &scene, uint32_t tri_count, void *table, void *stream);
void launch_signed(const SceneBuffers &scene, uint32_t node_count, uint32_t tri_count, const void *points, const void *order, uint32_t n,
                   float max_distance, uint32_t walk, const QueryOutputs &out, uint8_t *feature, float *pseudonormal4, const void *table,
                   const void *coords_flag, void *stream);
void launch_signed_grid(const SceneBuffers &scene, uint32_t node_count, uint32_t tri_count, const float origin[3], const float spacing[3],
                        uint32_t nx, uint32_t ny, uint32_t nz, uint32_t z_first, float max_distance, uint32_t walk, float *distance,
                        uint32_t *leaf, const void *table, const void *coords_flag, void *stream);
void launch_segments(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, bool closest, const void *from, const void *to,
                     const void *order, uint32_t n, float t_lo, float t_hi, const QueryOutputs &out, uint32_t *instance, void *stream);
void launch_visibility(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, const void *points, uint32_t np,
                       const void *targets, uint32_t nt, const void *order, float t_lo, float t_hi, uint32_t *mask, uint32_t *count,
                       void *stream);
void launch_multihit(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, const void *origins, const void *directions,
                     const void *order, uint32_t n, float max_distance, uint32_t k, void *list, const MultiHitOutputs &out, uint32_t *instance,
                     void *stream);
void launch_ao_query(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, int ao_mode, uint32_t rays_per_point,
                     uint32_t divisor, float max_distance, const void *points, const void *normals, const uint32_t *seeds, const void *order,
                     uint32_t n, uint32_t *count, float *ao, void *stream);
void launch_ao_directional(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, int ao_mode, uint32_t rays_per_point, uint32_t divisor,
                           float max_distance, const void *points, const void *normals, const uint32_t *seeds, const void *order, uint32_t n,
                           uint32_t *mask, uint32_t *occluded, float *ao, float *bent, void *stream);
void launch_ao_rays(const SceneBuffers &scene, int ao_mode, uint32_t rays_per_point, const void *points, const void *normals,
                    const uint32_t *seeds, uint32_t n, void *origins, void *directions, void *stream);
void launch_layers(const SceneBuffers &scene, const KernelParams &P, const InstanceBuffers *set, const void *poses, const CameraPose &pose,
                   bool posed, uint32_t views, const LayerOutputs &out, uint32_t *instance, float *value, float *ao, float *product,
                   const ViewList *list, void *stream);
void launch_views_scatter(const ViewList &list, const uint32_t *count, uint32_t divisor, float *ao, float *product, uint32_t listed,
                          void *stream);
void launch_views_resize(const float *value, unsigned char *image, const KernelParams &P, uint32_t out_width, uint32_t out_height,
                         uint32_t n, uint32_t views, void *stream);

}  // namespace ocrt
