// device_renderer.h -- owns the HIP device state of one render host: scene
// buffers, image buffers, stream, timing events.  All failures are reported as
// exceptions (ocrt::DeviceError / std::invalid_argument); the two front ends
// (HipHost with the reference's print-and-exit convention, the C ABI with
// return codes) decide what to do with them.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_types.h"
#include "ray_tracer.h"
#include "scene_pack.h"

namespace ocrt {

struct DeviceError : std::runtime_error {
	using std::runtime_error::runtime_error;
};

// Number of visible HIP devices (0 when the runtime reports none or fails).
int visible_device_count();
// Initialises the HIP runtime, the device's context and this library's code object on it (device < 0: $OCRT_DEVICE or
// 0); never fails -- whatever is wrong shows up again, properly reported, when a renderer is created.  These one-off
// costs (100-200 ms) are independent of the scene: a front end runs this on a second thread while it loads the mesh
// and builds the BVH (render.cc).
void warm_up_device(int device);

// One uploaded scene on one GPU: node arrays, leaf records, normals, direction table.  Immutable once made and
// reference-counted, so that every renderer of that GPU that renders the scene -- the hosts of a frame ring -- walks
// the SAME arrays: one upload, one copy in HBM, and the frames that overlap on the device find each other's nodes in
// the XCDs' L2 and the scalar caches instead of competing for them with identical copies (the reference uploads a scene
// once, src/opencl_host.cc:120-136).  Holds what the launch constants need to know of it as well.
class DeviceScene {
	public:
		// Blocking upload; `options`: the direction table (AO samples, angles, method) and the any-hit rays' reach
		// (AO_MAX_DISTANCE, which sizes the walk array's margins) are baked in -- servesOptions() says whether another
		// renderer's options agree.
		// (`for_a_stream`: make_walk_array's -- what only pays over many frames of the scene)
		// (`eye`: make_walk_array's -- where the primary rays of the renderers that will adopt the scene start; nullptr: the
		// reference's camera.  The walk array is made for that eye: servesEye() says whether a renderer's agrees.)
		// (Returned non-const: the renderer that made the scene and shares it with nobody may refit it -- updateVertices below.
		// Everybody it is handed on to gets a pointer to const.)
		static std::shared_ptr<DeviceScene> create(int device, const PackedScene &scene, const RayTracer::Options &options, bool for_a_stream = true,
		                                           const float *eye = nullptr);
		// A scene's arrays live in ONE device allocation.  A front end that knows the size of what is coming before it has
		// the arrays (the triangle count of a mesh file's header) can have that allocation made ahead of time -- on the
		// thread that brings the device up -- and create() takes it over if it is large enough (else it is dropped).
		// bytesFor: an upper bound of the allocation for a mesh of that many triangles.
		static void reserve(int device, size_t bytes);
		static size_t bytesFor(size_t triangles, size_t ao_directions);
		~DeviceScene();
		DeviceScene(const DeviceScene &) = delete;
		DeviceScene &operator=(const DeviceScene &) = delete;
		bool servesOptions(const RayTracer::Options &options) const;
		bool servesEye(const float *eye) const { return same_eye(walk_eye, eye); }

		SceneBuffers buffers() const { return SceneBuffers{ d_nodes, d_walk, d_tris, d_shade, d_ao }; }
		int device() const { return device_index; }
		size_t bytes() const { return device_bytes; }  // requested on the device
		uint32_t nodeCount() const { return node_count; }
		uint32_t triCount() const { return tri_count; }
		uint32_t aoDirs() const { return ao_dirs; }
		const SceneFacts &facts() const { return scene_facts_; }
		// Every box holds the triangles beneath it: the packer checked the uploaded arrays (PackedScene::enclosing), or the boxes
		// are the refit rule's -- after an update or a device-side build, whose coordinates the host may not have seen: the
		// closest-point queries hold a flag on the device against those (RayQueries::updateDevice).
		bool boxesEnclose() const { return scene_facts_.boxes_enclose; }

		// Vertex updates (include/rt_hip_update.h; kernels/refit.hip.h).  The records of `nodes`, `tris` and `shade` are made
		// again on the device from `vertices4` (float4 per vertex, vertexCount() of them) and, where given, `vnormals4`;
		// enqueued on `stream`, nothing is waited for.  What the launches need beside the records -- the leaf-ordered faces,
		// the leaf -> node map, the schedule of the inner boxes -- is kept on the HOST from the upload on and goes to the
		// device, into an allocation of its own, with the first update: bytes(), bytesFor() and the arena are an upload's as
		// they always were.  `group_nodes`: RefitSchedule's (0: the default); the schedule is made again when it changes.
		// The padded walk array is NOT remade: it stays the old positions'.
		uint32_t vertexCount() const { return vertex_count; }
		void updateVertices(const float *vertices4, const float *vnormals4, uint32_t group_nodes, void *stream);
		uint32_t refitPasses() const { return (uint32_t) (refit_pass_first.empty() ? 0 : refit_pass_first.size() - 1); }
		size_t refitBytes() const { return refit_bytes; }  // the allocation of the first update (0 before it)

		// Device-side builds (include/rt_hip_build.h; kernels/build.hip.h, build_sort.hip, lbvh.h): a scene made ON the device
		// from `num_faces` faces (three vertex ids each) over `num_vertices` vertices and normals (float4 each), all in device
		// memory -- the exact node records, the leaf records, the shading normals and the options' direction table; no padded
		// walk array.  Enqueued on `stream`, which is waited for ONCE: the skips come back to the host (4 bytes per node) for
		// the schedule of the inner boxes, and with them the flag a face index out of range raised (std::invalid_argument
		// then; nothing was read out of bounds) and the face of every leaf.  The scene keeps the leaf-ordered faces, the
		// leaf -> node map and the schedule: its first updateVertices prepares nothing.  `scratch`: buildScratchBytes(num_faces)
		// bytes of the caller's, free again when `stream` has run.  `events`: four events recorded around the two runs of
		// launches, before and after the wait; `host_ms`: what the download and the schedule took on the host.
		static size_t buildScratchBytes(uint32_t num_faces);
		static std::shared_ptr<DeviceScene> build(int device, const RayTracer::Options &options, const float *vertices4, const float *vnormals4,
		                                          uint32_t num_vertices, const uint32_t *faces, uint32_t num_faces, uint32_t group_nodes,
		                                          void *scratch, void *stream, void *const events[4], float *host_ms);
		// The leaf-ordered faces (three vertex ids per leaf), for what is made of the topology beside the records (the signed
		// distance queries' sign table, ray_query.cc): on the device where a build or a first update has put them, else
		// null; on the host where an upload kept them, else null.
		const void *deviceFaces() const { return d_faces; }
		const std::vector<uint32_t> *hostFaces() const { return leaf_faces.get(); }
		// the file-order face of every leaf of a built scene (empty: the scene was uploaded)
		const std::vector<uint32_t> &builtFaces() const { return built_faces; }

	private:
		DeviceScene() = default;
		std::vector<float> takeOptions(const RayTracer::Options &options);  // what of the options a scene holds; returns the direction table
		void finishTable(const RayTracer::Options &options, size_t table_bytes);
		void uploadSchedule(uint32_t wanted);
		std::vector<uint32_t> built_faces;
		// host side of the vertex updates: kept from the upload on
		std::shared_ptr<const std::vector<uint32_t>> leaf_faces;  // three vertex ids per leaf
		std::vector<uint32_t> node_skips, leaf_nodes;             // the tree's shape; the node of every leaf
		uint32_t vertex_count = 0;
		// device side: made by the first update
		void *refit_arena = nullptr;
		void *d_faces = nullptr, *d_leaf_nodes = nullptr, *d_entries = nullptr, *d_children = nullptr, *d_groups = nullptr;
		size_t refit_bytes = 0, schedule_capacity = 0;
		void *d_schedule = nullptr;  // entries, children, groups of the schedule in use (one allocation, remade with group_nodes)
		uint32_t refit_group_nodes = 0;  // the schedule on the device was made for this (0: none yet)
		std::vector<uint32_t> refit_pass_first;
		void prepareRefit(uint32_t group_nodes);
		int device_index = 0;
		void *arena = nullptr;  // the one allocation the five arrays below point into
		void *d_nodes = nullptr, *d_walk = nullptr, *d_tris = nullptr, *d_shade = nullptr, *d_ao = nullptr;
		size_t device_bytes = 0;
		uint32_t node_count = 0, tri_count = 0, ao_dirs = 0;
		SceneFacts scene_facts_;
		// what of the options went into it
		bool ao_on = false;
		int ao_method = 0;
		unsigned int ao_samples = 0;
		int ao_alpha_min = 0, ao_alpha_max = 0;
		float walk_distance = 0.0f;
		float walk_eye[3] = { 0.0f, 0.0f, 2.0f };  // the eye the walk array was made for
};

class DeviceRenderer {
	public:
		// `ring_slot`: this renderer's index among the renderers that take frames in turn on its GPU (FrameRing), -1 for
		// a renderer on its own.  It picks the priority class of the renderer's stream, see the constructor.
		// `spare_top_class`: leave the highest stream-priority class to somebody else (the ring's exchange step, whose
		// stream must never queue behind a frame).
		DeviceRenderer(const RayTracer::Options &options, int device, unsigned int rank, unsigned int nranks, int ring_slot = -1,
		               bool spare_top_class = false);
		~DeviceRenderer();
		DeviceRenderer(const DeviceRenderer &) = delete;
		DeviceRenderer &operator=(const DeviceRenderer &) = delete;

		// Blocking upload of a packed scene; returns the bytes requested on the device (scene + this renderer's buffers).
		size_t upload(const PackedScene &scene);
		// Renders a scene that is on the device already (DeviceScene::create on this renderer's device, for options that
		// agree with this renderer's: std::invalid_argument otherwise); returns the bytes of this renderer's own buffers.
		// `layout_from`: a renderer of the SAME scene, options and partition that has adopted it already (a ring's first
		// host): the hit list's layout is copied from it instead of being counted again.
		size_t adopt(std::shared_ptr<const DeviceScene> scene, const DeviceRenderer *layout_from = nullptr);
		const std::shared_ptr<const DeviceScene> &deviceScene() const { return scene_on_device; }
		// Vertex updates (include/rt_hip_update.h): the scene this renderer uploaded ITSELF and shares with nobody, for
		// writing -- null where there is none, `why` then says which of the two it is.  A scene that was adopted, or that
		// another renderer has adopted from this one, stays one copy with many readers.
		DeviceScene *updatableScene(const char **why);
		// After an update the frame path is closed until the next upload: the padded walk array, the hit list's size, the
		// claim orders and the walk intervals were all made for the old positions (enqueueRender, enqueueFrame,
		// prepareFrame, the calibrations and expectFrames throw std::logic_error).  The queries, layers and views walk
		// the exact records and go on.
		void markSceneUpdated() { scene_updated = true; }
		bool sceneUpdated() const { return scene_updated; }
		// Device-side builds (include/rt_hip_build.h): `scene`, made by DeviceScene::build on this renderer's device for its
		// options, takes the place of whatever scene the renderer had -- its own, for writing.  It has no padded walk array and
		// nothing an upload prepares for the renderer's one view: the frame path is closed as after an update, until the
		// next upload.  sceneIsShared(): the renderer's scene has other readers (a ring's hosts): no build may replace it.
		void adoptBuilt(std::shared_ptr<DeviceScene> scene);
		bool sceneIsShared() const;
		const RayTracer::Options &options() const { return opts; }
		// (include/rt_hip_debug.h) the schedule's group size for this renderer's updates; 0: the default
		void setRefitGroup(uint32_t nodes) { refit_group = nodes; }
		uint32_t refitGroup() const { return refit_group; }
		// The camera pose (device_types.h: CameraPose): where this renderer's primary rays start and the basis their
		// directions are made in, used as given.  BEFORE the upload only (std::logic_error afterwards): the walk array, the
		// hit list's size, the tile order and the walk intervals are all made once per upload, for one view.  A renderer
		// that is never given a pose renders the reference's view with the kernels that hold it as constants.
		void setCamera(const CameraPose &pose);
		bool cameraIsSet() const { return pose_set; }
		const CameraPose &camera() const { return pose; }

		// Enqueues the ray-casting kernel for this rank's bands on the stream.
		void enqueueRender();
		// Enqueues the device-side resize of this rank's bands into the compact
		// uint8 band buffer (localRows() x width bytes).
		void enqueueResize();
		// Same, but writes into caller-provided DEVICE memory (e.g. a torch tensor).
		void enqueueResizeInto(void *device_u8);
		// One whole frame -- counters, primary pass, ordering step, ambient-occlusion pass, resolve, device resize into
		// `device_u8` (nullptr: this renderer's own band buffer) -- enqueued as ONE replay of a captured hipGraph
		// (setGraphMode(false): as the same sequence of launches).  The graph is captured at the first call and again
		// whenever what it bakes in has changed (scene, destination, stream, share of the device).
		void enqueueFrame(void *device_u8 = nullptr);
		// Captures the frame for that destination now (graph mode; a few milliseconds), so that the first enqueueFrame for
		// it is a replay like every later one.
		void prepareFrame(void *device_u8 = nullptr);
		void setGraphMode(bool on) { graph_mode = on; }
		bool sceneReady() const { return scene_ready; }
		bool graphMode() const { return graph_mode; }
		// Waits for everything enqueued so far and folds pending event pairs into
		// the kernel-time statistics.
		void synchronize();
		void waitForStream();  // the wait alone (synchronize() then finds the stream idle)
		// Frame time stamps: with an epoch event set (recorded by the caller on any stream of this device), synchronize()
		// also keeps, for the last frame it folds, the milliseconds from the epoch to the frame's begin, to the start and
		// the end of its ambient-occlusion kernel (0 for a frame without one) and to its end -- what a test needs to see
		// that frames of different renderers really overlap on the device.
		void setEpochEvent(void *event) { epoch_event = event; }
		// A frame replayed from the captured graph holds no HIP events that could be timed; with this on, synchronize()
		// reads the device-clock stamps the kernels left in the frame's counters (a 24-byte blocking copy per frame)
		// for the ao_kernel times.  Plain launches always carry their own events.
		void setKeepStamps(bool on) { keep_stamps = on; }
		const float *lastFrameTimes() const { return last_times; }

		// The compact uint8 band buffer on this renderer's device (localRows() x width bytes), valid after
		// enqueueResize() has completed; and the stream everything is enqueued on.
		const void *deviceBands() const { return d_u8; }
		void *streamHandle() const { return stream; }
		// How many hosts take frames in turn on this GPU.  Alone, the persistent ambient-occlusion pass fills the chip
		// (8 workgroups per CU); in company it leaves room -- 4.5 per CU with up to five hosts, 3 from six on (the small
		// shares of a frame split over many GPUs) -- so that the other frames' passes run beside it all the time and not
		// only while it runs out (rounds 2-3 measured 5.5 per CU; re-swept on round 4's kernels, profiles/r04_notes.md
		// section 14: three hosts, whole frame, 5.5 -> 4.5 per CU: headline -1.5 %, interior -3.5 %, 600^2 +-0; an eighth
		// of the headline frame with twelve hosts 0.162 -> 0.153 ms, a quarter with six 0.289 -> 0.272).
		void setDeviceShare(unsigned hosts) {
			device_share = hosts < 1u ? 1u : hosts;
			kp.shared_device = device_share > 1u ? 1 : 0;
		}
		// Which form of the ambient-occlusion pass's node loop is launched: with (default) or without the look-ahead loads
		// of kernels.hip, OCRT_PF_SUCCESSORS -- same results, the faster one depends on the scene.  calibrateAoPrefetch()
		// renders a few frames one at a time with each form (plain launches, HIP events around the ao_kernel), keeps the
		// faster one and returns the two medians in ms (a frame ring does this once per uploaded scene).
		void setAoPrefetch(bool on);
		// Where the tiles' any-hit walks enter the tree (sizeHitList, entry_kernel): of the tiles with hits, how many walk
		// less than the whole tree, and the mean share of the node records a tile's rays are confined to.
		struct WalkEntries {
			uint32_t tiles_hit, tiles_narrowed;
			double mean_share;         // ... by the tile's own interval (any ray from the tile)
			double mean_packet_share;  // ... by the intervals its packets use (a full tile's: one per table direction)
		};
		WalkEntries walkEntries() const;
		// Where the intervals the packets use END, read back from the device and held against the records they index (the
		// centre / half-extent copy): the any-hit loop checks `end` only where a miss jump or the step off a leaf can land on
		// it (kernels/walk.hip.h, OCRT_DESCEND_UNCHECKED), which rests on ends being subtree ends.
		struct IntervalEnds {
			uint32_t intervals;      // the intervals looked at: per tile with hits the ones its packets use
			uint32_t whole_array;    // ... that end at or behind the array's end (a one-shot host's: all)
			uint32_t after_leaf;     // ... that end behind a leaf record: the end of a subtree
			uint32_t after_inner;    // ... that end behind an inner node, on its first child (entry_kernel's `end = n`): a descend can land there
			uint32_t last_is_leaf;   // of after_leaf: the last child taken is a leaf itself (left by the step off it, or its miss)
			uint32_t last_is_inner;  // of after_leaf: ... an inner node whose miss jump lands exactly on the end
		};
		IntervalEnds walkIntervalEnds() const;
		bool aoPrefetch() const { return ao_prefetch; }
		// How many frames of the scene the caller is going to render (default 1: the reference's use, one frame per
		// process, src/render.cc:86-111).  What an upload prepares beyond the scene itself only pays over a stream of frames:
		// the walk intervals (a second pass of the primary kernel + entry_kernel: ~0.55 ms at 1080p, worth ~0.04 ms per
		// headline frame, ~0.15 ms per frame of the interior scene) are made from FRAMES_WORTH_INTERVALS announced frames on,
		// and a frame ring -- which announces a stream -- also measures the tiles' costs and the form of the node loop.
		// Callable before or after the upload (after: the hit list is laid out again if the answer changes).
		static constexpr uint64_t FRAMES_WORTH_INTERVALS = 16;
		static constexpr float CHEAP_BELOW_DEFAULT = 0.15f;  // (OrderPolicy::cheap_below; swept over 0 / 0.15 / 0.25 / 0.4: profiles/ao_cheap_claims_notes.md)
		void expectFrames(uint64_t frames);
		uint64_t expectedFrames() const { return expected_frames; }
		bool walkIntervalsInUse() const { return intervals_in_use; }
		// What the tiles' ambient-occlusion packets really cost, and the order the pass claims them in made from that
		// (orderByMeasuredCost): `frames` frames one at a time (plain launches) whose AO pass books every claim's duration
		// -- device clock, between the workgroup's barriers -- to the claim's tiles.  Once per upload, for callers that
		// announce a stream of frames (a frame ring); returns false where there is nothing to measure.
		// `reorder` false: the costs are taken and the list in place stays as it is, its split prefix and cheap suffix with it.
		bool measureTileCosts(unsigned frames = 2, bool reorder = true);
		// ... and the order another renderer of the same frame (scene, options, partition) has arrived at
		void takeOrderFrom(const DeviceRenderer &other);
		bool orderIsMeasured() const { return tile_cost.size() == tile_count && tile_count != 0; }
		void setOrderPolicy(float heavy, float runway, float split_above = -1.0f);  // (split_above < 0: unchanged)
		// primary pass: tiles of cost class `above` or more (the leaves their packet stops at, 1 ... 64) are cast in quarters by
		// the four waves of a workgroup (0: none); re-makes the pass's list
		void setPrimarySplit(uint32_t above);
		// (test aid, include/rt_hip_debug.h: fills the hit list and the occlusion counts with 0xFF between frames -- a frame
		// that leaned on what the one before it left there would show it)
		void poisonHitList();
		// (diagnostics / experiments, include/rt_hip_debug.h: the list as it is, and a list made elsewhere put in its place --
		// any order of the same tiles renders the same image)
		void tileOrder(std::vector<uint32_t> &order, std::vector<uint32_t> &constants, std::vector<uint32_t> &words, std::vector<float> &cost) const;
		void setTileOrder(const std::vector<uint32_t> &order, const std::vector<uint32_t> &constants);
		// (... per group: how many tiles at the head of its list the pass claims half a tile at a time)
		const std::array<uint32_t, XCD_GROUPS> &splitTiles() const { return split_tiles; }
		// (... and how many at its END are claimed four whole tiles at a time, one per wave: the cheap suffix)
		const std::array<uint32_t, XCD_GROUPS> &cheapTiles() const { return cheap_tiles; }
		// (test aid, include/rt_hip_debug.h: the suffix's boundary in reference costs -- 0: no region --; re-orders from the costs held)
		void setCheapClaims(float cheap_below);
		bool calibrateAoPrefetch(float *ms_without = nullptr, float *ms_with = nullptr);
		// (A scene far beyond the caches is another matter: its pass waits for memory, and what it needs is loads in
		// flight -- every host keeps the full grid: 2 M-triangle field, three hosts, 11.93 ms per frame with 4.5 per CU,
		// 11.64 with 5.5, 11.32 with 8.)
		uint32_t aoWorkgroups() const {
			if (scene_beyond_caches)
				return compute_units * 8u;
			return device_share >= 6u ? compute_units * 3u : device_share > 1u ? compute_units * 9u / 2u : compute_units * 8u;
		}
		uint32_t globalRowOf(uint32_t local_row) const;  // output row of a local band row (may be >= height: padding)

		void downloadFloat(float *host_image);          // full totalWidth x totalHeight (rows of other ranks' bands: 0)
		void downloadResizedLocal(unsigned char *host); // localRows() x width, compact
		void downloadResizedFull(unsigned char *host);  // width x height (needs nranks == 1)

		// Run on an externally owned hipStream_t (nullptr = the HIP default stream) /
		// go back to the private non-blocking stream.
		void setStream(void *hip_stream);
		void usePrivateStream();

		RenderStats stats();   // ray counts of the last frame (device counters)
		float lastKernelMs() const { return last_ms; }      // all passes of the last frame
		float lastAoMs() const { return last_ao_ms; }       // the ao_kernel launch alone (0 when the frame has no AO pass)
		double totalKernelMs() const { return total_ms; }
		double totalAoMs() const { return total_ao_ms; }
		uint64_t kernelLaunches() const { return launches; }
		uint64_t aoLaunches() const { return ao_launches; }  // frames whose ao_kernel launch was timed (totalAoMs)
		void resetTimers() { total_ms = total_ao_ms = 0; launches = ao_launches = 0; last_ms = last_ao_ms = 0; }

		uint32_t localRows() const { return local_out_rows; }  // output rows this rank owns
		uint32_t width() const { return opts.width; }
		uint32_t height() const { return opts.height; }
		const RayTracer &rayTracer() const { return rt; }
		const KernelParams &params() const { return kp; }
		int deviceIndex() const { return device; }
		std::string deviceName() const;

	private:
		void freeScene();
		void useDevice() const;

		RayTracer::Options opts;
		RayTracer rt;
		int device;
		Partition part;
		CameraPose pose = default_camera_pose();
		bool pose_set = false;
		KernelParams kp;
		uint32_t grid;            // supersample grid side
		uint32_t local_out_rows;
		void *own_stream, *stream;
		std::shared_ptr<const DeviceScene> scene_on_device;
		std::shared_ptr<DeviceScene> scene_of_my_own;  // the same scene for writing, where upload() made it (null after adopt() alone)
		bool scene_updated = false;
		uint32_t refit_group = 0;
		void requireFramePath(const char *what) const;
		void *d_image, *d_u8, *d_hits, *d_occluded, *d_tile_hits, *d_tile_base, *d_tile_entry, *d_order, *d_counters;
		size_t hit_slots;     // slots of the hit list: the scene's hit sub-pixels in this rank's bands (sizeHitList)
		size_t entryBytes() const { return (size_t) tile_count * kp.entry_stride * 2 * sizeof(uint32_t); }  // the tiles' walk intervals (entry_kernel)
		std::shared_ptr<void> tile_entry_owner;  // d_tile_entry: one table for the hosts of a ring (sizeHitList)
		void allocEntries(size_t bytes);
		void sizeHitList(const DeviceRenderer *layout_from);  // counts the hits per tile with one pass of the primary kernel (or copies another renderer's count) and sizes the list by them
		// The order the ambient-occlusion pass claims the tiles in, made once per upload on the host (orderTiles): from the
		// tile words of the pass that sizes the hit list (hit count | cost class), or from measured costs per tile.
		std::vector<uint32_t> tile_words, order_host;
		std::vector<float> tile_cost;  // measured: device-clock ticks per tile (empty: not measured)
		std::array<std::array<uint32_t, 3>, XCD_GROUPS> queue_static{};  // per group: non-empty tiles, sum of cost classes, hit sub-pixels
		std::vector<uint32_t> blocks_by_cost_host;            // primary_kernel: the groups' 2 x 2 blocks by falling cost (0xFFFFFFFF: no block)
		void *d_blocks_by_cost = nullptr;
		size_t blocks_by_cost_capacity = 0;  // (entries)
		size_t primary_quartered = 0;        // tiles the primary pass casts in quarters (orderBlocksByCost)
		bool primary_by_cost = true;
		void orderBlocksByCost();
		void uploadBlocksByCost();
		std::array<uint32_t, XCD_GROUPS> split_tiles{};  // per group: the tiles at the head of its list that are claimed half a tile at a time
		std::array<uint32_t, XCD_GROUPS> cheap_tiles{};  // per group: the tiles at the end of its list that are claimed whole, one per wave
		struct OrderPolicy {  // (orderByMeasuredCost; swept in profiles/r05_order_policies.txt)
			float heavy = 2.0f;   // tiles beyond this many reference costs (the upper quartile) are claimed first
			float runway = 2.0f;  // what is held back for the end, by falling cost: this many reference claims per workgroup
			uint32_t primary_split_waves = 4096;  // ... unless those tiles, four waves each, are more than this many waves (half the chip's slots: then the slots are full anyway)
			uint32_t primary_split_above = 64;  // primary pass: tiles of this cost class (leaves their packet stops at, 1 ... 64) or more are cast in quarters (0: none)
			float split_above = 0.25f;  // tiles that cost more than this share of the pass's ideal length: half a tile per claim (0: none)
			float cheap_below = CHEAP_BELOW_DEFAULT;  // tiles at the list's end below this many reference costs: a whole tile per wave and claim (0: none)
		} order_policy;
		void orderTiles();
		std::vector<uint32_t> orderByMeasuredCost(const std::vector<float> &cost, uint32_t *split = nullptr, uint32_t *cheap = nullptr) const;
		void installOrder(const std::vector<uint32_t> &order, const std::array<std::array<uint32_t, 3>, XCD_GROUPS> &constants,
		                  const std::array<uint32_t, XCD_GROUPS> &splits = {}, const std::array<uint32_t, XCD_GROUPS> &cheap = {});
		size_t image_bytes;  // float image of this rank's bands
		size_t tile_count;
		uint32_t compute_units;
		uint32_t device_share;  // hosts that take frames in turn on this GPU (setDeviceShare), 1 = this one alone
		bool scene_beyond_caches = false;  // the uploaded scene is several times the L2s (upload: wider strips, full AO grids)
		bool scene_ready, frame_ready;
		struct FrameEvents {
			void *start, *ao_start, *ao_stop, *stop;  // frame begin, around the ao_kernel launch alone, frame end
			bool ao_timed = false;                    // the frame had an AO pass (ao_start / ao_stop were recorded)
			bool graph_ao = false;                    // ... as a replayed graph: the graph's own events hold the AO times
		};
		std::vector<FrameEvents> pending_events, free_events;
		FrameEvents takeEvents();
		void launchFrame(void *device_u8, void *ao_start, void *ao_stop, void *tile_cost = nullptr);  // the launches of one frame, resize included
		// the captured frame (enqueueFrame) and what it was captured for
		struct FrameGraph {
			void *graph = nullptr, *exec = nullptr;
			void *dst = nullptr, *stream = nullptr;
			uint64_t scene_version = 0;
			uint32_t device_share = 0;
			bool valid = false, ao_events = false;
		};
		std::vector<FrameGraph> frame_graphs;  // one per destination seen lately (a ring alternates between two per renderer)
		const FrameGraph *frameGraphFor(void *dst);
		void dropFrameGraphs();
		bool graph_mode;
		uint64_t expected_frames = 1;
		bool intervals_in_use = false;
		bool ao_prefetch;
		uint64_t scene_version;
		uint32_t ao_blocks_override;  // (debug-knob builds: OCRT_AO_BLOCKS)
		void *epoch_event;
		bool keep_stamps;
		float last_times[4];
		float last_ms, last_ao_ms;
		double total_ms, total_ao_ms;
		uint64_t launches, ao_launches;
};

// kernels.hip
void preload_kernels();
#ifdef OCRT_OCML_BUILTINS
uint32_t ocml_ao_table(void *table, uint32_t rings, int alpha_min, int alpha_max, uint32_t capacity);
#endif
void launch_primary(const SceneBuffers &scene, float *image, void *hits, void *occluded_of, void *tile_hits,
                    const void *tile_base, void *counters, const KernelParams &P, void *stream, const void *blocks_by_cost = nullptr);
void launch_entries(const SceneBuffers &scene, const void *hits, const void *tile_hits, const void *tile_base, void *tile_entry,
                    const KernelParams &P, void *stream);
void launch_ao(const SceneBuffers &scene, void *hits, void *occluded_of, void *order, const void *tile_base, const void *tile_entry,
               void *counters, const KernelParams &P, uint32_t workgroups, bool prefetch, void *stream, void *event_before_ao,
               void *event_after_ao, void *tile_cost = nullptr);
void launch_finish(float *image, const void *hits, const void *occluded_of, const void *tile_base,
                   unsigned char *out, const KernelParams &P, uint32_t out_width, uint32_t n, uint32_t local_out_rows, void *stream,
                   void *counters);
void launch_occluded_sum(const void *occluded_of, size_t slots, void *counters, void *stream);
void launch_resize(const float *tmp, unsigned char *out, const KernelParams &P, uint32_t out_width, uint32_t n,
                   uint32_t local_out_rows, void *stream);
void launch_refit_leaves(const void *faces, const void *leaf_nodes, const void *vertices4, const void *vnormals4, void *tris, void *shade,
                         void *nodes, uint32_t leaves, void *stream);
void launch_refit_inner(const void *entries, const void *children, const void *groups, void *nodes, uint32_t first_group, uint32_t groups_in_pass,
                        void *stream);
// Test aid: the any-hit node test in both forms (kernels/node_test_forms.hip.h)
void launch_node_test_forms(const void *records, uint32_t boxes, const void *rays6, uint32_t rays, void *out, void *stream);
// Device-side builds (kernels/build.hip.h; BuildBuffers: device_types.h)
uint32_t build_partials(uint32_t faces);
void launch_build_keys(const BuildBuffers &b, void *stream);
void launch_build_tree(const BuildBuffers &b, void *stream);
// Device-side instance sets (kernels/instance_build.hip.h; InstancePlanBuffers: device_types.h), around the same sort
void launch_instance_keys(const InstancePlanBuffers &b, void *stream);
void launch_instance_tree(const InstancePlanBuffers &b, void *stream);
// build_sort.hip
size_t build_sort_bytes(uint32_t pairs);
void launch_build_sort(void *temporary, size_t temporary_bytes, const void *keys_in, void *keys_out, const void *ids_in, void *ids_out,
                       uint32_t pairs, void *stream);

}  // namespace ocrt
