/* rt_hip_debug.h -- diagnostic and experiment entry points of libocrt_hip.so.
 *
 * NOT part of the drop-in boundary (include/rt_hip.h is): nothing here replaces a member of the reference's OpenCLHost
 * (include/opencl_host.h:6-144); tests, bench.py and the analysis tools use these to look inside a render host.  None of
 * them changes what a frame computes.
 */
#ifndef RT_HIP_DEBUG_H
#define RT_HIP_DEBUG_H

#include "rt_hip_ring.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HIP-event timing of the ray-casting passes on the launch stream beyond rt_last_kernel_ms (rt_hip.h): running totals in
 * ms and the number of frames since the reset; *_kernel_ms covers every pass of a frame, *_ao_ms the launch of the
 * ambient-occlusion kernel alone (0 for frames without AO). */
double rt_total_kernel_ms(const rt_host *h);
float rt_last_ao_ms(const rt_host *h);
double rt_total_ao_ms(const rt_host *h);
uint64_t rt_kernel_launches(const rt_host *h);
void rt_reset_timers(rt_host *h);

/* What the last upload put on the device: the bytes of the scene's arrays, how many copies of them exist among the
 * ring's hosts (ONE: the hosts share the arrays, like the single upload of src/opencl_host.cc:120-136) and the bytes
 * of everything requested, per-host frame buffers included.  Out pointers may be NULL. */
int rt_ring_device_bytes(const rt_ring *r, uint64_t *scene_bytes, uint32_t *scene_copies, uint64_t *total_bytes);

/* What a ring's calibration at upload (rt_hip_ring.h, rt_ring_set_calibration) measured: ms per ao_kernel launch without
 * / with the look-ahead loads (0 = not measured) and the form in use (1 = with); out pointers may be NULL.
 * rt_set_ao_prefetch: which form ONE host launches. */
int rt_ring_calibration(const rt_ring *r, float *ms_without, float *ms_with, int *prefetch_in_use);
int rt_set_ao_prefetch(rt_host *h, int on);

/* Walk intervals (new; results never depend on them): an upload finds, for every 8x8 tile of the host's band, the part of
 * the tree's node records -- an interval of the pre-order array -- outside which no leaf lies that an ambient-occlusion ray
 * of the tile can reach (AO_MAX_DISTANCE, src/intersect_kernel.cl:217, and the slab test of :21-61), once for any ray
 * from the tile and once for each table direction of a full tile (the 64 rays of one packet); the any-hit packets walk
 * their interval alone.  This reports, over the tiles with hits: their number, how many have a tile interval short of the
 * whole array, the mean share of the records inside the tile intervals, and the mean share inside the intervals the
 * packets actually use (1.0 = no narrowing: AO_MAX_DISTANCE of the scene's size).  Out pointers may be NULL.
 * RT_E_STATE without a scene. */
int rt_walk_entries(rt_host *h, uint32_t *tiles_hit, uint32_t *tiles_narrowed, double *mean_share, double *mean_packet_share);
/* Where those intervals END, read back and held against the node records they index: the any-hit loop compares its place
 * with the interval's end only where a miss jump or the step off a leaf can land on it, not where it descends to a first
 * child, which rests on every end being the end of a subtree.  Over the non-empty intervals the packets use (a full tile's:
 * one per table direction; any other tile's: one): out[0] their number, [1] those that end with the array (a one-shot
 * host's: all of them), [2] those that end behind a leaf record -- a subtree's end --, [3] those that end behind an inner
 * node, i.e. on its first child, [4] of [2] the ones no inner node's miss jump inside the interval lands on (left by the
 * step off the last leaf, or by its miss), [5] of [2] the ones some inner node's miss jump lands on exactly.  A test aid:
 * it copies the whole table and the records to the host.  RT_E_STATE without a scene. */
int rt_debug_walk_interval_ends(rt_host *h, uint32_t out[6]);

/* Time stamps of collected frames: ms from the last rt_ring_reset_clock to the frame's begin, the start and the end of
 * its ambient-occlusion kernel, its end.  Begin and end are HIP events on the host's stream; the kernel's times are HIP
 * events too for plain launches, and for graph replays -- whose event nodes cannot be timed -- the device's 100 MHz
 * clock as the kernels stamped it into the frame's counters, read only after rt_ring_keep_frame_times(r, 1) (a small
 * blocking copy per frame; 0 without it).  Kept for the last 256 frames (RT_E_STATE for older ones). */
int rt_ring_reset_clock(rt_ring *r);
int rt_ring_keep_frame_times(rt_ring *r, int on);
int rt_ring_frame_times(const rt_ring *r, uint64_t frame, float ms[4]);

/* Sums over the ring's hosts since rt_ring_reset_timers: kernel time of whole frames / of the ao_kernel launches alone
 * (HIP events) and how many frames each sum covers.  Any out pointer may be NULL. */
int rt_ring_timers(rt_ring *r, double *kernel_ms, uint64_t *frames, double *ao_ms, uint64_t *ao_frames);
void rt_ring_reset_timers(rt_ring *r);

/* What the frames collected since the last rt_ring_reset_clock cost the CPU: seconds inside submit (the launches),
 * inside collect waiting for the device, inside collect otherwise; and their number.  Out pointers may be NULL. */
int rt_ring_cpu_times(const rt_ring *r, double *submit_s, double *wait_s, double *collect_s, uint64_t *frames);

/* rt_ring_rccl_info: what the attached communicator says about itself -- ranks (ncclCommCount), RCCL's version code
 * (ncclGetVersion), -1 where unknown -- so that a run can state how many ranks RCCL really saw. */
int rt_ring_rccl_info(rt_ring *r, int *comm_ranks, int *rccl_version);
int rt_ring_rccl_self_test(rt_ring *r);  /* grouped self send/recv on the ring's communicator, checked */

/* The order in which the ambient-occlusion pass claims a frame's tiles (made once per upload on the host,
 * DeviceRenderer::orderTiles).  rt_debug_measure_tile_costs renders `frames` frames whose AO pass books every claim's
 * duration to its tiles (device-clock ticks of 10 ns), and, with `reorder` != 0, makes the order from them
 * (rt_debug_set_order_policy: `heavy`, `runway`, `split_above`, see DeviceRenderer::orderByMeasuredCost).
 * rt_debug_tile_order copies out: the list (`order`, rt_debug_tile_order_slots() words: eight segments, entry = tile |
 * (hit count - 1) << 26), 24 constants (per group: non-empty tiles, sum of cost classes, hit sub-pixels), the tile words
 * (hit count | cost class << 8) and the measured costs (`tiles` values each, 0 where nothing was measured); any pointer
 * may be null.  rt_debug_set_tile_order installs a list made by the caller (same size, same tiles: any order renders
 * the same image). */
int rt_debug_measure_tile_costs(rt_host *h, uint32_t frames, int reorder);
int rt_debug_set_order_policy(rt_host *h, float heavy, float runway, float split_above);  /* split_above < 0: unchanged */
/* The primary pass casts tiles whose packet stops at `above` leaves or more (their cost class, 1 ... 64) in quarters, the four
 * waves of a workgroup at once (DeviceRenderer::setPrimarySplit; 0: none) -- however many tiles that is: the rule an upload
 * applies by itself (class 64) stands back where more than an eighth of the chip's wave slots' worth of tiles qualify.
 * Results never depend on it. */
int rt_debug_set_primary_split(rt_host *h, uint32_t above);
uint32_t rt_debug_tile_order_slots(rt_host *h);
uint32_t rt_debug_tiles(rt_host *h);
int rt_debug_tile_order(rt_host *h, uint32_t *order, uint32_t *constants24, uint32_t *tile_words, float *tile_costs);
int rt_debug_set_tile_order(rt_host *h, const uint32_t *order, uint32_t slots, const uint32_t *constants24);
/* Per XCD group, how many tiles at the head of its list the pass claims HALF A TILE at a time (orderByMeasuredCost's
 * `split`; all 0 without measured costs, with an odd direction count, and with 0x8000 directions or more -- the cursor
 * that ends a half-tile claim holds 15 bits).  A read-only copy: a test that means to exercise those claims asserts from
 * it that there were some. */
int rt_debug_split_tiles(rt_host *h, uint32_t out[8]);
/* The cheap suffix of the lists: the tiles at a group's END whose measured cost lies below `cheap_below` x the reference
 * cost (the upper quartile) are claimed four whole tiles at a time, one per wave (orderByMeasuredCost's `cheap`).
 * rt_debug_set_cheap_claims sets the boundary -- 0: no region, a huge value: every tile that is not split -- and makes the
 * order again from the costs already held (nothing happens without measured costs).  rt_debug_cheap_tiles: per XCD group,
 * how many tiles the region holds; all 0 without measured costs.  Results never depend on either.  The region travels with
 * the list: rt_debug_measure_tile_costs without `reorder` keeps list, split prefix and region as they are (its measuring
 * frames themselves always claim as if there were no region, so that a tile's cost keeps its meaning);
 * rt_debug_set_tile_order installs the caller's list with neither. */
int rt_debug_set_cheap_claims(rt_host *h, float cheap_below);
int rt_debug_cheap_tiles(rt_host *h, uint32_t out[8]);

/* What the closest-hit walk's pruning rests on in the uploaded scene (scene_pack.h, WalkArray): `prune_margin` (+inf: this
 * host does not prune -- a one-shot host, or a scene no prunable tree can be formed of), the bytes at the head of the primary
 * rays' records inside which no limit is lowered (the faces without a bound) and the bytes of those records.  A read-only
 * copy; out pointers may be NULL.  RT_E_STATE without a scene. */
int rt_debug_prune_facts(rt_host *h, float *prune_margin, uint32_t *unpruned_bytes, uint32_t *primary_bytes);

/* Test aid for the hand-over between the two ray passes: overwrites the hit list (the records the primary pass leaves for
 * the ambient-occlusion pass) and the per-hit occlusion counts with 0xFF bytes -- NaN patterns and counts of 2^32 - 1.
 * Every frame must write both again before it reads them; frames of one scene are otherwise identical, so a frame that
 * leaned on what the one before it left there could never be seen without this.  Waits for the host's frames first. */
int rt_debug_poison_hit_list(rt_host *h);

/* Multi-view rendering (rt_hip_views.h).  rt_debug_set_views_chunk: a views call works through at most `max_views` views
 * per chunk (0, the default: as many as fit) -- so that a test can make several chunks of a few small views; results never
 * depend on it.  rt_debug_last_views: what the host's last views call did -- the views it rendered, the chunks it took,
 * and the points its ambient-occlusion step ran over: the sub-pixels that were hit, over all the views (0 for a call
 * without that step).  Zeros before the first call; out pointers may be NULL.  RT_E_STATE on the hosts of a frame ring. */
int rt_debug_set_views_chunk(rt_host *h, uint32_t max_views);
int rt_debug_last_views(rt_host *h, uint32_t *views, uint32_t *chunks, uint64_t *ao_points);

/* Closest-point queries (rt_hip_nearest.h), for tools/distance_bench.py.  rt_debug_set_nearest_walk: how the host's later
 * closest-point queries walk -- RT_DEBUG_NEAREST_NO_START: no lane descends for a starting bound; RT_DEBUG_NEAREST_NO_PRUNE:
 * no box is passed by (every leaf is tested); RT_DEBUG_NEAREST_COUNT: the kernel counts its tests.  Results never depend
 * on the flags.  Flags other than 0 are the A/B build's (-DOCRT_DEBUG_KNOBS): RT_E_STATE in the product library, whose
 * queries always walk the one way.  rt_debug_last_nearest_counts: per-point box tests and triangle tests of the host's
 * last counted query, summed over its points (waits for it; zeros without one).  RT_E_STATE on the hosts of a frame ring. */
#define RT_DEBUG_NEAREST_NO_START 1u
#define RT_DEBUG_NEAREST_NO_PRUNE 2u
#define RT_DEBUG_NEAREST_COUNT 4u
int rt_debug_set_nearest_walk(rt_host *h, uint32_t flags);
int rt_debug_last_nearest_counts(rt_host *h, uint64_t *node_tests, uint64_t *triangle_tests);

/* Vertex updates (rt_hip_update.h).  The inner boxes are refitted bottom-up by a schedule made on the host: the inner nodes
 * cut into groups of at most S, a workgroup per group, a launch per pass.  rt_debug_set_refit_group: S for this host's
 * updates (0, the default: 256; at most 1024) -- so that a small mesh can take several passes; results never depend on it.
 * rt_debug_refit_schedule: the schedule for a CPU-side scene's tree (`packed_tree` 0: its own node array; 1: the tree an
 * upload puts on the device, which may be a cheaper one over the same leaves whose inner nodes have more than two
 * children).  counts6: nodes, scheduled entries, child references, groups, passes, S as used; the arrays (any may be NULL;
 * call once with NULLs for the counts): `skips` (a word per node: subtree size, 1 = leaf), `entries` (4 words each: node,
 * first child reference, children, round within the group; in group order, by round within a group), `children` (a node
 * index, or 0x80000000 | the entry's position within its own group), `groups` (4 words each: first entry, entries, rounds,
 * pass from 1; in pass order).
 * rt_debug_record_counts / rt_debug_download_records: the scene on the device as every query walks it -- how many node
 * records (32 bytes: lo[3], skip, hi[3], leaf) and leaf records it has, and copies of the node records, the leaf records
 * (96 bytes: lo[3], pad, hi[3], inv_d, ta[3], u[3], v[3], n[3], uu, uv, vv, D) and the shading records (48 bytes: three
 * normals of four floats), taken once everything enqueued has finished; any pointer may be NULL.  RT_E_STATE without a
 * scene and on the hosts of a frame ring. */
int rt_debug_set_refit_group(rt_host *h, uint32_t nodes);
int rt_debug_refit_schedule(const rt_scene *s, uint32_t group_nodes, int packed_tree, uint32_t counts6[6], uint32_t *skips, uint32_t *entries,
                            uint32_t *children, uint32_t *groups);
int rt_debug_record_counts(const rt_host *h, uint32_t *nodes, uint32_t *leaves);
int rt_debug_download_records(rt_host *h, void *nodes_out, void *tris_out, void *shade_out);

/* Device-side builds (rt_hip_build.h): where the last build's time went, in ms -- the topology's kernels (keys, sort, shape,
 * layout; HIP events), the records' and boxes' kernels (HIP events), and the host's step between them: the schedule of the
 * inner boxes made from the downloaded skips and copied to the device (wall clock).  Zeros before the first build. */
int rt_debug_last_build_times(rt_host *h, float ms3[3]);

/* The any-hit walk's node test (kernels/walk.hip.h, OCRT_TEST_CE_SCALED: near and far of an axis from one packed fma, nine
 * vector instructions) held against the twelve-instruction form it replaced (a v_fma_f32 per value), on the device and on the
 * caller's data; needs no host and no scene.  records8: `boxes` records of the centre / half-extent copy of the walk array
 * (8 words: c.xyz, skip, e.xyz, leaf; 1 ... 65536).  rays6: `rays` walk rays (ix, iy, iz, oix, oiy, oiz: the scaled
 * reciprocals and -(o * i); a multiple of 64, 65536 at the most).  out9: nine words per (ray, record), ray-major -- near, far
 * (bit patterns) and the decision (0 / 1) of the old form, of the new form in the registers of the loop's node `a`, and of
 * the new form in those of node `b`. */
int rt_debug_node_test_forms(int device, const float *records8, uint32_t boxes, const float *rays6, uint32_t rays, uint32_t *out9);

#ifdef __cplusplus
}
#endif
#endif
