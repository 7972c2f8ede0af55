// refit.h -- vertex updates of a scene whose topology stays (include/rt_hip_update.h): the REFIT RULE, its host-side
// restatement over the reference-format arrays, and the schedule the device follows for the inner boxes
// (kernels/refit.hip.h).  Host only, no HIP headers.
//
// The refit rule.  Leaf order, tree shape, `skip` and `leaf` words stay.  A leaf's box is the builder's own
// (bvh.cc, Prims): per axis std::min(a, std::min(b, c)) and std::max(a, std::max(b, c)) of its three vertices.  An inner
// node's box is the union of its children's boxes by the comparison forms of AABB::merge -- lo = std::min(acc, next),
// hi = std::max(acc, next) --, started from the first child and taken in index order.  std::min(a, b) is (b < a) ? b : a
// and std::max(a, b) is (a < b) ? b : a: of two zeros of different sign the FIRST stays, which is what fixes the sign of a
// zero bound; fminf / fmaxf and the GPU's v_min / v_max order the zeros by sign and must not stand in for them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "vec3.h"

namespace ocrt {

// One axis of the rule (also what kernels/refit.hip.h spells out with selects).
inline float refit_min(float acc, float next) { return next < acc ? next : acc; }
inline float refit_max(float acc, float next) { return acc < next ? next : acc; }

// The rule over the reference-format arrays of a CPU-side scene: `skips` (subtree sizes in pre-order, 1 = leaf), the
// leaf-ordered faces (three vertex ids per leaf) and the vertices; writes aabbs[2 * i], aabbs[2 * i + 1] of every node.
// Inner nodes may have any number of children (sibling subtrees tile their parent's range).
void refit_boxes(const std::vector<uint32_t> &skips, const std::vector<uint32_t> &leaf_faces, const std::vector<Vec3f> &vertices,
                 std::vector<Vec3f> &aabbs);

// The largest group a launch is made for (kernels/refit.hip.h keeps a group's boxes in LDS) and the default.
constexpr uint32_t REFIT_MAX_GROUP = 1024u;
constexpr uint32_t REFIT_DEFAULT_GROUP = 256u;
constexpr uint32_t REFIT_LOCAL = 0x80000000u;  // a child reference that names a slot of the entry's own group

// The schedule of the inner boxes, bottom-up.  The inner nodes are cut into GROUPS of at most `group_nodes`; one workgroup
// refits one group, in rounds by the nodes' height inside the group with a barrier between rounds; a group's other inputs
// -- leaves, nodes of earlier passes -- were written by an earlier LAUNCH: one launch per pass, and nothing is ever handed
// from workgroup to workgroup inside one.
//   pass 1        every maximal subtree of at most group_nodes inner nodes (contiguous in pre-order), small ones packed
//                 together into a group in pre-order;
//   pass p + 1    the same with the finished subtrees counted as leaves: a node joins the pass of its latest child if the
//                 connected piece it would head there still fits a group, and opens the next pass otherwise.
// That is the least number of passes any cut into connected pieces of that size allows: about log(nodes) / log(group_nodes)
// + 1 for trees of the builders' shape -- two for the bunny's tree on the device at 256 --, and the node's height for a chain.
struct RefitSchedule {
	uint32_t group_nodes = 0;  // S as used (0 asked for: the default; clamped to 1 ... REFIT_MAX_GROUP)
	// per scheduled node, grouped: node index, first child reference, number of children, round inside the group
	std::vector<uint32_t> entries;   // 4 words each
	// child references in index order: a node index (written by an earlier launch), or REFIT_LOCAL | slot of the entry's group
	std::vector<uint32_t> children;
	std::vector<uint32_t> groups;    // 4 words each: first entry, entries, rounds, pass (from 1)
	std::vector<uint32_t> pass_first;  // passes + 1 entries: the first group of every pass, then the number of groups
	uint32_t passes() const { return pass_first.empty() ? 0u : (uint32_t) pass_first.size() - 1u; }
};
// `skips` must describe a tree as pack_scene validates it (every range inside its parent's, skips[0] == size).
RefitSchedule make_refit_schedule(const std::vector<uint32_t> &skips, uint32_t group_nodes);

}  // namespace ocrt
