// lbvh.h -- the tree of a device-side scene build (include/rt_hip_build.h): keys, shape and layout.  The arithmetic of a
// key, the search that finds a node's leaves and the count that places a node are written ONCE here, as functions both
// compilers take: kernels/build.hip.h calls them with a lane per node, lbvh.cc with a loop -- rt_scene_build_lbvh's tree on
// the CPU-side scene is the device's by construction, and tests/build_cases.py restates it independently (top-down).
// Host only apart from those functions; no HIP headers.
//
// The tree.  Leaf boxes by the refit rule (refit.h); the root box their per-axis minimum and maximum; per axis, in float32
// without contraction, c = (lo + hi) * 0.5f and cell = clamp((c - root_lo) * (1024.0f / (root_hi - root_lo)), 0, 1023)
// truncated, 0 where the extent is not positive and finite or the value is not a number; the key is the 30-bit Morton
// interleave of the cells, x in the highest bit of every triple, z in the lowest.  Leaf i is the i-th face of the stable
// order by key (equal keys: rising face id).  The shape is the binary radix tree over the 62-bit keys key << 32 | i: the
// node over leaves [l, r] splits behind the last leaf that shares with leaf l the highest bit in which the keys of l and r
// differ.  Nodes lie in pre-order: skip = 2 (r - l + 1) - 1, and the node over [l, r] has index 2 l + the number of its
// proper ancestors in whose FIRST child it lies (in front of it lie its ancestors, the l leaves to its left and the inner
// nodes above those leaves -- l less one per turn to the right on its path).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "vec3.h"

#ifdef __HIPCC__
#define OCRT_LBVH_FN __host__ __device__ inline
#else
#define OCRT_LBVH_FN inline
#endif

namespace ocrt {

constexpr uint32_t LBVH_NONE = 0xFFFFFFFFu;  // a parent link: the root's
constexpr uint32_t LBVH_FIRST = 0x80000000u;  // ... and the bit that says "I am my parent's first child"

// One axis of a key: the centre of a leaf's box, and its cell.
OCRT_LBVH_FN float lbvh_centre(float lo, float hi) { return (lo + hi) * 0.5f; }
OCRT_LBVH_FN uint32_t lbvh_cell(float c, float root_lo, float root_hi) {
	const float extent = root_hi - root_lo;
	if (!(extent > 0.0f) || !(extent <= 3.4028234663852886e38f))  // (false for a NaN too)
		return 0u;
	const float x = (c - root_lo) * (1024.0f / extent);
	if (!(x >= 0.0f))  // (a NaN too)
		return 0u;
	return x >= 1023.0f ? 1023u : (uint32_t) x;
}

// The ten bits of a cell, two zero bits between neighbours.
OCRT_LBVH_FN uint32_t lbvh_spread(uint32_t v) {
	v &= 0x3FFu;
	v = (v | (v << 16)) & 0x030000FFu;
	v = (v | (v << 8)) & 0x0300F00Fu;
	v = (v | (v << 4)) & 0x030C30C3u;
	v = (v | (v << 2)) & 0x09249249u;
	return v;
}

OCRT_LBVH_FN uint32_t lbvh_key(uint32_t cx, uint32_t cy, uint32_t cz) { return (lbvh_spread(cx) << 2) | (lbvh_spread(cy) << 1) | lbvh_spread(cz); }

// The leading bits that leaves i and j share, of their 64-bit words key << 32 | index; -1 where j is no leaf.  (i != j.)
OCRT_LBVH_FN int lbvh_shared(const uint32_t *keys, uint32_t leaves, uint32_t i, long long j) {
	if (j < 0 || j >= (long long) leaves)
		return -1;
	const unsigned long long a = ((unsigned long long) keys[i] << 32) | i, b = ((unsigned long long) keys[j] << 32) | (uint32_t) j;
	return a == b ? 64 : __builtin_clzll(a ^ b);
}

// Inner node i of `leaves` leaves (i < leaves - 1; node 0 is the root): its leaves [first, last] and the last leaf of its
// first child.  No node looks at another's result (Karras 2012: the node's direction, a doubling search for the far end,
// two bisections).
OCRT_LBVH_FN void lbvh_node(const uint32_t *keys, uint32_t leaves, uint32_t i, uint32_t *first, uint32_t *last, uint32_t *split) {
	const long long at = i;
	const long long d = lbvh_shared(keys, leaves, i, at + 1) > lbvh_shared(keys, leaves, i, at - 1) ? 1 : -1;
	const int least = lbvh_shared(keys, leaves, i, at - d);
	long long reach = 2;
	while (lbvh_shared(keys, leaves, i, at + reach * d) > least)
		reach *= 2;
	long long length = 0;
	for (long long t = reach / 2; t >= 1; t /= 2)
		if (lbvh_shared(keys, leaves, i, at + (length + t) * d) > least)
			length += t;
	const long long other = at + length * d;
	const int node = lbvh_shared(keys, leaves, i, other);
	long long s = 0, t = length;
	do {
		t = (t + 1) / 2;
		if (lbvh_shared(keys, leaves, i, at + (s + t) * d) > node)
			s += t;
	} while (t > 1);
	*split = (uint32_t) (at + s * d + (d < 0 ? -1 : 0));
	*first = (uint32_t) (d > 0 ? at : other);
	*last = (uint32_t) (d > 0 ? other : at);
}

// The proper ancestors of a node in whose first child it lies, from its parent link (LBVH_NONE, or the parent's inner index
// with LBVH_FIRST set where the node is its first child) and the inner nodes' own links.  At most 62 steps: every level
// spends a bit of the keys; a link out of range ends the count (damaged links cannot lead anywhere).
OCRT_LBVH_FN uint32_t lbvh_first_child_turns(const uint32_t *inner_links, uint32_t inner_nodes, uint32_t link) {
	uint32_t turns = 0;
	for (uint32_t step = 0; step < 64u && link != LBVH_NONE; ++step) {
		turns += link >> 31;
		const uint32_t parent = link & ~LBVH_FIRST;
		if (parent >= inner_nodes)
			break;
		link = inner_links[parent];
	}
	return turns;
}

// The whole tree on the host, over leaf-ordered arrays of the reference format.
struct LbvhTree {
	std::vector<uint32_t> keys;       // per leaf, rising
	std::vector<uint32_t> triangles;  // the face of every leaf (BVH::triangles)
	std::vector<uint32_t> nodes;      // subtree sizes in pre-order, 1 = leaf (BVH::nodes)
	std::vector<uint32_t> leaf_nodes; // the node of every leaf
};
// `faces`: three vertex ids per face, every one below vertices.size() (std::invalid_argument otherwise, and for no face).
LbvhTree lbvh_build(const std::vector<uint32_t> &faces, const std::vector<Vec3f> &vertices);
// The shape and layout alone, from rising keys (what the device makes of its sorted keys).
void lbvh_layout(const std::vector<uint32_t> &keys, std::vector<uint32_t> &nodes, std::vector<uint32_t> &leaf_nodes);

}  // namespace ocrt
