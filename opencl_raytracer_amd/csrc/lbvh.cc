// lbvh.cc -- the tree of a device-side scene build on the host (lbvh.h): what rt_scene_build_lbvh puts into a CPU-side scene.
#include "lbvh.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>

#include "refit.h"

namespace ocrt {

void lbvh_layout(const std::vector<uint32_t> &keys, std::vector<uint32_t> &nodes, std::vector<uint32_t> &leaf_nodes) {
	const uint32_t leaves = (uint32_t) keys.size();
	nodes.assign(leaves ? 2 * (size_t) leaves - 1 : 0, 0u);
	leaf_nodes.assign(leaves, 0u);
	if (leaves == 0)
		return;
	const uint32_t inner = leaves - 1;
	std::vector<uint32_t> first(inner), last(inner), inner_links(inner, LBVH_NONE), leaf_links(leaves, LBVH_NONE);
	for (uint32_t i = 0; i < inner; ++i) {
		uint32_t split;
		lbvh_node(keys.data(), leaves, i, &first[i], &last[i], &split);
		(first[i] == split ? leaf_links : inner_links)[split] = i | LBVH_FIRST;
		(last[i] == split + 1 ? leaf_links : inner_links)[split + 1] = i;
	}
	if (inner)
		inner_links[0] = LBVH_NONE;
	for (uint32_t i = 0; i < inner; ++i) {
		const size_t at = 2 * (size_t) first[i] + lbvh_first_child_turns(inner_links.data(), inner, inner_links[i]);
		nodes.at(at) = 2 * (last[i] - first[i] + 1) - 1;
	}
	for (uint32_t i = 0; i < leaves; ++i) {
		const size_t at = 2 * (size_t) i + lbvh_first_child_turns(inner_links.data(), inner, leaf_links[i]);
		nodes.at(at) = 1;
		leaf_nodes[i] = (uint32_t) at;
	}
}

LbvhTree lbvh_build(const std::vector<uint32_t> &faces, const std::vector<Vec3f> &vertices) {
	if (faces.empty() || faces.size() % 3 != 0)
		throw std::invalid_argument("build: faces must hold 3 vertex ids per triangle, and at least one triangle");
	const size_t count = faces.size() / 3;
	if (count >= ((size_t) 1 << 25))
		throw std::invalid_argument("build: scene too large for 32-bit device offsets");
	for (uint32_t v : faces)
		if (v >= vertices.size())
			throw std::invalid_argument("build: face references a vertex out of range");
	// leaf boxes by the refit rule, the root box over them
	std::vector<Vec3f> lo(count), hi(count);
	Vec3f root_lo, root_hi;
	for (size_t f = 0; f < count; ++f) {
		const Vec3f &a = vertices[faces[3 * f]], &b = vertices[faces[3 * f + 1]], &c = vertices[faces[3 * f + 2]];
		for (unsigned k = 0; k < 3; ++k) {
			lo[f][k] = std::min(a[k], std::min(b[k], c[k]));
			hi[f][k] = std::max(a[k], std::max(b[k], c[k]));
			root_lo[k] = f == 0 ? lo[f][k] : refit_min(root_lo[k], lo[f][k]);
			root_hi[k] = f == 0 ? hi[f][k] : refit_max(root_hi[k], hi[f][k]);
		}
	}
	std::vector<uint32_t> keys(count);
	for (size_t f = 0; f < count; ++f)
		keys[f] = lbvh_key(lbvh_cell(lbvh_centre(lo[f][0], hi[f][0]), root_lo[0], root_hi[0]), lbvh_cell(lbvh_centre(lo[f][1], hi[f][1]), root_lo[1], root_hi[1]),
		                   lbvh_cell(lbvh_centre(lo[f][2], hi[f][2]), root_lo[2], root_hi[2]));
	LbvhTree out;
	out.triangles.resize(count);
	std::iota(out.triangles.begin(), out.triangles.end(), 0u);
	std::stable_sort(out.triangles.begin(), out.triangles.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
	out.keys.resize(count);
	for (size_t i = 0; i < count; ++i)
		out.keys[i] = keys[out.triangles[i]];
	lbvh_layout(out.keys, out.nodes, out.leaf_nodes);
	return out;
}

}  // namespace ocrt
