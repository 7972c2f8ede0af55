// The host side of the vertex updates (csrc/refit.cc) under AddressSanitizer + UBSan: the schedule maker over a scene's own
// node array and over the tree an upload puts on the device (inner nodes with more than two children), for group sizes from
// 1 to the default, and the CPU refit -- an identity refit must give back the builder's boxes as values, a translated one
// boxes that hold their triangles.  A stand-alone program: tests/test_refit_cpu.py compiles and runs it on the meshes given.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "bvh.h"
#include "mesh.h"
#include "refit.h"
#include "scene_pack.h"

static void require(bool ok, const char *what) {
	if (!ok)
		throw std::logic_error(what);
}

// Every inner node once, no group beyond S, every child reference a leaf, an earlier slot of the same group or a node of an
// earlier pass.
static unsigned check_schedule(const std::vector<uint32_t> &skips, uint32_t group_nodes) {
	const ocrt::RefitSchedule s = ocrt::make_refit_schedule(skips, group_nodes);
	const size_t entries = s.entries.size() / 4, groups = s.groups.size() / 4;
	std::vector<uint32_t> pass_of(skips.size(), 0), seen(skips.size(), 0);
	for (size_t g = 0; g < groups; ++g) {
		const uint32_t first = s.groups[4 * g], count = s.groups[4 * g + 1], pass = s.groups[4 * g + 3];
		require(count >= 1 && count <= s.group_nodes && first + count <= entries, "group size");
		require(g >= s.pass_first[pass - 1] && g < s.pass_first[pass], "pass_first");
		for (uint32_t e = first; e < first + count; ++e) {
			const uint32_t node = s.entries[4 * e];
			require(node < skips.size() && skips[node] != 1 && !seen[node]++, "entry node");
			pass_of[node] = pass;
		}
	}
	size_t inner = 0;
	for (uint32_t skip : skips)
		inner += skip != 1;
	require(inner == entries, "every inner node once");
	for (size_t g = 0; g < groups; ++g) {
		const uint32_t first = s.groups[4 * g], count = s.groups[4 * g + 1];
		for (uint32_t e = first; e < first + count; ++e) {
			const uint32_t node = s.entries[4 * e], begin = s.entries[4 * e + 1], kids = s.entries[4 * e + 2];
			require(begin + kids <= s.children.size(), "child range");
			size_t c = node + 1;
			for (uint32_t k = 0; k < kids; ++k, c += skips[c]) {
				const uint32_t ref = s.children[begin + k];
				if (ref & ocrt::REFIT_LOCAL) {
					const uint32_t slot = ref & ~ocrt::REFIT_LOCAL;
					require(slot < e - first && s.entries[4 * (first + slot)] == c && s.entries[4 * (first + slot) + 3] < s.entries[4 * e + 3], "local reference");
				} else {
					require(ref == c && (skips[c] == 1 || pass_of[c] < pass_of[node]), "global reference");
				}
			}
			require(c == node + skips[node], "children tile the node's range");
		}
	}
	return s.passes();
}

int main(int argc, char **argv) {
	try {
		for (int m = 1; m < argc; ++m)
			for (int method = 0; method < 2; ++method) {
				Mesh mesh;
				load_off_mesh(argv[m], &mesh);
				compute_vertex_normals(&mesh);
				BVH bvh(method == 0 ? BVH::Method::CUT_LONGEST_AXIS : BVH::Method::SURFACE_AREA_HEURISTIC);
				bvh.buildBVH(mesh);
				const std::vector<uint32_t> sorted = sort_faces_by_leaf_order(mesh, bvh);
				const ocrt::PackedScene packed = ocrt::pack_scene(sorted, bvh.nodes, bvh.aabbs, mesh.vertices, mesh.vnormals);
				std::vector<uint32_t> packed_skips;
				for (const ocrt::NodeRec &n : packed.nodes)
					packed_skips.push_back(n.skip);
				unsigned passes = 0;
				for (uint32_t group_nodes : { 1u, 2u, 7u, 64u, 0u, 5000u }) {
					passes = check_schedule(bvh.nodes, group_nodes);
					check_schedule(packed_skips, group_nodes);
				}
				// identity: the builder's boxes as values
				std::vector<Vec3f> aabbs = bvh.aabbs;
				ocrt::refit_boxes(bvh.nodes, sorted, mesh.vertices, aabbs);
				for (size_t i = 0; i < aabbs.size(); ++i)
					for (unsigned k = 0; k < 3; ++k)
						require(aabbs[i][k] == bvh.aabbs[i][k], "identity refit");
				// translated: every node's box holds the boxes below it, the root's holds every vertex that a face uses
				std::vector<Vec3f> moved = mesh.vertices;
				for (Vec3f &v : moved)
					v = v + Vec3f(7.0f, -5.0f, 3.0f);
				ocrt::refit_boxes(bvh.nodes, sorted, moved, aabbs);
				for (size_t i = 0; i < bvh.nodes.size(); ++i)
					for (size_t c = i + 1; c < i + bvh.nodes[i]; c += bvh.nodes[c])
						for (unsigned k = 0; k < 3; ++k)
							require(aabbs[2 * i][k] <= aabbs[2 * c][k] && aabbs[2 * c + 1][k] <= aabbs[2 * i + 1][k], "nested after a refit");
				for (uint32_t v : sorted)
					for (unsigned k = 0; k < 3; ++k)
						require(aabbs[0][k] <= moved[v][k] && moved[v][k] <= aabbs[1][k], "the root holds the mesh");
				std::printf("%s method %d: %zu nodes (%zu on the device), %u passes by default ok\n", argv[m], method, bvh.nodes.size(),
				            packed.nodes.size(), passes);
			}
		// what the maker refuses
		for (const std::vector<uint32_t> &bad : { std::vector<uint32_t>{ 2, 1, 1 }, std::vector<uint32_t>{ 3, 3, 1 }, std::vector<uint32_t>{ 3, 0, 1 } }) {
			bool refused = false;
			try {
				ocrt::make_refit_schedule(bad, 4);
			} catch (const std::invalid_argument &) {
				refused = true;
			}
			require(refused, "a damaged skip array must be refused");
		}
		require(ocrt::make_refit_schedule({}, 4).passes() == 0 && ocrt::make_refit_schedule({ 1 }, 4).passes() == 0, "no inner nodes, no passes");
	} catch (const std::exception &e) {
		std::printf("refit_sanitize: FAILED: %s\n", e.what());
		return 1;
	}
	std::printf("refit_sanitize: ok\n");
	return 0;
}
