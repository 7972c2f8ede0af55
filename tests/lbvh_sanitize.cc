// lbvh_sanitize.cc -- a stand-alone program for -fsanitize=address,undefined: the host-only tree of a device-side build
// (lbvh.cc) and the schedule its inner boxes follow (refit.cc) on `stack` (every key equal), `flat` (no extent on one axis),
// a mesh file of one triangle and a random soup; every tree is checked for what the walk needs of it.
//   lbvh_sanitize single.off
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "lbvh.h"
#include "mesh.h"
#include "refit.h"

namespace {

int fail(const std::string &what, const char *why) {
	std::printf("%s: %s\n", what.c_str(), why);
	return 1;
}

int check(const std::string &what, const std::vector<Vec3f> &vertices, const std::vector<uint32_t> &faces) {
	const ocrt::LbvhTree tree = ocrt::lbvh_build(faces, vertices);
	const size_t leaves = faces.size() / 3, count = 2 * leaves - 1;
	if (tree.nodes.size() != count || tree.triangles.size() != leaves || tree.keys.size() != leaves || tree.leaf_nodes.size() != leaves)
		return fail(what, "sizes");
	if (tree.nodes[0] != count)
		return fail(what, "the root does not span the array");
	std::vector<unsigned char> seen(leaves, 0);
	for (size_t i = 0; i < leaves; ++i) {
		if (tree.triangles[i] >= leaves || seen[tree.triangles[i]]++)
			return fail(what, "a face twice, or none");
		if (i && (tree.keys[i - 1] > tree.keys[i] || (tree.keys[i - 1] == tree.keys[i] && tree.triangles[i - 1] > tree.triangles[i])))
			return fail(what, "order");
		if (tree.leaf_nodes[i] >= count || tree.nodes[tree.leaf_nodes[i]] != 1)
			return fail(what, "leaf -> node map");
	}
	size_t leaf = 0;
	for (size_t i = 0; i < count; ++i) {
		const uint32_t skip = tree.nodes[i];
		if (skip == 0 || i + skip > count || skip % 2 == 0)
			return fail(what, "a subtree size");
		if (skip == 1) {
			if (tree.leaf_nodes[leaf++] != i)
				return fail(what, "leaves out of pre-order");
			continue;
		}
		const size_t second = i + 1 + tree.nodes[i + 1];
		if (second >= i + skip || second + tree.nodes[second] != i + skip)
			return fail(what, "not a binary tree");
	}
	// the boxes by the refit rule, and the schedule at several group sizes
	std::vector<uint32_t> leaf_faces(faces.size());
	for (size_t i = 0; i < leaves; ++i)
		for (unsigned k = 0; k < 3; ++k)
			leaf_faces[3 * i + k] = faces[3 * (size_t) tree.triangles[i] + k];
	std::vector<Vec3f> aabbs(2 * count);
	ocrt::refit_boxes(tree.nodes, leaf_faces, vertices, aabbs);
	for (uint32_t group : { 1u, 2u, 7u, 256u, 0u }) {
		const ocrt::RefitSchedule s = ocrt::make_refit_schedule(tree.nodes, group);
		if (s.entries.size() / 4 != leaves - 1)
			return fail(what, "the schedule misses inner nodes");
	}
	std::printf("%s: %zu leaves, tree ok\n", what.c_str(), leaves);
	return 0;
}

}  // namespace

int main(int argc, char **argv) {
	int bad = 0;
	{  // stack: 70 copies of one triangle
		const std::vector<Vec3f> v = { Vec3f(0.1f, 0.2f, 0.3f), Vec3f(0.9f, 0.1f, 0.4f), Vec3f(0.3f, 0.8f, 0.2f) };
		std::vector<uint32_t> f;
		for (int i = 0; i < 70; ++i)
			f.insert(f.end(), { 0u, 1u, 2u });
		bad += check("stack", v, f);
	}
	{  // flat: a 9 x 7 grid in z = 0
		std::vector<Vec3f> v;
		std::vector<uint32_t> f;
		for (int y = 0; y < 7; ++y)
			for (int x = 0; x < 9; ++x)
				v.push_back(Vec3f(0.37f * (float) x, 0.53f * (float) y, 0.0f));
		for (uint32_t y = 0; y < 6; ++y)
			for (uint32_t x = 0; x < 8; ++x) {
				const uint32_t a = y * 9 + x;
				f.insert(f.end(), { a, a + 1, a + 9, a + 1, a + 10, a + 9 });
			}
		bad += check("flat", v, f);
	}
	for (int i = 1; i < argc; ++i) {
		Mesh mesh;
		load_off_mesh(argv[i], &mesh);
		bad += check(argv[i], mesh.vertices, mesh.faces);
	}
	{  // a soup of 5 000 random triangles, some of them far out, some degenerate
		std::mt19937 rng(7);
		std::uniform_real_distribution<float> u(-1.0f, 1.0f);
		std::vector<Vec3f> v;
		std::vector<uint32_t> f;
		for (uint32_t i = 0; i < 5000; ++i) {
			const float scale = i % 97 == 0 ? 1.0e6f : i % 13 == 0 ? 0.0f : 0.05f;
			const Vec3f c(u(rng), u(rng), u(rng));
			for (unsigned k = 0; k < 3; ++k)
				v.push_back(Vec3f(c.x + scale * u(rng), c.y + scale * u(rng), c.z + scale * u(rng)));
			f.insert(f.end(), { 3 * i, 3 * i + 1, 3 * i + 2 });
		}
		bad += check("soup", v, f);
	}
	// refusals: no face; an index out of range
	for (const std::vector<uint32_t> &f : { std::vector<uint32_t>{}, std::vector<uint32_t>{ 0u, 1u, 3u } }) {
		bool refused = false;
		try {
			ocrt::lbvh_build(f, { Vec3f(0.0f), Vec3f(1.0f), Vec3f(2.0f) });
		} catch (const std::invalid_argument &) {
			refused = true;
		}
		if (!refused)
			bad += fail("refusals", "accepted");
	}
	if (bad)
		return 1;
	std::printf("lbvh_sanitize: ok\n");
	return 0;
}
