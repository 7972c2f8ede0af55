// camera_margin_check.cc -- CPU check (no GPU) of what the fast walk and its pruning rest on when the eye is NOT the
// reference's (0, 0, 2) (scene_pack.cc, make_walk_array's `eye`; kernels/primary.hip.h, the posed form).  For eyes
// outside, on the surface of and inside the scene's root box, 1 x, 10 x and 1000 x its extent away, axis-aligned and
// oblique, the walk array made for that eye -- for a one-shot host and for a stream -- meets a grid of primary rays and
// rays through the mesh's vertices shaken by 3e-6, and three things must hold:
//   1. wherever the reference's slab test (src/intersect_kernel.cl:21-61) passes for a box, the kernel's fma test on its
//      padded record passes: every leaf whose own box the reference's test lets the ray into is REACHED by the padded
//      walk, and (records in the builder's order: a one-shot host) the same node by node;
//   2. every hit the reference's triangle test accepts (:65-114) lies inside its leaf's grown box of the primary rays'
//      copy;
//   3. that box's near value AS THE KERNEL COMPUTES IT (fma(plane, inv, -(o * inv)), max3) -- and that of every box above
//      it -- is <= d * 1.00001f + prune_margin for the accepted hit's distance d: a lane with that hit still enters it.
// Exit code 0 = no violation.   usage: camera_margin_check bunny.off interior_hard.off [stale]
// `stale`: the self-check -- the array is made as if the eye were still (0, 0, 2) and met by rays from the 1000 x eyes;
// the run must then REPORT violations (exit code 0 if it does, 1 if the check has no teeth).
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "bvh.h"
#include "camera.h"
#include "mesh.h"
#include "reference_tests.h"
#include "scene_pack.h"

using namespace ocrt;

namespace {

const float INF = std::numeric_limits<float>::infinity();

// the reference's slab and triangle tests and the kernel's node test on a padded record: reference_tests.h
using reference_tests::Accepted;
using reference_tests::kernel_near;
using reference_tests::kernel_ray;
using reference_tests::KernelRay;
using reference_tests::reference_slab;
using reference_tests::reference_triangle;
using reference_tests::selectable;

PackedScene pack(Mesh &m) {
	compute_vertex_normals(&m);
	BVH bvh(BVH::Method::CUT_LONGEST_AXIS);
	bvh.buildBVH(m);
	const auto sorted = sort_faces_by_leaf_order(m, bvh);
	return pack_scene(sorted, bvh.nodes, bvh.aabbs, m.vertices, m.vnormals);
}

struct Totals {
	unsigned long long rays = 0, pairs = 0, hits = 0, missed_boxes = 0, outside = 0, pruned = 0, exact = 0;
	unsigned long long violations() const { return missed_boxes + outside + pruned; }
};

// One eye, one walk array.
void check(const Mesh &mesh, const PackedScene &scene, const WalkArray &walk, bool in_builder_order, const float eye[3], const float centre[3], uint32_t seed,
           Totals &t) {
	const size_t count = walk.primary_bytes / sizeof(NodeRec);
	const NodeRec *rec = walk.nodes.data();
	const size_t loose_end = walk.unpruned_bytes / sizeof(NodeRec);
	const bool pruning = std::isfinite(walk.prune_margin);
	std::vector<uint32_t> parent(count, 0xFFFFFFFFu), record_of(scene.tris.size(), 0xFFFFFFFFu);
	{
		std::vector<size_t> stack;  // (ends of the open subtrees)
		std::vector<uint32_t> open;
		for (size_t i = 0; i < count; ++i) {
			while (!stack.empty() && stack.back() <= i) {
				stack.pop_back();
				open.pop_back();
			}
			if (!open.empty())
				parent[i] = open.back();
			const size_t skip = rec[i].skip / sizeof(NodeRec);
			if (skip > 1) {
				stack.push_back(i + skip);
				open.push_back((uint32_t) i);
			} else if (rec[i].leaf < scene.tris.size()) {
				record_of[rec[i].leaf] = (uint32_t) i;
			}
		}
	}
	// the rays: a grid through the pose that looks at the scene's centre, and rays through shaken vertices
	std::vector<std::array<float, 3>> directions;
	CameraPose pose;
	const float up_a[3] = { 0, 1, 0 }, up_b[3] = { 1, 0, 0 };
	if (camera_look_at(eye, centre, up_a, &pose) || camera_look_at(eye, centre, up_b, &pose)) {
		const int G = 12;
		for (int y = 0; y < G; ++y)
			for (int x = 0; x < G; ++x) {
				const float a = (float) G, cx = ((float) x + 0.5f) / a - (float) G / (2.0f * a), cy = -(((float) y + 0.5f) / a - (float) G / (2.0f * a));
				float w[3];
				for (int k = 0; k < 3; ++k)
					w[k] = ((pose.right[k] * cx) + (pose.up[k] * cy)) + pose.forward[k];
				const float l = std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
				directions.push_back({ w[0] / l, w[1] / l, w[2] / l });
			}
	}
	std::mt19937 rng(seed);
	std::uniform_real_distribution<float> shake(-1.0f, 1.0f);
	for (int ray = 0; ray < 160; ++ray) {
		const Vec3f &v = mesh.vertices[rng() % mesh.vertices.size()];
		float d[3] = { v.x - eye[0] + 3e-6f * shake(rng), v.y - eye[1] + 3e-6f * shake(rng), v.z - eye[2] + 3e-6f * shake(rng) };
		const float len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
		if (!(len > 0.0f))
			continue;
		directions.push_back({ d[0] / len, d[1] / len, d[2] / len });
	}
	std::vector<char> reached(count);
	for (const auto &dir : directions) {
		const float *d = dir.data();
		if (!selectable(eye, d, walk.origin_limit)) {  // (the kernel casts such a packet in the exact form: nothing to hold here)
			++t.exact;
			continue;
		}
		++t.rays;
		const KernelRay kr = kernel_ray(eye, d);
		const float below = std::nextafterf(100000.0f, 0.0f);
		// the padded walk without pruning: which records the kernel enters
		std::fill(reached.begin(), reached.end(), 0);
		for (size_t i = 0; i < count;) {
			float far;
			const float near = kernel_near(rec[i], kr, &far);
			if (near <= std::fmin(far, below)) {
				reached[i] = 1;
				++i;
			} else {
				i += rec[i].skip / sizeof(NodeRec);
			}
		}
		// 1. leaf by leaf (any order of the records), and node by node where the records are the builder's
		for (size_t leaf = 0; leaf < scene.tris.size(); ++leaf) {
			const TriRec &tri = scene.tris[leaf];
			if (!reference_slab(tri.lo, tri.hi, eye, d, 100000.0f))
				continue;
			++t.pairs;
			const uint32_t at = record_of[leaf];
			if (at == 0xFFFFFFFFu || !reached[at]) {
				++t.missed_boxes;
				continue;
			}
			// 2. and 3.: the triangle test's accepted hits against the grown boxes (a pruning array; not the faces no box
			// promises anything about, which lie where no limit is lowered)
			const Accepted h = reference_triangle(tri, eye, d);
			if (!h.ok)
				continue;
			++t.hits;
			if (!pruning || (at >= 1 && at < loose_end) || !(h.distance < INF))
				continue;
			bool inside = true;
			for (int k = 0; k < 3; ++k)
				inside = inside && h.ip[k] >= rec[at].lo[k] && h.ip[k] <= rec[at].hi[k];
			t.outside += !inside;
			const float limit = h.distance * 1.00001f + walk.prune_margin;
			for (uint32_t up = at; up != 0xFFFFFFFFu; up = parent[up]) {
				float far;
				if (kernel_near(rec[up], kr, &far) > limit) {
					++t.pruned;
					break;
				}
			}
		}
		if (in_builder_order && count == scene.nodes.size())
			for (size_t i = 0; i < count; ++i)
				if (reference_slab(scene.nodes[i].lo, scene.nodes[i].hi, eye, d, 100000.0f)) {
					++t.pairs;
					float far;
					const float near = kernel_near(rec[i], kr, &far);
					t.missed_boxes += !(near <= std::fmin(far, below));
				}
	}
}

}  // namespace

int main(int argc, char **argv) {
	if (argc < 3)
		return 2;
	const bool stale = argc > 3 && std::string(argv[3]) == "stale";
	Totals all;
	int bad = 0;
	for (int which = 1; which <= 2; ++which) {
		Mesh mesh;
		load_off_mesh(argv[which], &mesh);
		const PackedScene scene = pack(mesh);
		float lo[3], hi[3], centre[3], extent = 0.0f;
		for (int k = 0; k < 3; ++k) {
			lo[k] = scene.nodes[0].lo[k];
			hi[k] = scene.nodes[0].hi[k];
			centre[k] = 0.5f * (lo[k] + hi[k]);
			extent = std::fmax(extent, std::fmax(std::fabs(lo[k]), std::fabs(hi[k])));
		}
		struct Eye {
			const char *name;
			float p[3];
			bool far;
		};
		std::vector<Eye> eyes;
		for (float scale : { 1.0f, 10.0f, 1000.0f }) {
			const float r = 1.5f * scale * extent;  // (outside the root box from 1 x on)
			eyes.push_back({ "on +z", { centre[0], centre[1], centre[2] + r }, scale == 1000.0f });
			eyes.push_back({ "on -x", { centre[0] - r, centre[1], centre[2] }, scale == 1000.0f });
			eyes.push_back({ "oblique", { centre[0] + 0.61f * r, centre[1] - 0.37f * r, centre[2] + 0.70f * r }, scale == 1000.0f });
		}
		eyes.push_back({ "on the root box's surface", { centre[0], hi[1], centre[2] }, false });
		eyes.push_back({ "on a corner of the root box", { lo[0], lo[1], hi[2] }, false });
		eyes.push_back({ "inside the root box", { centre[0] + 0.13f * (hi[0] - lo[0]), centre[1] - 0.21f * (hi[1] - lo[1]), centre[2] + 0.07f * (hi[2] - lo[2]) }, false });
		eyes.push_back({ "at the centre", { centre[0], centre[1], centre[2] }, false });
		uint32_t seed = 20261016u + 1000u * (uint32_t) which;
		for (const Eye &e : eyes) {
			if (stale && !e.far)
				continue;
			for (int stream = 0; stream < 2; ++stream) {
				WalkArray walk = make_walk_array(scene, 0.2f, stream != 0, stale ? nullptr : e.p);
				if (walk.nodes.empty()) {
					std::printf("FAILED: %s has no walk array\n", argv[which]);
					return 1;
				}
				if (stale)  // (as if only the limit had followed the eye: the margins, the growth and prune_margin are (0, 0, 2)'s)
					walk.origin_limit = std::fmax(walk.origin_limit, std::fmax(std::fabs(e.p[0]), std::fmax(std::fabs(e.p[1]), std::fabs(e.p[2]))));
				else if (!walk.eye_covered) {
					std::printf("FAILED: the eye %s of %s is not covered by the fast walk\n", e.name, argv[which]);
					++bad;
					continue;
				}
				Totals t;
				check(mesh, scene, walk, stream == 0, e.p, centre, seed++, t);
				std::printf("camera_margin_check: %s eye (%g, %g, %g) %s, %s: %llu rays (%llu exact), %llu pairs, %llu accepted hits, margin %g: %llu boxes missed, %llu hits outside their box, %llu pruned wrongly\n",
				            argv[which], (double) e.p[0], (double) e.p[1], (double) e.p[2], e.name, stream ? "stream" : "one-shot", t.rays, t.exact, t.pairs, t.hits,
				            (double) walk.prune_margin, t.missed_boxes, t.outside, t.pruned);
				all.rays += t.rays; all.pairs += t.pairs; all.hits += t.hits; all.exact += t.exact;
				all.missed_boxes += t.missed_boxes; all.outside += t.outside; all.pruned += t.pruned;
			}
		}
	}
	std::printf("camera_margin_check: %llu rays, %llu (ray, box) pairs, %llu accepted hits: %llu violations\n", all.rays, all.pairs, all.hits, all.violations());
	if (stale) {
		if (all.violations() == 0) {
			std::printf("camera_margin_check: the stale array shows no violation: the check has no teeth\n");
			return 1;
		}
		std::printf("camera_margin_check: stale array reported, as it must\n");
		return 0;
	}
	if (all.rays < 1000 || all.hits < 1000) {
		std::printf("FAILED: too few rays or hits to mean anything\n");
		++bad;
	}
	if (all.violations() == 0 && !bad)
		std::printf("camera_margin_check: ok\n");
	return all.violations() || bad ? 1 : 0;
}
