// refit.cc -- the refit rule on the host and the schedule of the device's inner-box passes (refit.h).
#include "refit.h"

#include <algorithm>
#include <stdexcept>

namespace ocrt {

void refit_boxes(const std::vector<uint32_t> &skips, const std::vector<uint32_t> &leaf_faces, const std::vector<Vec3f> &vertices,
                 std::vector<Vec3f> &aabbs) {
	const size_t count = skips.size();
	if (aabbs.size() != 2 * count)
		throw std::invalid_argument("refit: aabbs must hold a (min,max) pair per node");
	// leaf index of a node = the leaves in front of it
	std::vector<uint32_t> leaf_of(count, 0);
	uint32_t leaves = 0;
	for (size_t i = 0; i < count; ++i)
		if (skips[i] == 1)
			leaf_of[i] = leaves++;
	if ((size_t) leaves * 3 != leaf_faces.size())
		throw std::invalid_argument("refit: leaf count differs from triangle count");
	for (size_t i = count; i-- > 0;) {
		Vec3f lo, hi;
		if (skips[i] == 1) {
			const uint32_t *f = &leaf_faces[(size_t) leaf_of[i] * 3];
			const Vec3f &a = vertices.at(f[0]), &b = vertices.at(f[1]), &c = vertices.at(f[2]);
			for (unsigned k = 0; k < 3; ++k) {
				lo[k] = std::min(a[k], std::min(b[k], c[k]));
				hi[k] = std::max(a[k], std::max(b[k], c[k]));
			}
		} else {
			bool first = true;
			for (size_t c = i + 1; c < i + skips[i] && c < count; c += skips[c] ? skips[c] : 1) {
				if (first) {
					lo = aabbs[2 * c];
					hi = aabbs[2 * c + 1];
					first = false;
					continue;
				}
				for (unsigned k = 0; k < 3; ++k) {
					lo[k] = refit_min(lo[k], aabbs[2 * c][k]);
					hi[k] = refit_max(hi[k], aabbs[2 * c + 1][k]);
				}
			}
		}
		lo.w = hi.w = 0.0f;
		aabbs[2 * i] = lo;
		aabbs[2 * i + 1] = hi;
	}
}

RefitSchedule make_refit_schedule(const std::vector<uint32_t> &skips, uint32_t group_nodes) {
	RefitSchedule out;
	const uint32_t S = group_nodes == 0 ? REFIT_DEFAULT_GROUP : std::min(group_nodes, REFIT_MAX_GROUP);
	out.group_nodes = S;
	const size_t count = skips.size();
	if (count == 0)
		return out;
	if (skips[0] != count)
		throw std::invalid_argument("refit schedule: skips[0] must equal the node count");
	constexpr uint32_t NONE = 0xFFFFFFFFu;
	// Bottom-up: the pass of every inner node, the size of the piece of its own pass that hangs below it (itself included),
	// and its height inside that piece.  (Leaves: pass 0, written by the leaves' launch.)
	std::vector<uint32_t> pass(count, 0), piece(count, 0), round(count, 0), parent(count, NONE);
	uint32_t passes = 0;
	for (size_t i = count; i-- > 0;) {
		if (skips[i] == 1)
			continue;
		if (skips[i] == 0 || i + skips[i] > count)
			throw std::invalid_argument("refit schedule: subtree size runs past the node array");
		uint32_t latest = 1;
		for (size_t c = i + 1; c < i + skips[i]; c += skips[c]) {
			if (skips[c] == 0 || c + skips[c] > i + skips[i])
				throw std::invalid_argument("refit schedule: a child's range leaves its parent's");
			parent[c] = (uint32_t) i;
			latest = std::max(latest, pass[c]);
		}
		uint64_t joined = 1;
		uint32_t height = 0;
		for (size_t c = i + 1; c < i + skips[i]; c += skips[c])
			if (pass[c] == latest) {
				joined += piece[c];
				height = std::max(height, round[c] + 1u);
			}
		if (joined <= S) {
			pass[i] = latest;
			piece[i] = (uint32_t) joined;
			round[i] = height;
		} else {
			pass[i] = latest + 1u;
			piece[i] = 1u;
			round[i] = 0u;
		}
		passes = std::max(passes, pass[i]);
	}
	if (passes == 0)
		return out;  // (the root is a leaf)
	// Pieces into groups, first fit in pre-order with one open group per pass: a pass-1 group is a run of whole subtrees.
	std::vector<uint32_t> group_of(count, NONE), group_pass, group_size, group_rounds;
	std::vector<uint32_t> open(passes + 1, NONE);
	for (size_t i = 0; i < count; ++i) {
		if (skips[i] == 1)
			continue;
		const bool heads = parent[i] == NONE || pass[parent[i]] != pass[i];
		if (!heads) {
			group_of[i] = group_of[parent[i]];
		} else {
			uint32_t g = open[pass[i]];
			if (g == NONE || group_size[g] + piece[i] > S) {
				g = (uint32_t) group_pass.size();
				group_pass.push_back(pass[i]);
				group_size.push_back(0);
				group_rounds.push_back(0);
				open[pass[i]] = g;
			}
			group_size[g] += piece[i];
			group_of[i] = g;
		}
		group_rounds[group_of[i]] = std::max(group_rounds[group_of[i]], round[i] + 1u);
	}
	// the groups by pass (stable: pre-order within a pass), their entries by (round, node)
	const uint32_t groups = (uint32_t) group_pass.size();
	std::vector<uint32_t> by_pass(groups), place(groups), first(groups + 1, 0);
	for (uint32_t g = 0; g < groups; ++g)
		by_pass[g] = g;
	std::stable_sort(by_pass.begin(), by_pass.end(), [&](uint32_t a, uint32_t b) { return group_pass[a] < group_pass[b]; });
	for (uint32_t k = 0; k < groups; ++k)
		place[by_pass[k]] = k;
	for (uint32_t k = 0; k < groups; ++k)
		first[k + 1] = first[k] + group_size[by_pass[k]];
	std::vector<uint32_t> members(first[groups]), filled(groups, 0);
	for (size_t i = 0; i < count; ++i)
		if (skips[i] != 1) {
			const uint32_t k = place[group_of[i]];
			members[first[k] + filled[k]++] = (uint32_t) i;
		}
	std::vector<uint32_t> slot(count, NONE);
	for (uint32_t k = 0; k < groups; ++k) {
		std::sort(members.begin() + first[k], members.begin() + first[k + 1],
		          [&](uint32_t a, uint32_t b) { return round[a] != round[b] ? round[a] < round[b] : a < b; });
		for (uint32_t e = first[k]; e < first[k + 1]; ++e)
			slot[members[e]] = e - first[k];
	}
	out.entries.reserve((size_t) members.size() * 4);
	out.children.reserve(count);
	for (uint32_t k = 0; k < groups; ++k) {
		const uint32_t g = by_pass[k];
		out.groups.insert(out.groups.end(), { first[k], group_size[g], group_rounds[g], group_pass[g] });
		for (uint32_t e = first[k]; e < first[k + 1]; ++e) {
			const size_t i = members[e];
			const uint32_t begin = (uint32_t) out.children.size();
			for (size_t c = i + 1; c < i + skips[i]; c += skips[c])
				out.children.push_back(skips[c] != 1 && pass[c] == pass[i] ? REFIT_LOCAL | slot[c] : (uint32_t) c);
			out.entries.insert(out.entries.end(), { (uint32_t) i, begin, (uint32_t) out.children.size() - begin, round[i] });
		}
	}
	out.pass_first.assign(passes + 1, groups);
	for (uint32_t k = groups; k-- > 0;)
		out.pass_first[group_pass[by_pass[k]] - 1] = k;
	for (uint32_t p = passes; p-- > 0;)  // (a pass always has a group; kept monotone all the same)
		out.pass_first[p] = std::min(out.pass_first[p], out.pass_first[p + 1]);
	return out;
}

}  // namespace ocrt
