// signed_check.cc -- the signed distance oracle (tests/signed_oracle.c over csrc/signed_point.h) as a stand-alone program, for
// a run under the sanitizers: g++ -fsanitize=address,undefined ... tests/signed_check.cc && ./signed_check FILE ...
// TEST INFRASTRUCTURE ONLY.
//
// FILE: uint32 leaves, vertices, points; uint32 faces[3 leaves] (leaf order); float vertices[4 V], normals[4 V],
// points[4 P]; float expected[P] -- the signed distances another build of the oracle gave.  The program makes the table,
// answers every point with every output on, and compares the distances word for word.
#include <cstdio>
#include <cstring>
#include <vector>

#include "signed_oracle.c"

namespace {

template <class T> bool read(std::FILE *in, std::vector<T> &to, size_t n) {
	to.resize(n);
	return n == 0 || std::fread(to.data(), sizeof(T), n, in) == n;
}

int check(const char *path) {
	std::FILE *in = std::fopen(path, "rb");
	uint32_t head[3];
	if (!in || std::fread(head, sizeof head, 1, in) != 1) {
		std::printf("%s: cannot read\n", path);
		return 1;
	}
	const uint32_t leaves = head[0], vertices = head[1], points = head[2];
	std::vector<uint32_t> faces, leaf;
	std::vector<float> v4, n4, q4, expected;
	const bool ok = read(in, faces, 3u * (size_t) leaves) && read(in, v4, 4u * (size_t) vertices) && read(in, n4, 4u * (size_t) vertices) &&
	                read(in, q4, 4u * (size_t) points) && read(in, expected, points);
	std::fclose(in);
	if (!ok) {
		std::printf("%s: short file\n", path);
		return 1;
	}
	for (uint32_t id : faces)
		if (id >= vertices) {
			std::printf("%s: a face names vertex %u of %u\n", path, id, vertices);
			return 1;
		}
	std::vector<float> table((size_t) SP_REC_FLOATS * leaves), distance(points), bary(3u * (size_t) points), pos(3u * (size_t) points),
	    normal(3u * (size_t) points), pseudo(4u * (size_t) points);
	std::vector<uint8_t> found(points), feature(points);
	leaf.resize(points);
	if (so_table(faces.data(), leaves, v4.data(), vertices, table.data()) != 0)
		return 1;
	so_signed_distance(faces.data(), leaves, v4.data(), n4.data(), table.data(), q4.data(), points, INFINITY, found.data(), distance.data(),
	                   leaf.data(), bary.data(), pos.data(), normal.data(), feature.data(), pseudo.data());
	unsigned mismatches = 0, inside = 0, classes[7] = { 0, 0, 0, 0, 0, 0, 0 };
	for (uint32_t i = 0; i < points; ++i) {
		mismatches += std::memcmp(&distance[i], &expected[i], sizeof(float)) != 0;
		inside += distance[i] < 0.0f;
		if (feature[i] < 7u)
			++classes[feature[i]];
	}
	std::printf("%s: %u points, inside %u, face %u, vertices %u, edges %u, mismatches %u\n", path, points, inside, classes[0],
	            classes[1] + classes[2] + classes[3], classes[4] + classes[5] + classes[6], mismatches);
	return mismatches != 0;
}

}  // namespace

int main(int argc, char **argv) {
	int failed = 0;
	for (int k = 1; k < argc; ++k)
		failed |= check(argv[k]);
	return failed;
}
