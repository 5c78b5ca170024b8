// StageCarve (substrata_amd/csrc/sgp_stage_carve.h) with the regions the five query entry points request, at n = 1 and n = 2^20: every region starts on a
// 16-byte boundary behind the one before it, the total is the last region's end, and the first and last byte of every region lie inside a buffer of `total`
// bytes.  Host only; built with -fsanitize=address,undefined by tests/test_stage_carve.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/sgp.h"
#include "../../substrata_amd/csrc/sgp_stage_carve.h"

struct uint2_ { uint32_t x, y; };      // (the pair lists' entry: HIP's uint2)

static int check(const char* what, uint64_t n, const std::vector<size_t>& sizes)
{
	StageCarve c;
	std::vector<size_t> offs;
	size_t end = 0;
	for (size_t bytes : sizes) {
		const size_t off = c.add(bytes);
		if (off % 16 != 0 || off < end || off - end >= 16) { printf("%s n=%llu: region at %zu after %zu\n", what, (unsigned long long)n, off, end); return 1; }
		end = off + bytes;
		if (c.total != end) { printf("%s n=%llu: total %zu, last region ends at %zu\n", what, (unsigned long long)n, c.total, end); return 1; }
		offs.push_back(off);
	}
	char* buf = (char*)malloc(c.total ? c.total : 1);
	if (!buf) { printf("%s n=%llu: no %zu bytes\n", what, (unsigned long long)n, c.total); return 1; }
	for (size_t i = 0; i < sizes.size(); ++i) if (sizes[i]) {
		char* r = StageCarve::at<char>(buf, offs[i]);
		r[0] = (char)i; r[sizes[i] - 1] = (char)i;      // (out of bounds here is the sanitizer's to report)
	}
	for (size_t i = 0; i < sizes.size(); ++i) if (sizes[i] && (StageCarve::at<char>(buf, offs[i])[0] != (char)i || StageCarve::at<char>(buf, offs[i])[sizes[i] - 1] != (char)i)) { printf("%s: regions overlap\n", what); return 1; }
	free(buf);
	printf("%s n=%llu: %zu regions, %zu bytes\n", what, (unsigned long long)n, sizes.size(), c.total);
	return 0;
}

int main()
{
	int bad = 0;
	for (uint64_t n : { (uint64_t)1, (uint64_t)1 << 20 }) {
		const size_t cap = (size_t)(4 * n + 1), pcap = (size_t)(2 * n + 1) > 64 ? (size_t)(2 * n + 1) : 64;      // the first guesses of the list calls
		bad += check("sgp_raycast", n, { sizeof(sgp_ray) * n, sizeof(sgp_hit) * n });
		bad += check("sgp_spherecast", n, { sizeof(sgp_ray) * n, sizeof(float) * n, sizeof(sgp_hit) * n });
		bad += check("sgp_collide_capsules", n, { sizeof(sgp_capsule_query) * n, sizeof(sgp_query_contact) * cap, 16 });
		bad += check("sgp_collide_shapes", n, { sizeof(sgp_shape_query) * n, 16, sizeof(sgp_query_contact) * cap, 3 * sizeof(uint2_) * pcap });
		bad += check("sgp_cast_shapes", n, { sizeof(sgp_shape_cast) * n, 32, sizeof(sgp_cast_hit) * 3 * pcap, 3 * sizeof(uint2_) * pcap });
	}
	bad += check("empty regions", 0, { 0, 5, 0, 16, 1 });
	return bad ? 1 : 0;
}
