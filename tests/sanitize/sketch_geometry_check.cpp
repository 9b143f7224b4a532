// sketch_geometry_check.cpp — sketch_plan_geometry (csrc/dg_plan.cpp) under
// ASan + UBSan, as its own program (tests/test_sketch_cpu.py compiles it with
// dg_plan.cpp and dg_format.cpp).
//
// argv: p K [off:len]...  Prints "ok <chunk_bytes> <shift>" and one line
// "<span> <chunk>" per work item in grid order, or "fail <status> <message>".
// The constants are checked here: powc[k] = 263^(p-1-k) mod 2^61 - 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../delta-compression_amd/csrc/dg_plan.h"

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	const uint32_t p = (uint32_t)strtoul(argv[1], nullptr, 10), K = (uint32_t)strtoul(argv[2], nullptr, 10);
	std::vector<dg_span_t> spans;
	for (int i = 3; i < argc; ++i) {
		char* end = nullptr;
		dg_span_t s;
		s.off = strtoull(argv[i], &end, 10);
		if (*end != ':') return 2;
		s.len = strtoull(end + 1, nullptr, 10);
		spans.push_back(s);
	}
	dg::SketchGeometry g;
	std::string err;
	const int rc = dg::sketch_plan_geometry(spans.data(), (uint32_t)spans.size(), p, K, 0, g, err);
	if (rc) {
		printf("fail %d %s\n", rc, err.c_str());
		return err.empty() ? 2 : 0;
	}
	if (g.powc.size() != p || g.powc[p - 1] != 1) return 2;
	for (uint32_t k = 0; k + 1 < p; ++k)
		if (g.powc[k] != (uint64_t)((unsigned __int128)g.powc[k + 1] * 263 % ((1ull << 61) - 1))) return 2;
	printf("ok %u %u\n", g.chunk_bytes, g.shift);
	for (const dgsk::SkItem& it : g.items) printf("%u %u\n", it.span, it.chunk);
	return 0;
}
