// update_check.cpp — dg_update_plan_create's descriptor checks
// (update_check_descs, dg_plan.cpp: no HIP) under AddressSanitizer + UBSan
// (tests/test_update_plan_cpu.py).  Prints one line per case: name, status.
#include <cstdio>
#include <string>
#include <vector>

#include "../../delta-compression_amd/csrc/dg_plan.h"

static void show(const char* name, const std::vector<dg_update_desc_t>& d) {
	std::string err;
	const int rc = dg::update_check_descs(d.empty() ? nullptr : d.data(), (uint32_t)d.size(), err);
	printf("%s %d %s\n", name, rc, rc ? err.c_str() : "-");
}

int main() {
	const uint64_t G4 = 1ull << 32;
	show("empty", {});
	show("one", {{0, 100, 50, 0, 40}});
	show("zero_cap", {{7, 0, 0, 0, 0}, {7, 10, 3, 0, 30}});
	show("touching", {{1, 100, 50, 0, 40}, {101, 100, 100, 40, 40}, {201, 1, 0, 80, 26}});
	show("touching_unsorted", {{201, 1, 0, 80, 26}, {1, 100, 50, 0, 40}, {101, 100, 100, 40, 40}});
	show("overlap_one_byte", {{0, 100, 50, 0, 40}, {99, 100, 50, 40, 40}});
	show("overlap_inside", {{0, 1000, 50, 0, 40}, {5000, 10, 5, 40, 40}, {500, 10, 5, 80, 40}});
	show("overlap_same", {{64, 10, 5, 0, 40}, {64, 10, 5, 40, 40}});
	show("cap_4g", {{0, G4, 50, 0, 40}});
	show("ref_4g", {{0, 100, G4, 0, 40}});
	show("delta_4g", {{0, 100, 50, 0, G4}});
	show("cap_below_4g", {{0, G4 - 1, G4 - 1, 0, G4 - 1}});
	show("far_offset", {{G4 * 1000, 100, 50, G4 * 2000, 40}});
	show("wraps", {{~0ull - 5, 100, 50, 0, 40}});
	// many regions back to back, listed in reverse: the sort and the sweep
	std::vector<dg_update_desc_t> many;
	for (uint32_t i = 0; i < 5000; ++i) many.push_back({(4999ull - i) * 37, 37, 30, i * 50ull, 50});
	show("many_touching", many);
	many[1234].buf_cap = 38;
	show("many_one_overlap", many);
	return 0;
}
