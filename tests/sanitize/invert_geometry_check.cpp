// invert_geometry_check.cpp — the sizing of the invert plan
// (invert_plan_geometry{,_for}, csrc/dg_plan.cpp, no HIP) under ASan + UBSan, as
// its own program (tests/test_invert_cpu.py compiles it with dg_plan.cpp and
// dg_format.cpp and compares the figures it prints).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../delta-compression_amd/csrc/dg_plan.h"

using namespace dg;

#define CHECK(c)                                                 \
	do {                                                         \
		if (!(c)) {                                              \
			printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);   \
			return 1;                                            \
		}                                                        \
	} while (0)

int main() {
	const uint64_t G4 = 1ull << 32;
	std::string err;
	// one descriptor per capacity, against a reference of 1000 bytes
	for (uint64_t cap : std::vector<uint64_t>{0, 25, 26, 38, 39, 51, 52, G4 - 1}) {
		const dg_invert_desc_t d{7, 1000, 3, cap};
		InvertGeometry g;
		const int rc = invert_plan_geometry(&d, 1, g, err);
		CHECK(rc == DG_OK && g.descs.size() == 1);
		const dgiv::IvDesc& x = g.descs[0];
		CHECK(x.ref_off == 7 && x.ref_len == 1000 && x.delta_off == 3 && x.delta_cap == cap && x.work_off == 0);
		CHECK(x.max_copies == invert_max_copies(cap));
		CHECK(g.work % 16 == 0);
		printf("cap %llu %d %u %llu %llu\n", (unsigned long long)cap, rc, x.max_copies, (unsigned long long)g.work,
		       (unsigned long long)g.bound);
	}
	{
		InvertGeometry g;
		const int rc = invert_plan_geometry(nullptr, 0, g, err);
		CHECK(err.empty());
		printf("empty %d %llu %llu\n", rc, (unsigned long long)g.work, (unsigned long long)g.bound);
		const EncodePlanView none{nullptr, nullptr, DG_ALGO_ONEPASS, 16};
		CHECK(invert_plan_geometry_for(none, 0, g, err) == DG_OK && g.descs.empty() && g.work == 0 && g.bound == 0);
	}
	{
		InvertGeometry g;
		dg_invert_desc_t d{0, 1000, 0, G4};
		printf("cap_4g %d\n", invert_plan_geometry(&d, 1, g, err));
		CHECK(!err.empty());
		d = dg_invert_desc_t{0, G4, 0, 100};
		printf("ref_4g %d\n", invert_plan_geometry(&d, 1, g, err));
		d = dg_invert_desc_t{0, G4 - 1, 0, 100};
		printf("ref_below_4g %d\n", invert_plan_geometry(&d, 1, g, err));
		const dg_invert_desc_t two[2] = {{0, 10, 0, 100}, {10, 10, 100, G4}};
		printf("last_4g %d\n", invert_plan_geometry(two, 2, g, err));
	}
	{
		const dg_invert_desc_t three[3] = {{0, 10, 0, 26}, {10, 20, 26, 39}, {30, 30, 65, 26 + 7 * 13 + 12}};
		InvertGeometry g;
		const int rc = invert_plan_geometry(three, 3, g, err);
		CHECK(rc == DG_OK && g.descs.size() == 3);
		CHECK(g.descs[0].max_copies == 0 && g.descs[1].max_copies == 1 && g.descs[2].max_copies == 7);
		CHECK(g.work == g.descs[2].work_off + dgiv::work_bytes(7));
		printf("three %d %llu %llu %llu %llu\n", rc, (unsigned long long)g.descs[0].work_off,
		       (unsigned long long)g.descs[1].work_off, (unsigned long long)g.descs[2].work_off, (unsigned long long)g.bound);
	}
	for (dg_algorithm_t algo : {DG_ALGO_ONEPASS, DG_ALGO_CORRECTING, DG_ALGO_GREEDY}) {
		const std::vector<dg_pair_t> pairs = {{4096, 65536, 0, 65536}, {100, 3000, 65536, 3000}, {69632, 0, 68544, 0}};
		dg_diff_options_t o{};
		o.p = 16;
		o.q = DG_TABLE_SIZE;
		o.buf_cap = DG_BUF_CAP;
		o.max_table = DG_MAX_TABLE_SIZE;
		EncodeGeometry eg;
		CHECK(encode_geometry(algo, o, pairs.data(), 3, PlanEnv(), eg, err) == DG_OK);
		const EncodePlanView view{pairs.data(), eg.pp.data(), algo, 16};
		InvertGeometry g;
		CHECK(invert_plan_geometry_for(view, 3, g, err) == DG_OK && g.descs.size() == 3);
		uint64_t work = 0, bound = 0;
		for (uint32_t i = 0; i < 3; ++i) {
			const dgiv::IvDesc& x = g.descs[i];
			CHECK(x.delta_off == 0 && x.work_off == work);
			work += dgiv::work_bytes(x.max_copies);
			bound += dgiv::out_bound(x.max_copies, x.ref_len);
			printf("for %d %u %llu %llu %llu %u %u\n", (int)algo, i, (unsigned long long)x.ref_off, (unsigned long long)x.ref_len,
			       (unsigned long long)x.delta_cap, x.max_copies, eg.pp[i].rec_cap);
		}
		CHECK(g.work == work && g.bound == bound);
	}
	return 0;
}
