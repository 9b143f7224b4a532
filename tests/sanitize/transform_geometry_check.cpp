// transform_geometry_check.cpp — the sizing of the in-place and compose plans
// (inplace_plan_geometry, compose_plan_geometry, their encode-plan variants and
// pair_out_bound; dg_plan.cpp: no HIP) under AddressSanitizer + UBSan
// (tests/test_transform_geometry_cpu.py).  The invariants are checked here (a
// miss prints FAIL and the exit status is 1); the figures the test pins are
// printed, one line per case.
#include <cstdio>
#include <string>
#include <vector>

#include "../../delta-compression_amd/csrc/dg_plan.h"

using namespace dg;

static int g_fail = 0;
#define CHECK(cond)                                              \
	do {                                                         \
		if (!(cond)) {                                           \
			printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
			g_fail = 1;                                          \
		}                                                        \
	} while (0)

static const uint64_t G4 = 1ull << 32;

// work regions: 16-byte aligned, ascending, back to back, each work_bytes long
static void check_inplace(const InplaceGeometry& g, const std::vector<uint64_t>& extra) {
	uint64_t at = 0, bound = 0;
	CHECK(g.descs.size() == extra.size());
	for (size_t i = 0; i < g.descs.size(); ++i) {
		const dgip::IpDesc& d = g.descs[i];
		CHECK(d.work_off % 16 == 0);
		CHECK(d.work_off == at);
		at += dgip::work_bytes(d.max_copies, d.max_adds);
		bound += d.delta_cap + extra[i];
	}
	CHECK(g.work == at);
	CHECK(g.bound == bound);
}

static void check_compose(const ComposeGeometry& g) {
	uint64_t at = 0;
	for (const dgcp::CpDesc& d : g.descs) {
		CHECK(d.work_off % 16 == 0);
		CHECK(d.work_off == at);
		at += dgcp::work_bytes(d.max_a, d.max_b);
	}
	CHECK(g.work == at);
}

// what dg_inplace_plan_create takes as the bytes delta i's COPYs can turn into
// ADD payload: every possible COPY the whole reference, capped at 4 GiB
static uint64_t extra_of(const dg_inplace_desc_t& d, uint32_t max_copies) {
	const uint64_t e = (uint64_t)max_copies * d.ref_len;
	return e < G4 ? e : G4;
}

static void one_capacity(uint64_t cap) {
	std::string err;
	InplaceGeometry ig;
	const dg_inplace_desc_t id{64, 1000, 128, cap};
	const int irc = inplace_plan_geometry(&id, 1, ig, err);
	CHECK((irc != 0) == !err.empty());
	if (irc == DG_OK) {
		CHECK(ig.descs[0].ref_off == 64 && ig.descs[0].ref_len == 1000 && ig.descs[0].delta_off == 128 && ig.descs[0].delta_cap == cap);
		check_inplace(ig, {extra_of(id, ig.descs[0].max_copies)});
		printf("inplace %llu %d %u %u %llu %llu\n", (unsigned long long)cap, irc, ig.descs[0].max_copies, ig.descs[0].max_adds,
		       (unsigned long long)ig.bound, (unsigned long long)ig.work);
	} else {
		printf("inplace %llu %d - - - -\n", (unsigned long long)cap, irc);
	}
	err.clear();
	ComposeGeometry cg;
	const dg_compose_desc_t cd{0, cap, 4096, 38};
	const int crc = compose_plan_geometry(&cd, 1, cg, err);
	CHECK((crc != 0) == !err.empty());
	if (crc == DG_OK) {
		CHECK(cg.descs[0].a_off == 0 && cg.descs[0].a_cap == cap && cg.descs[0].b_off == 4096 && cg.descs[0].b_cap == 38);
		CHECK(cg.descs[0].max_a == compose_max_cmds(cap));
		check_compose(cg);
		printf("compose %llu %d %u %u %llu\n", (unsigned long long)cap, crc, cg.descs[0].max_a, cg.descs[0].max_b,
		       (unsigned long long)cg.work);
	} else {
		printf("compose %llu %d - - -\n", (unsigned long long)cap, crc);
	}
	// the same capacity as stream B
	err.clear();
	const dg_compose_desc_t cb{0, 38, 4096, cap};
	const int brc = compose_plan_geometry(&cb, 1, cg, err);
	CHECK(brc == crc);
	if (brc == DG_OK) CHECK(cg.descs[0].max_b == compose_max_cmds(cap) && cg.descs[0].max_a == 1);
}

static void empty_batches() {
	std::string err;
	InplaceGeometry ig;
	CHECK(inplace_plan_geometry(nullptr, 0, ig, err) == DG_OK && ig.descs.empty() && ig.work == 0 && ig.bound == 0);
	ComposeGeometry cg;
	CHECK(compose_plan_geometry(nullptr, 0, cg, err) == DG_OK && cg.descs.empty() && cg.work == 0);
	const EncodePlanView none{nullptr, nullptr, DG_ALGO_ONEPASS, 16};
	CHECK(inplace_plan_geometry_for(none, 0, ig, err) == DG_OK && ig.descs.empty() && ig.work == 0 && ig.bound == 0);
	CHECK(compose_plan_geometry_for(none, none, 0, cg, err) == DG_OK && cg.descs.empty() && cg.work == 0);
	CHECK(err.empty());
	printf("empty 0\n");
}

static void large_reference() {
	std::string err;
	InplaceGeometry ig;
	const dg_inplace_desc_t big{0, G4, 0, 100};
	const int rc = inplace_plan_geometry(&big, 1, ig, err);
	CHECK(!err.empty());
	printf("ref_4g %d\n", rc);
	err.clear();
	const dg_inplace_desc_t below{0, G4 - 1, 0, 100};
	const int rc2 = inplace_plan_geometry(&below, 1, ig, err);
	printf("ref_below_4g %d\n", rc2);
	// a batch whose last stream is too large fails as a whole
	err.clear();
	const dg_inplace_desc_t mixed[3] = {{0, 10, 0, 100}, {10, 10, 100, 100}, {20, 10, 200, G4}};
	printf("last_4g %d\n", inplace_plan_geometry(mixed, 3, ig, err));
	ComposeGeometry cg;
	const dg_compose_desc_t cm[2] = {{0, 100, 0, 100}, {100, 100, 100, G4}};
	printf("compose_last_4g %d\n", compose_plan_geometry(cm, 2, cg, err));
}

static void mixed_batch() {
	const uint32_t n = 1000;
	std::vector<dg_inplace_desc_t> id(n);
	std::vector<dg_compose_desc_t> cd(n);
	uint64_t x = 0x9E3779B97F4A7C15ull, ro = 0, dofs = 0;
	for (uint32_t i = 0; i < n; ++i) {
		x = x * 6364136223846793005ull + 1442695040888963407ull;
		// every tenth capacity from around the header and the first commands, the rest up to 64 KiB
		const uint64_t cap = i % 10 == 0 ? 20 + (x >> 33) % 24 : (x >> 33) % 65536;
		const uint64_t rl = (x >> 13) % 100000;
		id[i] = dg_inplace_desc_t{ro, rl, dofs, cap};
		cd[i] = dg_compose_desc_t{dofs, cap, ro, rl};
		ro += rl;
		dofs += cap;
	}
	std::string err;
	InplaceGeometry ig;
	CHECK(inplace_plan_geometry(id.data(), n, ig, err) == DG_OK && ig.descs.size() == n);
	std::vector<uint64_t> extra(n);
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t body = id[i].delta_cap > 25 ? id[i].delta_cap - 25 : 0;
		CHECK(ig.descs[i].max_copies == body / 13 && ig.descs[i].max_adds == body / 9);
		extra[i] = extra_of(id[i], ig.descs[i].max_copies);
	}
	check_inplace(ig, extra);
	ComposeGeometry cg;
	CHECK(compose_plan_geometry(cd.data(), n, cg, err) == DG_OK && cg.descs.size() == n);
	for (uint32_t i = 0; i < n; ++i)
		CHECK(cg.descs[i].max_a == compose_max_cmds(cd[i].a_cap) && cg.descs[i].max_b == compose_max_cmds(cd[i].b_cap));
	check_compose(cg);
	CHECK(err.empty());
	printf("mixed %u %llu %llu %llu\n", n, (unsigned long long)ig.work, (unsigned long long)ig.bound, (unsigned long long)cg.work);
}

static void encode_plan_variants() {
	const dg_algorithm_t algos[] = {DG_ALGO_ONEPASS, DG_ALGO_CORRECTING, DG_ALGO_GREEDY};
	const uint64_t ps[] = {1, 16, 21, 22, 23};
	for (dg_algorithm_t algo : algos)
		for (uint64_t p : ps) {
			const uint64_t vls[4] = {0, p - 1, p, 65536};
			std::vector<dg_pair_t> pairs;
			uint64_t ro = 0, vo = 0;
			for (uint64_t vl : vls) {
				pairs.push_back(dg_pair_t{ro, 4096, vo, vl});
				ro += 4096;
				vo += (vl + 15) & ~15ull;
			}
			const uint32_t n = (uint32_t)pairs.size();
			dg_diff_options_t o{};
			o.p = p;
			o.q = DG_TABLE_SIZE;
			o.buf_cap = DG_BUF_CAP;
			o.max_table = DG_MAX_TABLE_SIZE;
			EncodeGeometry eg;
			std::string err;
			CHECK(encode_geometry(algo, o, pairs.data(), n, PlanEnv(), eg, err) == DG_OK);
			uint64_t sum = 0;
			for (uint32_t i = 0; i < n; ++i) {
				const uint64_t b = pair_out_bound(algo, p, pairs[i].v_len);
				printf("bound %d %llu %llu %llu\n", (int)algo, (unsigned long long)p, (unsigned long long)pairs[i].v_len,
				       (unsigned long long)b);
				sum += b;
			}
			CHECK(sum == eg.out_bound);
			const EncodePlanView view{pairs.data(), eg.pp.data(), algo, p};
			InplaceGeometry ig;
			CHECK(inplace_plan_geometry_for(view, n, ig, err) == DG_OK && ig.descs.size() == n);
			std::vector<uint64_t> extra(n);
			for (uint32_t i = 0; i < n; ++i) {
				const dgip::IpDesc& d = ig.descs[i];
				CHECK(d.ref_off == pairs[i].r_off && d.ref_len == pairs[i].r_len && d.delta_off == 0);
				CHECK(d.delta_cap == pair_out_bound(algo, p, pairs[i].v_len));
				CHECK(d.max_copies == eg.pp[i].rec_cap && d.max_adds == eg.pp[i].rec_cap + 1);
				extra[i] = pairs[i].v_len;
			}
			check_inplace(ig, extra);
			CHECK(ig.bound == eg.out_bound + eg.v_total);
			ComposeGeometry cg;
			CHECK(compose_plan_geometry_for(view, view, n, cg, err) == DG_OK && cg.descs.size() == n);
			for (uint32_t i = 0; i < n; ++i) {
				const dgcp::CpDesc& d = cg.descs[i];
				const uint64_t cap = pair_out_bound(algo, p, pairs[i].v_len);
				const uint64_t cmds = 2ull * eg.pp[i].rec_cap + 1;
				CHECK(d.a_off == 0 && d.b_off == 0 && d.a_cap == cap && d.b_cap == cap);
				CHECK(d.max_a == (cmds < compose_max_cmds(cap) ? cmds : compose_max_cmds(cap)) && d.max_b == d.max_a);
			}
			check_compose(cg);
			CHECK(err.empty());
		}
}

int main() {
	empty_batches();
	for (uint64_t cap : std::vector<uint64_t>{0, 24, 25, 33, 34, 37, 38, G4 - 1, G4}) one_capacity(cap);
	large_reference();
	mixed_batch();
	encode_plan_variants();
	return g_fail;
}
