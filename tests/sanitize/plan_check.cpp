// plan_check.cpp — runs the library's plan arithmetic (dg_plan.cpp) on the
// CPU under AddressSanitizer + UBSan for tests/test_plan_cpu.py.
//
// Input: one case per line on stdin; output: one line of JSON per case.
//
//   geom ALGO P Q BUF_CAP MAX_TABLE FLAGS N_CU LDS POOL MEMBERS N (R_OFF R_LEN V_OFF V_LEN) x N
//       encode_geometry of the batch (MEMBERS: DG_LIMIT_ONEPASS_MEMBERS); prints
//       the status, the message and every field of the geometry
//   crc
//       crc_tables_build: the tables in hex and the layout constants
//   verbose ALGO P FLAGS R_LEN V_LEN TRUNC HEX
//       print_verbose (to stderr) of the delta HEX, and with TRUNC = 1 of each
//       of its prefixes; prints {"ok":1}
//
// The driver only reports; the test compares with the oracle.  Any memory
// error or UB aborts with a non-zero status.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../delta-compression_amd/csrc/dg_plan.h"

using namespace dg;

namespace {

template <class V, class F>
void list(const char* name, const V& v, F&& item) {
	printf(",\"%s\":[", name);
	for (size_t i = 0; i < v.size(); ++i) {
		if (i) printf(",");
		item(v[i]);
	}
	printf("]");
}

PlanEnv env_of(uint32_t n_cu, int lds, uint64_t pool, uint64_t members) {
	PlanEnv e;
	e.n_cu = n_cu;
	e.lds_bytes = lds;
	e.table_pool_bytes = pool;
	e.onepass_members = members;
	return e;
}

void geom(std::istringstream& in) {
	int algo;
	dg_diff_options_t o;
	uint32_t n_cu, n;
	int lds;
	uint64_t pool, members;
	in >> algo >> o.p >> o.q >> o.buf_cap >> o.max_table >> o.flags >> n_cu >> lds >> pool >> members >> n;
	std::vector<dg_pair_t> pairs(n);
	for (auto& d : pairs) in >> d.r_off >> d.r_len >> d.v_off >> d.v_len;
	EncodeGeometry g;
	std::string err;
	const int rc = encode_geometry((dg_algorithm_t)algo, o, pairs.data(), n, env_of(n_cu, lds, pool, members), g, err);
	printf("{\"rc\":%d,\"err\":\"%s\"", rc, err.c_str());
	if (rc == DG_OK) {
		printf(",\"out_bound\":%" PRIu64 ",\"total_rec\":%" PRIu64 ",\"qmax\":%" PRIu64 ",\"qmin\":%" PRIu64
		       ",\"ctab_entries\":%" PRIu64 ",\"greedy_heads\":%" PRIu64 ",\"greedy_entries\":%" PRIu64
		       ",\"max_seeds\":%" PRIu64 ",\"aligned16\":%d,\"v_total\":%" PRIu64 ",\"corr_lds_cap\":%u"
		       ",\"crc_fused\":%d,\"table_bytes\":%" PRIu64 ",\"n_tables\":%u,\"fused\":%d,\"members\":%d"
		       ",\"route_min\":%u,\"mem_slots\":%" PRIu64 ",\"n_chunks\":%u",
		       g.out_bound, g.total_rec, g.qmax, g.qmin, g.ctab_entries, g.greedy_heads, g.greedy_entries,
		       g.max_seeds, (int)g.aligned16, g.v_total, g.corr_lds_cap, (int)g.crc_fused, g.table_bytes,
		       g.n_tables, (int)g.fused, (int)g.members, g.route_min, g.mem_slots, g.n_chunks);
		list("pp", g.pp, [](const PairPlanDev& x) {
			printf("{\"q\":%" PRIu64 ",\"q_magic\":%" PRIu64 ",\"rec_base\":%" PRIu64 ",\"rec_cap\":%u,\"f_size\":%" PRIu64
			       ",\"f_magic\":%" PRIu64 ",\"m\":%" PRIu64 ",\"m_magic\":%" PRIu64 ",\"tab_base\":%" PRIu64
			       ",\"mem_base\":%" PRIu64 ",\"chunk_base\":%u,\"n_chunks\":%u,\"crc_unpad\":%" PRIu64 "}",
			       x.q, x.q_magic, x.rec_base, x.rec_cap, x.f_size, x.f_magic, x.m, x.m_magic, x.tab_base,
			       x.mem_base, x.chunk_base, x.n_chunks, x.crc_unpad);
		});
		list("powc", g.powc, [](uint64_t c) { printf("%" PRIu64, c); });
		list("gpairs", g.gpairs, [](uint32_t i) { printf("%u", i); });
		list("spans", g.spans, [](const CrcSpanDev& s) {
			printf("[%" PRIu64 ",%" PRIu64 ",%u,%u,%u,%u]", s.off, s.len, s.seg_base, s.nseg, s.which, s.out);
		});
		list("segs", g.segs, [](const CrcSegDev& s) { printf("[%u,%u]", s.span, s.j); });
		list("jobs", g.jobs, [](uint32_t w) { printf("%u", w); });
	}
	printf("}\n");
}

void crc() {
	CrcTables t;
	crc_tables_build(t);
	printf("{\"kseg\":\"%016" PRIx64 "\",\"levels\":%d,\"nib_words\":%d,\"fin_tabs\":%d,\"fin_x256\":%d,\"fin_x512\":%d"
	       ",\"fin_x48k\":%d,\"seg_bytes\":%u,\"rows16\":%u,\"rows8\":%u,\"rowk16\":%u,\"rowk8\":%u,\"r5_8\":%u,\"r5_16\":%u"
	       ",\"tab_words\":%u",
	       t.kseg, kCrcLevels, kCrcNibTabWords, kCrcFinTabs, kCrcFinX256, kCrcFinX512, kCrcFinX48K, kCrcSegBytes,
	       kCrcRows16, kCrcRows8, kCrcRowK16, kCrcRowK8, kCrc5R8, kCrc5R16, kCrcTabWords);
	auto hex = [](uint64_t w) { printf("\"%016" PRIx64 "\"", w); };
	list("tab", t.tab, hex);
	list("xinv", std::vector<uint64_t>(t.xinv, t.xinv + 16), hex);
	list("k32", std::vector<uint64_t>(t.k32, t.k32 + 1024), hex);
	printf("}\n");
}

void verbose(std::istringstream& in) {
	int algo, trunc;
	dg_diff_options_t o{0, DG_TABLE_SIZE, DG_BUF_CAP, DG_MAX_TABLE_SIZE, 0};
	dg_pair_t d{};
	std::string hex;
	in >> algo >> o.p >> o.flags >> d.r_len >> d.v_len >> trunc >> hex;
	std::vector<uint8_t> delta(hex.size() / 2);
	for (size_t i = 0; i < delta.size(); ++i) {
		unsigned b = 0;
		sscanf(hex.c_str() + 2 * i, "%2x", &b);
		delta[i] = (uint8_t)b;
	}
	EncodeGeometry g;
	std::string err;
	if (encode_geometry((dg_algorithm_t)algo, o, &d, 1, env_of(256, 65536, 0, 0), g, err) != DG_OK) {
		printf("{\"ok\":0}\n");
		return;
	}
	const uint64_t stats[8] = {5, 4, 3, 2, 1, 1, 0, 4};
	for (size_t len = trunc ? 0 : delta.size(); len <= delta.size(); ++len) {
		// an exact-size copy, so that a read past the prefix is a heap overflow
		std::vector<uint8_t> cut(delta.begin(), delta.begin() + len);
		print_verbose((dg_algorithm_t)algo, o, d, g.pp[0], stats, cut.data(), cut.size());
		if (algo == DG_ALGO_ONEPASS) print_verbose((dg_algorithm_t)algo, o, d, g.pp[0], nullptr, cut.data(), cut.size());
	}
	printf("{\"ok\":1}\n");
}

}  // namespace

int main() {
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string what;
		in >> what;
		if (what == "geom") geom(in);
		else if (what == "crc") crc();
		else if (what == "verbose") verbose(in);
		else if (!what.empty()) {
			fprintf(stderr, "unknown case %s\n", what.c_str());
			return 2;
		}
	}
	return 0;
}
