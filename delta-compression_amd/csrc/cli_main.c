/*
 * cli_main.c — `delta` command line over libdeltagpu.so.
 *
 * Same argv surface and stdout report lines as the reference CLI
 * (src/c/main.c:158-180 usage, :189-321 encode, :323-400 decode,
 * :402-425 info), so scripts that parse it (tests/transposition-benchmark.sh
 * :50-62) keep working.  All compute runs on the GPU through the C ABI.
 *
 *   delta encode <greedy|onepass|correcting> <ref> <ver> <delta> [options]
 *   delta decode <ref> <delta> <output> [--ignore-hash] [--tile-size N [--chunk-size C]]
 *   delta info <delta>
 *   delta inplace <ref> <delta_in> <delta_out> [--policy localmin|constant]
 *   delta compose <delta_ab> <delta_bc> <delta_out> [--ignore-hash]
 *   delta invert <ref> <delta_in> <delta_out> [--ignore-hash]
 *   delta pick [--seed-len P] [--bins K] <version> <candidate>...
 *   delta read <ref> <delta> <offset> <length> <output>
 *   delta lineage <ref> <offset> <length> <output> <delta>...
 *
 * --inplace / inplace run the CRWI conversion on the host (dg_make_inplace,
 * main.c:279-283 and :427-480).  --splay applies to greedy only (its tie-break
 * among the longest matches); with onepass or correcting it is not provided
 * by this build (exit 1 with a message).  compose joins delta(R -> V1) and
 * delta(V1 -> V2) into delta(R -> V2) on the host (dg_compose): no GPU and
 * none of R, V1 or V2.  invert turns R and delta(R -> V) into delta(V -> R) on
 * the host (dg_invert) without V; it first checks R's CRC against the delta's
 * (on the GPU, as decode does) unless --ignore-hash is given.  pick prints the
 * resemblance score equal/used of the version with every candidate, in argument
 * order, and the candidate to encode against (dg_sketch, dg_sketch_match: host
 * only, no GPU).  decode --tile-size N decodes with the whole GPU
 * (dg_decode_large): a chunked index of the delta (chunks of C bytes), then the
 * version read as tiles of N bytes; messages and exit codes are decode's.
 */
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "delta_gpu.h"

static uint8_t *read_file(const char *path, size_t *len)
{
	FILE *f = fopen(path, "rb");
	if (!f) {
		fprintf(stderr, "Error opening %s: %s\n", path, strerror(errno));
		exit(1);
	}
	fseek(f, 0, SEEK_END);
	long n = ftell(f);
	fseek(f, 0, SEEK_SET);
	uint8_t *b = malloc(n > 0 ? (size_t)n : 1);
	if (!b || (n > 0 && fread(b, 1, (size_t)n, f) != (size_t)n)) {
		fprintf(stderr, "Error reading %s\n", path);
		exit(1);
	}
	fclose(f);
	*len = (size_t)n;
	return b;
}

static void write_file(const char *path, const uint8_t *d, size_t n)
{
	FILE *f = fopen(path, "wb");
	if (!f) {
		fprintf(stderr, "Error writing %s: %s\n", path, strerror(errno));
		exit(1);
	}
	if (n && fwrite(d, 1, n, f) != n) {
		fprintf(stderr, "Error writing %s\n", path);
		exit(1);
	}
	fclose(f);
}

static double now(void)
{
	struct timespec t;
	clock_gettime(CLOCK_MONOTONIC, &t);
	return t.tv_sec + t.tv_nsec / 1e9;
}

static void hex(FILE *f, const uint8_t *b, size_t n)
{
	for (size_t i = 0; i < n; i++) fprintf(f, "%02x", b[i]);
}

static size_t parse_size_suffix(const char *s)   /* main.c:145-154 */
{
	char *end;
	unsigned long long n = strtoull(s, &end, 10);
	if (*end == 'k' || *end == 'K') n *= 1000ULL;
	else if (*end == 'M' || *end == 'm') n *= 1000000ULL;
	else if (*end == 'B' || *end == 'b') n *= 1000000000ULL;
	return (size_t)n;
}

static void usage(void)
{
	fprintf(stderr,
	    "Usage:\n"
	    "  delta encode <algorithm> <ref> <ver> <delta> [options]\n"
	    "  delta decode <ref> <delta> <output> [--ignore-hash] [--tile-size N [--chunk-size C]]\n"
	    "  delta info <delta>\n"
	    "  delta inplace <ref> <delta_in> <delta_out> [--policy P]\n"
	    "  delta compose <delta_ab> <delta_bc> <delta_out> [--ignore-hash]\n"
	    "  delta invert <ref> <delta_in> <delta_out> [--ignore-hash]\n"
	    "  delta pick [--seed-len P] [--bins K] <version> <candidate>...\n"
	    "  delta read <ref> <delta> <offset> <length> <output>\n"
	    "  delta lineage <ref> <offset> <length> <output> <delta>...\n"
	    "\n"
	    "Algorithms: greedy, onepass, correcting (MI355X)\n"
	    "\n"
	    "Options:\n"
	    "  --seed-len N     Seed length (default %d)\n"
	    "  --table-size N   Hash table size floor (default %lu)\n"
	    "  --max-table N    Max hash table size, k/M/B suffix ok (default %lu)\n"
	    "  --inplace        Produce in-place delta\n"
	    "  --policy P       Cycle policy: localmin (default), constant\n"
	    "  --verbose        Print diagnostics\n"
	    "  --splay          Use splay tree instead of hash table (greedy only)\n"
	    "  --segment-size N   encode: cut the version into segments of N bytes (a multiple of 16,\n"
	    "                     k/M/B suffix ok), encode them as one batch and splice the deltas\n"
	    "  --segment-window W bytes of the reference before and after a segment's own range\n"
	    "                     that it may copy from (default N)\n"
	    "  --tile-size N      decode: index the delta in chunks and read the version as tiles of N bytes,\n"
	    "                     one block per tile (0: the default, %u)\n"
	    "  --chunk-size C     with --tile-size: bytes of the delta per chunk of the index, a multiple\n"
	    "                     of 4096 (0: the default, %u)\n",
	    DG_SEED_LEN, (unsigned long)DG_TABLE_SIZE, (unsigned long)DG_MAX_TABLE_SIZE,
	    (unsigned)DG_TILE_BYTES_DEFAULT, (unsigned)DG_CHUNK_BYTES_DEFAULT);
	exit(1);
}

static dg_context_t *ctx_or_die(void)
{
	dg_context_t *ctx = NULL;
	int rc = dg_context_create(-1, &ctx);
	if (rc) {
		fprintf(stderr, "delta: no usable GPU (%s)\n", dg_status_string(rc));
		exit(1);
	}
	return ctx;
}

static int cmd_encode(int argc, char **argv)
{
	if (argc < 6) usage();
	const char *algo_str = argv[2], *ref_path = argv[3], *ver_path = argv[4], *delta_path = argv[5];
	dg_algorithm_t algo;
	if (strcmp(algo_str, "onepass") == 0) algo = DG_ALGO_ONEPASS;
	else if (strcmp(algo_str, "correcting") == 0) algo = DG_ALGO_CORRECTING;
	else if (strcmp(algo_str, "greedy") == 0) algo = DG_ALGO_GREEDY;
	else {
		fprintf(stderr, "Unknown algorithm: %s\n", algo_str);
		return 1;
	}
	dg_diff_options_t o;
	dg_diff_options_default(&o);
	const char *policy_str = "localmin";
	static struct option lo[] = {
		{"seed-len", required_argument, NULL, 's'},
		{"table-size", required_argument, NULL, 't'},
		{"max-table", required_argument, NULL, 'x'},
		{"inplace", no_argument, NULL, 'i'},
		{"policy", required_argument, NULL, 'p'},
		{"verbose", no_argument, NULL, 'v'},
		{"splay", no_argument, NULL, 'y'},
		{"segment-size", required_argument, NULL, 'S'},
		{"segment-window", required_argument, NULL, 'W'},
		{NULL, 0, NULL, 0}};
	uint64_t seg_bytes = 0, seg_window = 0;
	int have_window = 0;
	optind = 6;
	int opt;
	while ((opt = getopt_long(argc, argv, "", lo, NULL)) != -1) {
		switch (opt) {
		case 's': o.p = (size_t)atol(optarg); break;
		case 't': o.q = (size_t)atol(optarg); break;
		case 'x': o.max_table = parse_size_suffix(optarg); break;
		case 'v': o.flags |= 1ull << DG_OPT_VERBOSE; break;
		case 'i': o.flags |= 1ull << DG_OPT_INPLACE; break;
		case 'S': seg_bytes = parse_size_suffix(optarg); break;
		case 'W': seg_window = parse_size_suffix(optarg); have_window = 1; break;
		case 'y':
			if (algo != DG_ALGO_GREEDY) {
				fprintf(stderr, "--splay is not provided by the MI355X build\n");
				return 1;
			}
			o.flags |= 1ull << DG_OPT_SPLAY;
			break;
		case 'p':
			policy_str = optarg;
			if (strcmp(optarg, "constant") == 0) o.flags |= 1ull << DG_OPT_POLICY_CONSTANT;
			break;
		default: usage();
		}
	}
	if (o.p == 0) {
		fprintf(stderr, "error: --seed-len must be >= 1\n");
		return 1;
	}
	if (have_window && !seg_bytes) {
		fprintf(stderr, "error: --segment-window needs --segment-size\n");
		return 1;
	}
	if (!have_window) seg_window = seg_bytes;
	size_t rl, vl;
	uint8_t *r = read_file(ref_path, &rl), *v = read_file(ver_path, &vl);
	dg_context_t *ctx = ctx_or_die();
	dg_buffer_t d = {0};
	double t0 = now();
	/* --segment-size: the pair as segments of V against windows of R, their
	 * deltas spliced on the device into one standard delta */
	int rc = seg_bytes ? dg_encode_large(ctx, algo, r, rl, v, vl, &o, seg_bytes, seg_window, &d)
	                   : dg_encode(ctx, algo, r, rl, v, vl, &o, &d);
	double t1 = now();
	if (rc) {
		fprintf(stderr, "delta: encode failed: %s (%s)\n", dg_status_string(rc), dg_last_error(ctx));
		return 1;
	}
	write_file(delta_path, d.data, d.len);
	dg_delta_info_t inf;
	dg_delta_info(d.data, d.len, &inf);
	const char *splay_str = ((o.flags >> DG_OPT_SPLAY) & 1) ? " [splay]" : "";   /* main.c:298-304 */
	if ((o.flags >> DG_OPT_INPLACE) & 1)
		printf("Algorithm:    %s%s + in-place (%s)\n", algo_str, splay_str, policy_str);
	else
		printf("Algorithm:    %s%s\n", algo_str, splay_str);
	printf("Reference:    %s (%zu bytes)\n", ref_path, rl);
	printf("Version:      %s (%zu bytes)\n", ver_path, vl);
	printf("Delta:        %s (%zu bytes)\n", delta_path, d.len);
	printf("Compression:  %.4f (delta/version)\n", vl == 0 ? 0.0 : (double)d.len / vl);
	printf("Commands:     %llu copies, %llu adds\n", (unsigned long long)inf.num_copies,
	       (unsigned long long)inf.num_adds);
	printf("Copy bytes:   %llu\n", (unsigned long long)inf.copy_bytes);
	printf("Add bytes:    %llu\n", (unsigned long long)inf.add_bytes);
	printf("Src CRC:      "); hex(stdout, inf.src_crc, 8); printf("\n");
	printf("Dst CRC:      "); hex(stdout, inf.dst_crc, 8); printf("\n");
	/* The reference times diff+place only (main.c:262-287); here the whole
	 * device chain incl. CRC and transfers is inside the window. */
	printf("Time:         %.3fs\n", t1 - t0);
	dg_buffer_free(&d);
	dg_context_destroy(ctx);
	free(r);
	free(v);
	return 0;
}

static int cmd_decode(int argc, char **argv)
{
	if (argc < 5) usage();
	const char *ref_path = argv[2], *delta_path = argv[3], *out_path = argv[4];
	int ignore = 0, tiled = 0, chunked = 0;
	size_t tile = 0, chunk = 0;
	for (int a = 5; a < argc; a++) {
		if (strcmp(argv[a], "--ignore-hash") == 0) ignore = 1;
		else if (strcmp(argv[a], "--tile-size") == 0 && a + 1 < argc) { tiled = 1; tile = parse_size_suffix(argv[++a]); }
		else if (strcmp(argv[a], "--chunk-size") == 0 && a + 1 < argc) { chunked = 1; chunk = parse_size_suffix(argv[++a]); }
	}
	if (chunked && !tiled) {
		fprintf(stderr, "delta: --chunk-size needs --tile-size\n");
		return 1;
	}
	if (tile > 0xFFFFFFFFu || chunk > 0xFFFFFFFFu) {
		fprintf(stderr, "delta: --tile-size and --chunk-size are below 4 GiB\n");
		return 1;
	}
	size_t rl, dl;
	uint8_t *r = read_file(ref_path, &rl), *d = read_file(delta_path, &dl);
	dg_delta_info_t inf;
	if (dg_delta_info(d, dl, &inf) == DG_ERR_MALFORMED && (dl < DG_HEADER_SIZE || memcmp(d, "DLT\x03", 4))) {
		fprintf(stderr, "delta_decode: not a delta file\n");
		return 1;
	}
	dg_context_t *ctx = ctx_or_die();
	dg_buffer_t out = {0};
	uint8_t c[8];
	/* --ignore-hash: the checks still run, a mismatch only warns
	 * (main.c:342-356, :376-385) */
	if (ignore && dg_delta_info(d, dl, &inf) == DG_OK && dg_crc64_xz(ctx, r, rl, c) == DG_OK &&
	    memcmp(c, inf.src_crc, 8) != 0)
		fprintf(stderr, "warning: skipping source CRC check (--ignore-hash)\n");
	double t0 = now();
	int rc = tiled ? dg_decode_large(ctx, r, rl, d, dl, ignore, (uint32_t)chunk, (uint32_t)tile, &out)
	               : dg_decode(ctx, r, rl, d, dl, ignore, &out);
	double t1 = now();
	if (rc == DG_ERR_SRC_CRC) {
		dg_crc64_xz(ctx, r, rl, c);
		fprintf(stderr, "source file does not match delta: expected ");
		hex(stderr, inf.src_crc, 8);
		fprintf(stderr, ", got ");
		hex(stderr, c, 8);
		fprintf(stderr, "\n");
		return 1;
	}
	if (rc == DG_ERR_DST_CRC) {
		/* the reference writes the output, then fails its post-check */
		write_file(out_path, out.data, out.len);
		fprintf(stderr, "output integrity check failed\n");
		return 1;
	}
	if (rc) {
		fprintf(stderr, "delta_decode: %s\n", dg_status_string(rc));
		return 1;
	}
	write_file(out_path, out.data, out.len);
	if (ignore && dg_crc64_xz(ctx, out.data, out.len, c) == DG_OK && memcmp(c, inf.dst_crc, 8) != 0)
		fprintf(stderr, "warning: skipping output CRC check (--ignore-hash)\n");
	printf("Format:       %s\n", inf.inplace ? "in-place" : "standard");
	printf("Reference:    %s (%zu bytes)\n", ref_path, rl);
	printf("Delta:        %s (%zu bytes)\n", delta_path, dl);
	printf("Output:       %s (%llu bytes)\n", out_path, (unsigned long long)inf.version_size);
	if (!ignore) {
		printf("Src CRC:      "); hex(stdout, inf.src_crc, 8); printf("  OK\n");
		printf("Dst CRC:      "); hex(stdout, inf.dst_crc, 8); printf("  OK\n");
	}
	printf("Time:         %.3fs\n", t1 - t0);
	dg_buffer_free(&out);
	dg_context_destroy(ctx);
	free(r);
	free(d);
	return 0;
}

static int cmd_info(int argc, char **argv)
{
	if (argc < 3) usage();
	size_t dl;
	uint8_t *d = read_file(argv[2], &dl);
	dg_delta_info_t inf;
	int rc = dg_delta_info(d, dl, &inf);
	if (rc) {
		fprintf(stderr, "delta_decode: %s\n",
		        (dl < DG_HEADER_SIZE || memcmp(d, "DLT\x03", 4)) ? "not a delta file" : dg_status_string(rc));
		return 1;
	}
	printf("Delta file:   %s (%zu bytes)\n", argv[2], dl);
	printf("Format:       %s\n", inf.inplace ? "in-place" : "standard");
	printf("Version size: %llu bytes\n", (unsigned long long)inf.version_size);
	printf("Src CRC:      "); hex(stdout, inf.src_crc, 8); printf("\n");
	printf("Dst CRC:      "); hex(stdout, inf.dst_crc, 8); printf("\n");
	printf("Commands:     %llu\n", (unsigned long long)inf.num_commands);
	printf("  Copies:     %llu (%llu bytes)\n", (unsigned long long)inf.num_copies,
	       (unsigned long long)inf.copy_bytes);
	printf("  Adds:       %llu (%llu bytes)\n", (unsigned long long)inf.num_adds,
	       (unsigned long long)inf.add_bytes);
	printf("Output size:  %llu bytes\n", (unsigned long long)(inf.copy_bytes + inf.add_bytes));
	free(d);
	return 0;
}

static int cmd_inplace(int argc, char **argv)   /* main.c:427-480 */
{
	if (argc < 5) usage();
	const char *ref_path = argv[2], *in_path = argv[3], *out_path = argv[4];
	int policy = DG_POLICY_LOCALMIN;
	const char *policy_str = "localmin";
	for (int a = 5; a < argc; a++)
		if (strcmp(argv[a], "--policy") == 0 && a + 1 < argc) {
			policy_str = argv[++a];
			if (strcmp(policy_str, "constant") == 0) policy = DG_POLICY_CONSTANT;
		}
	size_t rl, dl;
	uint8_t *r = read_file(ref_path, &rl), *d = read_file(in_path, &dl);
	dg_buffer_t o = {0};
	dg_inplace_stats_t st;
	double t0 = now();
	int rc = dg_make_inplace(r, rl, d, dl, policy, &o, &st);
	double t1 = now();
	if (rc) {
		fprintf(stderr, "delta_decode: %s\n",
		        (dl < DG_HEADER_SIZE || memcmp(d, "DLT\x03", 4)) ? "not a delta file" : dg_status_string(rc));
		return 1;
	}
	write_file(out_path, o.data, o.len);
	if (st.already_inplace) {
		printf("Delta is already in-place format; copied unchanged.\n");
	} else {
		printf("Reference:    %s (%zu bytes)\n", ref_path, rl);
		printf("Input delta:  %s (%zu bytes)\n", in_path, dl);
		printf("Output delta: %s (%zu bytes)\n", out_path, o.len);
		printf("Format:       in-place (%s)\n", policy_str);
		printf("Commands:     %llu copies, %llu adds\n", (unsigned long long)st.num_copies,
		       (unsigned long long)st.num_adds);
		printf("Copy bytes:   %llu\n", (unsigned long long)st.copy_bytes);
		printf("Add bytes:    %llu\n", (unsigned long long)st.add_bytes);
		printf("Time:         %.3fs\n", t1 - t0);
	}
	dg_buffer_free(&o);
	free(r);
	free(d);
	return 0;
}

static int is_delta_file(const uint8_t *d, size_t dl)
{
	return dl >= DG_HEADER_SIZE && memcmp(d, "DLT\x03", 4) == 0;
}

static int cmd_compose(int argc, char **argv)
{
	if (argc < 5) usage();
	const char *a_path = argv[2], *b_path = argv[3], *out_path = argv[4];
	int ignore = 0;
	for (int k = 5; k < argc; k++)
		if (strcmp(argv[k], "--ignore-hash") == 0) ignore = 1;
	size_t al, bl;
	uint8_t *a = read_file(a_path, &al), *b = read_file(b_path, &bl);
	if (!is_delta_file(a, al) || !is_delta_file(b, bl)) {
		fprintf(stderr, "delta_compose: not a delta file\n");
		return 1;
	}
	dg_buffer_t o = {0};
	double t0 = now();
	int rc = dg_compose(a, al, b, bl, ignore, &o);
	double t1 = now();
	if (rc == DG_ERR_SRC_CRC) {
		fprintf(stderr, "second delta is not against the first delta's output: expected ");
		hex(stderr, a + 17, 8);
		fprintf(stderr, ", got ");
		hex(stderr, b + 9, 8);
		fprintf(stderr, "\n");
		return 1;
	}
	if (rc == DG_ERR_UNSUPPORTED) {
		fprintf(stderr, "delta_compose: unsupported input (an in-place delta, or commands not placed in sequence)\n");
		return 1;
	}
	if (rc) {
		fprintf(stderr, "delta_compose: %s\n", dg_status_string(rc));
		return 1;
	}
	write_file(out_path, o.data, o.len);
	dg_delta_info_t inf;
	dg_delta_info(o.data, o.len, &inf);
	printf("Input delta:  %s (%zu bytes)\n", a_path, al);
	printf("Input delta:  %s (%zu bytes)\n", b_path, bl);
	printf("Output delta: %s (%zu bytes)\n", out_path, o.len);
	printf("Commands:     %llu copies, %llu adds\n", (unsigned long long)inf.num_copies,
	       (unsigned long long)inf.num_adds);
	printf("Copy bytes:   %llu\n", (unsigned long long)inf.copy_bytes);
	printf("Add bytes:    %llu\n", (unsigned long long)inf.add_bytes);
	printf("Src CRC:      "); hex(stdout, inf.src_crc, 8); printf("\n");
	printf("Dst CRC:      "); hex(stdout, inf.dst_crc, 8); printf("\n");
	printf("Time:         %.3fs\n", t1 - t0);
	dg_buffer_free(&o);
	free(a);
	free(b);
	return 0;
}

static int cmd_invert(int argc, char **argv)
{
	if (argc < 5) usage();
	const char *ref_path = argv[2], *in_path = argv[3], *out_path = argv[4];
	int ignore = 0;
	for (int k = 5; k < argc; k++)
		if (strcmp(argv[k], "--ignore-hash") == 0) ignore = 1;
	size_t rl, dl;
	uint8_t *r = read_file(ref_path, &rl), *d = read_file(in_path, &dl);
	if (!is_delta_file(d, dl)) {
		fprintf(stderr, "delta_invert: not a delta file\n");
		return 1;
	}
	if (!ignore) {
		/* the library does not check R: the inverse would only fail when decoded */
		dg_context_t *ctx = ctx_or_die();
		uint8_t c[8];
		int rc = dg_crc64_xz(ctx, r, rl, c);
		dg_context_destroy(ctx);
		if (rc) {
			fprintf(stderr, "delta_invert: %s\n", dg_status_string(rc));
			return 1;
		}
		if (memcmp(c, d + 9, 8) != 0) {
			fprintf(stderr, "source file does not match delta: expected ");
			hex(stderr, d + 9, 8);
			fprintf(stderr, ", got ");
			hex(stderr, c, 8);
			fprintf(stderr, "\n");
			return 1;
		}
	}
	dg_buffer_t o = {0};
	double t0 = now();
	int rc = dg_invert(r, rl, d, dl, &o);
	double t1 = now();
	if (rc == DG_ERR_UNSUPPORTED) {
		fprintf(stderr, "delta_invert: unsupported input (an in-place delta, or commands not placed in sequence)\n");
		return 1;
	}
	if (rc) {
		fprintf(stderr, "delta_invert: %s\n", dg_status_string(rc));
		return 1;
	}
	write_file(out_path, o.data, o.len);
	dg_delta_info_t inf;
	dg_delta_info(o.data, o.len, &inf);
	printf("Reference:    %s (%zu bytes)\n", ref_path, rl);
	printf("Input delta:  %s (%zu bytes)\n", in_path, dl);
	printf("Output delta: %s (%zu bytes)\n", out_path, o.len);
	printf("Commands:     %llu copies, %llu adds\n", (unsigned long long)inf.num_copies,
	       (unsigned long long)inf.num_adds);
	printf("Copy bytes:   %llu\n", (unsigned long long)inf.copy_bytes);
	printf("Add bytes:    %llu\n", (unsigned long long)inf.add_bytes);
	printf("Src CRC:      "); hex(stdout, inf.src_crc, 8); printf("\n");
	printf("Dst CRC:      "); hex(stdout, inf.dst_crc, 8); printf("\n");
	printf("Time:         %.3fs\n", t1 - t0);
	dg_buffer_free(&o);
	free(r);
	free(d);
	return 0;
}

/* delta read <ref> <delta> <offset> <length> <output>: bytes [offset, offset +
 * length) of the version, by the host function (no GPU, no CRC check) */
static int cmd_read(int argc, char **argv)
{
	if (argc < 7) usage();
	char *e1 = NULL, *e2 = NULL;
	errno = 0;
	unsigned long long off = strtoull(argv[4], &e1, 10), len = strtoull(argv[5], &e2, 10);
	/* digits only: strtoull alone would take a sign or leading blanks */
	if (errno || argv[4][0] < '0' || argv[4][0] > '9' || *e1 || argv[5][0] < '0' || argv[5][0] > '9' || *e2) {
		fprintf(stderr, "delta_read: offset and length are decimal byte counts\n");
		return 1;
	}
	size_t rl, dl;
	uint8_t *r = read_file(argv[2], &rl), *d = read_file(argv[3], &dl);
	dg_buffer_t o = {0};
	int rc = dg_read(r, rl, d, dl, off, len, &o);
	free(r);
	free(d);
	if (rc) {
		fprintf(stderr, "delta_read: %s\n", dg_status_string(rc));
		return 1;
	}
	write_file(argv[6], o.data, o.len);
	dg_buffer_free(&o);
	return 0;
}

/* delta lineage <ref> <offset> <length> <output> <delta>...: bytes [offset,
 * offset + length) of the version the deltas make of <ref>, the first on <ref>,
 * each next one on the version before it; by the host function (no GPU, no
 * CRC check, no version rebuilt) */
static int cmd_lineage(int argc, char **argv)
{
	if (argc < 7) usage();
	char *e1 = NULL, *e2 = NULL;
	errno = 0;
	unsigned long long off = strtoull(argv[3], &e1, 10), len = strtoull(argv[4], &e2, 10);
	/* digits only: strtoull alone would take a sign or leading blanks */
	if (errno || argv[3][0] < '0' || argv[3][0] > '9' || *e1 || argv[4][0] < '0' || argv[4][0] > '9' || *e2) {
		fprintf(stderr, "delta_lineage: offset and length are decimal byte counts\n");
		return 1;
	}
	const int k = argc - 6;
	if (k > (int)DG_LINEAGE_MAX_DEPTH) {
		fprintf(stderr, "delta_lineage: at most %u deltas\n", (unsigned)DG_LINEAGE_MAX_DEPTH);
		return 1;
	}
	size_t rl, dl[DG_LINEAGE_MAX_DEPTH];
	uint8_t *d[DG_LINEAGE_MAX_DEPTH];
	uint8_t *r = read_file(argv[2], &rl);
	for (int j = 0; j < k; j++) d[j] = read_file(argv[6 + j], &dl[j]);
	dg_buffer_t o = {0};
	int rc = dg_read_lineage(r, rl, (const uint8_t *const *)d, dl, (uint32_t)k, off, len, &o);
	free(r);
	for (int j = 0; j < k; j++) free(d[j]);
	if (rc) {
		fprintf(stderr, "delta_lineage: %s\n", dg_status_string(rc));
		return 1;
	}
	write_file(argv[5], o.data, o.len);
	dg_buffer_free(&o);
	return 0;
}

/* delta pick [--seed-len P] [--bins K] <version> <candidate>...: which candidate
 * to encode the version against, by the host functions (no GPU) */
static int cmd_pick(int argc, char **argv)
{
	uint32_t p = DG_SEED_LEN, K = DG_SKETCH_BINS;
	static struct option lo[] = {
		{"seed-len", required_argument, NULL, 's'},
		{"bins", required_argument, NULL, 'b'},
		{NULL, 0, NULL, 0}};
	optind = 2;
	int opt;
	while ((opt = getopt_long(argc, argv, "", lo, NULL)) != -1) {
		if (opt != 's' && opt != 'b') usage();
		char *end = NULL;
		unsigned long v = strtoul(optarg, &end, 10);
		if (!*optarg || *end || v > 0xFFFFFFFFul) {
			fprintf(stderr, "delta_pick: bad option value: %s\n", optarg);
			return 1;
		}
		if (opt == 's') p = (uint32_t)v;
		else K = (uint32_t)v;
	}
	if (argc - optind < 2) usage();
	const int n = argc - optind - 1;   /* candidates */
	if (p < 1 || p > 64 || K < 16 || K > 1024 || (K & (K - 1))) {
		fprintf(stderr, "delta_pick: --seed-len must be 1..64 and --bins a power of two in 16..1024\n");
		return 1;
	}
	uint64_t *sk = malloc((size_t)(n + 1) * K * sizeof *sk);
	dg_match_t one;
	if (!sk) {
		fprintf(stderr, "delta_pick: out of memory\n");
		return 1;
	}
	for (int i = 0; i <= n; i++) {   /* sketch 0: the version */
		size_t len;
		uint8_t *d = read_file(argv[optind + i], &len);
		int rc = dg_sketch(d, len, p, K, sk + (size_t)i * K);
		free(d);
		if (rc) {
			fprintf(stderr, "delta_pick: %s: %s\n", argv[optind + i], dg_status_string(rc));
			return 1;
		}
	}
	for (int i = 1; i <= n; i++) {
		dg_sketch_match(sk, 1, sk + (size_t)i * K, 1, K, DG_MATCH_ALL, 0, 1, &one);
		if (one.best == DG_MATCH_NONE) {   /* below min_equal: report the plain counts */
			uint32_t used = 0;
			for (uint32_t b = 0; b < K; b++)
				used += sk[b] != DG_SKETCH_EMPTY || sk[(size_t)i * K + b] != DG_SKETCH_EMPTY;
			one.equal = 0, one.used = used;
		}
		printf("%u/%u\t%s\n", one.equal, one.used, argv[optind + i]);
	}
	dg_sketch_match(sk, 1, sk + K, (uint32_t)n, K, DG_MATCH_ALL, 0, 1, &one);
	if (one.best == DG_MATCH_NONE) printf("best: none\n");
	else printf("best: %s\n", argv[optind + 1 + one.best]);
	free(sk);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2) usage();
	if (strcmp(argv[1], "encode") == 0) return cmd_encode(argc, argv);
	if (strcmp(argv[1], "decode") == 0) return cmd_decode(argc, argv);
	if (strcmp(argv[1], "info") == 0) return cmd_info(argc, argv);
	if (strcmp(argv[1], "inplace") == 0) return cmd_inplace(argc, argv);
	if (strcmp(argv[1], "compose") == 0) return cmd_compose(argc, argv);
	if (strcmp(argv[1], "invert") == 0) return cmd_invert(argc, argv);
	if (strcmp(argv[1], "pick") == 0) return cmd_pick(argc, argv);
	if (strcmp(argv[1], "read") == 0) return cmd_read(argc, argv);
	if (strcmp(argv[1], "lineage") == 0) return cmd_lineage(argc, argv);
	usage();
	return 1;
}
