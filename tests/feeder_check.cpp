/*
 * tests/feeder_check.cpp -- the staging slot lifecycle of ntsmCount's host side (ntsm_amd/csrc/host/feeder.cpp) on the CPU,
 * against a fake of the few libntsm_hip calls it makes.  Linked with feeder.cpp and pack2.cpp only; built with
 * -fsanitize=address,undefined and run by tests/test_host_cpu.py.
 *
 * The fake allocates every slot with malloc at exactly the capacity it reports (a packed slot: cap / 4 and cap / 8 bytes),
 * so a write past a slot is the sanitizer's to find; it aborts on a protocol error (acquire while held, submit while not
 * held, more bytes / positions / reads than the slot has, packed positions that are no multiple of 8) and records every
 * call and every batch.  Slots are the 4096-byte minimum (80 reads).  For the context's own slots, a lane of raw bytes and
 * a lane of packed codes:
 *   order     reads of 0, 1, 7, 8, 31, 32, 33, 150, 4094, 4095, 4096 and 300 x 150 bytes over every byte class come back
 *             from the batches in order, each terminated once (one 'N'; packed: invalid up to the next multiple of 8)
 *   limit     200 one-base reads: a batch of raw bytes ends at 80 reads
 *   sink      has_room() true: feed() submits nothing; false: flush() submits exactly what was staged, feed() nothing
 *   growth    a read longer than the slot reopens it once, at (len + 1) * 3/2 bytes or (len + 64) * 3/2 positions
 *   discard   nothing that was discarded reaches a batch
 *   empty     discard(), then a read longer than the slot: one empty submit, one reopen, no write outside the slot
 *   chunk     submitChunk: own reads go first; a held but empty slot goes back; a chunk larger than the slot grows it to
 *             need * 3/2; an empty chunk does nothing; a Feeder of raw bytes ignores chunks
 *   armed     context with -m: a sync after every submit; early_stop at the third: earlyTerm(), nothing more is submitted
 *   finish    finish() flushes and closes the lane once, the destructor then closes nothing; without finish() it closes once
 * Prints "feeder check ok: <cases> cases" and exits 0, or the first failure and exits 1.  With a file name as argument the
 * trace of the fake's calls is written there.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ntsm_amd/csrc/host/early_ingest.hpp"
#include "../ntsm_amd/csrc/host/feeder.hpp"
#include "../ntsm_amd/csrc/host/pack2.hpp"

using ntsm::Feeder;
using ntsm::Options;
using ntsm::PackedChunk;

/* ------------------------------------------------------------------------------------------------ the fake library */
struct Batch {
	bool packed;
	std::string bytes;                       /* raw bytes, or one class letter per position ('.' = invalid) */
	std::vector<uint64_t> ends;
	uint32_t n_reads;
	uint64_t n_bases;
};

struct Slots {                               /* the pair of slots of a lane or of the context: one is out at a time */
	bool packed = false, held = false;
	uint64_t cap = 0, cap_reads = 0;
	uint8_t *a = nullptr, *b = nullptr;      /* bytes + read ends, or codes + validity */
	void release() { free(a); free(b); a = b = nullptr; held = false; }
};

struct ntsm_ctx { Slots own; };
struct ntsm_lane { Slots s; };

static std::vector<std::string> g_trace;
static std::vector<Batch> g_batches;
static std::vector<uint64_t> g_opens;        /* sizes the slots were opened with */
static int g_closes, g_submits, g_empty_submits, g_syncs, g_stop_at_sync, g_lanes_open;

static void note(const char *what, unsigned long long x = 0, unsigned long long y = 0, unsigned long long z = 0)
{
	char line[160];
	snprintf(line, sizeof line, "%s %llu %llu %llu", what, x, y, z);
	g_trace.push_back(line);
}

[[noreturn]] static void protocol(const char *what)
{
	fprintf(stderr, "feeder check: protocol error: %s\n", what);
	abort();
}

static void open_slots(Slots &s, bool packed, uint64_t cap, uint64_t cap_reads)
{
	if (s.held) protocol("slots resized while one is held");
	s.release();
	s.packed = packed;
	s.cap = packed ? cap & ~31ull : cap;
	s.cap_reads = cap_reads;
	g_opens.push_back(cap);
}

static void acquire(Slots &s)
{
	if (s.held) protocol("acquire while held");
	s.release();                             /* a fresh allocation every time: stale pointers are the sanitizer's */
	s.a = (uint8_t *) malloc(s.packed ? s.cap / 4 : s.cap);
	s.b = (uint8_t *) malloc(s.packed ? s.cap / 8 : s.cap_reads * 8);
	s.held = true;
}

static void submit(Slots &s, uint64_t n, uint32_t n_reads, uint64_t n_bases)
{
	if (!s.held) protocol("submit while not held");
	if (n > s.cap) protocol(s.packed ? "n_positions over cap_positions" : "n_bytes over cap_bytes");
	if (!s.packed && n_reads > s.cap_reads) protocol("n_reads over cap_reads");
	if (s.packed && n % 8) protocol("n_positions not a multiple of 8");
	g_submits++;
	if (n_reads == 0) g_empty_submits++;
	else {
		Batch bt { s.packed, std::string(), {}, n_reads, n_bases };
		if (s.packed)
			for (uint64_t p = 0; p < n; p++)
				bt.bytes += (s.b[p >> 3] >> (p & 7)) & 1 ? "ACGT"[(s.a[p >> 2] >> (2 * (p & 3))) & 3] : '.';
		else {
			bt.bytes.assign((const char *) s.a, n);
			bt.ends.assign((const uint64_t *) s.b, (const uint64_t *) s.b + n_reads);
		}
		g_batches.push_back(bt);
	}
	s.release();
}

extern "C" {
int ntsm_set_batch_capacity(ntsm_ctx *ctx, uint64_t cap_bytes, uint64_t cap_reads)
{
	note("set_batch_capacity", cap_bytes, cap_reads);
	open_slots(ctx->own, false, cap_bytes, cap_reads);
	return 0;
}
int ntsm_staging_acquire(ntsm_ctx *ctx, uint8_t **bases, uint64_t *cap_bytes, uint64_t **read_end, uint64_t *cap_reads)
{
	note("staging_acquire", ctx->own.cap, ctx->own.cap_reads);
	acquire(ctx->own);
	*bases = ctx->own.a, *cap_bytes = ctx->own.cap, *read_end = (uint64_t *) ctx->own.b, *cap_reads = ctx->own.cap_reads;
	return 0;
}
int ntsm_submit_staged(ntsm_ctx *ctx, uint64_t n_bytes, uint32_t n_reads)
{
	note("submit_staged", n_bytes, n_reads);
	submit(ctx->own, n_bytes, n_reads, 0);
	return 0;
}
int ntsm_lane_open(ntsm_ctx *, uint64_t cap_bytes, uint64_t cap_reads, ntsm_lane **out)
{
	note("lane_open", cap_bytes, cap_reads);
	*out = new ntsm_lane();
	open_slots((*out)->s, false, cap_bytes, cap_reads);
	g_lanes_open++;
	return 0;
}
int ntsm_lane_open_packed(ntsm_ctx *, uint64_t cap_positions, ntsm_lane **out)
{
	note("lane_open_packed", cap_positions);
	*out = new ntsm_lane();
	open_slots((*out)->s, true, cap_positions, 0);
	g_lanes_open++;
	return 0;
}
int ntsm_lane_acquire(ntsm_lane *lane, uint8_t **bases, uint64_t *cap_bytes, uint64_t **read_end, uint64_t *cap_reads)
{
	if (lane->s.packed) protocol("ntsm_lane_acquire on a packed lane");
	note("lane_acquire", lane->s.cap, lane->s.cap_reads);
	acquire(lane->s);
	*bases = lane->s.a, *cap_bytes = lane->s.cap, *read_end = (uint64_t *) lane->s.b, *cap_reads = lane->s.cap_reads;
	return 0;
}
int ntsm_lane_acquire_packed(ntsm_lane *lane, uint8_t **codes, uint8_t **valid, uint64_t *cap_positions)
{
	if (!lane->s.packed) protocol("ntsm_lane_acquire_packed on a lane of bytes");
	note("lane_acquire_packed", lane->s.cap);
	acquire(lane->s);
	*codes = lane->s.a, *valid = lane->s.b, *cap_positions = lane->s.cap;
	return 0;
}
int ntsm_lane_submit(ntsm_lane *lane, uint64_t n_bytes, uint32_t n_reads)
{
	if (lane->s.packed) protocol("ntsm_lane_submit on a packed lane");
	note("lane_submit", n_bytes, n_reads);
	submit(lane->s, n_bytes, n_reads, 0);
	return 0;
}
int ntsm_lane_submit_packed(ntsm_lane *lane, uint64_t n_positions, uint32_t n_reads, uint64_t n_bases)
{
	if (!lane->s.packed) protocol("ntsm_lane_submit_packed on a lane of bytes");
	note("lane_submit_packed", n_positions, n_reads, n_bases);
	submit(lane->s, n_positions, n_reads, n_bases);
	return 0;
}
int ntsm_lane_close(ntsm_lane *lane)
{
	note("lane_close");
	lane->s.release();
	delete lane;
	g_closes++;
	g_lanes_open--;
	return 0;
}
int ntsm_sync(ntsm_ctx *, ntsm_totals *totals)
{
	note("sync");
	memset(totals, 0, sizeof *totals);
	totals->early_stop = g_stop_at_sync && ++g_syncs >= g_stop_at_sync;
	totals->reads_consumed = 1;
	return 0;
}
const char *ntsm_strerror(int) { return "fake"; }
int ntsm_last_hip_error(void) { return 0; }
}

/* the two members of PackedChunk that early_ingest.cpp defines; the chunks here are plain malloc */
ntsm::PackedChunk::~PackedChunk() { free(mem); }
void ntsm::PackedChunk::reserve(uint64_t positions)
{
	cap = (positions + 31) & ~31ull;
	mem = malloc(cap / 4 + cap / 8);
	codes = (uint8_t *) mem;
	valid = codes + cap / 4;
}

/* ------------------------------------------------------------------------------------------------ the cases */
enum Mode { CONTEXT, LANE_BYTES, LANE_PACKED };
static const char *const mode_name[] = { "context", "lane of bytes", "packed lane" };

static uint64_t rng_state = 12345;
static uint32_t rnd(uint32_t n)
{
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t) ((rng_state >> 33) % n);
}

/* every class of the reference's byte table (vendor/KseqHashIterator.hpp:114-127), each in all its spellings */
static std::string read_of(uint64_t len)
{
	static const char alphabet[] = { 'A', 'a', 0, 'C', 'c', 1, 'G', 'g', 2, 'T', 't', 'U', 'u', 3, 'N', 'x', '\n', (char) 0xff };
	std::string s(len, 'A');
	uint32_t at = rnd(sizeof alphabet);
	for (char &c : s) {
		c = alphabet[at % sizeof alphabet];
		at += 1 + rnd(3);
	}
	return s;
}

static char class_of(char c)
{
	switch (c) {
	case 'A': case 'a': case 0: return 'A';
	case 'C': case 'c': case 1: return 'C';
	case 'G': case 'g': case 2: return 'G';
	case 'T': case 't': case 'U': case 'u': case 3: return 'T';
	}
	return '.';
}

static int g_cases;
static const char *g_case = "";
static Mode g_mode;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s, %s: %s (line %d)\n", g_case, mode_name[g_mode], #cond, __LINE__); exit(1); } } while (0)

/* the batches hold exactly `reads`, in order, each terminated once */
static void check_batches(const std::vector<std::string> &reads)
{
	size_t next = 0;
	for (const Batch &b : g_batches) {
		uint64_t at = 0, n_bases = 0;
		CHECK(next + b.n_reads <= reads.size());
		for (uint32_t i = 0; i < b.n_reads; i++, next++) {
			const std::string &r = reads[next];
			n_bases += r.size();
			CHECK(at + r.size() < b.bytes.size());
			if (!b.packed) {
				CHECK(b.ends[i] == at + r.size() && b.bytes.compare(at, r.size(), r) == 0 && b.bytes[b.ends[i]] == 'N');
				at = b.ends[i] + 1;
				continue;
			}
			for (uint64_t p = 0; p < r.size(); p++) CHECK(b.bytes[at + p] == class_of(r[p]));
			const uint64_t after = (at + r.size() + 8) & ~7ull;              /* pack2.hpp: the next read starts at a multiple of 8 */
			CHECK(after <= b.bytes.size());
			for (uint64_t p = at + r.size(); p < after; p++) CHECK(b.bytes[p] == '.');
			at = after;
		}
		CHECK(at == b.bytes.size());
		CHECK(!b.packed || b.n_bases == n_bases);
	}
	CHECK(next == reads.size());
}

struct Case {
	Options opt;
	ntsm_ctx ctx;
	Case(const char *name, Mode mode)
	{
		g_case = name;
		g_mode = mode;
		g_trace.push_back(std::string("== ") + name + ", " + mode_name[mode]);
		g_batches.clear();
		g_opens.clear();
		g_closes = g_submits = g_empty_submits = g_syncs = g_stop_at_sync = 0;
		opt.batch_bytes = 1;                                             /* the 4096-byte floor */
		opt.threads = 2;
		opt.pack = mode == LANE_PACKED;
	}
	~Case()
	{
		CHECK(g_lanes_open == 0);
		ctx.own.release();
		g_cases++;
	}
};

static uint64_t grown(Mode mode, uint64_t len)                           /* the size a read of len bytes reopens the slots with */
{
	const uint64_t need = mode == LANE_PACKED ? len + 64 : len + 1;
	return need + need / 2;
}

static void feed_all(Feeder &f, std::vector<std::string> &fed, const std::vector<uint64_t> &lens)
{
	for (uint64_t len : lens) {
		fed.push_back(read_of(len));
		f.feedRead(fed.back().data(), len);
	}
}

static void case_order(Mode mode)
{
	Case c("order", mode);
	std::vector<std::string> fed;
	{
		Feeder f(c.opt, &c.ctx, 0, mode != CONTEXT);
		std::vector<uint64_t> lens = { 0, 1, 7, 8, 31, 32, 33, 150, 4094, 4095, 4096 };
		lens.insert(lens.end(), 300, 150);
		feed_all(f, fed, lens);
		f.finish();
	}
	check_batches(fed);
	/* one reopen, at the first read that a 4096-byte slot does not take: 4096 + 1 bytes, or 4094 + 64 positions */
	CHECK(g_opens == (std::vector<uint64_t> { 4096, grown(mode, mode == LANE_PACKED ? 4094 : 4096) }));
	std::string seen;
	for (const std::string &r : fed) for (char ch : r) if (seen.find(class_of(ch)) == std::string::npos) seen += class_of(ch);
	CHECK(seen.size() == 5);
}

static void case_limit(Mode mode)
{
	Case c("limit", mode);
	std::vector<std::string> fed;
	{
		Feeder f(c.opt, &c.ctx, 0, mode != CONTEXT);
		feed_all(f, fed, std::vector<uint64_t>(200, 1));
		f.finish();
	}
	check_batches(fed);
	if (mode == LANE_PACKED) return;                                     /* 200 x 8 positions: one batch */
	CHECK(g_batches.size() == 3 && g_batches[0].n_reads == 80 && g_batches[1].n_reads == 80 && g_batches[2].n_reads == 40);
}

static void case_sink(Mode mode)
{
	Case c("sink", mode);
	std::vector<std::string> fed;
	int refused = 0;
	{
		Feeder f(c.opt, &c.ctx, 0, mode != CONTEXT);
		uint32_t staged = 0;
		for (int i = 0; i < 120; i++) {
			fed.push_back(read_of(100 + rnd(100)));
			if (!f.has_room(fed.back().size())) {
				const int before = g_submits;
				f.flush();
				CHECK(g_submits == before + 1 && g_batches.back().n_reads == staged);
				staged = 0;
				refused++;
			}
			const int before = g_submits;
			f.feed(fed.back().data(), fed.back().size());
			CHECK(g_submits == before);
			staged++;
		}
		f.finish();
	}
	CHECK(refused >= 3 && g_empty_submits == 0);
	check_batches(fed);
}

static void case_growth(Mode mode)
{
	Case c("growth", mode);
	std::vector<std::string> fed;
	{
		Feeder f(c.opt, &c.ctx, 0, mode != CONTEXT);
		feed_all(f, fed, { 150, 10000, 10000, 150, 9000 });
		f.finish();
	}
	check_batches(fed);
	CHECK(g_opens == (std::vector<uint64_t> { 4096, grown(mode, 10000) }));
}

static void case_discard(Mode mode)
{
	Case c("discard", mode);
	std::vector<std::string> fed, dropped;
	{
		Feeder f(c.opt, &c.ctx, 0, mode != CONTEXT);
		feed_all(f, fed, { 150, 150 });
		f.flush();
		feed_all(f, dropped, { 150, 33, 150, 150, 150 });
		f.discard();
		feed_all(f, fed, { 7, 150 });
		f.finish();
	}
	check_batches(fed);
	CHECK(g_empty_submits == 0 && g_opens.size() == 1);
}

static void case_empty(Mode mode)
{
	Case c("empty", mode);
	std::vector<std::string> fed, dropped;
	{
		Feeder f(c.opt, &c.ctx, 0, mode != CONTEXT);
		feed_all(f, dropped, { 150, 150, 150 });
		f.discard();
		CHECK(!f.has_room(6000));
		feed_all(f, fed, { 6000, 150 });
		f.finish();
	}
	check_batches(fed);
	CHECK(g_empty_submits == 1 && g_opens == (std::vector<uint64_t> { 4096, grown(mode, 6000) }));
}

static void fill_chunk(PackedChunk &c, std::vector<std::string> &fed, const std::vector<uint64_t> &lens)
{
	uint64_t room = 0;
	for (uint64_t len : lens) room += len + 8;                           /* a read and its 1..8 invalid positions */
	c.reserve(room + 64);
	for (uint64_t len : lens) {
		fed.push_back(read_of(len));
		c.pos = ntsm::pack2_append(c.codes, c.valid, c.pos, fed.back().data(), len);
		c.n_bases += len;
		c.n_reads++;
	}
}

static void case_chunk(Mode mode)
{
	{
		Case c("chunk after own reads", mode);
		std::vector<std::string> fed, in_chunk;
		{
			Feeder f(c.opt, &c.ctx, 0, mode != CONTEXT);
			feed_all(f, fed, { 150, 31, 150 });
			PackedChunk ch;
			fill_chunk(ch, in_chunk, { 150, 0, 33, 150 });
			f.submitChunk(ch);
			if (mode == LANE_PACKED) {
				CHECK(g_batches.size() == 2 && g_batches[0].n_reads == 3 && g_batches[1].n_reads == 4);
				fed.insert(fed.end(), in_chunk.begin(), in_chunk.end());
			} else
				CHECK(g_submits == 0);                                   /* ignored: the early ingest feeds packed lanes only */
			feed_all(f, fed, { 150 });
			f.finish();
		}
		check_batches(fed);
		CHECK(g_empty_submits == 0 && g_opens.size() == 1);
	}
	if (mode != LANE_PACKED) return;
	{
		Case c("chunk into a held but empty slot", mode);
		std::vector<std::string> fed, dropped;
		{
			Feeder f(c.opt, &c.ctx, 0, true);
			feed_all(f, dropped, { 150, 150 });
			f.discard();
			PackedChunk ch;
			fill_chunk(ch, fed, { 150, 150, 7 });
			f.submitChunk(ch);
			f.finish();
		}
		check_batches(fed);
		CHECK(g_empty_submits == 1 && g_submits == 2 && g_opens.size() == 1);
	}
	{
		Case c("chunk larger than the slot", mode);
		std::vector<std::string> fed;
		{
			Feeder f(c.opt, &c.ctx, 0, true);
			PackedChunk ch;
			fill_chunk(ch, fed, { 9000 });
			const uint64_t need = (ch.pos + 31) & ~31ull;
			f.submitChunk(ch);
			CHECK(g_opens == (std::vector<uint64_t> { 4096, need + need / 2 }));
			feed_all(f, fed, { 150 });
			f.finish();
		}
		check_batches(fed);
	}
	{
		Case c("chunk without reads", mode);
		{
			Feeder f(c.opt, &c.ctx, 0, true);
			PackedChunk ch;
			ch.reserve(64);
			const size_t calls = g_trace.size();
			f.submitChunk(ch);
			CHECK(g_trace.size() == calls);
			f.finish();
		}
		CHECK(g_submits == 0);
	}
}

static void case_armed()
{
	const size_t start = g_trace.size();
	Case c("armed", CONTEXT);
	c.opt.verbose = 1;
	g_stop_at_sync = 3;
	std::vector<std::string> fed, late;
	{
		Feeder f(c.opt, &c.ctx, 5, false);
		while (!f.earlyTerm()) {
			CHECK(fed.size() < 1000);
			feed_all(f, fed, { 150 });
		}
		fed.pop_back();                                                  /* the read that found the stop: not staged */
		const size_t calls = g_trace.size();
		feed_all(f, late, std::vector<uint64_t>(60, 150));
		f.flush();
		f.finish();
		CHECK(g_trace.size() == calls && f.earlyTerm());
	}
	check_batches(fed);
	CHECK(g_submits == 3 && g_syncs == 3);
	for (size_t i = start; i < g_trace.size(); i++)
		if (g_trace[i].compare(0, 13, "submit_staged") == 0) CHECK(i + 1 < g_trace.size() && g_trace[i + 1].compare(0, 4, "sync") == 0);
}

static void case_finish(Mode mode)
{
	const int lane = mode != CONTEXT;
	{
		Case c("finish, then the destructor", mode);
		std::vector<std::string> fed;
		{
			Feeder f(c.opt, &c.ctx, 0, lane);
			feed_all(f, fed, { 150, 150 });
			f.finish();
			CHECK(g_closes == lane && g_submits == 1);
		}
		CHECK(g_closes == lane);
		check_batches(fed);
	}
	{
		Case c("the destructor alone", mode);
		std::vector<std::string> fed;
		{
			Feeder f(c.opt, &c.ctx, 0, lane);
			feed_all(f, fed, { 150, 150 });
			CHECK(g_closes == 0);
		}
		CHECK(g_closes == lane && g_submits == 0);
	}
}

int main(int argc, char **argv)
{
	for (Mode mode : { CONTEXT, LANE_BYTES, LANE_PACKED }) {
		case_order(mode);
		case_limit(mode);
		case_sink(mode);
		case_growth(mode);
		case_discard(mode);
		case_empty(mode);
		case_chunk(mode);
		case_finish(mode);
	}
	case_armed();
	if (argc > 1) {
		FILE *fh = fopen(argv[1], "w");
		if (!fh) return 1;
		for (const std::string &line : g_trace) fprintf(fh, "%s\n", line.c_str());
		fclose(fh);
	}
	printf("feeder check ok: %d cases\n", g_cases);
	return 0;
}
