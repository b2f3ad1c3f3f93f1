/*
 * cli.hpp -- what the host programs of the cohort tools (ntsm_vcf_main.cpp, ntsm_pca_main.cpp, ntsm_eval_main.cpp) share,
 * each stated once: the refusal, the two ways a flag's value is read, the thread-count rule, the thread fan-out, the
 * lap timer, the input file as bytes and the cut of a byte range into line-aligned ranges.  Header only, no HIP.  FileBytes
 * is why gz_stream.hpp comes along; a program that never loads a file (ntsmEval) instantiates nothing of it.
 */
#ifndef NTSM_CLI_HPP
#define NTSM_CLI_HPP

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "gz_stream.hpp"

namespace ntsm {

[[noreturn]] inline void refuse(const std::string &msg)     /* an input this build does not take: exit status 1 */
{
	std::cerr << "Error: " << msg << std::endl;
	exit(EXIT_FAILURE);
}

/* A flag's value, in the two strictnesses the programs have.  read_prefix: the stream extracts a value (the reference's
 * flags: -k 1x is 1).  read_whole: and nothing follows it (ntsmPCA's flags and ntsmVCF's -n). */
template <typename T> bool read_prefix(const char *s, T &out) { std::stringstream c(s); return bool(c >> out); }
template <typename T> bool read_whole(const char *s, T &out) { std::stringstream c(s); return bool(c >> out) && c.eof(); }
inline void print_invalid_parameter(char flag, const char *value) { std::cerr << "Error - Invalid parameter " << flag << ": " << value << std::endl; }

/* the reference's flags (src/ntSeqMatchVCF.cpp:90-150, src/ntSeqMatchEval.cpp): a bad value prints its line, status 0 */
template <typename T> void reference_flag(char flag, const char *value, T &out)
{
	if (!read_prefix(value, out)) { print_invalid_parameter(flag, value); exit(EXIT_SUCCESS); }
}

/* this build's own flags: a value that does not read whole prints the same line and sets `die` (try_help_if, status 1) */
template <typename T> void whole_flag(char flag, const char *value, T &out, bool &die)
{
	if (!read_whole(value, out)) { print_invalid_parameter(flag, value); die = true; }
}

[[noreturn]] inline void print_version(const char *program, const char *what)   /* --version: two lines on stderr, status 0 */
{
	std::cerr << program << " (ntsm-mi355x)\n" << what << "\n" << std::endl;
	exit(EXIT_SUCCESS);
}

/* the end of the flag checks that are reported together */
inline void try_help_if(bool die) { if (die) { std::cerr << "Try '--help' for more information.\n"; exit(EXIT_FAILURE); } }

inline unsigned thread_count(unsigned requested)            /* -t: 0 asks for the machine's threads, at most 64; at most 256 when given */
{
	return requested ? std::min(requested, 256u) : std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
}

template <class F> void on_threads(unsigned n, F f)         /* f(0) ... f(n - 1), f(0) on the calling thread; returns when all have */
{
	std::vector<std::thread> pool;
	for (unsigned t = 1; t < n; ++t) pool.emplace_back(f, t);
	f(0u);
	for (auto &th : pool) th.join();
}

/* phase times on stderr, "<tag> <what>: %.4f s" (tools/vcf_bench.py and tools/pca_bench.py read these lines) */
struct LapTimer {
	const char *tag;
	bool on;
	std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now(), last = start;
	void lap(const char *what)
	{
		const auto t = std::chrono::steady_clock::now();
		if (on) fprintf(stderr, "%s %s: %.4f s\n", tag, what, std::chrono::duration<double>(t - last).count());
		last = t;
	}
	double total() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count(); }
};

/* An input file as bytes: a plain file is mapped, gzip / BGZF is decoded on `threads` decoders, anything else is read
 * through.  A directory reads as nothing; the caller says whether that is an empty input or a file that cannot be read. */
struct FileBytes {
	enum Directory { kDirectoryIsEmpty, kDirectoryIsUnreadable };
	const char *data = nullptr;
	size_t size = 0;
	std::vector<char> owned;
	void *map = nullptr;
	~FileBytes() { if (map) munmap(map, size); }
	bool load(const std::string &path, unsigned threads, Directory directory)
	{
		if (GzStream::is_gzip(path)) {
			GzStream::set_decoder_threads(threads);
			GzStream gz;
			if (!gz.open(path)) return false;
			std::vector<char> buf(1 << 22);
			for (int n; (n = gz.read(buf.data(), (unsigned) buf.size())) != 0;) {
				if (n < 0) return false;
				owned.insert(owned.end(), buf.data(), buf.data() + n);
			}
		} else {
			const int fd = open(path.c_str(), O_RDONLY);
			if (fd < 0) return false;
			struct stat st;
			if (fstat(fd, &st) != 0 || (directory == kDirectoryIsUnreadable && S_ISDIR(st.st_mode))) { close(fd); return false; }
			if (S_ISREG(st.st_mode) && st.st_size > 0) {
				size = (size_t) st.st_size;
				map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
				close(fd);
				if (map == MAP_FAILED) { map = nullptr; return false; }
				data = (const char *) map;
				return true;
			}
			std::vector<char> buf(1 << 20);
			for (ssize_t n; (n = read(fd, buf.data(), buf.size())) > 0;) owned.insert(owned.end(), buf.data(), buf.data() + n);
			close(fd);
		}
		data = owned.data();
		size = owned.size();
		return true;
	}
};

/* [begin, end) cut into T ranges [at[t], at[t + 1]) that start at line starts, and lines_before[t], the number of lines
 * in [begin, at[t]) (lines_before[T]: all of them).  A last line without '\n' is a line; ranges past the last line are
 * empty.  The lines are counted on T threads. */
struct LineCuts { std::vector<const char *> at; std::vector<uint64_t> lines_before; };
inline LineCuts cut_lines(const char *begin, const char *end, unsigned T)
{
	LineCuts c { std::vector<const char *>(T + 1, end), std::vector<uint64_t>(T + 1, 0) };
	c.at[0] = begin;
	for (unsigned t = 1; t < T; ++t) {
		const char *q = std::max(c.at[t - 1], begin + (size_t) (end - begin) / T * t);
		if (q > begin && q < end && q[-1] != '\n') {
			const char *nl = (const char *) memchr(q, '\n', (size_t) (end - q));
			q = nl ? nl + 1 : end;
		}
		c.at[t] = q;
	}
	on_threads(T, [&](unsigned t) {
		const char *a = c.at[t], *b = c.at[t + 1];
		c.lines_before[t + 1] = (uint64_t) std::count(a, b, '\n') + (b > a && b[-1] != '\n' ? 1 : 0);
	});
	for (unsigned t = 0; t < T; ++t) c.lines_before[t + 1] += c.lines_before[t];
	return c;
}

}  // namespace ntsm

#endif
