/*
 * pca_text.hpp -- the text side of the PCA that ntsmPCA (ntsm_pca_main.cpp) and `ntsmVCF --rotation` (ntsm_vcf_main.cpp)
 * share, so that the two routes cannot drift apart: how a matrix cell's text becomes a double, how the header line
 * becomes the sample names, what is refused and in which words, and how the rotation and the components are written.
 * Header only; the arithmetic is in libntsm_pca_hip.so (include/ntsm_pca_hip.h); on_threads comes from cli.hpp.
 */
#ifndef NTSM_PCA_TEXT_HPP
#define NTSM_PCA_TEXT_HPP

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/ntsm_pca_hip.h"
#include "cli.hpp"

namespace ntsm {

struct Name { const char *b; size_t len; };

/* [b, e) without the line's "\r" of a CRLF file */
inline const char *line_end(const char *b, const char *e) { return e > b && e[-1] == '\r' ? e - 1 : e; }

/* one cell of the matrix text: correctly rounded; no leading '+' or blanks; the whole field, and finite */
inline bool parse_cell(const char *b, const char *e, double &x)
{
	const auto r = std::from_chars(b, e, x);
	return r.ec == std::errc() && r.ptr == e && std::isfinite(x);
}

/* a row's centre as NAME_center.txt holds it, also the text of the row's undefined cells in NAME_matrix.tsv: the long double
 * quotient printed %.19Lg (printNormMatrix, MultiCount.hpp:148-201) */
inline std::string centre_text(double sum, uint32_t n_samples)
{
	char b[128];
	const long double sizeFloat = n_samples;
	const long double center = sum / sizeFloat;
	snprintf(b, sizeof b, "%.19Lg", center);
	return std::string(b);
}

/* The centre of a site of a cohort store from its tallies: n_half samples of genotype 0.5, n_one of
 * genotype 1 among the n_called that call the site.  n_one + 0.5 n_half is exact in a double; a site nobody calls is "0". */
inline std::string store_centre_text(uint32_t n_half, uint32_t n_one, uint32_t n_called)
{
	return n_called ? centre_text((double) n_one + 0.5 * (double) n_half, n_called) : std::string("0");
}

/* the value of that site's missing cells in the training matrix: what ntsmPCA would read back from the text */
inline double store_centre_value(uint32_t n_half, uint32_t n_one, uint32_t n_called)
{
	const std::string text = store_centre_text(n_half, n_one, n_called);
	double x = 0.0;
	(void) parse_cell(text.data(), text.data() + text.size(), x);                  /* %.19Lg of a quotient in [0, 1] always parses */
	return x;
}

/* the sample names of the header line [b, e) (no '\n'): alleleID <TAB> sample ... */
inline std::vector<Name> header_samples(const char *b, const char *e)
{
	std::vector<Name> samples;
	e = line_end(b, e);
	const char *t = (const char *) memchr(b, '\t', (size_t) (e - b));
	while (t) {
		const char *q = t + 1;
		t = (const char *) memchr(q, '\t', (size_t) (e - q));
		samples.push_back(Name { q, (size_t) ((t ? t : e) - q) });
	}
	return samples;
}

/* what is wrong with the shape of the matrix of `file` (samples from its header, p body lines), empty when nothing is */
inline std::string pca_shape_error(const std::string &file, size_t samples, uint64_t p)
{
	if (samples < 2) return "the header of " + file + " names " + std::to_string(samples) + " sample(s); a PCA needs at least 2";
	if (samples >= (1u << 24)) return "too many samples: " + std::to_string(samples);
	if (p == 0) return "the matrix file " + file + " has no sites (only a header)";
	if (p >= (1ull << 31)) return "too many sites: " + std::to_string(p);
	return std::string();
}

inline std::string pca_row_fields_error(uint64_t fields, uint32_t n)
{
	return "has " + std::to_string(fields) + " fields, the header has " + std::to_string(n + 1);
}

/* a refused line: k counts the body lines from 0 */
inline std::string pca_row_error(const std::string &file, uint64_t k, const Name &name, const std::string &what)
{
	return "line " + std::to_string(k + 2) + " of " + file + " (" + std::string(name.b, name.len) + "): " + what;
}

inline std::string pca_dims_low_error(long long d)
{
	return d < 1 ? "-n " + std::to_string(d) + ": the number of components must be at least 1" : std::string();
}

inline std::string pca_dims_high_error(long long d, uint32_t n, uint64_t p)
{
	if ((unsigned long long) d <= std::min<unsigned long long>(n, p)) return std::string();
	return "-n " + std::to_string(d) + " is more than min(samples, sites) = min(" + std::to_string(n) + ", " + std::to_string(p) + ")";
}

/* the message of a return code of ntsm_pca_run / ntsm_pca_run_cells, empty for 0 */
inline std::string pca_run_error(int rc, uint32_t bad, uint32_t d, int device)
{
	if (rc == 0) return std::string();
	if (rc == NTSM_PCA_E_SOLVER_MISSING) return "rocSOLVER cannot be loaded (librocsolver.so.0, librocsolver.so): the eigen step needs it";
	if (rc == NTSM_PCA_E_RANK)
		return "component " + std::to_string(bad) + " of the " + std::to_string(d) + " requested has no positive eigenvalue beyond rounding "
		    "(the centred matrix has rank " + std::to_string(bad) + " numerically): ask for fewer components";
	if (rc == NTSM_PCA_E_SOLVER) return "the eigen step failed (rocSOLVER dsyevd)";
	return "the device step failed (" + std::to_string(rc) + ") on HIP device " + std::to_string(device);
}

/* the device line of -v */
inline void pca_print_times(FILE *f, const ntsm_pca_times &tm, const double *expand_ms)
{
	fprintf(f, "[pca] device: upload %.3f ms, ", tm.upload_ms);
	if (expand_ms) fprintf(f, "expand %.3f ms, ", *expand_ms);
	fprintf(f, "centre %.3f ms, gram %.3f ms (%u tiles x %u pieces, %.3f TFLOP/s), eigen %.3f ms, "
	    "projection %.3f ms, download %.3f ms\n", tm.centre_ms, tm.gram_ms, tm.gram_tiles, tm.gram_split,
	    tm.gram_ms > 0 ? (double) tm.gram_flops / tm.gram_ms * 1e-9 : 0.0, tm.eigen_ms, tm.project_ms, tm.download_ms);
}

/* x as Python's repr writes it (pandas' to_csv): the shortest digits that read back to x; exponent form when the decimal
 * exponent is below -4 or at least 16, the exponent with a sign and at least two digits; "1.0", not "1" */
inline size_t format_repr(double x, char *out)
{
	char *o = out;
	if (std::signbit(x)) { *o++ = '-'; x = -x; }
	if (x == 0.0) { memcpy(o, "0.0", 3); return (size_t) (o + 3 - out); }
	char buf[40], dig[24];
	const auto r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::scientific);   /* d[.ddd]e[+-]XX, shortest */
	const char *ep = (const char *) memchr(buf, 'e', (size_t) (r.ptr - buf));
	int nd = 0;
	for (const char *q = buf; q < ep; ++q) if (*q != '.') dig[nd++] = *q;
	const int e10 = atoi(std::string(ep + 1, (const char *) r.ptr).c_str());
	if (e10 >= -4 && e10 < 16) {
		if (e10 >= 0) {
			for (int i = 0; i <= e10; ++i) *o++ = i < nd ? dig[i] : '0';
			*o++ = '.';
			if (nd > e10 + 1) for (int i = e10 + 1; i < nd; ++i) *o++ = dig[i];
			else *o++ = '0';
		} else {
			*o++ = '0';
			*o++ = '.';
			for (int i = 0; i < -e10 - 1; ++i) *o++ = '0';
			for (int i = 0; i < nd; ++i) *o++ = dig[i];
		}
	} else {
		*o++ = dig[0];
		if (nd > 1) { *o++ = '.'; for (int i = 1; i < nd; ++i) *o++ = dig[i]; }
		*o++ = 'e';
		*o++ = e10 < 0 ? '-' : '+';
		o += snprintf(o, 8, "%02d", std::abs(e10));
	}
	return (size_t) (o - out);
}

/* header + one line per name with d values, formatted on T threads in row order */
inline bool write_table(const std::string &path, const char *corner, const std::vector<Name> &names, const double *val, uint32_t d, unsigned T)
{
	const size_t rows = names.size();
	std::vector<std::string> part(T);
	on_threads(T, [&](unsigned t) {
		const size_t lo = rows * t / T, hi = rows * (t + 1) / T;
		std::string &s = part[t];
		char num[48];
		for (size_t k = lo; k < hi; ++k) {
			s.append(names[k].b, names[k].len);
			for (uint32_t i = 0; i < d; ++i) {
				s.push_back('\t');
				s.append(num, format_repr(val[k * d + i], num));
			}
			s.push_back('\n');
		}
	});
	FILE *f = fopen(path.c_str(), "wb");
	if (!f) return false;
	std::string head(corner);
	for (uint32_t i = 0; i < d; ++i) head += "\t" + std::to_string(i);
	head += "\n";
	bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
	for (const std::string &s : part) ok = ok && fwrite(s.data(), 1, s.size(), f) == s.size();
	return (fclose(f) == 0) && ok;
}

/* both outputs of a PCA; the name of the file that could not be written, empty when both were */
inline std::string write_pca_tables(const std::string &prefix, const std::vector<Name> &sites, const std::vector<Name> &samples,
		const double *rot, const double *comp, uint32_t d, unsigned T)
{
	const std::string rot_path = prefix + "_rotationalMatrix.tsv", comp_path = prefix + "_components.tsv";
	if (!write_table(rot_path, "AlleleID", sites, rot, d, T)) return rot_path;
	if (!write_table(comp_path, "SampleID", samples, comp, d, T)) return comp_path;
	return std::string();
}

}  // namespace ntsm

#endif
