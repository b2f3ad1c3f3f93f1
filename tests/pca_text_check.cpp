/*
 * pca_text_check.cpp -- test driver around the number text of ntsmPCA (tests/test_pca.py compiles it): every line of
 * stdin is converted as the program converts a cell (std::from_chars on the whole field) and printed as the program
 * prints a value (format_repr); "BAD" for a field the program would refuse.
 */
#define main ntsm_pca_main
#include "../ntsm_amd/csrc/host/ntsm_pca_main.cpp"
#undef main

int main()
{
	char line[256], out[64];
	while (fgets(line, sizeof line, stdin)) {
		size_t len = strlen(line);
		if (len && line[len - 1] == '\n') --len;
		double x = 0.0;
		const auto r = std::from_chars(line, line + len, x);
		if (r.ec != std::errc() || r.ptr != line + len || !std::isfinite(x)) { puts("BAD"); continue; }
		out[format_repr(x, out)] = 0;
		puts(out);
	}
	return 0;
}
