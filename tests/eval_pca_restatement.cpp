// tests/eval_pca_restatement.cpp -- TEST INFRASTRUCTURE: an independent CPU restatement of ntsmEval's PCA-guided search,
// written from the reference text (src/CompareCounts.hpp:116-211 projectPCs, :285-398 computeScorePCA, :926-932
// calcDistance; vendor/nanoflann.hpp:452-486 L2_Adaptor::evalMetric, :305-307 RadiusResultSet::addPoint).  It pins the HIP path
// (include/ntsm_eval_hip.h) against the same statement of the arithmetic, and is itself held to the unmodified reference
// class (oracle/_ref/ref_ntsmEval -p -n, tests/test_eval_reference.py).  Built by tests/test_eval_pca.py with g++ -O2 -std=c++11 -ffp-contract=off on x86-64, so
// long double is the x87 format, as in the reference's build.
//
//   project COUNTS.bin N M MIN_COV NORM.txt ROT.tsv DIM CLOUD.out NORM.out ROT.out
//       counts: uint32 [N][M][2]; writes the cloud (double [N][DIM]) and the parsed values as raw long double
//       (NORM.out [M], ROT.out [DIM][M]) so that a test can hand the library the very same numbers
//   candidates CLOUD.bin N DIM RADIUS.bin OUT.txt
//       radius: double [N]; writes "i<TAB>k<TAB>calcDistance as %a" per pair, in the one-thread print order; exact ties in
//       evalMetric are ordered by ascending k (the reference's order among ties is that of its kd-tree leaves)
#include <cfloat>
#include <limits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <utility>
#include <vector>
#include <algorithm>

using namespace std;

template <typename T> static vector<T> readBin(const char *path, size_t count)
{
	vector<T> v(count);
	FILE *f = fopen(path, "rb");
	if (!f || fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
	fclose(f);
	return v;
}

template <typename T> static void writeBin(const char *path, const vector<T> &v)
{
	FILE *f = fopen(path, "wb");
	if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
	fclose(f);
}

static int project(char **a)
{
	const unsigned n = (unsigned) atol(a[1]), m = (unsigned) atol(a[2]), minCov = (unsigned) atol(a[3]);
	const vector<uint32_t> counts = readBin<uint32_t>(a[0], (size_t) n * m * 2);
	const unsigned dim = (unsigned) atol(a[6]);
	// load in normalization values (:120-134)
	vector<long double> normVals;
	{
		ifstream fh(a[4]);
		string line;
		if (fh.is_open()) {
			while (getline(fh, line)) {
				stringstream ss(line);
				long double value;
				ss >> value;
				normVals.emplace_back(value);
			}
		}
	}
	// rotational components (:136-165)
	unsigned compNum = 0;
	ifstream fh(a[5]);
	string line;
	getline(fh, line);
	{
		stringstream ss(line);
		string val;
		ss >> val;
		while (ss >> val) ++compNum;
	}
	if (dim > compNum) { fprintf(stderr, "dim > compNum\n"); return 3; }
	vector<vector<long double>> rotVals(compNum, vector<long double>(normVals.size(), 0.0));
	unsigned index = 0;
	while (getline(fh, line)) {
		stringstream ss(line);
		string rsID;
		ss >> rsID;
		if (index >= normVals.size()) { fprintf(stderr, "more rows than norm values\n"); return 3; }
		for (unsigned i = 0; i < compNum; ++i) ss >> rotVals[i][index];
		++index;
	}
	if (index != normVals.size() || normVals.size() < m) { fprintf(stderr, "row / value count\n"); return 3; }
	// projection (:166-211)
	vector<double> cloud((size_t) n * dim);
	for (unsigned i = 0; i < n; ++i) {
		vector<double> vals(m, 0.0);
		for (unsigned j = 0; j < m; ++j) {
			const unsigned first = counts[((size_t) i * m + j) * 2], second = counts[((size_t) i * m + j) * 2 + 1];
			unsigned countAT = 0, countCG = 0;
			if (first > minCov) countAT = first;
			if (second > minCov) countCG = second;
			unsigned denom = countAT + countCG;
			if (denom == 0) {
				vals[j] = 0.0;
			} else {
				double nonNormGeno = double(countAT) / double(denom);
				vals[j] = ((nonNormGeno - 0.25) < 0.0 ? 0.0 : (nonNormGeno - 0.75) < 0.0 ? 0.5 : 1.0) - normVals[j];
			}
		}
		for (unsigned d = 0; d < dim; ++d)
			cloud[(size_t) i * dim + d] = inner_product(vals.begin(), vals.end(), rotVals.at(d).begin(), 0.0);
	}
	writeBin(a[7], cloud);
	vector<long double> nOut(normVals.begin(), normVals.begin() + m), rOut;
	for (unsigned d = 0; d < dim; ++d) rOut.insert(rOut.end(), rotVals[d].begin(), rotVals[d].begin() + m);
	writeBin(a[8], nOut);
	writeBin(a[9], rOut);
	return 0;
}

// nanoflann L2_Adaptor::evalMetric with the point b as data row
static double evalMetric(const double *a, const double *b, size_t size)
{
	double result = double();
	const double *last = a + size;
	const double *lastgroup = last - 3;
	size_t d = 0;
	while (a < lastgroup) {
		const double diff0 = a[0] - b[d++];
		const double diff1 = a[1] - b[d++];
		const double diff2 = a[2] - b[d++];
		const double diff3 = a[3] - b[d++];
		result += diff0 * diff0 + diff1 * diff1 + diff2 * diff2 + diff3 * diff3;
		a += 4;
	}
	while (a < last) {
		const double diff0 = *a++ - b[d++];
		result += diff0 * diff0;
	}
	return result;
}

static double calcDistance(const double *p1, const double *p2, unsigned dim)
{
	double dist = 0.0;
	for (unsigned i = 0; i < dim; ++i) dist += (p1[i] < p2[i] ? p2[i] - p1[i] : p1[i] - p2[i]) * (p1[i] < p2[i] ? p2[i] - p1[i] : p1[i] - p2[i]);
	return dist;
}

static int candidates(char **a)
{
	const unsigned n = (unsigned) atol(a[1]), dim = (unsigned) atol(a[2]);
	const vector<double> cloud = readBin<double>(a[0], (size_t) n * dim), radius = readBin<double>(a[3], n);
	FILE *out = fopen(a[4], "w");
	if (!out) return 2;
	const double MAXD = numeric_limits<double>::max();
	for (unsigned i = 0; i < n; ++i) {
		const double *pi = &cloud[(size_t) i * dim];
		if (radius[i] < MAXD) {
			vector<pair<size_t, double>> matches;                      // radiusSearch: every point with dist < radius
			for (unsigned k = 0; k < n; ++k) {
				const double dist = evalMetric(pi, &cloud[(size_t) k * dim], dim);
				if (dist < radius[i]) matches.emplace_back(k, dist);
			}
			stable_sort(matches.begin(), matches.end(), [](const pair<size_t, double> &x, const pair<size_t, double> &y) { return x.second < y.second; });
			for (size_t j = 0; j < matches.size(); ++j) {
				const unsigned k = (unsigned) matches[j].first;
				if (radius[i] == radius[k]) {
					if (k <= i) continue;
				} else if (radius[i] < radius[k]) {
					continue;
				}
				fprintf(out, "%u\t%u\t%a\n", i, k, calcDistance(pi, &cloud[(size_t) k * dim], dim));
			}
		} else {
			for (unsigned j = 0; j < n; ++j) {
				if (MAXD == radius[j] && j <= i) continue;
				fprintf(out, "%u\t%u\t%a\n", i, j, calcDistance(pi, &cloud[(size_t) j * dim], dim));
			}
		}
	}
	fclose(out);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 12 && string(argv[1]) == "project") return project(argv + 2);
	if (argc == 7 && string(argv[1]) == "candidates") return candidates(argv + 2);
	fprintf(stderr, "usage: see the file header\n");
	return 2;
}
