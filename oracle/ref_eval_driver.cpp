/*
 * oracle/ref_eval_driver.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
 *
 * Thin driver around the UNMODIFIED reference scoring class of ntsmEval.  It #includes the reference's header-only
 * CompareCounts class where it lies under /root/reference (nothing is copied into this repo), in the include order of
 * src/ntSeqMatchEval.cpp:6-19, and replays what the reference main does between its option loop and its exit
 * (src/ntSeqMatchEval.cpp:276-341):
 *
 *     omp_set_num_threads(opt::threads);                                   :276-279
 *     CompareCounts comp(inputFiles);                                      :285-304 (every file must exist: assert)
 *     one file   -> comp.computeScoreSingle();                             :305-310
 *     more files -> -o: nothing (needs -e)                                 :315-323
 *                   no -p: comp.computeScore();                            :325-328
 *                   -p:    comp.projectPCs(); comp.computeScorePCA();      :329-336
 *                   -e:    comp.mergeCounts();                             :338-340
 *
 * Why a driver instead of the reference's own main: src/ntSeqMatchEval.cpp takes PACKAGE_NAME and GIT_REVISION for --version
 * from the autoconf-generated config.h; autotools is not in this image and we do not write stand-ins for generated values, so
 * main() itself stays unbuilt and its option loop (:103-274) is followed by reading.  The class does build: its only tie to
 * config.h is the #include in vendor/kfunc.c:28, which uses nothing from it, so the empty oracle/ref_config/config.h on the
 * include path is enough and every instruction of the scoring comes from the reference's own text.
 *
 * Flags accepted here are the subset of the reference CLI that reaches the class, with the reference's meaning and its way of
 * reading a value (`stringstream >> opt::X`; on failure "Error - Invalid parameter X: VALUE" and return 0):
 *   -t INT  -s FLOAT  -a  -w FLOAT  -c INT  -g INT  -e FILE  -o  -p FILE  -n FILE  -d INT  -r FLOAT  -1 FLOAT  -2 FLOAT
 *   -S FLOAT  -l FLOAT  -v
 * stdout, stderr and the -e file are the class's own.  The reference prints its lines in another order with more than one
 * thread; comparisons run it with -t 1.
 */
#include <sstream>
#include <string>
#include <vector>
#include <fstream>
#include <iostream>
#include <stdlib.h>
#include <limits.h>
#include <assert.h>
#include <getopt.h>
#include "src/Options.h"
#include "src/Util.h"
#include "src/CompareCounts.hpp"

#include <omp.h>

template <typename T> static bool value(char flag, const char *text, T &into)
{
	std::stringstream convert(text);
	if (convert >> into) return true;
	std::cerr << "Error - Invalid parameter " << flag << ": " << text << std::endl;
	return false;
}

int main(int argc, char **argv)
{
	bool die = false;
	int c;
	while ((c = getopt(argc, argv, "t:vs:c:aw:g:p:n:d:r:e:o1:2:S:l:")) != -1) {
		bool ok = true;
		switch (c) {
		case 'a': opt::all = true; break;
		case 'o': opt::onlyMerge = true; break;
		case 'v': opt::verbose++; break;
		case 't': ok = value('t', optarg, opt::threads); break;
		case 's': ok = value('s', optarg, opt::scoreThresh); break;
		case 'w': ok = value('w', optarg, opt::covSkew); break;
		case 'c': ok = value('c', optarg, opt::minCov); break;
		case 'g': ok = value('g', optarg, opt::genomeSize); break;
		case 'e': ok = value('e', optarg, opt::merge); break;
		case 'p': ok = value('p', optarg, opt::pca); break;
		case 'n': ok = value('n', optarg, opt::norm); break;
		case 'd': ok = value('d', optarg, opt::dim); break;
		case 'r': ok = value('r', optarg, opt::pcErrorThresh); break;
		case '1': ok = value('1', optarg, opt::pcMissSite1); break;
		case '2': ok = value('2', optarg, opt::pcMissSite2); break;
		case 'S': ok = value('S', optarg, opt::pcSearchRadius1); break;
		case 'l': ok = value('l', optarg, opt::pcSearchRadius2); break;
		default: die = true; break;
		}
		if (!ok) return 0;
	}
	if (opt::threads > 0) omp_set_num_threads(opt::threads);         /* ntSeqMatchEval.cpp:276-279 */

	std::vector<std::string> inputFiles;                             /* :285-290 */
	for (; optind < argc; ++optind) {
		inputFiles.emplace_back(argv[optind]);
		assert(Util::fexists(inputFiles.back()));
	}
	if (inputFiles.size() == 0) {                                    /* :293-300 */
		std::cerr << "Error: Need Input File" << std::endl;
		die = true;
	}
	if (die) {
		std::cerr << "usage: ref_ntsmEval [-t T] [-s S] [-a] [-w W] [-c C] [-g G] [-e FILE [-o]] [-p ROT -n NORM [-d D] [-r R] "
		             "[-1 M1] [-2 M2] [-S R1] [-l R2]] counts..." << std::endl;
		return EXIT_FAILURE;
	}

	CompareCounts comp(inputFiles);                                  /* :304 */
	if (inputFiles.size() == 1) {
		comp.computeScoreSingle();                                   /* :309 */
		return 0;
	}
	if (opt::onlyMerge) {                                            /* :315-323 */
		if (opt::merge.empty()) {
			std::cerr << "(-l) cannot be used without --merge (-e) option." << std::endl;
			return EXIT_FAILURE;
		}
	} else if (opt::pca.empty()) {
		comp.computeScore();                                         /* :327 */
	} else {
		if (!Util::fexists(opt::norm))                               /* :330-333: said, then the class's own assert ends the run */
			std::cerr << "Error: Need normalization file" << std::endl;
		comp.projectPCs();                                           /* :334 */
		comp.computeScorePCA();                                      /* :335 */
	}
	if (!opt::merge.empty()) comp.mergeCounts();                     /* :339 */
	return 0;
}
