/*
 * eval_qc.hpp -- the text of the per-site table of ntsmEval --qc --sites-out.  Header only, host
 * only, no HIP: the integers are the device's (include/ntsm_eval_hip.h: ntsm_eval_store_profile), the doubles are formed here
 * from them, each in one stated expression and printed with std::to_string, so that a model can reproduce the bytes.
 *
 *   #locusID called miss homAT homCG het freqAT hetObs hetExp meanCov      (tabs between the fields)
 *   called  = homAT + homCG + het
 *   freqAT  = double(2 * homAT + het) / double(2 * called)
 *   hetObs  = double(het) / double(called)
 *   hetExp  = 2 * p * (1 - p), p = freqAT
 *   meanCov = double(site_cov) / double(n_samples)
 * freqAT, hetObs and hetExp read NA where called == 0.
 */
#ifndef NTSM_EVAL_QC_HPP
#define NTSM_EVAL_QC_HPP

#include <cstdint>
#include <string>

namespace ntsm {
namespace eval_qc {

constexpr const char *kSiteHeader = "#locusID\tcalled\tmiss\thomAT\thomCG\thet\tfreqAT\thetObs\thetExp\tmeanCov\n";

/* one line of the table, appended to out; tally = homAT, homCG, het, miss of the site */
inline void site_line(std::string &out, const char *locus, const uint32_t tally[4], uint64_t site_cov, uint64_t n_samples)
{
	const uint64_t homAT = tally[0], homCG = tally[1], het = tally[2], miss = tally[3];
	const uint64_t called = homAT + homCG + het;
	out += locus; out += "\t"; out += std::to_string(called); out += "\t"; out += std::to_string(miss);
	out += "\t"; out += std::to_string(homAT); out += "\t"; out += std::to_string(homCG); out += "\t"; out += std::to_string(het);
	if (called == 0) out += "\tNA\tNA\tNA";
	else {
		const double p = double(2 * homAT + het) / double(2 * called);
		const double hetObs = double(het) / double(called);
		const double hetExp = 2 * p * (1 - p);
		out += "\t"; out += std::to_string(p); out += "\t"; out += std::to_string(hetObs); out += "\t"; out += std::to_string(hetExp);
	}
	out += "\t"; out += std::to_string(double(site_cov) / double(n_samples)); out += "\n";
}

}  // namespace eval_qc
}  // namespace ntsm

#endif
