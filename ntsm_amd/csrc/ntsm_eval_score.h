/*
 * ntsm_eval_score.h -- the scoring step of ntsmEval on the device, stated once (reference: src/CompareCounts.hpp:591-624
 * computeScore and the functions it calls).  ntsm_eval.hip (all pairs, counts transposed to [site][sample]) and
 * ntsm_eval_pca.hip (listed pairs, counts as [sample][site][2]) differ in how they reach the counts of a pair at a site;
 * what they do with them is here, so the records of the two paths are bit-identical by construction.
 * Arithmetic: IEEE double, __dadd_rn / __dmul_rn / __ddiv_rn (no fused multiply-add): the reference binary is built
 * without FMA contraction on x86-64 and every sum is sequential over the sites.
 */
#ifndef NTSM_EVAL_SCORE_H
#define NTSM_EVAL_SCORE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ntsm_eval_hip.h"

/* the single-sample term of a (sample, site), first * freqAT + second * freqCG (computeSumLogPSingle, :971-987): it does not
 * depend on the partner, so it is computed once per cell and a pair only adds it where the site is valid for the pair */
__device__ inline double ntsm_eval_term(uint32_t a0, uint32_t a1, uint32_t min_cov)
{
	double fAT = 0, fCG = 0;
	if (a0 > min_cov) fAT = __ddiv_rn((double) a0, (double) (a0 + a1));
	if (a1 > min_cov) fCG = __ddiv_rn((double) a1, (double) (a0 + a1));
	return __dadd_rn(__dmul_rn((double) a0, fAT), __dmul_rn((double) a1, fCG));
}

/* one sample at one site: its counts, its term and what the pair update asks of it alone (a kernel that holds one sample
 * against several partners forms this once) */
struct ntsm_eval_side {
	uint32_t at, cg;
	double term;
	bool valid, het, has_at;                 /* has_at: for a homozygous site, which allele */
};

__device__ inline ntsm_eval_side ntsm_eval_side_of(uint32_t at, uint32_t cg, double term, uint32_t min_cov)
{
	return ntsm_eval_side { at, cg, term, at > min_cov || cg > min_cov, at > min_cov && cg > min_cov, at > min_cov };
}

struct ntsm_eval_acc {
	double joint = 0, s1 = 0, s2 = 0;
	uint32_t n = 0, hets1 = 0, homs1 = 0, hets2 = 0, homs2 = 0, sh_het = 0, sh_hom = 0, ibs0 = 0;

	/* one site of the pair (sample 1 = i, sample 2 = j), in site order */
	__device__ inline void add(const ntsm_eval_side &i, const ntsm_eval_side &j, uint32_t min_cov)
	{
		if (!(i.valid && j.valid)) return;                                      /* gatherValidEntries, :1057-1078 */
		n++;
		/* computeSumLogPJoint, :1018-1031 */
		const uint32_t cAT = i.at + j.at, cCG = i.cg + j.cg;
		const double den = (double) (cAT + cCG);
		double fAT = 0, fCG = 0;
		if (cAT > min_cov) fAT = __ddiv_rn((double) cAT, den);
		if (cCG > min_cov) fCG = __ddiv_rn((double) cCG, den);
		joint = __dadd_rn(joint, __dadd_rn(__dmul_rn((double) cAT, fAT), __dmul_rn((double) cCG, fCG)));
		s1 = __dadd_rn(s1, i.term);
		s2 = __dadd_rn(s2, j.term);
		/* calcRelatedness, :1151-1188 */
		hets1 += i.het; homs1 += !i.het;
		hets2 += j.het; homs2 += !j.het;
		if (i.het && j.het) sh_het++;
		else if (!i.het && !j.het) { if (i.has_at == j.has_at) sh_hom++; else ibs0++; }
	}

	__device__ inline ntsm_eval_record record() const
	{
		ntsm_eval_record r;
		r.sum_joint = joint; r.sum_single1 = s1; r.sum_single2 = s2;
		r.n_valid = n;
		r.hets1 = hets1; r.homs1 = homs1; r.hets2 = hets2; r.homs2 = homs2;
		r.shared_hets = sh_het; r.shared_homs = sh_hom; r.ibs0 = ibs0; r.ibs2 = sh_het + sh_hom;
		return r;
	}
};

#endif
