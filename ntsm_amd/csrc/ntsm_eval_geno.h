/*
 * ntsm_eval_geno.h -- the genotype rule of the bit-plane runs, stated once for ntsm_eval_trio.hip (--trios: bits along the sites)
 * and ntsm_eval_ld.hip (--ld: bits along the samples).  The text of the rule is include/ntsm_eval_hip.h's ("The genotype rule of
 * this run"): c = min_cov with strict >, D = min_depth gating the homozygotes only, t in 64 bits.  Internal: not part of include/.
 */
#ifndef NTSM_EVAL_GENO_H
#define NTSM_EVAL_GENO_H

#include <hip/hip_runtime.h>

#include <cstdint>

/* the class of a cell (a, g) = (countAT, countCG): 0 homAT, 1 het, 2 homCG, 3 miss */
__device__ __host__ inline int ntsm_eval_class_of(uint32_t a, uint32_t g, uint32_t min_cov, uint32_t min_depth)
{
	const bool A = a > min_cov, G = g > min_cov;
	if (A && G) return 1;
	if (A == G || (uint64_t) a + (uint64_t) g < min_depth) return 3;
	return A ? 0 : 2;
}

#endif
