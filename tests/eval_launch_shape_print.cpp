/*
 * eval_launch_shape_print.cpp -- what ntsm_eval_chunk.h's launch rule answers without forced values, for
 * tests/test_eval_many_samples.py: the arguments are pairs "rows columns"; one line "width group" per pair.  No device is touched.
 */
#define NTSM_HIP_TAG "eval_launch_shape_print"
#include "../ntsm_amd/csrc/ntsm_eval_chunk.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
	for (int i = 1; i + 1 < argc; i += 2) {
		uint32_t width = 0, group = 0;
		ntsm_eval_chunk::launch_shape((uint32_t) strtoul(argv[i], nullptr, 10), (uint32_t) strtoul(argv[i + 1], nullptr, 10), 0, 0, width, group);
		printf("%u %u\n", width, group);
	}
	return 0;
}
