/*
 * pca_store_text_check.cpp -- the centre of a cohort store's site as ntsmPCA --store writes it and as it reads back
 * (host/pca_text.hpp: store_centre_text, store_centre_value), for tests/test_pca_store.py.
 * stdin: lines "n_half n_one n_called".  stdout: per line the text, a tab, and the value it reads back as (%.17g).
 */
#include <cstdio>

#include "../ntsm_amd/csrc/host/pca_text.hpp"

int main()
{
	unsigned h, o, c;
	while (scanf("%u %u %u", &h, &o, &c) == 3)
		printf("%s\t%.17g\n", ntsm::store_centre_text(h, o, c).c_str(), ntsm::store_centre_value(h, o, c));
	return 0;
}
