# Top-level build.  `make all` = everything __graft_entry__.build() needs:
#   ntsm_amd/libntsm_hip.so   HIP kernels + C ABI (include/ntsm_hip.h), gfx950: csrc/kernels_*.hip + tables / runtime / rccl_bind / capi .cpp
#   ntsm_amd/libntsm_synth.so synthetic workload generator (host + device fills)
#   build/ntsmCount           host CLI (C++), links libntsm_hip.so
#   build/ntsm_synth          generator CLI
#   build/ntsm_host_test      host-logic test driver (no GPU calls)
#   ntsm_amd/libntsm_eval_hip.so, build/ntsmEval   all-pairs scoring of ntsmEval (HIP library + CLI mirror), its PCA-guided
#                                                  search, queries against a cohort store (--pack / --against) and the
#                                                  PCA-guided search against one (--index / --near), and both runs over
#                                                  the store's own samples (--within / --within-near), and one store
#                                                  against another (--between) and the PCA-guided search between
#                                                  two (--between-near), and the QC tables of a store (--qc), and the
#                                                  cross-sample contamination check over one (--contam), and the
#                                                  parent-parent-child trios in one (--trios), and the site-pair LD
#                                                  and prune over one (--ld)
#   ntsm_amd/libntsm_vcf_hip.so, build/ntsmVCF     multi-sample VCF to PCA matrix + centre file (HIP library + CLI mirror);
#                                                  with --rotation also the PCA, through libntsm_pca_hip.so
#                                                  with --counts / --store the genotypes as counts files and cohort-store records
#   ntsm_amd/libntsm_pca_hip.so, build/ntsmPCA     exact PCA of the ntsmVCF matrix: rotation for ntsmEval -p (HIP library + CLI)
#   ntsm_amd/libntsm_sitegen_hip.so, build/ntsmSiteGen   sites files from a genome and a VCF of SNPs (HIP library + CLI)
#   ntsm_amd/libntsm_sitegen_gap_hip.so                  the device step of `ntsmSiteGen -g`: one-base gapped places as well
#   oracle/                   CPU checker (+ oracle/_ref when /root/reference is present)
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
ARCH     ?= gfx950
CXXFLAGS ?= -O3 -std=c++17 -Wall -Wextra -fPIC
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wextra -Wno-unused-parameter
CSRC     := ntsm_amd/csrc

HOST     := $(CSRC)/host
HOSTSRC  := $(HOST)/seq_reader.cpp $(HOST)/site_set.cpp $(HOST)/report.cpp $(HOST)/parallel_fastq.cpp \
            $(HOST)/inflate.cpp $(HOST)/inflate_spec.cpp $(HOST)/gz_stream.cpp $(HOST)/gz_parallel.cpp $(HOST)/crc32_fast.cpp $(HOST)/pack2.cpp
HOSTHDR  := $(wildcard $(HOST)/*.hpp) include/ntsm_host.h include/ntsm_hip.h

all: oracle_all build/ntsm_synth build/gather_bench build/ntsm_feed_bench build/ubench/inflate_wave ntsm_amd/libntsm_hip.so ntsm_amd/libntsm_synth.so ntsm_amd/libntsm_host.so build/ntsmCount ntsm_amd/libntsm_eval_hip.so build/ntsmEval ntsm_amd/libntsm_vcf_hip.so build/ntsmVCF ntsm_amd/libntsm_pca_hip.so build/ntsmPCA ntsm_amd/libntsm_sitegen_hip.so ntsm_amd/libntsm_sitegen_gap_hip.so build/ntsmSiteGen ref_gpu_binding

# host-only pieces (reader, site loader, report formatting): no HIP dependency
ntsm_amd/libntsm_host.so: $(HOSTSRC) $(HOST)/early_ingest.cpp $(HOST)/host_capi.cpp $(HOSTHDR)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOSTSRC) $(HOST)/early_ingest.cpp $(HOST)/host_capi.cpp -lz -pthread

build/ntsmCount: $(HOSTSRC) $(HOST)/feeder.cpp $(HOST)/fingerprint.cpp $(HOST)/early_ingest.cpp $(HOST)/ntsm_count_main.cpp $(HOSTHDR) ntsm_amd/libntsm_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $(HOSTSRC) $(HOST)/feeder.cpp $(HOST)/fingerprint.cpp $(HOST)/early_ingest.cpp $(HOST)/ntsm_count_main.cpp \
	    -Lntsm_amd -lntsm_hip -lz -pthread -Wl,-rpath,'$$ORIGIN/../ntsm_amd' -Wl,-rpath,/opt/rocm/lib

# libntsm_hip.so = four device translation units (the kernels + their launchers; kernels_sites.hip with its two entry points) and four host-only ones
HIPLIB_DEV  := $(CSRC)/kernels_generic.hip $(CSRC)/kernels_mz.hip $(CSRC)/kernels_run.hip $(CSRC)/kernels_sites.hip
HIPLIB_HOST := $(CSRC)/tables.cpp $(CSRC)/runtime.cpp $(CSRC)/rccl_bind.cpp $(CSRC)/capi.cpp
HIPLIB_HDR  := $(CSRC)/ntsm_internal.h $(CSRC)/kernels_common.h $(CSRC)/ntsm_hooks.h $(CSRC)/ntsm_device.h include/ntsm_hip.h
HIPLIB_TAB  := $(CSRC)/ntsm_tab_kernel.inc $(CSRC)/ntsm_tab_launch.inc $(CSRC)/ntsm_tab_runtime.inc $(CSRC)/ntsm_tab_tables.inc
# $(call hiplib,output,extra flags,object dir): every source to its own object (in parallel; stale objects removed first and every
# compile's exit status collected, so a failed translation unit fails the recipe instead of linking an old object), then one link
define hiplib
	@mkdir -p $(3) $(dir $(1))
	rm -f $(3)/*.o
	pids=""; for f in $(HIPLIB_DEV) $(HIPLIB_HOST); do $(HIPCC) $(HIPFLAGS) -fvisibility=hidden $(2) -c $$f -o $(3)/$$(basename $$f).o & pids="$$pids $$!"; done; \
	rc=0; for p in $$pids; do wait $$p || rc=1; done; exit $$rc
	$(HIPCC) $(HIPFLAGS) -shared -o $(1) $(foreach f,$(HIPLIB_DEV) $(HIPLIB_HOST),$(3)/$(notdir $(f)).o) -ldl
endef

ntsm_amd/libntsm_hip.so: $(HIPLIB_DEV) $(HIPLIB_HOST) $(HIPLIB_HDR)
	$(call hiplib,$@,,build/obj)

# Experiment and negative-result builds of the same ABI live under build/lib/, NOT in the package directory: the package ships
# libntsm_hip.so, libntsm_host.so, libntsm_synth.so and libntsm_eval_hip.so only.  NTSM_HIP_LIB=<bare name> finds them there
# (ntsm_amd/capi.py).
# the same ABI with the tabulated k = 19 kernel compiled in (ntsm_set_kernel(ctx, 3)): a measured negative result kept
# buildable and tested (tests/test_gpu_parity.py::test_tabulated_kernel_paths loads it through NTSM_HIP_LIB), not shipped
tab: build/lib/libntsm_hip_tab.so
build/lib/libntsm_hip_tab.so: $(HIPLIB_DEV) $(HIPLIB_HOST) $(HIPLIB_HDR) $(HIPLIB_TAB)
	$(call hiplib,$@,-DNTSM_WITH_TAB,build/obj_tab)

# design-study build: the two-level form with 12-mer minimizers instead of 14-mers, i.e. a
# minimizer Bloom in front of the one-level kernel's own blocks -- tools/mid_study.sh measures it on the 2.5 M-key set
m12: build/lib/libntsm_hip_m12.so
build/lib/libntsm_hip_m12.so: $(HIPLIB_DEV) $(HIPLIB_HOST) $(HIPLIB_HDR)
	$(call hiplib,$@,-DNTSM_TWO_M=12,build/obj_m12)

# experiment builds of the same ABI: make xlib XNAME=run96 XFLAGS="-DNTSM_RUN_C=96 ..." -> build/lib/libntsm_hip_run96.so (NTSM_HIP_LIB selects it)
xlib:
	$(call hiplib,build/lib/libntsm_hip_$(XNAME).so,$(XFLAGS),build/obj_$(XNAME))

# ntsmEval all-pairs scoring: own library, own CLI
# + the PCA-guided pair search (-p / -n): ntsm_eval_pca.hip with the x87 add of xprec.h
# + queries against a cohort store (--against): ntsm_eval_cross.hip; the store itself is host code (host/eval_store.hpp)
# + the PCA-guided search against a store (--index / --near): ntsm_eval_near.hip; it shares the staging of a chunk with the cross
#   path (ntsm_eval_chunk.h) and the search's steps with the session search (ntsm_eval_pca.h); the index is host code (host/eval_index.hpp)
# + the pairs inside a store (--within / --within-near): ntsm_eval_within.hip, staging through ntsm_eval_chunk.h too; the band and
#   pass arithmetic is host code that the library and the CLI share (host/eval_within.hpp)
# + one store against another (--between): ntsm_eval_between.hip, the rectangle tile and the staging of a store whose locus table
#   differs; the locus map and the band rule are host code that the library and the CLI share (host/eval_between.hpp)
# + the PCA-guided search between two stores (--between-near): ntsm_eval_between_near.hip, the row remap of a store whose locus
#   table differs in front of the projection and the listed-pair scorer; its candidate search is ntsm_eval_near.hip's kernels
# + the QC tables of a store (--qc): ntsm_eval_profile.hip, one fused kernel over each chunk's dense rows; the chunk rule and the
#   2-D copy are ntsm_eval_chunk.h's, the site table's text is host code (host/eval_qc.hpp)
# + the cross-sample contamination check over a store (--contam): ntsm_eval_contam.hip, the rectangle of ordered pairs (target,
#   source) in integers; the chunk rule and the 2-D copy are ntsm_eval_chunk.h's, the band rule and both tables' text are host
#   code (host/eval_contam.hpp)
# + parent-parent-child trios in a store (--trios): ntsm_eval_trio.hip, bit-planes of genotype classes and popcount kernels over
#   site words; the chunk rule and the 2-D copy are ntsm_eval_chunk.h's, the candidate rule, the batches, the pedigree and the
#   text are host code (host/eval_trio.hpp)
# + site-pair LD over a store (--ld): ntsm_eval_ld.hip, bit-planes with the samples along the bits and a popcount GEMM over
#   sites x sites; the genotype rule is ntsm_eval_geno.h's, shared with --trios; the chunk rule and the 2-D copy are
#   ntsm_eval_chunk.h's; the moments and r^2 (compiled for the device too), the band rule, the text and the prune are host code
#   (host/eval_ld.hpp)
# + what those store paths share on the host side of their HIP calls: ntsm_eval_chunk.h also states the check of a store argument,
#   the launch rule of the row-group kernels (cross, contam, the trio duo kernel) and the timed launch; ntsm_eval_band.h states the
#   band session of --within, --between and --contam once: the holding of a store's columns, resident or streamed, and the band walk
EVALSRC := $(CSRC)/ntsm_eval.hip $(CSRC)/ntsm_eval_pca.hip $(CSRC)/ntsm_eval_cross.hip $(CSRC)/ntsm_eval_near.hip $(CSRC)/ntsm_eval_within.hip \
           $(CSRC)/ntsm_eval_between.hip $(CSRC)/ntsm_eval_between_near.hip $(CSRC)/ntsm_eval_profile.hip $(CSRC)/ntsm_eval_contam.hip \
           $(CSRC)/ntsm_eval_trio.hip $(CSRC)/ntsm_eval_ld.hip
ntsm_amd/libntsm_eval_hip.so: $(EVALSRC) $(CSRC)/ntsm_eval_geno.h $(HOST)/eval_ld.hpp $(CSRC)/ntsm_eval_score.h $(CSRC)/ntsm_eval_chunk.h $(CSRC)/ntsm_eval_band.h $(CSRC)/ntsm_eval_pca.h $(CSRC)/ntsm_hip_scope.h $(CSRC)/xprec.h \
                              $(HOST)/eval_within.hpp $(HOST)/eval_between.hpp $(HOST)/eval_store.hpp include/ntsm_eval_hip.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -shared -o $@ $(EVALSRC)

build/ntsmEval: $(HOST)/ntsm_eval_main.cpp $(HOST)/eval_cli_args.hpp $(HOST)/eval_cli_rows.hpp $(HOST)/cli.hpp $(HOST)/eval_store.hpp $(HOST)/eval_index.hpp $(HOST)/eval_qc.hpp $(HOST)/eval_contam.hpp $(HOST)/eval_trio.hpp $(HOST)/eval_ld.hpp $(HOST)/eval_within.hpp $(HOST)/eval_between.hpp $(HOST)/crc32_fast.cpp $(HOST)/crc32_fast.hpp \
                $(HOST)/gz_stream.hpp $(CSRC)/xprec.h include/ntsm_eval_hip.h ntsm_amd/libntsm_eval_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -ffp-contract=off -o $@ $(HOST)/ntsm_eval_main.cpp $(HOST)/crc32_fast.cpp -Lntsm_amd -lntsm_eval_hip -lz \
	    -Wl,-rpath,'$$ORIGIN/../ntsm_amd' -Wl,-rpath,/opt/rocm/lib

# the store's writer and reader on their own under the host sanitizers (tools/eval_store_check.cpp; not part of `all`)
store_check: build/eval_store_check
build/eval_store_check: tools/eval_store_check.cpp $(HOST)/eval_store.hpp
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/eval_store_check.cpp

# the index's writer, reader, append and validity failures likewise (tools/eval_index_check.cpp; not part of `all`)
index_check: build/eval_index_check
build/eval_index_check: tools/eval_index_check.cpp $(HOST)/eval_index.hpp $(HOST)/eval_store.hpp $(HOST)/crc32_fast.cpp $(HOST)/crc32_fast.hpp
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/eval_index_check.cpp $(HOST)/crc32_fast.cpp -lz

# the band offsets, the band rule and the pass packing of --within / --within-near against brute force likewise
# (tools/eval_within_check.cpp; not part of `all`)
within_check: build/eval_within_check
	build/eval_within_check
build/eval_within_check: tools/eval_within_check.cpp $(HOST)/eval_within.hpp include/ntsm_eval_hip.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/eval_within_check.cpp

# the locus map and the band rule of --between on their cases likewise (tools/eval_between_check.cpp; not part of `all`)
between_check: build/eval_between_check
	build/eval_between_check
build/eval_between_check: tools/eval_between_check.cpp $(HOST)/eval_between.hpp $(HOST)/eval_store.hpp
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/eval_between_check.cpp

# what --between-near decides on the host likewise: whether B's index serves, the runs of dense rows, and the pass cut over
# lists that name two stores (tools/eval_between_near_check.cpp; not part of `all`)
between_near_check: build/eval_between_near_check
	build/eval_between_near_check
build/eval_between_near_check: tools/eval_between_near_check.cpp $(HOST)/eval_between.hpp $(HOST)/eval_within.hpp $(HOST)/eval_store.hpp
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/eval_between_near_check.cpp

# the band rule and the text of both tables of --contam likewise (tools/eval_contam_check.cpp; not part of `all`)
contam_check: build/eval_contam_check
	build/eval_contam_check
build/eval_contam_check: tools/eval_contam_check.cpp $(HOST)/eval_contam.hpp include/ntsm_eval_hip.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/eval_contam_check.cpp

# the candidate rule, the batch cutter, the pedigree parser, the name matcher, the row text and both runs of --trios over a model
# of the device likewise (tools/eval_trio_check.cpp; not part of `all`)
trio_check: build/eval_trio_check
	build/eval_trio_check
build/eval_trio_check: tools/eval_trio_check.cpp $(HOST)/eval_trio.hpp $(HOST)/eval_contam.hpp include/ntsm_eval_hip.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/eval_trio_check.cpp

# the moments and r^2, the band rule and its halving, the row text and the prune of --ld over a model of the device likewise
# (tools/eval_ld_check.cpp; not part of `all`)
ld_check: build/eval_ld_check
	build/eval_ld_check
build/eval_ld_check: tools/eval_ld_check.cpp $(HOST)/eval_ld.hpp include/ntsm_eval_hip.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/eval_ld_check.cpp

# the integer x87 add of the projection against the x87 itself likewise: every constructed class and 10^6 random operands, every
# branch of ntsm_x87_acc reached (tests/xprec_check.cpp; not part of `all`)
xprec_check: build/xprec_check
	build/xprec_check 1000000 7
build/xprec_check: tests/xprec_check.cpp $(CSRC)/xprec.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tests/xprec_check.cpp

# the host side of `ntsmCount --cohort` likewise: manifest parser, site lists, and the record builder against counts text +
# --pack, byte for byte (tools/cohort_count_check.cpp; not part of `all`)
cohort_check: build/cohort_count_check
	@mkdir -p build/cohort_check_tmp
	build/cohort_count_check build/cohort_check_tmp
build/cohort_count_check: tools/cohort_count_check.cpp $(HOST)/cohort.hpp $(HOST)/eval_store.hpp $(HOST)/site_set.hpp $(HOST)/report.cpp $(HOST)/report.hpp
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tools/cohort_count_check.cpp $(HOST)/report.cpp

# ntsmVCF (multi-sample VCF -> PCA matrix and centre file; --counts / --store: counts files and cohort-store records): own library, own CLI
ntsm_amd/libntsm_vcf_hip.so: $(CSRC)/ntsm_vcf.hip $(CSRC)/ntsm_hip_scope.h include/ntsm_vcf_hip.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -shared -o $@ $(CSRC)/ntsm_vcf.hip

VCFSRC := $(HOST)/seq_reader.cpp $(HOST)/site_set.cpp $(HOST)/inflate.cpp $(HOST)/inflate_spec.cpp $(HOST)/gz_stream.cpp \
          $(HOST)/gz_parallel.cpp $(HOST)/crc32_fast.cpp
build/ntsmVCF: $(VCFSRC) $(HOST)/ntsm_vcf_main.cpp $(HOSTHDR) include/ntsm_vcf_hip.h include/ntsm_pca_hip.h ntsm_amd/libntsm_vcf_hip.so \
               ntsm_amd/libntsm_pca_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -ffp-contract=off -o $@ $(VCFSRC) $(HOST)/ntsm_vcf_main.cpp -Lntsm_amd -lntsm_vcf_hip -lntsm_pca_hip -lz -pthread \
	    -Wl,-rpath,'$$ORIGIN/../ntsm_amd' -Wl,-rpath,/opt/rocm/lib

# ntsmPCA (NAME_matrix.tsv -> NAME_rotationalMatrix.tsv, NAME_components.tsv): own library, own CLI.  rocSOLVER is bound with
# dlopen on first use (the rpath lets a bare `librocsolver.so.0` resolve), so nothing links against it
# + the matrix from a cohort store (ntsmPCA --store): the genotype step shares the chunk rule and the 2-D copy with the store
#   paths of ntsmEval (ntsm_eval_chunk.h), the genotype code with its projection (ntsm_eval_pca.h) and the centre's text with
#   ntsmVCF (host/pca_text.hpp)
ntsm_amd/libntsm_pca_hip.so: $(CSRC)/ntsm_pca.hip $(CSRC)/ntsm_hip_scope.h include/ntsm_pca_hip.h $(CSRC)/ntsm_eval_chunk.h $(CSRC)/ntsm_eval_pca.h \
                             $(CSRC)/ntsm_eval_score.h $(CSRC)/xprec.h include/ntsm_eval_hip.h $(HOST)/pca_text.hpp $(HOST)/cli.hpp $(HOST)/gz_stream.hpp
	$(HIPCC) $(HIPFLAGS) -fvisibility=hidden -ffp-contract=off -shared -o $@ $(CSRC)/ntsm_pca.hip -ldl -Wl,-rpath,/opt/rocm/lib

PCASRC := $(HOST)/inflate.cpp $(HOST)/inflate_spec.cpp $(HOST)/gz_stream.cpp $(HOST)/gz_parallel.cpp $(HOST)/crc32_fast.cpp
build/ntsmPCA: $(PCASRC) $(HOST)/ntsm_pca_main.cpp $(HOSTHDR) include/ntsm_pca_hip.h ntsm_amd/libntsm_pca_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -ffp-contract=off -o $@ $(PCASRC) $(HOST)/ntsm_pca_main.cpp -Lntsm_amd -lntsm_pca_hip -lz -pthread \
	    -Wl,-rpath,'$$ORIGIN/../ntsm_amd' -Wl,-rpath,/opt/rocm/lib

# ntsmSiteGen (genome + VCF of SNPs -> NAME_n{i}.fa sites files): own library, own CLI
# both device libraries share their host side: the table builder and scan session (ntsm_sitegen_tables.h) and the staging
# state machine (ntsm_sitegen_stage.h)
SITEGENHDR := $(CSRC)/ntsm_sitegen_tables.h $(CSRC)/ntsm_sitegen_stage.h $(CSRC)/ntsm_hip_scope.h
ntsm_amd/libntsm_sitegen_hip.so: $(CSRC)/ntsm_sitegen.hip $(SITEGENHDR) include/ntsm_sitegen_hip.h
	$(HIPCC) $(HIPFLAGS) -fvisibility=hidden -shared -o $@ $(CSRC)/ntsm_sitegen.hip

# the second device library of ntsmSiteGen (-g): substitutions and one-base gaps in one pass (include/ntsm_sitegen_gap_hip.h)
ntsm_amd/libntsm_sitegen_gap_hip.so: $(CSRC)/ntsm_sitegen_gap.hip $(SITEGENHDR) include/ntsm_sitegen_gap_hip.h
	$(HIPCC) $(HIPFLAGS) -fvisibility=hidden -shared -o $@ $(CSRC)/ntsm_sitegen_gap.hip

SITEGENSRC := $(HOST)/seq_reader.cpp $(HOST)/inflate.cpp $(HOST)/inflate_spec.cpp $(HOST)/gz_stream.cpp $(HOST)/gz_parallel.cpp \
              $(HOST)/crc32_fast.cpp
build/ntsmSiteGen: $(SITEGENSRC) $(HOST)/ntsm_sitegen_main.cpp $(HOSTHDR) include/ntsm_sitegen_hip.h include/ntsm_sitegen_gap_hip.h \
                   ntsm_amd/libntsm_sitegen_hip.so ntsm_amd/libntsm_sitegen_gap_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $(SITEGENSRC) $(HOST)/ntsm_sitegen_main.cpp -Lntsm_amd -lntsm_sitegen_hip -lntsm_sitegen_gap_hip -lz -pthread \
	    -Wl,-rpath,'$$ORIGIN/../ntsm_amd' -Wl,-rpath,/opt/rocm/lib

# ablation builds (never shipped: wrong counts by construction).  `make ablation`: the default kernels with the switches of
# ntsm_ablation.inc (NTSM_DEBUG_KERNEL ...) -> build/lib/libntsm_hip_abl.so; `make ablation ABL="1 2 4"`: the tabulated
# kernel's compile-time ablations as well -> build/lib/libntsm_hip_abl<N>.so (tools/ablate.sh drives both)
ablation: $(HIPLIB_DEV) $(HIPLIB_HOST) $(HIPLIB_HDR) $(HIPLIB_TAB) $(CSRC)/ntsm_ablation.inc
	$(call hiplib,build/lib/libntsm_hip_abl.so,-DNTSM_ABLATION $(ABLFLAGS),build/obj_abl)
	for a in $(ABL); do $(MAKE) --no-print-directory abl_tab A=$$a; done
abl_tab:
	$(call hiplib,build/lib/libntsm_hip_abl$(A).so,-DNTSM_WITH_TAB -DNTSM_ABLATION -DNTSM_TAB_ABL=$(A),build/obj_abl$(A))

ntsm_amd/libntsm_synth.so: $(CSRC)/synth_dev.hip $(CSRC)/synth_host.cpp $(CSRC)/synth.h include/ntsm_synth.h
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(CSRC)/synth_dev.hip $(CSRC)/synth_host.cpp -lz

oracle_all:
	$(MAKE) -C oracle all
# INTEGRATION.md section 2 compiled around the unmodified reference class and linked against the product library (test
# infrastructure: oracle/ref_gpu_binding.cpp -> oracle/_ref/ref_gpu_ntsmCount; only where /root/reference exists)
ref_gpu_binding: ntsm_amd/libntsm_hip.so
	$(MAKE) -C oracle refgpu

build/ntsm_synth: tools/ntsm_synth.cpp $(CSRC)/synth_host.cpp $(CSRC)/synth.h include/ntsm_synth.h
	@mkdir -p build
	$(CXX) $(CXXFLAGS) tools/ntsm_synth.cpp $(CSRC)/synth_host.cpp -o $@ -lz

# the host-fed path on a PCIe roofline (bench.py other_configs.feed)
build/ntsm_feed_bench: tools/feed_bench.cpp $(HOST)/pack2.cpp $(HOSTHDR) include/ntsm_synth.h ntsm_amd/libntsm_hip.so ntsm_amd/libntsm_host.so ntsm_amd/libntsm_synth.so
	@mkdir -p build
	$(HIPCC) -O3 -std=c++17 -Wall -Wextra -o $@ tools/feed_bench.cpp $(HOST)/pack2.cpp -Lntsm_amd -lntsm_hip -lntsm_host -lntsm_synth -pthread \
	    -Wl,-rpath,'$$ORIGIN/../ntsm_amd' -Wl,-rpath,/opt/rocm/lib

# gate for a device-side inflate of FASTQ .gz: one wave per chunk of a deflate stream
build/ubench/inflate_wave: tools/ubench/inflate_wave.hip $(CSRC)/synth_host.cpp $(CSRC)/synth.h include/ntsm_synth.h
	@mkdir -p build/ubench
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -Wall -Wextra -o $@ tools/ubench/inflate_wave.hip $(CSRC)/synth_host.cpp -lz -pthread

build/gather_bench: tools/gather_bench.hip
	@mkdir -p build
	$(HIPCC) -O3 --offload-arch=$(ARCH) tools/gather_bench.hip -o $@

clean:
	rm -rf build ntsm_amd/*.so
	$(MAKE) -C oracle clean
.PHONY: all oracle_all ref_gpu_binding clean ablation abl_tab tab m12 xlib store_check index_check within_check between_check between_near_check contam_check trio_check ld_check cohort_check xprec_check
