/*
 * oracle/ref_config/config.h -- TEST INFRASTRUCTURE ONLY, and empty on purpose: no definitions.
 *
 * The reference's scoring class (src/CompareCounts.hpp:19) includes vendor/kfunc.c, whose line 28 includes autoconf's
 * "config.h".  kfunc.c takes nothing from that file: it tests no HAVE_* macro and names no PACKAGE_* value.  This file only
 * lets that one include line resolve, so that oracle/ref_eval_driver.cpp can compile the unmodified class
 * (oracle/Makefile, target ref, puts this directory first on the include path).  It stands in for no generated value; the
 * reference's main, which does take PACKAGE_NAME and GIT_REVISION from the generated file, is not built.
 */
