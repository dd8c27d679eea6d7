# The host sources without a backend, and every file they include: the one list of csrc/Makefile (pgmsa) and oracle/Makefile
# (pgmsa_oracle and its sanitized build).  The including Makefile sets HOST to this directory; build with $(HOSTDEFS).
HOSTSRC = $(HOST)/alphabet.cpp $(HOST)/model_factory.cpp $(HOST)/graph.cpp $(HOST)/graph_align.cpp \
          $(HOST)/phytree.cpp $(HOST)/host_threads.cpp $(HOST)/progressive.cpp $(HOST)/root_search.cpp $(HOST)/repeats.cpp $(HOST)/guidance.cpp $(HOST)/transfer.cpp \
          $(HOST)/distance.cpp $(HOST)/mldist.cpp $(HOST)/bionj.cpp $(HOST)/wls.cpp $(HOST)/csprofile.cpp \
          $(HOST)/driver_options.cpp $(HOST)/driver_family.cpp $(HOST)/driver_analyses.cpp $(HOST)/driver_stats.cpp $(HOST)/main.cpp
HOSTINC = $(HOST)/pgm_host.h $(HOST)/progressive_internal.h $(HOST)/nnls.h $(HOST)/treelik.inc $(HOST)/treelik_rates.inc $(HOST)/treelik_anc.inc $(HOST)/treelik_nni.inc $(HOST)/treelik_support.inc \
          $(HOST)/driver_options.h $(HOST)/driver_family.h $(HOST)/driver.h $(HOST)/../csrc/pgm_pool.h $(HOST)/../../include/pgm_hip.h
HOSTDEFS = -DPGM_HOST_SPLIT=3
