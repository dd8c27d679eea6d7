# The host sources without a backend, and every file they include: the one list of csrc/Makefile (pgmsa) and oracle/Makefile
# (pgmsa_oracle and its sanitized build).  The including Makefile sets HOST to this directory.
HOSTSRC = $(HOST)/alphabet.cpp $(HOST)/model_factory.cpp $(HOST)/treelik.cpp $(HOST)/treelik_rates.cpp $(HOST)/treelik_anc.cpp $(HOST)/treelik_joint.cpp $(HOST)/treelik_nni.cpp $(HOST)/treelik_spr.cpp $(HOST)/treelik_support.cpp $(HOST)/graph.cpp $(HOST)/graph_align.cpp \
          $(HOST)/phytree.cpp $(HOST)/host_threads.cpp $(HOST)/progressive.cpp $(HOST)/root_search.cpp $(HOST)/repeats.cpp $(HOST)/guidance.cpp $(HOST)/transfer.cpp \
          $(HOST)/distance.cpp $(HOST)/mldist.cpp $(HOST)/bionj.cpp $(HOST)/wls.cpp $(HOST)/csprofile.cpp \
          $(HOST)/driver_options.cpp $(HOST)/driver_family.cpp $(HOST)/driver_analyses.cpp $(HOST)/driver_stats.cpp $(HOST)/main.cpp
HOSTINC = $(HOST)/pgm_host.h $(HOST)/progressive_internal.h $(HOST)/nnls.h $(HOST)/treelik.h $(HOST)/treelik_internal.h \
          $(HOST)/driver_options.h $(HOST)/driver_family.h $(HOST)/driver.h $(HOST)/../csrc/pgm_pool.h $(HOST)/../csrc/pgm_treelik_check.h $(HOST)/../../include/pgm_hip.h
