// driver.h — what driver_analyses.cpp and driver_stats.cpp give main.cpp.
#pragma once
#include "driver_family.h"
#include "driver_options.h"

namespace pgm {

// driver_analyses.cpp: what --bootstrap, --ml_tree and --guidance compute from a final alignment and write
void doBootstrap(const Alphabet &a, const DriverOptions &o, const Family &fam, const std::map<std::string, sequence_t> &alignment);
void doMlTree(const Alphabet &a, const DriverOptions &o, const Family &fam, const std::map<std::string, sequence_t> &alignment);
void doGuidance(const Alphabet &a, const DriverOptions &o, const Family &fam, const CSProfile *csprofile);
// driver_stats.cpp: the --stats line (batch: with the keys of --batch)
void print_stats(const DriverOptions &o, double t_init, double t_tree, double t_prog, bool batch);

}  // namespace pgm
