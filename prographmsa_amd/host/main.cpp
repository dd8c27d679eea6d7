// main.cpp — command-line driver mirroring the reference's main()/doAlign (src/main.cpp:32-483) for
// the flags the hot path's configurations use.  Built twice: `pgmsa` (HIP backend, the product) and, for tests only,
// `oracle/_build/pgmsa_oracle` (CPU oracle backend).  Here: the solo run and the --batch run around the loop of
// driver_family.cpp; the command line is driver_options.cpp, the analyses of a final alignment driver_analyses.cpp, the
// --stats line driver_stats.cpp.
#include "driver.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <malloc.h>
#include <unistd.h>
#include <thread>

using namespace pgm;

// The backend (device contexts: the HIP runtime's start-up takes 80-400 ms) is created on a thread of its own while the
// sequences are read and the models are set up; doAlign waits for it before the clocks of the stages start.
namespace {
struct BackendStartup {
    std::thread thr;
    double seconds = 0;
    std::string err;
    void start() {
        thr = std::thread([this]() {
            const auto t0 = std::chrono::steady_clock::now();
            try { default_backend(); }
            catch (std::exception &e) { err = e.what(); }
            seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        });
    }
    void wait() {
        if (thr.joinable()) thr.join();
        if (!err.empty()) throw pgm_exception(err);
    }
    ~BackendStartup() { if (thr.joinable()) thr.join(); }
} g_startup;
}  // namespace

// the device contexts (HIP runtime start-up, code object load) exist before the clocks of the stages start; init_s is the
// time their creation took (it ran beside the set-up), init_wait_s what of it was left to wait for here
static double wait_for_backend(const CSProfile *csprofile) {
    auto t0 = std::chrono::steady_clock::now();
    g_startup.wait();
    default_backend();
    double t_preload = 0;
    if (csprofile) {   // the profile library goes to the devices with the rest of the start-up (counted in init_s)
        const auto tp = std::chrono::steady_clock::now();
        default_backend().csprofile_preload(*csprofile);
        t_preload = std::chrono::duration<double>(std::chrono::steady_clock::now() - tp).count();
    }
    const double t_init = (g_startup.seconds > 0 ? g_startup.seconds : std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()) + t_preload;
    if (host_switches().profile)
        fprintf(stderr, "backend start-up %.1f ms, of which %.1f ms waited for after the set-up\n", t_init * 1e3,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return t_init;
}

// The solo run: the loop of a --batch chunk on a list of this one family, its trees from TreeNJ; a failure ends the run with the
// family's message.
static void doAlign(const Alphabet &a, const DriverOptions &o, Family &fam) {
    fam.prepare(a);
    std::unique_ptr<CSProfile> csprofile;
    if (!cmdlineopts.cs_file.empty()) csprofile.reset(new CSProfile(cmdlineopts.cs_file));
    const double t_init = wait_for_backend(csprofile.get());
    std::map<std::string, std::vector<repeat_t>> reps;   // main.cpp:367-370 (detection by T-REKS itself is not built here: --read_repeats only)
    if (!cmdlineopts.readreps_file.empty()) reps = read_repeats(a, cmdlineopts.readreps_file, fam.seqs2);
    fam.repeats = &reps;
    const std::vector<Family *> one(1, &fam);
    auto check = [&]() { if (!fam.failure.empty()) throw pgm_exception(fam.failure); };
    auto t0 = std::chrono::steady_clock::now();
    if (!fam.topo_file.empty()) fam.read_topology();
    if (!fam.tree_file.empty()) fam.read_tree();
    initial_trees(a, one, true);
    check();
    double t_tree = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    t0 = std::chrono::steady_clock::now();
    // further rounds of alignment followed by estimation of an improved tree from the induced pairwise distances
    // (main.cpp:404-430; the default is two such rounds when no tree is given), then the final alignment
    align_rounds(a, one, csprofile.get(), true);
    check();
    if (host_switches().profile) fprintf(stderr, "[%.1f ms] back in main\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    double t_prog = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (o.bootstrap.given || o.mltree.tree_given) {   // (with -T the final alignment is computed for them alone, once: what is printed stays the tree)
        ProgressiveAlignmentResult own;
        if (cmdlineopts.onlytree_flag) own = progressive_alignment(a, fam.seqs2, *fam.tree, csprofile.get(), *fam.model_factory, fam.repeats);
        const std::map<std::string, sequence_t> &alignment = cmdlineopts.onlytree_flag ? own.aligned_sequences : fam.result.aligned_sequences;
        if (o.bootstrap.given) doBootstrap(a, o, fam, alignment);
        if (o.mltree.tree_given) doMlTree(a, o, fam, alignment);
    }
    if (o.guidance.given) doGuidance(a, o, fam, csprofile.get());

    fam.finish(a);
    if (cmdlineopts.repeats_flag) {
        if (cmdlineopts.readreps_file.empty()) error("-R: tandem-repeat detection (T-REKS, a Java program) is not built here; supply the repeats with --read_repeats");
        std::cerr << "TR indels: " << fam.result.n_tr_indels << std::endl;   // main.cpp:447-449
    }
    if (!cmdlineopts.profile_file.empty()) fam.write_profiles(a, cmdlineopts.profile_file);
    if (o.stats) print_stats(o, t_init, t_tree, t_prog, false);
}

static int doBatch(const Alphabet &a, const DriverOptions &o) {
    const std::string &list_file = o.batch_list;
    std::vector<std::unique_ptr<Family>> fams;
    {
        std::ifstream in(list_file.c_str());
        if (!in) error("cannot open the list of families %s", list_file.c_str());
        std::string line;
        for (int lineno = 1; std::getline(in, line); ++lineno) {
            if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
            if (line.empty() || line[0] == '#') continue;
            std::vector<std::string> field(1);
            for (char c : line) { if (c == '\t') field.emplace_back(); else field.back() += c; }
            bool blank = true;
            for (char c : line) blank = blank && (c == '\t' || c == ' ');
            if (blank) continue;
            if (field.size() < 2 || field.size() > 4 || field[0].empty() || field[1].empty())
                error("--batch: line %d of %s: expected input<TAB>output[<TAB>tree[<TAB>topology]], found %zu field(s)", lineno, list_file.c_str(), field.size());
            std::unique_ptr<Family> f(new Family);
            f->input = field[0]; f->output = field[1];
            if (field.size() >= 3) f->tree_file = field[2];
            if (field.size() == 4) f->topo_file = field[3];
            f->iters = (!o.iters_set && !f->tree_file.empty()) ? 0 : cmdlineopts.iters;   // no iterations with a guide tree (main.cpp:243-246)
            fams.push_back(std::move(f));
        }
    }
    BatchStats &run = batch_stats;
    run.families = (int)fams.size();
    g_startup.start();
    parallel_for(64, [](size_t) {});   // (the driver's host threads start while the device runtime does)
    std::unique_ptr<CSProfile> csprofile;
    if (!cmdlineopts.cs_file.empty()) csprofile.reset(new CSProfile(cmdlineopts.cs_file));
    parallel_for(fams.size(), [&](size_t k) {
        Family &f = *fams[k];
        try {
            f.seqs = read_fasta(f.input, f.input_order);
            f.prepare(a);
            if (!f.tree_file.empty()) f.read_tree();
            if (!f.topo_file.empty()) f.read_topology();
            f.cells = estimate_cells(f);
        } catch (std::exception &e) { f.failure = e.what(); }
    });
    const double t_init = wait_for_backend(csprofile.get());
    const auto t0 = std::chrono::steady_clock::now();
    auto report = [&](Family &f) {
        std::cerr << "family " << f.input << ": ERROR:" << f.failure << std::endl;
        ++run.failed;
    };
    // chunks: families in list order while the estimated cells of a pass stay within the bound; a larger family alone
    std::vector<std::vector<Family *>> chunks;
    {
        double cells = 0;
        for (auto &f : fams) {
            if (!f->failure.empty()) continue;
            if (chunks.empty() || (!chunks.back().empty() && cells + f->cells > o.batch_cells)) { chunks.emplace_back(); cells = 0; }
            chunks.back().push_back(f.get());
            cells += f->cells;
        }
    }
    run.chunks = (int)chunks.size();
    for (auto &f : fams) if (!f->failure.empty()) report(*f);
    for (const std::vector<Family *> &chunk : chunks) {
        try {   // the families of the chunk through the stages in lock-step: every device stage once for all of them
            std::vector<uint64_t> cost(chunk.size());   // dealt to the device contexts, longest first (a family never spans contexts)
            for (size_t k = 0; k < chunk.size(); ++k) cost[k] = (uint64_t)chunk[k]->cells + 1u;
            const std::vector<std::vector<uint32_t>> shards = farm_shards(cost, default_backend().workers());
            for (size_t w = 0; w < shards.size(); ++w) for (uint32_t k : shards[w]) chunk[k]->worker = (int)w;
            initial_trees(a, chunk, false);
            align_rounds(a, chunk, csprofile.get(), false);
        }
        catch (std::exception &e) { for (Family *f : chunk) if (f->failure.empty()) f->failure = e.what(); }   // (a stage all its families share)
        const std::vector<Family *> ok = alive(chunk);
        parallel_for(ok.size(), [&](size_t k) {
            Family &f = *ok[k];
            try {
                f.finish(a);
                std::ofstream out(f.output.c_str());
                if (!out) error("error opening output file");
                f.write(out);
            } catch (std::exception &e) { f.failure = e.what(); }
        });
        for (Family *f : chunk) {
            if (!f->failure.empty()) report(*f);
            f->seqs.clear(); f->seqs2.clear(); f->aligned.clear();
            f->result = ProgressiveAlignmentResult(); f->old_result = ProgressiveAlignmentResult();
            delete f->tree; f->tree = nullptr;
            delete f->topo; f->topo = nullptr;
            f->model_factory.reset();
        }
    }
    const double t_prog = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (o.stats) print_stats(o, t_init, 0.0, t_prog, true);
    return run.failed ? 2 : 0;
}

// The outputs are complete.  Releasing the contexts' gigabytes of device memory and pinned blocks and shutting the HIP runtime
// down in an orderly way takes 30-70 ms that the kernel driver spends anyway when the process is gone: leave directly
// (PGM_FULL_EXIT=1 for runs under a profiler or a sanitizer, whose reports are written by exit handlers).
static int leave(int rc) {
    if (!getenv("PGM_FULL_EXIT") && std::string(default_backend().name()) == "hip") {
        std::cout.flush(); std::cerr.flush(); fflush(nullptr);
        _exit(rc);
    }
    return rc;
}

int main(int argc, char **argv) {
    const auto t_main = std::chrono::steady_clock::now();
    // The graphs of a level are hundreds of vectors of 0.1-1 MB built and dropped by the host threads: with glibc's defaults
    // each is an mmap / munmap of its own (page faults on every reuse, the address-space lock shared by all threads), and
    // the heap is trimmed back to the system whenever its top is freed.  Keep them in the heaps instead.
    if (!getenv("PGM_MALLOC_DEFAULTS")) {
        mallopt(M_MMAP_THRESHOLD, 1 << 30);
        mallopt(M_TRIM_THRESHOLD, 0x7fffffff);
        mallopt(M_TOP_PAD, 64 << 20);
    }
    try {
        DriverOptions o;
        const int rc = parse_driver_options(argc, argv, o);
        if (rc >= 0) return rc;
        if (!o.dump.empty()) set_job_dump(o.dump);
        if (!o.dist_dump.empty()) set_dist_dump(o.dist_dump);
        if (!o.joins_dump.empty()) set_joins_dump(o.joins_dump);
        const AlphabetKind kind = cmdlineopts.codon_flag ? ALPHA_CODON : cmdlineopts.dna_flag ? ALPHA_DNA : ALPHA_AA;
        if (!o.batch_list.empty()) {
            const Alphabet a(kind);
            if (!cmdlineopts.fasta_flag && !cmdlineopts.onlytree_flag) std::cerr << "note: Stockholm output is not built here; writing FASTA" << std::endl;
            return leave(doBatch(a, o));
        }

        g_startup.start();
        parallel_for(64, [](size_t) {});   // (the driver's host threads start while the device runtime does)
        Family fam;
        fam.input = cmdlineopts.sequence_file; fam.tree_file = cmdlineopts.tree_file; fam.topo_file = o.topo_file; fam.iters = cmdlineopts.iters;
        fam.seqs = read_fasta(cmdlineopts.sequence_file, fam.input_order);
        if (o.bootstrap.given && fam.seqs.size() < 4) error("--bootstrap needs at least 4 sequences");
        if (o.guidance.given && fam.seqs.size() < 4) error("--guidance needs at least 4 sequences");
        if (o.mltree.tree_given && fam.seqs.size() < 3) error("--ml_tree needs at least 3 sequences");
        if (o.mltree.support_given && fam.seqs.size() < 4) error("--ml_support needs at least 4 sequences");
        if (o.mltree.tree_given && o.mltree.start_given) {   // (--ml_start is read as -t reads a tree, and refused before any work or file)
            std::ifstream ts(o.mltree.start.c_str());
            if (!ts) error("cannot open the --ml_start tree file %s", o.mltree.start.c_str());
            o.mltree.start_tree.reset(parse_newick(ts));
            std::vector<std::string> held, own;
            std::function<void(const PhyTree &)> walk = [&](const PhyTree &t) {
                if (t.isLeaf()) { held.push_back(t.getName()); return; }
                if (t.n_children() < 2) error("--ml_start: an inner node with one child");
                for (index_t c = 0; c < t.n_children(); ++c) walk(t[(int)c]);
            };
            walk(*o.mltree.start_tree);
            for (const auto &kv : fam.seqs) own.push_back(kv.first);
            std::sort(held.begin(), held.end());
            std::sort(own.begin(), own.end());
            if (held != own) error("--ml_start: the leaves of the tree are not the sequences of the input");
        }
        std::ofstream custom_out;
        std::ostream *out = &std::cout;
        if (!cmdlineopts.output_file.empty()) {
            custom_out.open(cmdlineopts.output_file.c_str());
            if (!custom_out) error("error opening output file");
            out = &custom_out;
        }
        const Alphabet a(kind);
        doAlign(a, o, fam);
        if (!cmdlineopts.onlytree_flag && !cmdlineopts.fasta_flag) std::cerr << "note: Stockholm output is not built here; writing FASTA" << std::endl;
        fam.write(*out);
        if (host_switches().profile)
            fprintf(stderr, "main: output written %.1f ms after its start\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_main).count());
        custom_out.close();
        return leave(0);
    } catch (std::exception &e) {
        std::cerr << "ERROR:" << e.what() << std::endl;
        return 2;
    }
}
