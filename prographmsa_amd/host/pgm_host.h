// pgm_host.h — host-side C++ mirror of the reference's progressive-alignment call surface.
//
// Dependency-free C++17 (no Eigen, no TCLAP).  Names, argument meaning and error behaviour
// follow acg-team/ProGraphMSA so that the scaffolding around the hot path reads like the
// reference; the three hot functions themselves (alignGraphs, DistanceFactoryAlign::alignPair,
// CSProfile::createProfile) are thin wrappers over the C ABI of include/pgm_hip.h.
//
// Reference files mirrored (all under /root/reference/src):
//   Alphabet.{h,cpp}  Model.h  ModelFactory.{h,cpp}  ModelFactoryWag.cpp  ModelFactoryEcm.cpp
//   Graph.h  SequenceGraph.h  CleanedGraph.h  GraphAlign.h  ProgressiveAlignment.{h,cpp}
//   PhyTree.{h,cpp}  newick.cpp  Fasta.cpp  TreeNJ.{h,cpp}  DistanceFactory*.{h,cpp}
//   CSProfile.{h,cpp}  main.{h,cpp}
#ifndef PGM_HOST_H_
#define PGM_HOST_H_

#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include <functional>

#include "../../include/pgm_hip.h"

namespace pgm {

typedef double score_t;      // main.h:31
typedef float dp_score_t;    // main.h:32
typedef uint32_t index_t;    // main.h:33
typedef double distance_t;   // main.h:34

// ---------------------------------------------------------------------------------------
// cmdlineopts (main.h:37-82) with the defaults of main.cpp:37-169
struct cmdlineopts_t {
    int iters = 2;
    bool fasta_flag = false, noforcealign_flag = false, nwdist_flag = false, onlytree_flag = false;
    bool mldist_flag = false, mldist_gap_flag = false, codon_flag = false, inputorder_flag = false;
    bool ancestral_flag = false;
    bool earlyref_flag = false;       // --early_refinement (ProgressiveAlignment.h:102-110)
    int wlsrefine_flag = 0;           // -W / --wls_refine, counted (main.cpp:120): 1 = quartet moves, 2 or more = quintet moves too (LeastSquares.cpp:683)
    int reroot_flag = 0;              // -r / --reroot, counted (main.cpp:117): 1 = every branch, 2 or more = hill climbing (FindRoot.h:276-320)
    std::string profile_file;   // --profile_out (main.cpp:132)
    std::string readreps_file;  // --read_repeats (main.cpp:108)
    bool repeats_flag = false;  // -R: here only the "TR indels" lines on stderr (T-REKS itself is not run: --read_repeats supplies the repeats)
    double indel_rate = 0.0093359375;
    double end_indel_prob = 0.12;
    double gapext_prob = 0.6119140625;
    double edge_halflife = 0.3;
    double altsplice_prob = 0.328125;
    double pseudo_count = 1000;
    double cutoff_dist = 2.2;
    double repeat_rate = 0.1;
    double repeatext_prob = 0.3;
    double max_dist = 2.2, min_dist = 0.05, max_pdist = 0.8, min_pdist = 0.05;
    std::string output_file, sequence_file, tree_file, cs_file;
    bool dna_flag = false;      // --dna (main.cpp:55-57, 219-223)
    std::string cmodel_file;    // --custom_model (main.cpp:135, 178)
    bool aafreqs_flag = false;  // -F / --estimate_aafreqs (main.cpp:138, 204); -C / --aafreqs_pseudocount sets pseudo_count
};
extern cmdlineopts_t cmdlineopts;

// error() of debug.cpp:43-52 prints and abort()s; the mirror throws so that the C-level
// callers (and tests) can observe it.  main() maps it to exit code 2 like main.cpp:315-319.
struct pgm_exception : std::runtime_error {
    explicit pgm_exception(const std::string &m) : std::runtime_error(m) {}
};
[[noreturn]] void error(const char *fmt, ...);

// ---------------------------------------------------------------------------------------
// Alphabets (Alphabet.h:37-115).  A symbol is stored as the reference stores it in `data`:
// AA and DNA keep the raw character, Codon keeps the codon index (61 = unknown, 62 = gap, -1 = invalid).
// DNA values follow dna_translation_table (Alphabet.cpp:22-40): T=0 C=1 A=2 G=3, unknown 4.
enum AlphabetKind { ALPHA_AA = 0, ALPHA_CODON = 1, ALPHA_DNA = 2 };
struct Alphabet {
    AlphabetKind kind;
    int DIM;
    explicit Alphabet(AlphabetKind k) : kind(k), DIM(k == ALPHA_AA ? 20 : k == ALPHA_DNA ? 4 : 61) {}
    bool rawChars() const { return kind != ALPHA_CODON; }   // one character per symbol, kept as read
    int value(int8_t data) const;                  // AA::value / Codon::value
    bool isValid(int8_t data) const { int v = value(data); return v >= 0 && v < DIM; }
    int8_t gap() const;                            // ALPHABET::GAP
    int8_t unknown() const;                        // ALPHABET::X
    bool isGap(int8_t d) const { return d == gap(); }
    char asChar(int8_t data) const;
    std::string asString(int8_t data) const;
    bool stripsStart(int8_t first) const;          // main.cpp:340
    bool stripsEnd(int8_t last) const;             // main.cpp:348
};
typedef std::basic_string<int8_t> sequence_t;
sequence_t sequenceFromString(const Alphabet &a, const std::string &str);             // Alphabet.h:118
std::string stringFromSequence(const Alphabet &a, const sequence_t &seq);             // :136
std::string stringFromSequence(const Alphabet &a, const sequence_t &seq, const std::string &orig);  // :148

// ---------------------------------------------------------------------------------------
// Model (Model.h:8-24); matrices are dim x dim column-major.
struct Model {
    int dim = 0;
    std::vector<double> M, P, Q, pi;
    double delta = 0, epsilon = 0;
    distance_t distance = 0, divergence = 0;
};

// ModelFactory (ModelFactory.h:11-34) with the WAG (ModelFactoryWag.cpp) and ECM
// (ModelFactoryEcm.cpp) rate matrices, a custom model read from a file (ModelFactoryCustom.h) and frequencies
// estimated from the input (ModelFactoryPlusF.h).  P(t) = exp(Q t) by scaling-and-squaring instead of Eigen's
// general EigenSolver; agrees to ~1e-14.
class ModelFactory {
public:
    // ModelFactory.cpp:11-90: --custom_model, else WAG / ECM (DNA: a custom model is required); -F then re-estimates the frequencies
    static ModelFactory *getDefault(const Alphabet &a, const std::map<std::string, sequence_t> &seqs);
    Model getModel(distance_t distance) const;                   // ModelFactory.h:48-67
    Model getModel(distance_t distance, distance_t gap_distance) const;  // :70-90
    // P(t) = exp(Q t) as getModel builds it, for the distance t itself (none of parseDistance's clamps): dim x dim column-major
    std::vector<double> transition(distance_t t) const;
    double getEpsilon(distance_t) const { return cmdlineopts.gapext_prob; }
    double getDelta(distance_t distance) const;
    int dim() const { return dim_; }
    const std::vector<double> &Qmat() const { return Q_; }
    const std::vector<double> &freqs() const { return freqs_; }
    // eigen form P(d) = V diag(exp(sigma d)) V^-1 (only for reversible rate matrices: WAG)
    bool has_eigen() const { return use_eigen_; }
    const std::vector<double> &eigV() const { return V_; }
    const std::vector<double> &eigVi() const { return Vi_; }
    const std::vector<double> &eigSigma() const { return sigma_; }

private:
    ModelFactory(int dim, const std::string &qmat_file);
    explicit ModelFactory(int dim) : dim_(dim) {}
    static ModelFactory *readCustom(int dim, const std::string &file);                      // ModelFactoryCustom.h:36-70
    void estimateFreqs(const Alphabet &a, const std::map<std::string, sequence_t> &seqs);   // ModelFactoryPlusF.h:72-105
    void normalise();   // diagonal reset, rate normalisation and the choice of the eigen form (Q_ off the diagonal and freqs_ set)
    static void parseDistance(distance_t distance, Model &model);  // ModelFactory.h:104-127
    void fillP(Model &model) const;
    int dim_;
    std::vector<double> freqs_, Q_, V_, Vi_, sigma_;
    bool use_eigen_ = false;
};

// ---------------------------------------------------------------------------------------
// Graph (Graph.h:20-502): profile matrix + two CSR matrices (edges float, repeats uint).
class Graph {
public:
    typedef std::map<std::pair<index_t, index_t>, dp_score_t> EdgeMap;   // key (to,from)
    typedef std::map<std::pair<index_t, index_t>, index_t> RepeatMap;

    Graph() : Graph(20) {}
    explicit Graph(int dim);                                                    // Graph.h:141-150
    Graph(int dim, const std::vector<std::vector<double>> &nodes);              // :104-120
    Graph(int dim, const std::vector<std::vector<double>> &nodes, const EdgeMap &edges,
          const RepeatMap &repeats);                                            // :122-139
    // the same from flat data (mergeGraphs' hot path): profiles dim x n column-major (columns 0 and n - 1 are taken as zero),
    // edge / repeat lists sorted by (to, from) without duplicates — what iterating the two maps above yields
    struct EdgeRec { index_t to, from; dp_score_t cost; };
    struct RepeatRec { index_t to, from, units; };
    Graph(int dim, index_t n, const double *profiles, const std::vector<EdgeRec> &edges, const std::vector<RepeatRec> &repeats);
    // a chain of n nodes whose profiles live on the device only (a leaf graph of a resident pass: setDevSites)
    struct NoSites {};
    Graph(int dim, index_t n, NoSites);

    index_t size() const { return n_; }
    int dim() const { return dim_; }
    const double *col(index_t i) const { return &sites_[(size_t)dim_ * i]; }
    const std::vector<double> &getSites() const { return sites_; }
    // A merged graph whose profiles were left on the device (Backend::merge_profiles_batch_res) has no host copy of them
    // (sites_ empty): devSites() is the dim x n matrix in HBM.  A CleanedGraph of such a graph refers to the same matrix
    // through its node mapping (nodeMap()).
    const double *devSites() const { return dev_sites_; }
    void setDevSites(const double *p) { dev_sites_ = p; }
    bool hasHostSites() const { return !sites_.empty(); }
    pgm_graph flat() const;  // view for the C ABI (valid while *this is alive and unchanged)

    // PredIterator (Graph.h:180-248)
    class PredIterator {
    public:
        PredIterator(const Graph &g, index_t row, dp_score_t repeat_init, dp_score_t repeat_ext);
        PredIterator &operator++() { if (i_ < iend_) ++i_; else ++j_; return *this; }
        bool isRepeat() const { return !(i_ < iend_); }
        index_t repeatUnits() const { return g_->r_units_[j_]; }
        explicit operator bool() const { return i_ < iend_ || j_ < jend_; }
        dp_score_t value() const;
        dp_score_t rawValue() const { return g_->e_val_[i_]; }
        index_t operator*() const { return i_ < iend_ ? g_->e_col_[i_] : g_->r_col_[j_]; }
    private:
        const Graph *g_;
        int32_t i_, iend_, j_, jend_;
        dp_score_t repeatInit_, repeatExt_;
    };
    PredIterator getPreds(index_t node, dp_score_t repeat_init, dp_score_t repeat_ext) const {
        return PredIterator(*this, node, repeat_init, repeat_ext);
    }

protected:
    void fillInitialEdges();                            // :35-46
    void setEdgesFromMap(const EdgeMap &edge_map);      // :81-90
    void setRepeatsFromMap(const RepeatMap &rep_map);   // :92-100
public:
    // tandem-repeat edges from the unit homologies of the graph's nodes (Graph.h:48-79, 458-469): tr_homology[i] = column of
    // node i + 1 inside its repeat unit, -1 outside a repeat; replaces the repeat matrix
    void addRepeats(const std::vector<std::vector<int>> &tr_homologies);
    // early refinement (Graph.h:369-426): every profile column but START / END set to ones; nodes [first, first + count) removed
    // with every edge that touches them
    void reset();
    void rmNodes(index_t first, index_t count = 1);
private:
    int dim_;
    index_t n_;
    const double *dev_sites_ = nullptr;
    std::vector<double> sites_;  // dim x n column-major
    std::vector<int32_t> e_rowptr_;
    std::vector<uint32_t> e_col_;
    std::vector<float> e_val_;
    std::vector<int32_t> r_rowptr_;
    std::vector<uint32_t> r_col_;
    std::vector<uint32_t> r_units_;
    friend class CleanedGraph;
};

// SequenceGraph (SequenceGraph.h:101-121)
Graph SequenceGraph(const Alphabet &a, const sequence_t &seq);
Graph SequenceGraphFromProfile(int dim, index_t nnodes, const std::vector<double> &sites);  // :111-121

// CleanedGraph (CleanedGraph.h:39-160)
class CleanedGraph : public Graph {
public:
    explicit CleanedGraph(const Graph &original);
    index_t getMapping(index_t i) const { return outmapping_[i]; }
    const index_t *nodeMap() const { return outmapping_.data(); }   // node of the cleaned graph -> node of the original
    index_t originalSize() const { return original_size_; }         // nodes of the original (columns of its profile matrix)
    void uncleanMapping(std::vector<index_t> &mapping) const;
private:
    std::vector<index_t> outmapping_;
    index_t original_size_ = 0;
};

// ---------------------------------------------------------------------------------------
// GraphAlign.h
struct AlignmentResult {   // GraphAlign.h:6-12
    dp_score_t score = 0;
    index_t n_tr_indels = 0;
    std::vector<index_t> mapping1, mapping2;
};
struct AncestralResult {   // GraphAlign.h:14-20
    Graph graph;
    std::vector<index_t> mapping1, mapping2;
    std::vector<bool> is_matched;
};
double averageAlignmentLength(const Graph &g);                                        // :82-96
pgm_scores DynProgScores(const Graph &g1, const Graph &g2, const Model &model);       // :98-143

// Environment switches of the host side, read ONCE per process (host_switches()): which path runs is decided at start-up and shown by
// `pgmsa --stats` ("switches"), not re-read per pass.  All of them are test / measurement aids; the defaults are the product.
struct HostSwitches {
    bool profile = false;        // PGM_HOST_PROFILE: per-stage timings on stderr
    bool host_merge = false;     // PGM_HOST_MERGE: the node profiles of mergeGraphs on the host instead of pgm_merge_profiles_batch (same bits)
    bool no_resident = false;    // PGM_NO_RESIDENT: merged profiles travel through the host between the levels
    bool host_counts = false;    // PGM_HOST_COUNTS: pair counts of an alignment on the host instead of pgm_prealigned_counts (same integers)
    bool device_mldist = false;  // PGM_DEVICE_MLDIST: ML distances by pgm_mldist_batch (last-bit differences to the host's estimator)
    bool device_bionj = false;   // PGM_DEVICE_BIONJ: the joins of every guide tree of 4 taxa and more by pgm_bionj_multi (same bits)
    bool host_bionj = false;     // PGM_HOST_BIONJ: the joins of every guide tree by the host loop
    bool host_transfer = false;    // PGM_HOST_TRANSFER: the transfer indices of --bootstrap_tbe and the counts of --bootstrap_taxa by the host loop (same integers)
    bool device_transfer = false;  // PGM_DEVICE_TRANSFER: ... by pgm_transfer_min / pgm_transfer_taxa at every size
    bool host_treelik = false;     // PGM_HOST_TREELIK: the likelihood evaluations of --ml_tree by the host loop (same bits)
    bool device_treelik = false;   // PGM_DEVICE_TREELIK: ... by pgm_tree_likelihood at every size
    std::string describe() const;   // the switches that are on, comma separated ("" = the product's defaults)
};
const HostSwitches &host_switches();

// Backend = the C ABI entry points of include/pgm_hip.h behind a context.  The product binds
// them to libpgm_hip.so (HIP kernels); tests bind the oracle.  There is no CPU fallback: when
// the HIP library cannot create a context this throws.
struct Backend {
    virtual ~Backend() {}
    virtual const char *name() const = 0;
    // Every batch call takes the worker (device context) it runs on, 0 <= worker < workers(); calls with different workers may
    // run concurrently.  The host code shards a batch's independent units over the workers (farm_shards below): jobs of a
    // guide-tree level, leaves, merges, sequence pairs — no exchange between workers, results independent of their number.
    // res1 / res2 (may be NULL): graphs whose profiles the device already holds (include/pgm_hip.h: pgm_site_ref)
    virtual void align_graphs_batch(uint32_t njobs, const pgm_graph *const *g1, const pgm_graph *const *g2,
                                    const pgm_model *const *model, const pgm_scores *scores,
                                    pgm_align_out *out, int worker = 0, const pgm_site_ref *res1 = nullptr, const pgm_site_ref *res2 = nullptr) = 0;
    // the merged graphs' profiles may stay on the device between the levels of a progressive pass (one context, nobody reads
    // them on the host): merge_profiles_batch_res leaves them there and returns their device addresses
    virtual bool resident() const { return false; }
    virtual bool resident_onehot(uint32_t, uint32_t, const int8_t *, const uint32_t *, const double **, int = 0) { return false; }   // leaf graphs built on the device
    virtual void resident_reset() {}   // start of a progressive pass: the previous pass's device-resident profiles are dead
    virtual bool merge_profiles_batch_res(uint32_t, const pgm_merge_job *, const double **, int = 0) { return false; }
    // a resident matrix of worker `src` copied to worker `dst` (a pass sharded by subtree: the parent of two subtrees needs both children's
    // profiles where it runs); the address on `dst`, valid like every resident address until resident_reset
    virtual const double *resident_import(int /*dst*/, int /*src*/, const double *, size_t /*count*/) { return nullptr; }
    // One tile of alignPair jobs in two halves (include/pgm_hip.h: pgm_nw_pairs_submit / pgm_nw_pairs_wait): a worker keeps two
    // tiles in flight.  flags & PGM_NW_REDUCED: counts = (ident, total) per pair.  Result buffers come from host_alloc.
    virtual int nw_pairs_submit(uint32_t dim, const int32_t *score, int32_t go, int32_t ge, uint32_t nseq,
                                const int8_t *syms, const uint32_t *offs, uint32_t npairs, const uint32_t *pi,
                                const uint32_t *pj, uint32_t flags, int32_t *counts, uint32_t *gaps, int worker = 0) = 0;
    virtual void nw_pairs_wait(int ticket, int worker = 0) = 0;
    virtual void *host_alloc(size_t bytes) { return malloc(bytes); }
    virtual void host_free(void *p) { free(p); }
    // number of device contexts the farms may drive, one host thread each
    virtual int workers() const { return 1; }
    // batched DistanceFactoryML::computeDistance and the pair counts of an alignment on the device;
    // false = this backend has no such kernel (the host estimator is used)
    virtual bool mldist_batch(const pgm_mldist_model &, uint32_t, const int32_t *, const uint32_t *, const double *, double *, double *, int = 0) { return false; }
    // mldist_batch also takes a model in general form (Q alone, V == Vi == sigma == NULL, dim <= 64: the codon model, a generator
    // that is not reversible); false = eigen form with dim <= 20 only, the host estimator keeps the other models
    virtual bool mldist_general() const { return false; }
    uint64_t mldist_device_pairs = 0;     // pairs whose estimate came from mldist_batch (--stats, with PGM_DEVICE_MLDIST)
    double mldist_kernel_ms = 0;          // device time of their kernels
    virtual bool prealigned_counts_batch(uint32_t, uint32_t, uint32_t, const int8_t *, uint32_t, const uint32_t *, const uint32_t *, int32_t *, uint32_t *, int = 0) { return false; }
    // cosine matrix of the k-mer count vectors (DistanceFactoryAngle.h:100): counts nseq x ncols row-major -> nseq x nseq column-major
    virtual void kmer_cosine(uint32_t nseq, uint32_t ncols, const int32_t *counts, double *cosine, int worker = 0) = 0;
    // The two stages above for many families in one call (--batch; include/pgm_hip.h: pgm_kmer_cosine_multi,
    // pgm_prealigned_counts_multi).  counts: the families' count rows back to back, cosine: their nseq_f x nseq_f column-major blocks
    // back to back.  rows: every family's nrows_f x ncols_f matrix back to back; pair p compares rows pi[p], pj[p] of family fam[p].
    // The defaults loop over the families through the per-family entries above: a backend without kernels of its own computes
    // the same values one family at a time.
    virtual void kmer_cosine_multi(uint32_t nfam, const uint32_t *nseq, uint32_t ncols, const int32_t *counts, double *cosine, int worker = 0);
    virtual bool prealigned_counts_multi(uint32_t dim, uint32_t nfam, const uint32_t *nrows, const uint32_t *ncols, const int8_t *rows, uint32_t npairs,
                                         const uint32_t *fam, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker = 0);
    // The pair counts of nrep resamplings of the columns of one alignment in one call (--bootstrap; include/pgm_hip.h:
    // pgm_prealigned_counts_resampled): replicate r is the matrix whose column k is column cols[r * ncols + k] of rows; counts and gaps
    // hold the replicates' results back to back, each laid out as prealigned_counts_batch lays them out.  The default gathers every
    // replicate's matrix on the host and hands it to prealigned_counts_batch: a backend without a kernel of its own computes the same
    // integers one replicate at a time (false where it has no pair-count entry at all).
    virtual bool prealigned_counts_resampled(uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows, uint32_t nrep, const uint32_t *cols,
                                             uint32_t npairs, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker = 0);
    // The residue-pair agreement counts of --guidance (include/pgm_hip.h: pgm_msa_agreement): where is nrep x nrows x ncols, res_hits
    // nrows x ncols and pair_hits nrows x nrows are overwritten.  The default is the host statement, msa_agreement_host.
    virtual void msa_agreement(uint32_t nrows, uint32_t ncols, uint32_t nrep, const int32_t *where, uint32_t *res_hits, uint32_t *pair_hits, int worker = 0);
    // The transfer indices of --bootstrap_tbe (include/pgm_hip.h: pgm_transfer_min): phi[e * nrep + r] of reference set e against the
    // sets of replicate r, overwritten.  The default is the host statement, transfer_min_host.
    virtual void transfer_min(uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep, uint32_t *phi,
                              int worker = 0);
    // The moved-taxon counts of --bootstrap_taxa (include/pgm_hip.h: pgm_transfer_taxa): phi, arg (nref x nrep), moved (nref x nleaves)
    // and counted (nref), overwritten.  The default is the host statement, transfer_taxa_host.
    virtual void transfer_taxa(uint32_t nleaves, uint32_t nref, const uint64_t *ref, const uint32_t *thr, uint32_t nrep, const uint32_t *rep_off,
                               const uint64_t *rep, uint32_t *phi, uint32_t *arg, uint32_t *moved, uint32_t *counted, int worker = 0);
    // The site likelihoods of an alignment on a rooted tree and the derivatives of lnL by every branch length (--ml_tree;
    // include/pgm_hip.h: pgm_tree_likelihood).  The default is the host statement, tree_likelihood_host: the same bits.
    virtual void tree_likelihood(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                 const double *P, int derivs, double *site_l, int32_t *site_k, double *d1, double *d2, int worker = 0);
    // The same under a mixture of rate categories (--ml_gamma; include/pgm_hip.h: pgm_tree_likelihood_rates).  The default is the host
    // statement, tree_likelihood_rates_host: the same bits.
    virtual void tree_likelihood_rates(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                       uint32_t ncat, const double *w, const double *P, int derivs, double *site_l, int32_t *site_k, double *post, double *d1, double *d2,
                                       int worker = 0);
    // The marginal ancestral states of every inner node under the same mixture (--ml_ancestral; include/pgm_hip.h: pgm_tree_ancestral).
    // The default is the host statement, tree_ancestral_host: the same bits.
    virtual void tree_ancestral(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                uint32_t ncat, const double *w, const double *P, double *site_l, int32_t *site_k, double *post, int8_t *anc_state, double *anc_prob,
                                double *anc_post, int worker = 0);
    // The jointly most probable states of the inner nodes under the column's most probable category (--ml_ancestral_joint;
    // include/pgm_hip.h: pgm_tree_ancestral_joint).  The default is the host statement, tree_ancestral_joint_host: the same bits.
    virtual void tree_ancestral_joint(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                      uint32_t ncat, const double *w, const double *P, double *site_l, int32_t *site_k, double *post, uint8_t *cat, int8_t *joint_state,
                                      double *joint_l, int32_t *joint_k, int worker = 0);
    // nsamp draws of (category, every inner state) from their posterior at every column (--ml_ancestral_samples; include/pgm_hip.h:
    // pgm_tree_ancestral_sample).  The default is the host statement, tree_ancestral_sample_host: the same bytes.
    virtual void tree_ancestral_sample(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi,
                                       uint32_t ncat, const double *w, const double *P, uint32_t nsamp, uint64_t first_sample, uint64_t seed, double *site_l,
                                       int32_t *site_k, double *post, uint8_t *samp_cat, int8_t *samp_state, int worker = 0);
    // The likelihood ratio of every nearest-neighbour interchange at every column (--ml_search; include/pgm_hip.h: pgm_tree_nni).  The
    // default is the host statement, tree_nni_host: the same bits.
    virtual void tree_nni(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                          const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, double *site_l,
                          int32_t *site_k, double *post, double *rho, int worker = 0);
    // The same with the candidates' own matrices of the edge above v, and the derivatives of every neighbour's lnL by that edge's length
    // (--ml_nni_opt; include/pgm_hip.h: pgm_tree_nni_edge).  The default is the host statement, tree_nni_edge_host: the same bits.
    virtual void tree_nni_edge(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                               const double *w, const double *P, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_a, const uint32_t *cand_c, const double *Pc,
                               double *site_l, int32_t *site_k, double *post, double *rho, double *d1, double *d2, int worker = 0);
    // The likelihood ratio of every subtree pruning and regrafting at every column (--ml_spr; include/pgm_hip.h: pgm_tree_spr).  The
    // default is the host statement, tree_spr_host: the same bits.
    virtual void tree_spr(uint32_t dim, uint32_t nleaves, uint32_t nnodes, const uint32_t *parent, uint32_t ncols, const int8_t *rows, const double *pi, uint32_t ncat,
                          const double *w, const double *P, const double *Ph, uint32_t ncand, const uint32_t *cand_v, const uint32_t *cand_y, double *site_l,
                          int32_t *site_k, double *post, double *rho, int worker = 0);
    // The sums of every row of x over nrep resamplings of its columns (--ml_support; include/pgm_hip.h: pgm_resampled_sums).  The
    // default is the host statement, resampled_sums_host: the same bits.
    virtual void resampled_sums(uint32_t nrow, uint32_t ncols, const double *x, uint32_t nrep, const uint32_t *cols, double *out, int worker = 0);
    // calls the host code made of the align-batch entry and of the distance entries (all-pairs tiles, pair counts, cosine, ML
    // distances): `pgmsa --batch --stats` shows with them that a stage was shared by the families of a chunk
    std::atomic<uint64_t> calls_align{0}, calls_dist{0};
    // the joins of BioNJ for many families in one call (include/pgm_hip.h: pgm_bionj_multi; every n[f] >= 4, every entry finite):
    // the join records and final_d of bionj_joins_host, bit for bit.  false = this backend has no such kernel (the host loop runs)
    virtual bool bionj_multi(uint32_t, const uint32_t *, const double *, const double *, pgm_bionj_join *, double *, int = 0) { return false; }
    // the same with the pair of every join given (pgm_bionj_plan_multi: n[f] - 3 pairs per family): bionj_joins_host with that plan
    virtual bool bionj_plan_multi(uint32_t, const uint32_t *, const double *, const double *, const pgm_bionj_pair *, pgm_bionj_join *, double *, int = 0) { return false; }
    double seconds_bionj = 0;                                // host wall of the joins of all guide trees, either path (--stats)
    uint64_t bionj_device_calls = 0, bionj_launches = 0;     // bionj_multi / bionj_plan_multi calls that ran on the device, the kernels they launched
    // node profiles of a batch of merged graphs on the device (numeric part); false = host arithmetic
    virtual bool merge_profiles_batch(uint32_t, const pgm_merge_job *, int = 0) { return false; }
    double seconds_merge_profiles = 0;
    // the root search (FindRoot.h, GapParsimony.h): gap masks carried through a height's merges, and the gap parsimony scores of
    // the candidate alignments (include/pgm_hip.h); false = this backend has no such kernel (the host's own code runs)
    virtual bool gapmask_extend_batch(uint32_t, const pgm_gapmask_job *, int = 0) { return false; }
    virtual bool gap_parsimony_batch(uint32_t, const pgm_parsimony_job *, uint32_t *, int = 0) { return false; }
    // the weighted least-squares refinement of a guide tree (LeastSquares.cpp): the n x n distance and weight matrices are
    // loaded once per refined tree, then the subtree pair sums of many edges (include/pgm_hip.h: pgm_wls_pair_sums_batch).  The
    // defaults are the host's own statement of the kernels' summation order (wls_pair_sums_host): the same bits.
    virtual void wls_load(uint32_t n, const double *D, const double *W, int worker = 0);
    virtual void wls_pair_sums_batch(uint32_t njobs, const pgm_wls_job *jobs, double *out, int worker = 0);
    uint64_t wls_launches = 0;   // kernels the pair sums launched (0 for the host defaults)
    double seconds_wls_kernels = 0;
    virtual void csprofile_create_batch(const class CSProfile &lib, uint32_t nseq, const int8_t *syms, const uint32_t *offs,
                                        const double *tau, const double *pi, const double *p_uniform, double *out,
                                        const uint64_t *out_offs, int worker = 0) = 0;
    // the profile library handed to every worker ahead of the first createProfile batch (start-up: before the clocks of the stages)
    virtual void csprofile_preload(const class CSProfile &) {}
    // ... left on the device of `worker` (resident pass): dev[s] = the 20 x (len + 2) matrix of sequence s; false = not available
    virtual bool csprofile_create_batch_res(const class CSProfile &, uint32_t, const int8_t *, const uint32_t *, const double *, const double *,
                                            const double *, const double **, int = 0) { return false; }
    std::vector<double> wls_D, wls_W;   // the host defaults' copy of the loaded matrices
    uint32_t wls_n = 0;
    int farm_workers = 0, farm_tiles = 0;   // what the last all-pairs farm used (logs / --stats)
    int farm_level_workers = 0, farm_leaf_workers = 0;   // most workers a guide-tree level's jobs / the leaves' profiles were dealt to
    bool resident_pass = false; int resident_imports = 0;   // the last progressive pass kept its profiles on the devices; matrices copied between them
    uint64_t cells_aligned = 0;   // Σ (n1-2)(n2-2)
    uint64_t cells_nw = 0;        // Σ L1*L2
    double seconds_align = 0, seconds_nw = 0, seconds_mldist = 0;
};
Backend &default_backend();            // defined by exactly one backend_*.cpp linked into the program
// Units of a batch dealt to `nw` workers: longest first, each to the worker with the least load so far (ties: the lowest
// worker).  Deterministic; shard w lists its units in descending cost.  With one worker or one unit: everything to worker 0.
std::vector<std::vector<uint32_t>> farm_shards(const std::vector<uint64_t> &cost, int nw);
// runs fn(w) for every non-empty shard, worker 0 on the calling thread, the others on threads of their own
void farm_run(const std::vector<std::vector<uint32_t>> &shards, const std::function<void(int)> &fn);
// the entries of a batch's array that belong to shard `sh`, in the shard's order
template <class T> std::vector<T> shard_pick(const std::vector<T> &v, const std::vector<uint32_t> &sh) {
    std::vector<T> q(sh.size());
    for (size_t k = 0; k < sh.size(); ++k) q[k] = v[sh[k]];
    return q;
}
void set_job_dump(const std::string &path);  // if set, every alignGraphs job is appended to this file
bool job_dump_active();
void set_dist_dump(const std::string &path); // if set, every distance matrix TreeNJ estimates is appended (dim, D, V as raw doubles)
void set_joins_dump(const std::string &path); // if set, the join record of every guide tree is appended (n, n - 3 joins, the 9 doubles of final_d)

// alignGraphs (GraphAlign.h:200-534): one job; and the batched form the scheduler uses.
AlignmentResult alignGraphs(const Graph &g1, const Graph &g2, const Model &model);
// (res1 / res2: per job, where the device holds the graphs' profiles — empty vectors or entries with dev_sites == NULL: nowhere)
std::vector<AlignmentResult> alignGraphsBatch(const std::vector<const Graph *> &g1,
                                              const std::vector<const Graph *> &g2,
                                              const std::vector<const Model *> &model,
                                              const std::vector<pgm_site_ref> &res1 = std::vector<pgm_site_ref>(),
                                              const std::vector<pgm_site_ref> &res2 = std::vector<pgm_site_ref>(),
                                              const std::vector<int> *worker_of = nullptr);   // (given: job k runs on worker (*worker_of)[k] — where its profiles are)
// mergeGraphs (GraphAlign.h:550-727)
// mergeGraphs in three parts, so that the profiles of all merges of a guide-tree level can be computed in one device batch:
//   planMerge     the "unify" walk over the two mappings (GraphAlign.h:569-620 without the arithmetic): per node of the
//                 merged graph its source nodes, whether a skipped g2 node is propagated with model1.P (:591), is_matched
//   merge profiles  host: mergeProfilesHost; device: Backend::merge_profiles_batch (bit-identical)
//   finishMerge   homologous path, inverse mappings, penalties, edge maps, Graph (:626-727)
struct MergePlan {
    std::vector<index_t> mapping1, mapping2;   // result.mapping1 / mapping2 (PGM_GAP = none)
    std::vector<bool> is_matched;
    std::vector<uint8_t> g2_with_P1;
};
MergePlan planMerge(const Graph &g1, const Graph &g2, const std::vector<index_t> &mapping1, const std::vector<index_t> &mapping2);
void mergeProfilesHost(const Graph &g1, const Graph &g2, const Model &model1, const Model &model2, const MergePlan &plan,
                       std::vector<double> &profiles);   // dim x nnodes column-major
AncestralResult finishMerge(const Graph &g1, const Graph &g2, const MergePlan &plan, const double *profiles /* NULL: they stay on the device */,
                            double support1, double support2);
AncestralResult mergeGraphs(const Graph &g1, const Graph &g2, const std::vector<index_t> &mapping1,
                            const std::vector<index_t> &mapping2, const Model &model1, const Model &model2,
                            double support1, double support2);
// GraphAlign.h:729-882: the graph of an early refinement grows by one aligned descendant at a time (one model, no penalties)
AncestralResult mergeGraphsIncremental(const Graph &anc_graph, const Graph &graph, const std::vector<index_t> &anc_mapping,
                                       const std::vector<index_t> &mapping, const Model &model);

// ---------------------------------------------------------------------------------------
// PhyTree (PhyTree.h) + newick (newick.cpp)
class PhyTree {
public:
    explicit PhyTree(std::string name = "") : parent_(nullptr), branch_length_(0), branch_support_(1), name_(std::move(name)) {}
    ~PhyTree();
    PhyTree(const PhyTree &) = delete;
    PhyTree *copy() const;
    void addChild(PhyTree *child, double branch_length = 0, double branch_support = 1);
    void pluck();
    PhyTree *pluckChild(index_t index);
    index_t indexOf() const;
    const std::string &getName() const { return name_; }
    PhyTree *getParent() { return parent_; }
    double getBranchLength() const { return branch_length_; }
    double getBranchSupport() const { return branch_support_; }
    PhyTree &operator[](int i) { return *children_[i]; }
    const PhyTree &operator[](int i) const { return *children_[i]; }
    index_t n_children() const { return (index_t)children_.size(); }
    bool isLeaf() const { return children_.empty(); }
    std::string formatNewick() const;
    // the same text with labels[node] printed between ')' and ':' for every internal node that has one (--bootstrap_out), the root's
    // between ')' and ';' (--ml_ancestral_tree; the labels of the bootstrap outputs hold no root)
    std::string formatNewick(const std::map<const PhyTree *, uint32_t> &labels) const;
    std::string formatNewick(const std::map<const PhyTree *, std::string> &labels) const;   // (--bootstrap_tbe: labels as text)
private:
    std::string formatNewickR(const std::map<const PhyTree *, std::string> *labels) const;
    std::string formatNewickR() const;
    std::vector<PhyTree *> children_;
    PhyTree *parent_;
    double branch_length_, branch_support_;
    std::string name_;
};
PhyTree *midpointRoot(PhyTree *root);                      // PhyTree.cpp:60-116
// Bootstrap support (--bootstrap): for every internal edge of `tree`, the number of `replicates` whose unrooted tree has the same
// bipartition of the leaves.  A bipartition is a bit set over the leaves in sorted-name order, the side without leaf 0.  The key
// is the node below the edge; the two edges below a bifurcating root are one bipartition and get the same number; an edge that
// cuts off a single leaf (a trivial bipartition: every tree has it) gets no entry.  Every replicate must have the leaves of `tree`;
// where it is rooted, and how many children its root has, does not matter.
std::map<const PhyTree *, uint32_t> bipartition_support(const PhyTree &tree, const std::vector<const PhyTree *> &replicates);
// The walk both support measures share: the leaves of `tree` numbered in sorted-name order, and the non-trivial bipartitions of a
// tree over those leaves in post-order, (node below the edge, canonical side as (nleaves + 63) / 64 little-endian words).
struct LeafNumbering {
    std::map<std::string, size_t> index;
    size_t nleaves = 0, words = 0;
};
LeafNumbering leaf_numbering(const PhyTree &tree);
std::vector<std::pair<const PhyTree *, std::vector<uint64_t>>> bipartitions_of(const LeafNumbering &num, const PhyTree &t);
std::vector<std::string> get_tree_order(const PhyTree *tree);  // PhyTree.cpp:164-182
PhyTree *parse_newick(std::istream &in);                   // newick.cpp:127-147

// Fasta.cpp
std::map<std::string, std::string> read_fasta(const std::string &file, std::vector<std::string> &order);
void write_fasta(const std::map<std::string, std::string> &aln, const std::vector<std::string> &order, std::ostream &out);

// ---------------------------------------------------------------------------------------
// CSProfile (CSProfile.{h,cpp})
class CSProfile {
public:
    explicit CSProfile(const std::string &filename);   // parser CSProfile.cpp:29-170
    int nprof() const { return nprof_; }
    int ncols() const { return ncols_; }
    const std::vector<double> &lprofiles() const { return lprofiles_; }  // [k][col][21]
    const std::vector<double> &centre() const { return centre_; }        // [k][20]
    const std::vector<double> &priors() const { return priors_; }
private:
    int nprof_ = -1, ncols_ = -1;
    std::vector<double> lprofiles_, centre_, priors_;
};

// ---------------------------------------------------------------------------------------
// ProgressiveAlignment.{h,cpp}
struct Profile { int dim = 0; index_t cols = 0; std::vector<double> data; };   // Model<A>::Profile: dim x cols, column-major
struct repeat_t { index_t len = 0, start = 0; std::vector<int> tr_hom; };        // Repeat.h
// --read_repeats: T-REKS output (RepeatDetectionTReks.cpp:62-157; repeats.cpp) against the (start / stop stripped) sequences
std::map<std::string, std::vector<repeat_t>> read_repeats(const Alphabet &a, const std::string &filename, const std::map<std::string, sequence_t> &seqs);
struct ProgressiveAlignmentResult {   // ProgressiveAlignment.h:27-37
    std::map<std::string, sequence_t> aligned_sequences;
    std::map<std::string, Profile> profiles;   // leaves always; ancestors with --ancestral_seqs (:73, :362, :410)
    std::vector<std::vector<int>> tr_homologies;   // per annotated repeat: unit column of every node of the graph (without START / END), -1 elsewhere
    std::vector<std::string> tr_source;
    Graph graph;
    score_t score = 0;
    index_t n_tr_indels = 0;
    bool is_csprofile = false;
};
// fn(0..n-1) on the host threads (PGM_HOST_THREADS, at most 16); exceptions are rethrown on the caller (host_threads.cpp)
void parallel_for(size_t n, const std::function<void(size_t)> &fn);

// progressive_alignment (ProgressiveAlignment.cpp:12-71): same post-order results as the reference's
// recursion; internal nodes whose children are finished are aligned together in one batch:
// align_progressive_results (ProgressiveAlignment.h:413-476) for a whole guide-tree level at once.
ProgressiveAlignmentResult progressive_alignment(const Alphabet &a, const std::map<std::string, sequence_t> &sequences,
                                                 const PhyTree &tree, const CSProfile *csprofile,
                                                 const ModelFactory &model_factory,
                                                 const std::map<std::string, std::vector<repeat_t>> *repeats = nullptr);
// The same pass over many guide trees at once (--batch): the nodes of all trees in one set, one batch per height.  Per family the
// sequences, the tree, the model factory (-F estimates the frequencies per family) and where the result goes; the alphabet and the
// profile library are the run's.  `worker`: the device context the family's nodes run on (a family never spans contexts).
// `error`: set by the pass for a family whose tree cannot be used (the message the solo pass throws); that family gets no result.
// progressive_alignment is this pass for one tree.
struct ForestFamily {
    const std::map<std::string, sequence_t> *sequences = nullptr;
    const PhyTree *tree = nullptr;
    const ModelFactory *model_factory = nullptr;
    const std::map<std::string, std::vector<repeat_t>> *repeats = nullptr;
    ProgressiveAlignmentResult *result = nullptr;
    int worker = 0;
    std::string error;
};
void progressive_alignment_forest(const Alphabet &a, std::vector<ForestFamily> &families, const CSProfile *csprofile);
struct BatchStats {   // `pgmsa --batch --stats`
    int families = 0, failed = 0, chunks = 0;
    uint64_t passes = 0, levels = 0;   // forest passes; run_level calls of all passes
};
extern BatchStats batch_stats;
// progressive_alignment_find_root (FindRoot.h:236-336): the alignment of the guide tree rerooted on the branch of the lowest gap
// parsimony score, every branch (cmdlineopts.reroot_flag == 1) or a hill climb over neighbouring branches; prints the score.
// The directed subtree merges of all candidates run as one DAG, height by height, through the level machinery of the plain pass.
struct RootSearchStats {
    bool ran = false;
    int merges = 0, candidates = 0, heights = 0, batches = 0;
    double align_s = 0, host_merge_s = 0, gapmask_s = 0, parsimony_s = 0, select_s = 0;
    uint64_t cells = 0;
};
extern RootSearchStats root_search_stats;
ProgressiveAlignmentResult progressive_alignment_find_root(const Alphabet &a, const std::map<std::string, sequence_t> &sequences,
                                                           const PhyTree &tree, const ModelFactory &model_factory,
                                                           const std::map<std::string, std::vector<repeat_t>> *repeats = nullptr);

// ---------------------------------------------------------------------------------------
// Distances / guide tree
struct DistanceMatrix {   // DistanceFactory.h:12-18
    int dim;
    std::vector<double> distances, variances;   // dim x dim
    explicit DistanceMatrix(int d) : dim(d), distances((size_t)d * d, 0.0), variances((size_t)d * d, 0.0) {}
    double &D(int i, int j) { return distances[(size_t)i * dim + j]; }
    double &V(int i, int j) { return variances[(size_t)i * dim + j]; }
};
struct distvar_t { distance_t dist, var; };
// the limits of an estimate per alphabet (DistanceFactoryML.cpp:5-32): what computeDistance clamps to, and pgm_mldist_batch with it
void mldist_limits(const Alphabet &a, double &DIST_MAX, double &VAR_MAX, double &VAR_MIN);
class DistanceFactoryML {   // DistanceFactoryML.h
public:
    DistanceFactoryML(const Alphabet &a, const ModelFactory *mf) : alphabet(a), model_factory(mf) {}
    distvar_t computeDistance(const std::vector<int32_t> &counts, index_t gaps, double seqlen) const;  // :137-190
    distvar_t computeDistance(double ident, double total, const std::vector<int32_t> *counts, index_t gaps, double seqlen) const;
protected:
    distvar_t computeMLDist(const std::vector<int32_t> &counts, index_t gaps, double seqlen, double dist0, double var0) const;  // :66-135
    Alphabet alphabet;
    const ModelFactory *model_factory;
};
class DistanceFactoryAlign : public DistanceFactoryML {   // DistanceFactoryAlign.h: the scores of alignPair (the farm itself: distance.cpp)
public:
    DistanceFactoryAlign(const Alphabet &a, const ModelFactory *mf);
    const std::vector<int32_t> &scoring_matrix() const { return scoring_matrix_; }
    int gap_open = -10, gap_extend = -2;
private:
    std::vector<int32_t> scoring_matrix_;   // (DIM+1)^2 column-major
};
// TreeNJ.cpp:132-281; topo: the tree keeps this topology (--topology) and only its branch lengths are estimated
PhyTree *buildNJTree(std::vector<std::string> seqs_order, DistanceMatrix dist, const PhyTree *topo = nullptr);
// buildNJTree in two parts: the joins (the O(n^3) loop; pgm_bionj_multi computes the same record on the device) and the tree of
// a join record.  final_d: the 3 x 3 row-major D of the clusters left (of all min(n, 3) clusters when n < 4).
// plan: the pairs to join, one per join while it has entries (build_topo_plan; a join is then O(n): two column sums, no scan;
// pgm_bionj_plan_multi on the device); nullptr: every pair is the criterion's minimum
void bionj_joins_host(DistanceMatrix dist, std::vector<pgm_bionj_join> &joins, double *final_d, const std::vector<pgm_bionj_pair> *plan = nullptr);
// TreeNJ.cpp:31-130: the joins that give the tree over seqs_order the topology `topo`, in the reference's order; leaves of topo
// that are no sequence are pruned; throws for a sequence topo does not hold and for a node that has not two children
std::vector<pgm_bionj_pair> build_topo_plan(const std::vector<std::string> &seqs_order, const PhyTree *topo);
PhyTree *bionj_tree(std::vector<std::string> seqs_order, const std::vector<pgm_bionj_join> &joins, const double *final_d);
// the support of an edge of length d, 1 - 2^(-d / edge_halflife) within [0, 1] (TreeNJ.cpp:22-29, LeastSquares.cpp:16-23)
double edge_support(double d);
// The joins of the families whose matrices are `dist` (nseq[f] taxa each; plan_of(f): the pairs a fixed topology prescribes, or
// nullptr) in one device call or by bionj_joins_host per family: joins[f], final_d[9 f ..] and the message of a family that failed
void bionj_joins_families(std::vector<DistanceMatrix> &dist, const std::vector<uint32_t> &nseq,
                          const std::function<const std::vector<pgm_bionj_pair> *(uint32_t)> &plan_of, std::vector<std::vector<pgm_bionj_join>> &joins,
                          std::vector<double> &final_d, std::vector<std::string> &join_error);
// families of this many taxa and more go to the device by default: the smallest measured size from which the device's joins
// took less time than the host's at every larger size
const uint32_t kBionjDeviceMin = 256;
// LeastSquares::refineTree (LeastSquares.cpp:661-710; TreeNJ.h:52-54 when -W is given): nearest-neighbour interchanges by weighted
// least squares on the unrooted tree, quartets (and with -WW quintets) swept until the fit stops falling, then every edge's support
struct WlsStats {
    int trees = 0, sweeps = 0;
    uint64_t quartets = 0, quintets = 0, batches = 0;
    double seconds = 0, pair_sums_s = 0;
};
extern WlsStats wls_stats;
PhyTree *refineTree(PhyTree *tree, const std::vector<std::string> &leaf_order, const DistanceMatrix &dist);
// the pair sums of pgm_wls_pair_sums_batch in the kernels' order (D, W: n x n row-major)
void wls_pair_sums_host(uint32_t n, const double *D, const double *W, uint32_t njobs, const pgm_wls_job *jobs, double *out);
// TreeNJ.h:27-59: distances from the k-mer count vectors (DistanceFactoryAngle.h:55-131, the default), from an all-pairs alignment
// (-a; both prealigned == false) or induced by an existing alignment (prealigned == true, the guide-tree re-estimation of
// main.cpp:404-430), the estimate of every pair on the host threads or, with PGM_DEVICE_MLDIST, on the device for the models the
// backend's kernels take; then BioNJ, with -W the least-squares refinement, and the midpoint rooting.
// topo (--topology): BioNJ joins the pairs this topology prescribes and estimates the branch lengths only.
PhyTree *TreeNJ(const Alphabet &a, const std::map<std::string, sequence_t> &seqs, const ModelFactory *mf, bool prealigned = false, const PhyTree *topo = nullptr);

// TreeNJ for the families of a --batch chunk.  Both are one implementation over a list of families (TreeNJ: a list of one), so every
// family's tree is the one TreeNJ gives it alone; the distance stage runs once for all families (one farm of all-pairs tiles over the
// concatenated sequences; one cosine call or one pair-count call where TreeNJ makes the per-family calls), BioNJ and the rooting per
// family on the host threads.  `error`: the message TreeNJ throws for this family.
struct TreeJob {
    const std::map<std::string, sequence_t> *seqs = nullptr;
    const ModelFactory *model_factory = nullptr;
    const PhyTree *topo = nullptr;   // the family's fixed topology, if it has one
    PhyTree *tree = nullptr;
    std::string error;
};
void TreeNJ_multi(const Alphabet &a, std::vector<TreeJob> &jobs, bool prealigned = false);

// --bootstrap: nrep resamplings of the columns of an alignment (rows: its sequences, all of one length, at least 4) and the
// unrooted BioNJ tree of each.  Replicate r draws ncols source columns cols[r][c] = splitmix64() % ncols, c ascending, replicates
// in order, from one stream seeded with `seed`.  The pair counts of every replicate come from Backend::prealigned_counts_resampled,
// in groups of replicates whose counts stay within kBootstrapCountBytes per call; the estimator and the joins are those of TreeNJ
// (prealigned == true) without -W and without rooting.  The caller owns the trees.
// bootstrap_columns: those columns, nrep x ncols: what bootstrap_trees and --ml_support both draw.
inline uint64_t splitmix64(uint64_t &state) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline std::vector<uint32_t> bootstrap_columns(uint32_t nrep, uint32_t ncols, uint64_t seed) {
    std::vector<uint32_t> cols((size_t)nrep * ncols);
    uint64_t state = seed;
    for (size_t k = 0; k < cols.size(); ++k) cols[k] = (uint32_t)(splitmix64(state) % ncols);
    return cols;
}
const size_t kBootstrapCountBytes = (size_t)1 << 30;   // count output of one prealigned_counts_resampled call
struct BootstrapStats {   // `pgmsa --bootstrap --stats`
    int replicates = 0;
    double seconds = 0;
    uint64_t counts_calls = 0;
};
extern BootstrapStats bootstrap_stats;
std::vector<PhyTree *> bootstrap_trees(const Alphabet &a, const std::map<std::string, sequence_t> &rows, const ModelFactory *mf, uint32_t nrep, uint64_t seed);

// --guidance: how often the residue pairs of the base alignment stand in one column again in the alignments of N bootstrap guide
// trees (host/guidance.cpp; the flow is doGuidance in driver_analyses.cpp).
// guidance_where: one replicate's residue map, where[i * ncols + c] = the column of `rep` that holds the residue row i of `base`
//   has in column c, -1 for a gap (rows as written, one symbol a column; both alignments hold the same residues in the same order).
// msa_agreement_host: the counts of pgm_msa_agreement by plain loops on the host threads (Backend::msa_agreement's default).
// guidance_call_replicates: the most replicates one agreement call takes for `where` to stay within where_bytes and for the sums
//   to fit 32 bits (nrep * (nrows - 1), nrep * ncols), at least 1.
// format_newick_exact: formatNewick()'s text with every branch length printed with %.17g (reading it back gives the same doubles).
// guidance_write: the two score files from the summed counts; where0 is any replicate's map (only its gaps are read).
const size_t kGuidanceWhereBytes = (size_t)1 << 30;   // `where` of one msa_agreement call
struct GuidanceStats {   // `pgmsa --guidance --stats`
    int replicates = 0;
    double seconds = 0, align_s = 0, agreement_s = 0;
    uint64_t passes = 0, agreement_calls = 0;
};
extern GuidanceStats guidance_stats;
struct GuidanceCounts {
    uint32_t nrows = 0, ncols = 0, nrep = 0;
    std::vector<uint64_t> res_hits, pair_hits;   // nrows x ncols, nrows x nrows
};
void guidance_where(const Alphabet &a, const std::vector<sequence_t> &base, const std::vector<sequence_t> &rep, int32_t *where);
void msa_agreement_host(uint32_t nrows, uint32_t ncols, uint32_t nrep, const int32_t *where, uint32_t *res_hits, uint32_t *pair_hits);
uint32_t guidance_call_replicates(uint32_t nrows, uint32_t ncols, size_t where_bytes = kGuidanceWhereBytes);
std::string format_newick_exact(const PhyTree &tree);
void guidance_write(const GuidanceCounts &g, const std::vector<std::string> &names, const int32_t *where0, uint64_t seed, std::ostream &out, std::ostream *residues);

// --bootstrap_tbe: the transfer bootstrap expectation (Lemoine et al. 2018) of every internal edge (host/transfer.cpp).
// transfer_min_host: pgm_transfer_min (include/pgm_hip.h) by plain loops on the host threads, the same contract; what it rejects is
//   an error().  Backend::transfer_min's default.
// transfer_call_replicates: the most replicates of at most max_sets sets each that one call takes for `rep` to stay within
//   rep_bytes and nref * nrep within 32 bits, at least 1.
// transfer_support: per labelled node of `tree` (the nodes bipartition_support labels) S = the sum of its transfer indices over
//   the replicates and p = the smaller side of its bipartition.  be: the backend whose transfer_min runs, nullptr for the host loop.
// transfer_labels: "%.6f" of 1.0 - (double)S / ((double)nrep * (double)(p - 1)) per node.
const size_t kTransferRepBytes = (size_t)1 << 30;   // `rep` of one transfer_min call
// families of this many taxa and more go to the device by default (the smallest measured size at which it is faster)
const uint32_t kTransferDeviceMin = 256;
struct TransferStats {   // `pgmsa --bootstrap_tbe --stats`
    double seconds = 0, kernel_ms = 0;
    uint64_t calls = 0;
};
extern TransferStats transfer_stats;
struct TransferEdge { uint64_t S = 0; uint32_t p = 0; };
void transfer_min_host(uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep, uint32_t *phi);
uint32_t transfer_call_replicates(uint32_t nleaves, uint32_t nref, size_t max_sets, size_t rep_bytes = kTransferRepBytes);
std::map<const PhyTree *, TransferEdge> transfer_support(const PhyTree &tree, const std::vector<const PhyTree *> &replicates, Backend *be = nullptr);
std::map<const PhyTree *, std::string> transfer_labels(const std::map<const PhyTree *, TransferEdge> &support, uint32_t nrep);

// --bootstrap_taxa: the taxon side of the transfer bootstrap, which leaves the transfer indices move (host/transfer.cpp).
// transfer_taxa_host: pgm_transfer_taxa (include/pgm_hip.h) by plain loops on the host threads, the same contract; what it rejects
//   is an error().  Backend::transfer_taxa's default.
// taxa_support: the replicates' sets sorted (as vectors of words) and equal ones dropped, the reference edges that share a
//   bipartition as one row, thr = floor(cutoff * (p - 1)), the replicates in calls of transfer_call_replicates, sums in 64 bits.
//   be: the backend whose transfer_taxa runs, nullptr for the host loop.
// taxa_text, taxa_edges_text: the files of --bootstrap_taxa and --bootstrap_taxa_edges.
const uint32_t kTransferNone = 0xffffffffu;   // PGM_TRANSFER_NONE
extern TransferStats taxa_stats;              // `pgmsa --bootstrap_taxa --stats`
struct TaxaEdge { uint32_t p = 0; uint64_t counted = 0; std::vector<uint64_t> moved; };   // moved: per leaf
struct TaxaSupport {
    std::vector<std::string> names;   // the leaves in sorted-name order
    std::vector<uint64_t> moved;      // per leaf, summed over the distinct bipartitions
    uint64_t counted = 0;             // K: the counted (edge, replicate) pairs of the distinct bipartitions
    size_t edges = 0, replicates = 0; // E: the distinct non-trivial bipartitions of the tree; N
    std::vector<TaxaEdge> nodes;      // per labelled node, in the order of the labels in formatNewick's text
};
void transfer_taxa_host(uint32_t nleaves, uint32_t nref, const uint64_t *ref, const uint32_t *thr, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep,
                        uint32_t *phi, uint32_t *arg, uint32_t *moved, uint32_t *counted);
TaxaSupport taxa_support(const PhyTree &tree, const std::vector<const PhyTree *> &replicates, double cutoff, Backend *be = nullptr);
std::string taxa_text(const TaxaSupport &t, double cutoff);
std::string taxa_edges_text(const TaxaSupport &t);

std::string data_dir();   // directory holding wag.qmat etc.

}  // namespace pgm

#include "treelik.h"   // the --ml_* analyses
#endif
