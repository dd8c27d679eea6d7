// distance.cpp — the distance stages of the guide tree, the guide-tree pipeline over families and the bootstrap driver
// (reference src/TreeNJ.h, DistanceFactory.cpp, DistanceFactoryAngle.h, DistanceFactoryAlign.h, DistanceFactoryPrealigned.h).
// Three stages fill the families' matrices behind the C ABI: the k-mer cosine matrix (the default), the O(L^2) Needleman-Wunsch of
// every pair (-a: alignPair, a farm over the device contexts) and the pair counts of an alignment; the estimate of every pair is
// mldist.cpp's, on the host threads or, with PGM_DEVICE_MLDIST, behind pgm_mldist_batch.
// Then the joins (bionj.cpp), -W (wls.cpp) and the rooting per family: TreeNJ (one family) and TreeNJ_multi (--batch) are one
// implementation.  --bootstrap runs the replicates of an alignment through the same count stage, estimator and joins.
#include "pgm_host.h"
#include <quadmath.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <fstream>
#include <functional>
#include <thread>

namespace pgm {
static std::string g_dist_dump;
void set_dist_dump(const std::string &path) { g_dist_dump = path; }
static void dump_distances(const DistanceMatrix &d) {
    if (g_dist_dump.empty()) return;
    std::ofstream f(g_dist_dump.c_str(), std::ios::binary | std::ios::app);
    const int32_t n = d.dim;
    f.write((const char *)&n, 4);
    f.write((const char *)d.distances.data(), 8 * d.distances.size());
    f.write((const char *)d.variances.data(), 8 * d.variances.size());
}

static std::string g_joins_dump;
void set_joins_dump(const std::string &path) { g_joins_dump = path; }
// (here, with tree_nj, and not in bionj_joins_families: the replicates of --bootstrap go through that, and are not dumped)
static void dump_joins(int32_t n, const std::vector<pgm_bionj_join> &joins, const double *final_d) {
    if (g_joins_dump.empty()) return;
    std::ofstream f(g_joins_dump.c_str(), std::ios::binary | std::ios::app);
    f.write((const char *)&n, 4);
    for (const pgm_bionj_join &j : joins) {
        const int32_t idx[2] = {(int32_t)j.index1, (int32_t)j.index2};
        const double d[2] = {j.dist1, j.dist2};
        f.write((const char *)idx, 8);
        f.write((const char *)d, 16);
    }
    f.write((const char *)final_d, 8 * 9);
}

// ---- distances induced by an alignment (DistanceFactoryPrealigned.h:34-90) -----------------------------------------
// Pair counts over the columns where both rows have a residue (only residues with value() in 0..19, for every alphabet:
// the reference's literal 20), one gap per opening of a run in which exactly one of the two rows has a residue.
// a row of an alignment as the pair-count kernels read it: value() per residue, -1 for a gap, -2 for a residue without a value (and
// for the DNA unknown, value 4: the kernel counts every value below 20)
static void prealigned_row(const Alphabet &alphabet, const sequence_t &row, int8_t *out) {
    const bool dna = alphabet.kind == ALPHA_DNA;
    for (size_t k = 0; k < row.size(); ++k) {
        const int8_t c = row[k];
        const int v = alphabet.isGap(c) ? -1 : alphabet.value(c);
        out[k] = (int8_t)(alphabet.isGap(c) ? -1 : (v < 0 || (dna && v >= alphabet.DIM) ? -2 : v));
    }
}

// the same scan on the host (PGM_HOST_COUNTS, or a backend without the kernel): c is the pair's zeroed D x D count matrix; returns
// the gap openings
static uint32_t prealigned_count_pair(const Alphabet &alphabet, const sequence_t &s1, const sequence_t &s2, int32_t *c) {
    const size_t D = (size_t)alphabet.DIM;
    const int cmax = alphabet.kind == ALPHA_DNA ? (int)D : 20;   // (the DNA unknown is not counted: see the device rows above)
    uint32_t g = 0;
    bool open1 = false, open2 = false;
    for (size_t k = 0; k < s1.size(); ++k) {
        const bool g1 = alphabet.isGap(s1[k]), g2 = alphabet.isGap(s2[k]);
        if (!g1 && !g2) {
            const int c1 = alphabet.value(s1[k]), c2 = alphabet.value(s2[k]);
            if (c1 >= 0 && c1 < cmax && c2 >= 0 && c2 < cmax) ++c[(size_t)c1 + D * (size_t)c2];
            open1 = false; open2 = false;
        } else if (g1 && g2) {
            // skip
        } else if (!g1 && !open1) {
            ++g; open1 = true; open2 = false;
        } else if (!g2 && !open2) {
            ++g; open1 = false; open2 = true;
        }
    }
    return g;
}

// K = 2 for amino acids and codons, 6 for DNA (DistanceFactory.cpp:9-60): ncols = D^K = 400, 3721, 4096
static uint32_t angle_ncols(const Alphabet &a) {
    const uint32_t D = (uint32_t)a.DIM, K = a.kind == ALPHA_DNA ? 6u : 2u;
    uint32_t ncols = 1;
    for (uint32_t k = 0; k < K; ++k) ncols *= D;
    return ncols;
}
// DistanceFactoryAngle.h:63-94: the index of the last K values, none of them invalid (counts: one zeroed row of ncols)
static void angle_count_row(const Alphabet &a, const sequence_t &seq, uint32_t ncols, int32_t *counts) {
    const uint32_t D = (uint32_t)a.DIM, K = a.kind == ALPHA_DNA ? 6u : 2u;
    uint32_t index = 0, run = 0;   // (run: valid values at the end of the window so far)
    for (size_t j = 0; j < seq.size(); ++j) {
        const int v = a.value(seq[j]);
        if (v < 0 || v >= (int)D) { run = 0; index = 0; continue; }
        index = (index * D + (uint32_t)v) % ncols;
        if (++run >= K) counts[index] += 1;
    }
}
// from the cosine matrix as kmer_cosine wrote it to the distances and variances (DistanceFactoryAngle.h:100-113); `spread`: the rows
// on the host threads
static void angle_finish(DistanceMatrix &distances, const std::vector<double> &seq_len, bool spread) {
    const uint32_t n = (uint32_t)distances.dim;
    // kmer_cosine writes element (i, j) at i + n j (the reference's column-major matrix); DistanceMatrix::D(i, j) reads i n + j.  The
    // matrix is NOT symmetric in its last bits — ((c_i / |c_i|) . c_j) / |c_j| is rounded differently from the (j, i) element — and
    // BioNJ reads it by rows, by columns and at (index1, index2) / (index2, index1): the orientation has to be the reference's.
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j) std::swap(distances.distances[(size_t)i * n + j], distances.distances[(size_t)j * n + i]);
    const bool ml = cmdlineopts.mldist_flag || cmdlineopts.mldist_gap_flag;
    // log and exp of the reference binary are those of the glibc it is linked with statically (2.17: IBM's correctly rounded ones);
    // today's libm is within 0.52 ulp, which moved the exact final tie of 3 trees in 60.  Correctly rounded here: the long double
    // function when its result is not within 2^-9 ulp of a rounding boundary, binary128 (libquadmath) otherwise.
    auto correctly_rounded = [](long double y, __float128 (*exact)(__float128), double x) {
        const double lo = (double)(y - fabsl(y) * 0x1p-62L), hi = (double)(y + fabsl(y) * 0x1p-62L);
        return lo == hi ? lo : (double)exact((__float128)x);
    };
    auto cr_log = [&](double x) { return correctly_rounded(logl((long double)x), logq, x); };
    auto cr_exp = [&](double x) { return correctly_rounded(expl((long double)x), expq, x); };
    auto row = [&](size_t r) {   // :101-105, row by row
        for (uint32_t c = 0; c < n; ++c) {
            double &d = distances.distances[r * n + c];
            d = -1.0 * cr_log((d * d + 0.4) / 1.4);
            if (!ml) {
                const double e = cr_exp(d);
                d = -0.5 * (5.0 * e - std::sqrt(45.0 * (e * e) - 20.0 * e)) * (1.0 / e);
            }
        }
    };
    if (spread) parallel_for((size_t)n, row);
    else for (size_t r = 0; r < n; ++r) row(r);
    for (uint32_t j = 0; j < n; ++j)   // :107-113: variances = distances / ((len_i + len_j) / 2), at least 1e-5
        for (uint32_t i = 0; i < n; ++i) {
            double v = 1.0 / ((seq_len[j] + seq_len[i]) / 2);
            v *= distances.D((int)i, (int)j);
            distances.V((int)i, (int)j) = std::max(v, 1e-5);
        }
}

// ==== the guide tree: TreeNJ for one family, TreeNJ_multi for the families of a --batch chunk ===========================
// The defaults of the two multi-family entries: the per-family entries, one family after the other (a backend without segmented
// kernels of its own: the CPU oracle).
void Backend::kmer_cosine_multi(uint32_t nfam, const uint32_t *nseq, uint32_t ncols, const int32_t *counts, double *cosine, int worker) {
    size_t row0 = 0, out0 = 0;
    for (uint32_t f = 0; f < nfam; ++f) {
        kmer_cosine(nseq[f], ncols, counts + row0 * ncols, cosine + out0, worker);
        row0 += nseq[f];
        out0 += (size_t)nseq[f] * nseq[f];
    }
}

bool Backend::prealigned_counts_multi(uint32_t dim, uint32_t nfam, const uint32_t *nrows, const uint32_t *ncols, const int8_t *rows, uint32_t npairs,
                                      const uint32_t *fam, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker) {
    std::vector<size_t> base(nfam + 1, 0);
    for (uint32_t f = 0; f < nfam; ++f) base[f + 1] = base[f] + (size_t)nrows[f] * ncols[f];
    std::vector<std::vector<uint32_t>> of_family(nfam);
    for (uint32_t p = 0; p < npairs; ++p) of_family[fam[p]].push_back(p);
    const size_t dd = (size_t)dim * dim;
    for (uint32_t f = 0; f < nfam; ++f) {
        const std::vector<uint32_t> &mine = of_family[f];
        if (mine.empty()) continue;
        const uint32_t m = (uint32_t)mine.size();
        std::vector<uint32_t> qi(m), qj(m), g(m, 0);
        std::vector<int32_t> c((size_t)m * dd, 0);
        for (uint32_t k = 0; k < m; ++k) { qi[k] = pi[mine[k]]; qj[k] = pj[mine[k]]; }
        if (!prealigned_counts_batch(dim, nrows[f], ncols[f], rows + base[f], m, qi.data(), qj.data(), c.data(), g.data(), worker)) return false;
        for (uint32_t k = 0; k < m; ++k) {
            std::copy(c.begin() + (std::ptrdiff_t)(k * dd), c.begin() + (std::ptrdiff_t)((k + 1) * dd), counts + (size_t)mine[k] * dd);
            gaps[mine[k]] = g[k];
        }
    }
    return true;
}

namespace {
// the pairs [p0, p0 + np) of a call's shared pair arrays are those of one family
struct PairBlock {
    const ModelFactory *model_factory;
    size_t p0;
    uint32_t np;
};

// The families of one call.  Their sequences stand one after the other in `seq` (family f: first[f] .. first[f + 1], in std::map key
// order like TreeNJ.h:34-39), their pairs i < j one after the other in pfam / pi / pj (family f: blocks[f]; pi, pj count within the
// family; df[f] estimates them into dist[f]).  One family is the solo run: first[0] = p0 = 0.
struct Families {
    uint32_t nfam = 0;
    std::vector<uint32_t> nseq, first;
    std::vector<const sequence_t *> seq;
    std::vector<std::vector<std::string>> order;
    std::vector<DistanceFactoryML> df;
    std::vector<DistanceMatrix> dist;
    std::vector<uint32_t> pfam, pi, pj;
    std::vector<PairBlock> blocks;
    const sequence_t &row(uint32_t f, uint32_t i) const { return *seq[first[f] + i]; }
    uint32_t np() const { return (uint32_t)pi.size(); }

    // a family joins the call: n taxa without sequences (a replicate of the bootstrap: nothing may read its rows), or its sequences
    uint32_t add_family(const Alphabet &a, const ModelFactory *mf, uint32_t n) {
        nseq.push_back(n); first.push_back((uint32_t)seq.size()); order.emplace_back();
        df.emplace_back(a, mf); dist.emplace_back((int)n); blocks.push_back(PairBlock{mf, 0, 0});
        return nfam++;
    }
    void add_family(const Alphabet &a, const ModelFactory *mf, const std::map<std::string, sequence_t> &seqs) {
        const uint32_t f = add_family(a, mf, (uint32_t)seqs.size());
        for (const auto &kv : seqs) { order[f].push_back(kv.first); seq.push_back(&kv.second); }
    }
    // the pairs of family f, the one added last, where they are given (all_pairs lists them itself)
    void add_pairs(uint32_t f, const std::vector<uint32_t> &qi, const std::vector<uint32_t> &qj) {
        blocks[f].p0 = pi.size(); blocks[f].np = (uint32_t)qi.size();
        pfam.insert(pfam.end(), qi.size(), f); pi.insert(pi.end(), qi.begin(), qi.end()); pj.insert(pj.end(), qj.begin(), qj.end());
    }
    // the pairs i < j of every family, in row-major order or (the all-pairs farm) the longest pairs of a family first
    void all_pairs(bool longest_first) {
        for (uint32_t f = 0; f < nfam; ++f) {
            std::vector<std::pair<uint32_t, uint32_t>> pr;
            for (uint32_t i = 0; i < nseq[f]; ++i)
                for (uint32_t j = i + 1; j < nseq[f]; ++j) pr.push_back({i, j});
            if (longest_first) {
                auto cost = [&](const std::pair<uint32_t, uint32_t> &p) { return (uint64_t)row(f, p.first).size() * row(f, p.second).size(); };
                std::stable_sort(pr.begin(), pr.end(), [&](const std::pair<uint32_t, uint32_t> &x, const std::pair<uint32_t, uint32_t> &y) { return cost(x) > cost(y); });
            }
            blocks[f].p0 = pi.size();
            blocks[f].np = (uint32_t)pr.size();
            for (const auto &p : pr) { pfam.push_back(f); pi.push_back(p.first); pj.push_back(p.second); }
        }
    }
    void set(uint32_t p, double d, double v) {   // the estimate of pair p into its family's symmetric matrices
        DistanceMatrix &dm = dist[pfam[p]];
        dm.D(pi[p], pj[p]) = dm.D(pj[p], pi[p]) = d;
        dm.V(pi[p], pj[p]) = dm.V(pj[p], pi[p]) = v;
    }
};

// The model as pgm_mldist_batch takes it: in eigen form when it has one of at most 20 states, else in general form (Q alone: the
// 61-state ECM model, a generator that is not reversible)
pgm_mldist_model mldist_model(const Alphabet &a, const ModelFactory &mf, bool eigen_form) {
    double DIST_MAX, VAR_MAX, VAR_MIN;
    mldist_limits(a, DIST_MAX, VAR_MAX, VAR_MIN);
    pgm_mldist_model m;
    m.dim = (uint32_t)a.DIM; m.Q = mf.Qmat().data();
    m.V = eigen_form ? mf.eigV().data() : nullptr; m.Vi = eigen_form ? mf.eigVi().data() : nullptr;
    m.sigma = eigen_form ? mf.eigSigma().data() : nullptr;
    m.dist_max = DIST_MAX; m.var_max = VAR_MAX; m.var_min = VAR_MIN; m.cutoff_dist = cmdlineopts.cutoff_dist;
    m.min_dist = cmdlineopts.min_dist; m.max_dist = cmdlineopts.max_dist; m.indel_rate = cmdlineopts.indel_rate;
    m.mldist = cmdlineopts.mldist_flag ? 1 : 0; m.mldist_gap = cmdlineopts.mldist_gap_flag ? 1 : 0;
    return m;
}

// computeDistance of every pair from its count matrix.  On the device (PGM_DEVICE_MLDIST): one pgm_mldist_batch call over the pairs
// of all families that share a model — every family without -F, one call per family with it —, in the form that model takes (eigen
// form: one wavefront per pair, general form: one workgroup per pair, if the backend's kernel takes that); the arithmetic is
// computeDistance's except for the device library's exp / log (last-bit differences: see csrc/pgm_dist_kernels.h) and, for a model
// of more than 20 states that has an eigen form, P(d) = exp(Q d) by expm instead of that form.  Else on the host: Newton on d per
// pair, each step a P(d), independent per pair, so the pairs are dealt to the host threads; every pair's arithmetic is the
// single-threaded one, the matrix entries written are disjoint.
void estimate_distances(const Alphabet &a, Families &F, const int32_t *counts, const uint32_t *gaps, const double *seqlen) {
    const uint32_t D = (uint32_t)a.DIM;
    const size_t dd = (size_t)D * D;
    const std::vector<PairBlock> &blocks = F.blocks;
    Backend &be = default_backend();
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<char> on_device(blocks.size(), 0);
    if (host_switches().device_mldist)
        for (size_t b0 = 0; b0 < blocks.size();) {
            const size_t b1 = cmdlineopts.aafreqs_flag ? b0 + 1 : blocks.size();   // (the blocks are contiguous in the pair arrays)
            const ModelFactory &mf = *blocks[b0].model_factory;
            const bool eigen_form = mf.has_eigen() && D <= 20;
            const size_t p0 = blocks[b0].p0, p1 = blocks[b1 - 1].p0 + blocks[b1 - 1].np;
            bool ok = eigen_form || (be.mldist_general() && D <= 64);
            std::vector<double> dist(p1 - p0), var(p1 - p0);
            if (ok && p1 > p0) {
                const pgm_mldist_model m = mldist_model(a, mf, eigen_form);
                ++be.calls_dist;
                ok = be.mldist_batch(m, (uint32_t)(p1 - p0), counts + p0 * dd, gaps + p0, seqlen + p0, dist.data(), var.data());
            }
            for (size_t b = b0; b < b1 && ok; ++b) on_device[b] = 1;
            for (size_t p = p0; p < p1 && ok; ++p) F.set((uint32_t)p, dist[p - p0], var[p - p0]);
            b0 = b1;
        }
    std::vector<uint32_t> work;   // the pairs left to the host
    for (size_t b = 0; b < blocks.size(); ++b)
        for (uint32_t k = 0; k < blocks[b].np && !on_device[b]; ++k) work.push_back((uint32_t)blocks[b].p0 + k);
    const size_t grain = 16;   // pairs per index handed out
    parallel_for((work.size() + grain - 1) / grain, [&](size_t g) {
        std::vector<int32_t> c(dd);
        for (size_t q = g * grain; q < std::min(work.size(), (g + 1) * grain); ++q) {
            const size_t p = work[q];
            std::copy(counts + p * dd, counts + (p + 1) * dd, c.begin());
            const distvar_t dv = F.df[F.pfam[p]].computeDistance(c, gaps[p], seqlen[p]);
            F.set((uint32_t)p, dv.dist, dv.var);
        }
    });
    be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
}

// fn(w) for every worker w < nw, one host thread per device context (worker 0 on this thread).  An exception does not leave its
// thread (that would end the process): the first one is thrown here once all have joined.
void on_workers(int nw, const std::function<void(int)> &fn) {
    std::vector<std::string> errs((size_t)nw);
    auto run = [&](int w) { try { fn(w); } catch (std::exception &e) { errs[(size_t)w] = e.what(); } };
    std::vector<std::thread> th;
    for (int w = 1; w < nw; ++w) th.emplace_back(run, w);
    run(0);
    for (auto &t : th) t.join();
    for (const std::string &e : errs) if (!e.empty()) throw pgm_exception(e);
}

// symbols of the all-pairs alignment: value(), negative -> 20 for amino acids and codons (the reference's quirk,
// DistanceFactoryAlign.h:72,79); DNA has no negative values (sequenceFromString refuses other characters) and its unknown is DIM, the
// X row of its scoring matrix
void nw_symbols(const Alphabet &a, const std::vector<const sequence_t *> &seq, std::vector<int8_t> &syms, std::vector<uint32_t> &offs) {
    const int unknown_sym = a.kind == ALPHA_DNA ? a.DIM : 20;
    offs.assign(1, 0);
    for (const sequence_t *s : seq) {
        for (int8_t c : *s) {
            const int v = a.value(c);
            syms.push_back((int8_t)(v < 0 ? unknown_sym : v));
        }
        offs.push_back((uint32_t)syms.size());
    }
}

// The reference's i < j double loop (DistanceFactoryAlign.h:35-53) is a farm of independent alignPair jobs.  Here: the pairs (gi, gj:
// by their sequences' places among the nseq of the call) cut into tiles, and one host thread per device context pulling tile numbers
// from an atomic counter (no collective, no static partition: a slower device simply takes fewer tiles).  Every tile is one
// pgm_nw_pairs_submit call on the worker's own context; the outputs of a pair land at the pair's position, whoever computed it, so
// the result does not depend on the number of workers.
void nw_farm(const DistanceFactoryAlign &dfa, uint32_t D, uint32_t nseq, const std::vector<int8_t> &syms, const std::vector<uint32_t> &offs,
             const std::vector<uint32_t> &gi, const std::vector<uint32_t> &gj, bool reduced, int32_t *counts, uint32_t *gaps) {
    Backend &be = default_backend();
    const uint32_t np = (uint32_t)gi.size();
    const size_t per = reduced ? 2 : (size_t)D * D;
    const int nw = std::max(1, be.workers());
    // Tile size.  A call costs ~0.3 ms beside its kernel (staging of the inputs, launch, the last D2H: bench.py all_pairs_nw
    // rank0_fixed_ms_per_call) and a worker hides that of tile k under the kernel of tile k+1 (two tiles in flight), so what
    // matters is (a) that a tile fills a device — its persistent grid holds 7168 pairs at once; fewer pairs leave CUs idle —
    // and (b) that the last tiles of the ticket queue are small against a worker's share.  Three tiles per worker, at least
    // 256 pairs; the pairs are sorted by cost, so the last tiles are also the cheapest.  PGM_NW_TILE overrides.
    uint32_t tile = std::max<uint32_t>(256u, (np + 3u * (uint32_t)nw - 1u) / (3u * (uint32_t)nw));
    if (const char *e = getenv("PGM_NW_TILE")) tile = (uint32_t)std::max(1, atoi(e));
    const uint32_t ntiles = np ? (np + tile - 1) / tile : 0;
    std::atomic<uint32_t> next_tile(0);
    be.farm_workers = nw; be.farm_tiles = (int)ntiles;
    on_workers(nw, [&](int w) {
        int pending = -1;
        for (;;) {
            const uint32_t t = next_tile.fetch_add(1);
            if (t >= ntiles) break;
            const uint32_t p0 = t * tile, cnt = std::min(tile, np - p0);
            ++be.calls_dist;
            const int ticket = be.nw_pairs_submit(D, dfa.scoring_matrix().data(), dfa.gap_open, dfa.gap_extend, nseq, syms.data(), offs.data(), cnt,
                                                  gi.data() + p0, gj.data() + p0, reduced ? 1u : 0u, counts + (size_t)p0 * per, gaps + p0, w);
            if (pending >= 0) be.nw_pairs_wait(pending, w);
            pending = ticket;
        }
        if (pending >= 0) be.nw_pairs_wait(pending, w);
    });
}

// -a (DistanceFactoryAlign.h:29-56): one farm of alignPair tiles over the sequences of all families, within-family pairs only
void nw_distances(const Alphabet &a, Families &F) {
    const uint32_t D = (uint32_t)a.DIM;
    Backend &be = default_backend();
    DistanceFactoryAlign dfa(a, F.blocks[0].model_factory);   // (the scoring matrix and the gap costs: the run's)
    std::vector<int8_t> syms;
    std::vector<uint32_t> offs;
    nw_symbols(a, F.seq, syms, offs);
    F.all_pairs(true);
    const uint32_t np = F.np();
    std::vector<uint32_t> gi(np), gj(np);
    for (uint32_t p = 0; p < np; ++p) { gi[p] = F.first[F.pfam[p]] + F.pi[p]; gj[p] = F.first[F.pfam[p]] + F.pj[p]; }
    auto len = [&](uint32_t s) { return offs[s + 1] - offs[s]; };
    // Without --mldist / --mldist_gap the distance of a pair reads (ident, total) of its count matrix and nothing else
    // (DistanceFactoryML.h:143-146, 175-178): the device reduces them and 8 B per pair come back instead of 4 D^2.
    const bool reduced = !(cmdlineopts.mldist_flag || cmdlineopts.mldist_gap_flag);
    const size_t per = reduced ? 2 : (size_t)D * D;
    // result buffers in pinned memory (the D2H copies write them directly), not zero-filled: every pair's slice is written by its tile
    int32_t *counts = (int32_t *)be.host_alloc(std::max<size_t>(sizeof(int32_t) * (size_t)np * per, 16));
    uint32_t *gaps = (uint32_t *)be.host_alloc(std::max<size_t>(4 * (size_t)np, 16));
    try {
        for (uint32_t p = 0; p < np; ++p) be.cells_nw += (uint64_t)len(gi[p]) * len(gj[p]);
        const auto t0 = std::chrono::steady_clock::now();
        nw_farm(dfa, D, (uint32_t)F.seq.size(), syms, offs, gi, gj, reduced, counts, gaps);
        be.seconds_nw += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::vector<double> seqlen(np);
        for (uint32_t p = 0; p < np; ++p) seqlen[p] = ((double)len(gi[p]) + (double)len(gj[p])) / 2.0;
        if (reduced) {
            for (uint32_t p = 0; p < np; ++p) {
                const distvar_t dv = F.df[F.pfam[p]].computeDistance((double)counts[2 * (size_t)p], (double)counts[2 * (size_t)p + 1], nullptr, gaps[p], seqlen[p]);
                F.set(p, dv.dist, dv.var);
            }
        } else {
            estimate_distances(a, F, counts, gaps, seqlen.data());
        }
    } catch (...) {
        be.host_free(counts);
        be.host_free(gaps);
        throw;
    }
    be.host_free(counts);
    be.host_free(gaps);
}

// The pair counts of np pairs behind the backend, the part its callers share: none with PGM_HOST_COUNTS.  The entry points take 20 to
// 64 states (pair_count_dim): DNA rows (values 0..3, -2) are counted as 20-state rows and the 4 x 4 corner of each 20 x 20 matrix is
// kept.  call(Dk, cdst, gaps) makes the backend's calls for Dk states and says whether all of them ran.  false: the counts are the
// caller's to scan on the host, after a zero-fill (a device call that failed may have written).
uint32_t pair_count_dim(uint32_t D) { return std::max<uint32_t>(D, 20u); }
template <class Call> bool device_pair_counts(uint32_t D, size_t np, int32_t *counts, uint32_t *gaps, std::vector<int32_t> &wide, const Call &call) {
    if (host_switches().host_counts) return false;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t Dk = pair_count_dim(D);
    const size_t dd = (size_t)D * D, ddk = (size_t)Dk * Dk;
    wide.assign(Dk != D ? np * ddk : 0, 0);   // (the caller's: a loop of calls keeps its storage)
    const bool done = call(Dk, Dk != D ? wide.data() : counts, gaps);
    if (done && Dk != D)
        for (size_t p = 0; p < np; ++p)
            for (uint32_t b = 0; b < D; ++b)
                for (uint32_t c = 0; c < D; ++c) counts[p * dd + c + (size_t)D * b] = wide[p * ddk + c + (size_t)Dk * b];
    default_backend().seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return done;
}

// Distances induced by the families' alignments: pair counts on the device (integer counts, bit-exact: on by default, unlike the ML
// estimates that follow), on the host threads with PGM_HOST_COUNTS or a backend without the kernel, then the estimates.
// per_family_calls: see tree_nj.
void prealigned_distances(const Alphabet &a, Families &F, bool per_family_calls) {
    const uint32_t D = (uint32_t)a.DIM, nfam = F.nfam;
    const size_t dd = (size_t)D * D;
    Backend &be = default_backend();
    F.all_pairs(false);
    const uint32_t np = F.np();
    std::vector<uint32_t> ncols(nfam);
    for (uint32_t f = 0; f < nfam; ++f) ncols[f] = (uint32_t)F.row(f, 0).size();
    std::vector<int32_t> counts((size_t)np * dd, 0);
    std::vector<uint32_t> gaps(np, 0);
    std::vector<int32_t> wide;
    const bool done = device_pair_counts(D, np, counts.data(), gaps.data(), wide, [&](uint32_t Dk, int32_t *cdst, uint32_t *gdst) {
        std::vector<size_t> base(nfam + 1, 0);   // every family's nseq x ncols matrix, back to back
        for (uint32_t f = 0; f < nfam; ++f) base[f + 1] = base[f] + (size_t)F.nseq[f] * ncols[f];
        std::vector<int8_t> mat(base[nfam]);
        parallel_for(nfam, [&](size_t f) {
            for (uint32_t i = 0; i < F.nseq[f]; ++i) prealigned_row(a, F.row((uint32_t)f, i), mat.data() + base[f] + (size_t)i * ncols[f]);
        });
        if (!per_family_calls) {
            ++be.calls_dist;
            return be.prealigned_counts_multi(Dk, nfam, F.nseq.data(), ncols.data(), mat.data(), np, F.pfam.data(), F.pi.data(), F.pj.data(), cdst, gdst);
        }
        bool all = true;
        for (uint32_t f = 0; f < nfam; ++f) {
            // every pair costs the same (one scan of the columns): contiguous ranges of the family's pairs, one per device context
            const size_t q0 = F.blocks[f].p0;
            const uint32_t nq = F.blocks[f].np;
            const int nw = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, be.workers()), nq));
            std::vector<char> ok((size_t)nw, 0);
            on_workers(nw, [&](int w) {
                const uint32_t p0 = (uint32_t)((uint64_t)nq * (uint32_t)w / (uint32_t)nw), p1 = (uint32_t)((uint64_t)nq * ((uint32_t)w + 1u) / (uint32_t)nw);
                if (p1 != p0) ++be.calls_dist;
                ok[(size_t)w] = (p1 == p0 || be.prealigned_counts_batch(Dk, F.nseq[f], ncols[f], mat.data() + base[f], p1 - p0, F.pi.data() + q0 + p0,
                                                                       F.pj.data() + q0 + p0, cdst + (q0 + p0) * Dk * Dk, gdst + q0 + p0, w)) ? 1 : 0;
            });
            for (char c : ok) all = all && c;
        }
        return all;
    });
    if (!done) {
        const auto t1 = std::chrono::steady_clock::now();
        const size_t grain = 16;   // pairs per index handed out
        parallel_for(((size_t)np + grain - 1) / grain, [&](size_t g) {
            for (size_t p = g * grain; p < std::min<size_t>(np, (g + 1) * grain); ++p) {
                std::fill(counts.begin() + (std::ptrdiff_t)(p * dd), counts.begin() + (std::ptrdiff_t)((p + 1) * dd), 0);   // (a device call that failed may have written)
                gaps[p] = prealigned_count_pair(a, F.row(F.pfam[p], F.pi[p]), F.row(F.pfam[p], F.pj[p]), counts.data() + p * dd);
            }
        });
        be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    }
    std::vector<double> seqlen(np);
    for (size_t p = 0; p < np; ++p) seqlen[p] = ((double)ncols[F.pfam[p]] + (double)ncols[F.pfam[p]]) / 2.0;
    const auto tq0 = std::chrono::steady_clock::now();
    estimate_distances(a, F, counts.data(), gaps.data(), seqlen.data());
    if (host_switches().profile && nfam == 1)
        fprintf(stderr, "  prealigned distances: pair counts %s, estimates %.1f ms\n", done ? "on the device" : "on the host",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq0).count());
}

// DistanceFactory::getDefault (DistanceFactory.cpp:9-20), DistanceFactoryAngle<ALPHABET, K> (DistanceFactoryAngle.h:55-131): the
// default initial distances (no -a), the cosine of the k-mer count vectors turned into a distance.  The count rows of all families
// back to back; per_family_calls: see tree_nj.
void angle_distances(const Alphabet &a, Families &F, bool per_family_calls) {
    const uint32_t nfam = F.nfam, ncols = angle_ncols(a);
    Backend &be = default_backend();
    std::vector<size_t> out0(nfam + 1, 0);
    for (uint32_t f = 0; f < nfam; ++f) out0[f + 1] = out0[f] + (size_t)F.nseq[f] * F.nseq[f];
    std::vector<int32_t> counts(F.seq.size() * ncols, 0);
    std::vector<double> cosine(out0[nfam], 0.0);
    parallel_for(F.seq.size(), [&](size_t s) { angle_count_row(a, *F.seq[s], ncols, counts.data() + s * ncols); });
    const auto t0 = std::chrono::steady_clock::now();
    if (!per_family_calls) {
        ++be.calls_dist;
        be.kmer_cosine_multi(nfam, F.nseq.data(), ncols, counts.data(), cosine.data());
    } else
        for (uint32_t f = 0; f < nfam; ++f) {
            ++be.calls_dist;
            be.kmer_cosine(F.nseq[f], ncols, counts.data() + (size_t)F.first[f] * ncols, cosine.data() + out0[f]);   // :100
        }
    be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // one family: its rows on the host threads; several: the families
    parallel_for(nfam, [&](size_t f) {
        std::copy(cosine.begin() + (std::ptrdiff_t)out0[f], cosine.begin() + (std::ptrdiff_t)out0[f + 1], F.dist[f].distances.begin());
        std::vector<double> seq_len(F.nseq[f]);
        for (uint32_t i = 0; i < F.nseq[f]; ++i) seq_len[i] = (double)F.row((uint32_t)f, i).size();
        angle_finish(F.dist[f], seq_len, nfam == 1);
    });
}

// TreeNJ.h:27-59 for a list of families: one of the three distance stages over the pairs of all of them, then BioNJ, the -W
// refinement (TreeNJ.h:52-54) and the rooting per family.  per_family_calls is all that tells the two entry points apart: the
// cosine matrix and the pair counts of an alignment through the per-family entries of the backend (TreeNJ: kmer_cosine, and
// prealigned_counts_batch over every device context), or through the entries that take all families in one call on worker 0
// (TreeNJ_multi).  Either way a family's matrices, and so its tree, are the same.
void tree_nj(const Alphabet &a, std::vector<TreeJob> &jobs, bool prealigned, bool per_family_calls) {
    const auto tq0 = std::chrono::steady_clock::now();
    std::vector<size_t> act;
    for (size_t j = 0; j < jobs.size(); ++j) {
        jobs[j].tree = nullptr;
        jobs[j].error.clear();
        if (jobs[j].seqs->size() < 2) { jobs[j].error = "cannot construct tree from < 2 sequences"; continue; }
        if (prealigned) {
            const size_t L = jobs[j].seqs->begin()->second.size();
            bool same = true;
            for (const auto &kv : *jobs[j].seqs) same = same && kv.second.size() == L;
            if (!same) { jobs[j].error = "prealigned distances: rows of different length"; continue; }
        }
        act.push_back(j);
    }
    // the plans of the families with a fixed topology (std::map key order is the order of the matrix: TreeNJ.h:34-39); a family
    // whose topology does not fit leaves with the message before any distance is estimated
    std::vector<std::vector<pgm_bionj_pair>> plans(jobs.size());
    {
        std::vector<size_t> fits;
        for (size_t j : act) {
            if (jobs[j].topo) {
                std::vector<std::string> order;
                for (const auto &kv : *jobs[j].seqs) order.push_back(kv.first);
                try { plans[j] = build_topo_plan(order, jobs[j].topo); }
                catch (std::exception &e) { jobs[j].error = e.what(); continue; }
            }
            fits.push_back(j);
        }
        act.swap(fits);
    }
    if (act.empty()) return;
    Families F;
    for (size_t j : act) F.add_family(a, jobs[j].model_factory, *jobs[j].seqs);
    const uint32_t nfam = F.nfam;
    if (prealigned) prealigned_distances(a, F, per_family_calls);
    else if (!cmdlineopts.nwdist_flag) angle_distances(a, F, per_family_calls);
    else nw_distances(a, F);
    for (const DistanceMatrix &d : F.dist) dump_distances(d);   // (--dump_dist: refused with --batch, so one matrix per call)
    const auto tq1 = std::chrono::steady_clock::now();
    std::vector<std::vector<pgm_bionj_join>> joins;
    std::vector<double> final_d;
    std::vector<std::string> join_error;
    auto plan_of = [&](uint32_t f) -> const std::vector<pgm_bionj_pair> * { return jobs[act[f]].topo ? &plans[act[f]] : nullptr; };
    bionj_joins_families(F.dist, F.nseq, plan_of, joins, final_d, join_error);
    for (uint32_t f = 0; f < nfam; ++f) dump_joins((int32_t)F.nseq[f], joins[f], &final_d[9 * (size_t)f]);   // (--dump_joins: refused with --batch)
    // the trees, -W and the rooting per family on the host threads (-W is refused with --batch: refineTree loads one tree's
    // matrices into the backend)
    parallel_for(nfam, [&](size_t f) {
        TreeJob &job = jobs[act[f]];
        try {
            if (!join_error[f].empty()) throw pgm_exception(join_error[f]);
            DistanceMatrix &d = F.dist[f];
            PhyTree *tree = bionj_tree(F.order[f], joins[f], &final_d[9 * f]);
            if (cmdlineopts.wlsrefine_flag) tree = refineTree(tree, F.order[f], d);
            job.tree = midpointRoot(tree);
        } catch (std::exception &e) { job.error = e.what(); }
    });
    if (host_switches().profile && prealigned && nfam == 1)
        fprintf(stderr, "  TreeNJ: distances %.1f ms, BioNJ + rooting %.1f ms\n", std::chrono::duration<double, std::milli>(tq1 - tq0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq1).count());
}
}  // namespace

PhyTree *TreeNJ(const Alphabet &a, const std::map<std::string, sequence_t> &seqs, const ModelFactory *mf, bool prealigned, const PhyTree *topo) {
    std::vector<TreeJob> job(1);
    job[0].seqs = &seqs;
    job[0].model_factory = mf;
    job[0].topo = topo;
    tree_nj(a, job, prealigned, true);
    if (!job[0].error.empty()) throw pgm_exception(job[0].error);
    return job[0].tree;
}

void TreeNJ_multi(const Alphabet &a, std::vector<TreeJob> &jobs, bool prealigned) { tree_nj(a, jobs, prealigned, false); }

// ==== --bootstrap: the trees of resampled columns of one alignment =====================================================
BootstrapStats bootstrap_stats;

bool Backend::prealigned_counts_resampled(uint32_t dim, uint32_t nrows, uint32_t ncols, const int8_t *rows, uint32_t nrep, const uint32_t *cols,
                                          uint32_t npairs, const uint32_t *pi, const uint32_t *pj, int32_t *counts, uint32_t *gaps, int worker) {
    std::vector<int8_t> gathered((size_t)nrows * ncols);
    for (uint32_t r = 0; r < nrep; ++r) {
        const uint32_t *c = cols + (size_t)r * ncols;
        for (uint32_t i = 0; i < nrows; ++i)
            for (uint32_t k = 0; k < ncols; ++k) gathered[(size_t)i * ncols + k] = rows[(size_t)i * ncols + c[k]];
        if (!prealigned_counts_batch(dim, nrows, ncols, gathered.data(), npairs, pi, pj, counts + (size_t)r * npairs * dim * dim, gaps + (size_t)r * npairs, worker))
            return false;
    }
    return true;
}

std::vector<PhyTree *> bootstrap_trees(const Alphabet &a, const std::map<std::string, sequence_t> &rows, const ModelFactory *mf, uint32_t nrep, uint64_t seed) {
    const uint32_t n = (uint32_t)rows.size(), D = (uint32_t)a.DIM;
    if (n < 4) error("bootstrap: fewer than 4 sequences");
    const size_t L = rows.begin()->second.size();
    std::vector<std::string> order;   // (std::map key order: the order of the matrices, TreeNJ.h:34-39)
    std::vector<const sequence_t *> seq;
    for (const auto &kv : rows) {
        if (kv.second.size() != L) error("bootstrap: rows of different length");
        order.push_back(kv.first);
        seq.push_back(&kv.second);
    }
    if (L == 0 || L > 0xffffffffull) error("bootstrap: an alignment of %zu columns", L);
    const uint32_t ncols = (uint32_t)L;
    Backend &be = default_backend();
    std::vector<int8_t> mat((size_t)n * ncols);
    parallel_for(n, [&](size_t i) { prealigned_row(a, *seq[i], mat.data() + i * ncols); });
    const std::vector<uint32_t> cols = bootstrap_columns(nrep, ncols, seed);
    std::vector<uint32_t> pi, pj;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j) { pi.push_back(i); pj.push_back(j); }
    const uint32_t np = (uint32_t)pi.size(), Dk = pair_count_dim(D);
    const size_t dd = (size_t)D * D;
    const uint32_t group = (uint32_t)std::max<size_t>(1, std::min<size_t>(nrep, kBootstrapCountBytes / (sizeof(int32_t) * Dk * Dk * np)));
    std::vector<PhyTree *> trees(nrep, nullptr);
    try {
        std::vector<int32_t> wide, counts;
        std::vector<uint32_t> gaps;
        for (uint32_t r0 = 0; r0 < nrep; r0 += group) {
            const uint32_t g = std::min(group, nrep - r0);
            const size_t gp = (size_t)g * np;
            const uint32_t *gcols = cols.data() + (size_t)r0 * ncols;
            counts.assign(gp * dd, 0); gaps.assign(gp, 0);
            const bool done = device_pair_counts(D, gp, counts.data(), gaps.data(), wide, [&](uint32_t dim, int32_t *cdst, uint32_t *gdst) {
                ++bootstrap_stats.counts_calls; ++be.calls_dist;
                return be.prealigned_counts_resampled(dim, n, ncols, mat.data(), g, gcols, np, pi.data(), pj.data(), cdst, gdst);
            });
            if (!done) {   // (PGM_HOST_COUNTS, or a backend without the kernel: the host's scan of the gathered rows)
                const auto t1 = std::chrono::steady_clock::now();
                std::fill(counts.begin(), counts.end(), 0);
                for (uint32_t r = 0; r < g; ++r) {
                    std::vector<sequence_t> grow(n, sequence_t(ncols, 0));
                    parallel_for(n, [&](size_t i) { for (uint32_t k = 0; k < ncols; ++k) grow[i][k] = (*seq[i])[gcols[(size_t)r * ncols + k]]; });
                    parallel_for(np, [&](size_t p) { gaps[(size_t)r * np + p] = prealigned_count_pair(a, grow[pi[p]], grow[pj[p]], counts.data() + ((size_t)r * np + p) * dd); });
                }
                be.seconds_mldist += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
            }
            // the replicates of the group as families of one call: the estimator and the joins of tree_nj
            Families F;
            for (uint32_t f = 0; f < g; ++f) F.add_pairs(F.add_family(a, mf, n), pi, pj);
            const std::vector<double> seqlen(gp, ((double)ncols + (double)ncols) / 2.0);
            estimate_distances(a, F, counts.data(), gaps.data(), seqlen.data());
            std::vector<std::vector<pgm_bionj_join>> joins;
            std::vector<double> final_d;
            std::vector<std::string> join_error;
            bionj_joins_families(F.dist, F.nseq, [](uint32_t) -> const std::vector<pgm_bionj_pair> * { return nullptr; }, joins, final_d, join_error);
            for (uint32_t f = 0; f < g; ++f) {
                if (!join_error[f].empty()) throw pgm_exception(join_error[f]);
                trees[r0 + f] = bionj_tree(order, joins[f], &final_d[9 * (size_t)f]);
            }
        }
    } catch (...) {
        for (PhyTree *t : trees) delete t;
        throw;
    }
    bootstrap_stats.replicates += (int)nrep;
    return trees;
}
}  // namespace pgm
