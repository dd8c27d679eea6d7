// transfer.cpp — the host parts of `pgmsa --bootstrap_tbe` and `--bootstrap_taxa`: the host statement of the transfer indices
// (Backend::transfer_min's default, what pgmsa_oracle runs), the bounds of one call, and the support of every internal edge of a
// tree.  The leaf numbering and the bipartition walk are those of bipartition_support (phytree.cpp); the flow that writes the
// files is doBootstrap in driver_analyses.cpp.
// --bootstrap_taxa (below the TBE part): the host statement of the moved-taxon counts (Backend::transfer_taxa's default), the
// per-taxon sums over the distinct bipartitions of a tree, and the two file texts.
#include "pgm_host.h"

#include <algorithm>
#include <chrono>
#include <cstdio>

namespace pgm {

TransferStats transfer_stats;

// what both host statements refuse (the checks of the C entries, include/pgm_hip.h); `what` opens the message
static void transfer_check_host(const char *what, uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep,
                                const void *out) {
    if (nleaves < 4 || nref == 0 || nrep == 0) error("%s: nleaves must be at least 4, nref and nrep at least 1", what);
    if ((uint64_t)nref * nrep > 0xffffffffull) error("%s: nref * nrep does not fit 32 bits", what);
    if (!ref || !rep_off || !out) error("%s: null argument", what);
    if (rep_off[0] != 0) error("%s: rep_off[0] must be 0", what);
    for (uint32_t r = 0; r < nrep; ++r)
        if (rep_off[r + 1] < rep_off[r]) error("%s: rep_off must ascend", what);
    if (!rep && rep_off[nrep] != 0) error("%s: null argument", what);
    const size_t words = ((size_t)nleaves + 63) / 64;
    const uint64_t tail = nleaves % 64 ? ~(uint64_t)0 << (nleaves % 64) : 0;   // the bits of the last word no leaf has
    for (size_t e = 0; e < nref; ++e) {
        size_t size = 0;
        for (size_t w = 0; w < words; ++w) size += (size_t)__builtin_popcountll(ref[e * words + w]);
        if (ref[e * words + words - 1] & tail) error("%s: reference set %zu has a bit at or above nleaves", what, e);
        if (size == 0 || size == nleaves) error("%s: reference set %zu is empty or full", what, e);
    }
    for (size_t s = 0; s < rep_off[nrep]; ++s)
        if (rep[s * words + words - 1] & tail) error("%s: replicate set %zu has a bit at or above nleaves", what, s);
}

void transfer_min_host(uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep, uint32_t *phi) {
    transfer_check_host("transfer min", nleaves, nref, ref, nrep, rep_off, rep, phi);
    const size_t words = ((size_t)nleaves + 63) / 64;

    parallel_for(nref, [&](size_t e) {
        const uint64_t *A = ref + e * words;
        uint32_t size = 0;
        for (size_t w = 0; w < words; ++w) size += (uint32_t)__builtin_popcountll(A[w]);
        const uint32_t p = std::min(size, nleaves - size);
        for (uint32_t r = 0; r < nrep; ++r) {
            uint32_t best = p - 1;   // (what the single-leaf edges of any tree give)
            for (size_t s = rep_off[r]; s < rep_off[r + 1]; ++s) {
                const uint64_t *B = rep + s * words;
                uint32_t h = 0;
                for (size_t w = 0; w < words; ++w) h += (uint32_t)__builtin_popcountll(A[w] ^ B[w]);
                best = std::min(best, std::min(h, nleaves - h));
            }
            phi[e * nrep + r] = best;
        }
    });
}

void Backend::transfer_min(uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep, uint32_t *phi, int) {
    transfer_min_host(nleaves, nref, ref, nrep, rep_off, rep, phi);
}

uint32_t transfer_call_replicates(uint32_t nleaves, uint32_t nref, size_t max_sets, size_t rep_bytes) {
    const uint64_t words = ((uint64_t)nleaves + 63) / 64;
    uint64_t m = rep_bytes / std::max<uint64_t>(1, 8 * words * (uint64_t)max_sets);
    if (nref > 0) m = std::min<uint64_t>(m, 0xffffffffull / nref);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(m, 0xffffffffull));
}

std::map<const PhyTree *, TransferEdge> transfer_support(const PhyTree &tree, const std::vector<const PhyTree *> &replicates, Backend *be) {
    const auto t0 = std::chrono::steady_clock::now();
    const LeafNumbering num = leaf_numbering(tree);
    const auto edges = bipartitions_of(num, tree);
    std::map<const PhyTree *, TransferEdge> support;
    if (edges.empty() || replicates.empty()) return support;
    if (num.nleaves < 4 || num.nleaves > 0xffffffffull) error("transfer support: a tree of %zu leaves", num.nleaves);
    const uint32_t n = (uint32_t)num.nleaves, nref = (uint32_t)edges.size();
    const size_t words = num.words;
    std::vector<uint64_t> ref(nref * words);
    for (size_t e = 0; e < nref; ++e) std::copy(edges[e].second.begin(), edges[e].second.end(), ref.begin() + e * words);

    std::vector<std::vector<uint64_t>> sets(replicates.size());   // every replicate's non-trivial bipartitions back to back
    size_t max_sets = 1;
    parallel_for(replicates.size(), [&](size_t r) {
        for (const auto &b : bipartitions_of(num, *replicates[r])) sets[r].insert(sets[r].end(), b.second.begin(), b.second.end());
    });
    for (const auto &s : sets) max_sets = std::max(max_sets, s.size() / words);
    const uint32_t per_call = transfer_call_replicates(n, nref, max_sets);

    std::vector<uint64_t> S(nref, 0), rep;
    std::vector<uint32_t> rep_off, phi;
    for (size_t r0 = 0; r0 < replicates.size(); r0 += per_call) {
        const uint32_t m = (uint32_t)std::min<size_t>(per_call, replicates.size() - r0);
        rep.clear();
        rep_off.assign(1, 0);
        for (uint32_t r = 0; r < m; ++r) {
            rep.insert(rep.end(), sets[r0 + r].begin(), sets[r0 + r].end());
            if (rep.size() / words > 0xffffffffull) error("transfer support: more than 2^32 - 1 replicate sets in one call");
            rep_off.push_back((uint32_t)(rep.size() / words));
        }
        phi.assign((size_t)nref * m, 0);
        if (be) be->transfer_min(n, nref, ref.data(), m, rep_off.data(), rep.empty() ? nullptr : rep.data(), phi.data());
        else transfer_min_host(n, nref, ref.data(), m, rep_off.data(), rep.empty() ? nullptr : rep.data(), phi.data());
        ++transfer_stats.calls;
        for (size_t e = 0; e < nref; ++e)
            for (uint32_t r = 0; r < m; ++r) S[e] += phi[e * m + r];
    }
    for (size_t e = 0; e < nref; ++e) {
        uint32_t size = 0;
        for (uint64_t w : edges[e].second) size += (uint32_t)__builtin_popcountll(w);
        TransferEdge &t = support[edges[e].first];
        t.S = S[e];
        t.p = std::min(size, n - size);
    }
    transfer_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return support;
}

std::map<const PhyTree *, std::string> transfer_labels(const std::map<const PhyTree *, TransferEdge> &support, uint32_t nrep) {
    std::map<const PhyTree *, std::string> labels;
    for (const auto &kv : support) {
        char buf[40];
        snprintf(buf, sizeof buf, "%.6f", 1.0 - (double)kv.second.S / ((double)nrep * (double)(kv.second.p - 1)));
        labels[kv.first] = buf;
    }
    return labels;
}

// ---- --bootstrap_taxa: which taxa the transfer indices move ------------------------------------------------------------
TransferStats taxa_stats;

void transfer_taxa_host(uint32_t nleaves, uint32_t nref, const uint64_t *ref, const uint32_t *thr, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep,
                        uint32_t *phi, uint32_t *arg, uint32_t *moved, uint32_t *counted) {
    if (!thr || !arg || !moved || !counted) error("transfer taxa: null argument");
    if (nleaves > 0x7fffffffu) error("transfer taxa: nleaves is beyond 2^31 - 1");
    if ((uint64_t)nref * nleaves > 0xffffffffull) error("transfer taxa: nref * nleaves does not fit 32 bits");
    transfer_check_host("transfer taxa", nleaves, nref, ref, nrep, rep_off, rep, phi);
    const size_t words = ((size_t)nleaves + 63) / 64;

    parallel_for(nref, [&](size_t e) {
        const uint64_t *A = ref + e * words;
        uint32_t size = 0;
        for (size_t w = 0; w < words; ++w) size += (uint32_t)__builtin_popcountll(A[w]);
        const uint32_t p = std::min(size, nleaves - size);
        uint32_t *row = moved + e * nleaves;
        std::fill(row, row + nleaves, 0u);
        uint32_t n_counted = 0;
        for (uint32_t r = 0; r < nrep; ++r) {
            uint32_t best = p - 1, at = kTransferNone;   // (the clamp names no set)
            bool complement = false;
            for (size_t s = rep_off[r]; s < rep_off[r + 1]; ++s) {
                const uint64_t *B = rep + s * words;
                uint32_t h = 0;
                for (size_t w = 0; w < words; ++w) h += (uint32_t)__builtin_popcountll(A[w] ^ B[w]);
                const uint32_t d = std::min(h, nleaves - h);
                if (d < best || (d == best && at == kTransferNone)) { best = d; at = (uint32_t)s; complement = h > nleaves - h; }   // the lowest s of the lowest d
            }
            phi[e * nrep + r] = best;
            arg[e * nrep + r] = at;
            if (at == kTransferNone || best > thr[e]) continue;
            ++n_counted;
            const uint64_t *B = rep + (size_t)at * words;
            for (uint32_t t = 0; t < nleaves; ++t)
                row[t] += (uint32_t)((((A[t / 64] ^ B[t / 64]) >> (t % 64)) & 1) != (uint64_t)complement);
        }
        counted[e] = n_counted;
    });
}

void Backend::transfer_taxa(uint32_t nleaves, uint32_t nref, const uint64_t *ref, const uint32_t *thr, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep,
                            uint32_t *phi, uint32_t *arg, uint32_t *moved, uint32_t *counted, int) {
    transfer_taxa_host(nleaves, nref, ref, thr, nrep, rep_off, rep, phi, arg, moved, counted);
}

TaxaSupport taxa_support(const PhyTree &tree, const std::vector<const PhyTree *> &replicates, double cutoff, Backend *be) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!(cutoff >= 0.0 && cutoff < 1.0)) error("taxa support: the cutoff must be in [0, 1)");
    const LeafNumbering num = leaf_numbering(tree);
    const auto nodes = bipartitions_of(num, tree);   // post-order: the order of the labels in formatNewick's text
    if (num.nleaves < 4 || num.nleaves > 0x7fffffffull) error("taxa support: a tree of %zu leaves", num.nleaves);
    const uint32_t n = (uint32_t)num.nleaves;
    const size_t words = num.words;
    TaxaSupport out;
    for (const auto &kv : num.index) out.names.push_back(kv.first);   // (a map: sorted, the numbering's order)
    out.moved.assign(n, 0);
    out.replicates = replicates.size();

    // reference edges that share a bipartition (the two below a bifurcating root) are one row of every call
    std::map<std::vector<uint64_t>, size_t> row_of;
    std::vector<size_t> node_row;
    std::vector<uint64_t> ref;
    std::vector<uint32_t> thr, p_of;
    for (const auto &e : nodes) {
        const auto it = row_of.emplace(e.second, row_of.size());
        node_row.push_back(it.first->second);
        if (!it.second) continue;
        ref.insert(ref.end(), e.second.begin(), e.second.end());
        uint32_t size = 0;
        for (uint64_t w : e.second) size += (uint32_t)__builtin_popcountll(w);
        p_of.push_back(std::min(size, n - size));
        thr.push_back((uint32_t)(cutoff * (double)(p_of.back() - 1)));   // floor: the product is not negative
    }
    const size_t nref = p_of.size();
    out.edges = nref;
    if ((uint64_t)nref * n > 0xffffffffull) error("taxa support: %zu edges of %u leaves do not fit one call", nref, n);
    std::vector<uint64_t> moved64(nref * (size_t)n, 0), counted64(nref, 0);

    if (nref > 0 && !replicates.empty()) {
        // every replicate's non-trivial sets in the canonical order: ascending as vectors of words, equal sets once
        std::vector<std::vector<uint64_t>> sets(replicates.size());
        size_t max_sets = 1;
        parallel_for(replicates.size(), [&](size_t r) {
            std::vector<std::vector<uint64_t>> mine;
            for (auto &b : bipartitions_of(num, *replicates[r])) mine.push_back(std::move(b.second));
            std::sort(mine.begin(), mine.end());
            mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
            for (const auto &b : mine) sets[r].insert(sets[r].end(), b.begin(), b.end());
        });
        for (const auto &s : sets) max_sets = std::max(max_sets, s.size() / words);
        const uint32_t per_call = transfer_call_replicates(n, (uint32_t)nref, max_sets);

        std::vector<uint64_t> rep;
        std::vector<uint32_t> rep_off, phi, arg, moved((size_t)nref * n), counted(nref);
        for (size_t r0 = 0; r0 < replicates.size(); r0 += per_call) {
            const uint32_t m = (uint32_t)std::min<size_t>(per_call, replicates.size() - r0);
            rep.clear();
            rep_off.assign(1, 0);
            for (uint32_t r = 0; r < m; ++r) {
                rep.insert(rep.end(), sets[r0 + r].begin(), sets[r0 + r].end());
                if (rep.size() / words >= 0xffffffffull) error("taxa support: more than 2^32 - 2 replicate sets in one call");
                rep_off.push_back((uint32_t)(rep.size() / words));
            }
            phi.assign(nref * (size_t)m, 0);
            arg.assign(nref * (size_t)m, 0);
            const uint64_t *rp = rep.empty() ? nullptr : rep.data();
            if (be) be->transfer_taxa(n, (uint32_t)nref, ref.data(), thr.data(), m, rep_off.data(), rp, phi.data(), arg.data(), moved.data(), counted.data());
            else transfer_taxa_host(n, (uint32_t)nref, ref.data(), thr.data(), m, rep_off.data(), rp, phi.data(), arg.data(), moved.data(), counted.data());
            ++taxa_stats.calls;
            for (size_t k = 0; k < moved.size(); ++k) moved64[k] += moved[k];
            for (size_t e = 0; e < nref; ++e) counted64[e] += counted[e];
        }
    }
    for (size_t e = 0; e < nref; ++e) {
        out.counted += counted64[e];
        for (uint32_t t = 0; t < n; ++t) out.moved[t] += moved64[e * n + t];
    }
    for (size_t k = 0; k < nodes.size(); ++k) {
        TaxaEdge edge;
        edge.p = p_of[node_row[k]];
        edge.counted = counted64[node_row[k]];
        edge.moved.assign(moved64.begin() + node_row[k] * (size_t)n, moved64.begin() + (node_row[k] + 1) * (size_t)n);
        out.nodes.push_back(std::move(edge));
    }
    taxa_stats.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return out;
}

std::string taxa_text(const TaxaSupport &t, double cutoff) {
    char buf[160];
    snprintf(buf, sizeof buf, "# replicates %zu cutoff %g edges %zu counted %llu\n", t.replicates, cutoff, t.edges, (unsigned long long)t.counted);
    std::string s = buf;
    s += "taxon\tmoved\tscore\n";
    for (size_t k = 0; k < t.names.size(); ++k) {
        snprintf(buf, sizeof buf, "\t%llu\t%.6f\n", (unsigned long long)t.moved[k], t.counted ? (double)t.moved[k] / (double)t.counted : 0.0);
        s += t.names[k] + buf;
    }
    return s;
}

std::string taxa_edges_text(const TaxaSupport &t) {
    std::string s = "edge\tp\tcounted";
    for (const std::string &name : t.names) s += "\t" + name;
    s += "\n";
    for (size_t k = 0; k < t.nodes.size(); ++k) {
        s += std::to_string(k) + "\t" + std::to_string(t.nodes[k].p) + "\t" + std::to_string(t.nodes[k].counted);
        for (uint64_t v : t.nodes[k].moved) s += "\t" + std::to_string(v);
        s += "\n";
    }
    return s;
}

}  // namespace pgm
