// transfer.inc — the host parts of `pgmsa --bootstrap_tbe` (included by progressive.cpp, like guidance.inc: they need parallel_for,
// and the source lists of the drivers are fixed): the host statement of the transfer indices (Backend::transfer_min's default, what
// pgmsa_oracle runs), the bounds of one call, and the support of every internal edge of a tree.  The leaf numbering and the
// bipartition walk are those of bipartition_support (phytree.cpp); the flow that writes the files is doBootstrap in main.cpp.

TransferStats transfer_stats;

void transfer_min_host(uint32_t nleaves, uint32_t nref, const uint64_t *ref, uint32_t nrep, const uint32_t *rep_off, const uint64_t *rep, uint32_t *phi) {
    if (nleaves < 4 || nref == 0 || nrep == 0) error("transfer min: nleaves must be at least 4, nref and nrep at least 1");
    if ((uint64_t)nref * nrep > 0xffffffffull) error("transfer min: nref * nrep does not fit 32 bits");
    if (!ref || !rep_off || !phi) error("transfer min: null argument");
    if (rep_off[0] != 0) error("transfer min: rep_off[0] must be 0");
    for (uint32_t r = 0; r < nrep; ++r)
        if (rep_off[r + 1] < rep_off[r]) error("transfer min: rep_off must ascend");
    if (!rep && rep_off[nrep] != 0) error("transfer min: null argument");
    const size_t words = ((size_t)nleaves + 63) / 64;
    const uint64_t tail = nleaves % 64 ? ~(uint64_t)0 << (nleaves % 64) : 0;   // the bits of the last word no leaf has
    for (size_t e = 0; e < nref; ++e) {
        size_t size = 0;
        for (size_t w = 0; w < words; ++w) size += (size_t)__builtin_popcountll(ref[e * words + w]);
        if (ref[e * words + words - 1] & tail) error("transfer min: reference set %zu has a bit at or above nleaves", e);
        if (size == 0 || size == nleaves) error("transfer min: reference set %zu is empty or full", e);
    }
    for (size_t s = 0; s < rep_off[nrep]; ++s)
        if (rep[s * words + words - 1] & tail) error("transfer min: replicate set %zu has a bit at or above nleaves", s);

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
