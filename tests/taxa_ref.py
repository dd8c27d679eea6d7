"""The taxon side of the transfer bootstrap (`--bootstrap_taxa`) stated independently of the C++: from the
`--bootstrap_out` line and the `--bootstrap_trees` lines alone, with transfer_ref's newick reader and Python-integer leaf sets, a
normalisation, sort and dedupe of its own, and plain loops with bin(x).count("1").

Definitions (n leaves in sorted-name order, A a reference set, B a set of a replicate): h = popcount(A xor B), d = min(h, n - h),
the moved set T = A xor B if h <= n - h, else its complement within the n leaves.  phi = min(p - 1, min d); the arg-min is the
lowest index s (in the replicate's canonical order) with d == phi, or NONE when no set is that near; a pair is counted iff it has
an arg-min and phi <= thr; moved[e][t] counts the counted replicates with t in T, counted[e] the counted replicates."""
import math

import transfer_ref as T

NONE = 0xFFFFFFFF


def word_key(s, n):
    """The order of std::vector<uint64_t>: 64-bit words compared word 0 first (not the order of the integers)."""
    return tuple(T.to_words([s], n)[0])


def canonical_sets(sets, n):
    """A replicate's sets on the side without leaf 0, ascending by words, equal ones once."""
    full = (1 << n) - 1
    return sorted({s ^ full if s & 1 else s for s in sets}, key=lambda s: word_key(s, n))


def moved_set(a, b, n):
    """(d, T) of two sets."""
    x = a ^ b
    h = T.popcount(x)
    if h <= n - h:
        return h, x
    return n - h, x ^ ((1 << n) - 1)


def arg_min(a, rep_sets, n, first=0):
    """(phi, index of the arg-min or NONE, T or None) of the set a against the sets of one replicate, which are numbered from `first`."""
    phi = T.p_of(a, n) - 1
    for b in rep_sets:
        phi = min(phi, moved_set(a, b, n)[0])
    for k, b in enumerate(rep_sets):
        d, t = moved_set(a, b, n)
        if d == phi:
            return phi, first + k, t
    return phi, NONE, None


def taxa_matrices(n, ref_sets, thr, reps):
    """What pgm_transfer_taxa returns, as lists: phi and arg (nref x nrep), moved (nref x n), counted (nref).  reps: a list of lists
    of sets, taken in the order given (the caller sorts); arg indexes the concatenation of the lists."""
    phi, arg, moved, counted = [], [], [], []
    first = [0]
    for r in reps:
        first.append(first[-1] + len(r))
    for a, limit in zip(ref_sets, thr):
        row_phi, row_arg, row_moved, c = [], [], [0] * n, 0
        for k, r in enumerate(reps):
            f, s, t = arg_min(a, r, n, first[k])
            row_phi.append(f)
            row_arg.append(s)
            if s != NONE and f <= limit:
                c += 1
                for leaf in range(n):
                    row_moved[leaf] += (t >> leaf) & 1
        phi.append(row_phi); arg.append(row_arg); moved.append(row_moved); counted.append(c)
    return phi, arg, moved, counted


def labelled_sets(tree_text):
    """The leaf set (as the node has it) below every labelled node of a --bootstrap_out line, in the order the labels appear in
    the text (a label follows its node's ')', so: post-order), and the sorted leaf names."""
    root = T.parse(tree_text)
    names = sorted(T.leaves(root))
    index = {s: k for k, s in enumerate(names)}
    out = []

    def walk(node):
        for kid, _, lab in node:
            if not isinstance(kid, str):
                walk(kid)
                if lab != "":
                    out.append(T.leaf_set(kid, index))

    walk(root)
    return out, names


def taxa_texts(tree_text, replicate_texts, cutoff_text="0.3"):
    """(the --bootstrap_taxa text, the --bootstrap_taxa_edges text, detail) for a --bootstrap_out line, the --bootstrap_trees lines
    and the text given to --bootstrap_taxa_cutoff.  detail: {"K", "moved", "pairs": [(canonical reference set, replicate, phi,
    [T of every set of the replicate at distance phi])] for the counted pairs}."""
    cutoff = float(cutoff_text)
    node_sets, names = labelled_sets(tree_text)
    n, N = len(names), len(replicate_texts)
    index = {s: k for k, s in enumerate(names)}
    full = (1 << n) - 1
    reps = []
    for t in replicate_texts:
        r = T.parse(t)
        assert sorted(T.leaves(r)) == names
        reps.append(canonical_sets(T.nontrivial_sets(r, index), n))
    canon = [s ^ full if s & 1 else s for s in node_sets]
    distinct = list(dict.fromkeys(canon))                        # reference edges that share a bipartition enter every sum once
    thr = [math.floor(cutoff * (T.p_of(a, n) - 1)) for a in distinct]
    _, _, moved, counted = taxa_matrices(n, distinct, thr, reps)
    K = sum(counted)
    total = [sum(moved[e][leaf] for e in range(len(distinct))) for leaf in range(n)]
    text = "# replicates %d cutoff %g edges %d counted %d\n" % (N, cutoff, len(distinct), K) + "taxon\tmoved\tscore\n"
    for leaf, name in enumerate(names):
        text += "%s\t%d\t%.6f\n" % (name, total[leaf], total[leaf] / K if K else 0.0)
    edges = "edge\tp\tcounted" + "".join("\t" + s for s in names) + "\n"
    for k, a in enumerate(canon):
        e = distinct.index(a)
        edges += "%d\t%d\t%d" % (k, T.p_of(a, n), counted[e]) + "".join("\t%d" % v for v in moved[e]) + "\n"
    pairs = []
    for a, limit in zip(distinct, thr):
        for r, rep in enumerate(reps):
            f, s, _ = arg_min(a, rep, n)
            if s != NONE and f <= limit:
                pairs.append((a, r, f, [t for d, t in (moved_set(a, b, n) for b in rep) if d == f]))
    return text, edges, {"K": K, "moved": total, "pairs": pairs}
