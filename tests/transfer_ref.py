"""The transfer bootstrap expectation (TBE; Lemoine et al., Nature 2018) stated independently of the C++: a newick
reader of its own, leaf sets as Python integers over the leaves in sorted-name order, the transfer index as a double loop with
bin(x).count("1"), the label "%.6f" % (1.0 - S / (N * (p - 1))), and a generator of random binary and multifurcating trees.

A tree is a leaf name (str) or a list of (child, branch length text, label text); a labelled tree text is rebuilt from the pieces
the reader kept, so everything but the labels is the input's own bytes."""
import re

_NAME = re.compile(r"[^,:();]+")
_LEN = re.compile(r":[^,();]+")
_LABEL = re.compile(r"[^,:();]*")


def parse(text):
    """One newick line "(...);" with a branch length on every edge and optional labels after ')'.
    Returns the root: nested lists [(child, ':length', label), ...], a leaf being its name."""
    pos = 0

    def node():
        nonlocal pos
        if text[pos] != "(":
            m = _NAME.match(text, pos)
            pos = m.end()
            return m.group(0)
        pos += 1
        kids = []
        while True:
            kid = node()
            label = ""
            if not isinstance(kid, str):
                m = _LABEL.match(text, pos)
                label = m.group(0)
                pos = m.end()
            m = _LEN.match(text, pos)
            assert m, "no branch length at %d" % pos
            pos = m.end()
            kids.append((kid, m.group(0), label))
            if text[pos] == ",":
                pos += 1
                continue
            assert text[pos] == ")", text[pos:pos + 20]
            pos += 1
            return kids

    root = node()
    assert text[pos:].strip() == ";", text[pos:pos + 20]
    return root


def leaves(node):
    return [node] if isinstance(node, str) else [x for kid, _, _ in node for x in leaves(kid)]


def popcount(x):
    return bin(x).count("1")


def leaf_set(node, index):
    s = 0
    for name in leaves(node):
        assert not (s >> index[name]) & 1, "leaf %s twice" % name
        s |= 1 << index[name]
    return s


def nontrivial_sets(root, index):
    """The leaf set below every non-root internal node whose bipartition has at least two leaves on either side (as the node has
    it: either side may be the stored one)."""
    n = len(index)
    out = []

    def walk(node):
        for kid, _, _ in node:
            if not isinstance(kid, str):
                walk(kid)
                s = leaf_set(kid, index)
                if 2 <= popcount(s) <= n - 2:
                    out.append(s)

    walk(root)
    return out


def p_of(s, n):
    return min(popcount(s), n - popcount(s))


def phi(a, rep_sets, n):
    """The transfer index of the set a against a replicate's non-trivial sets."""
    best = p_of(a, n) - 1
    for b in rep_sets:
        h = popcount(a ^ b)
        best = min(best, h, n - h)
    return best


def phi_matrix(n, ref_sets, reps):
    """[[phi(e, r) for r] for e]; reps: a list of lists of sets."""
    return [[phi(a, rep, n) for rep in reps] for a in ref_sets]


def label(S, N, p):
    return "%.6f" % (1.0 - S / (N * (p - 1)))


def tbe_text(tree_text, replicate_texts):
    """The --bootstrap_tbe line for the tree of a --bootstrap_out line (its labels are dropped) and the replicates' newick lines;
    also {leaf set of a labelled node: (S, p, [phi per replicate])}."""
    root = parse(tree_text)
    names = sorted(leaves(root))
    assert len(set(names)) == len(names)
    index = {s: k for k, s in enumerate(names)}
    n, N = len(names), len(replicate_texts)
    reps = []
    for t in replicate_texts:
        r = parse(t)
        assert sorted(leaves(r)) == names
        reps.append(nontrivial_sets(r, index))
    detail = {}

    def fmt(node):
        if isinstance(node, str):
            return node
        parts = []
        for kid, length, _ in node:
            text = fmt(kid)
            if not isinstance(kid, str):
                s = leaf_set(kid, index)
                p = p_of(s, n)
                if p >= 2:
                    row = [phi(s, rep, n) for rep in reps]
                    detail[s] = (sum(row), p, row)
                    text += label(sum(row), N, p)
            parts.append(text + length)
        return "(" + ",".join(parts) + ")"

    return fmt(root) + ";\n", detail


# ---- random trees ------------------------------------------------------------------------------------------------------
def random_tree(names, rng, multifurcating=False):
    """A random rooted tree over `names`: clusters are joined at random, two at a time, or up to four with `multifurcating`;
    the root of a binary tree may have two or three children."""
    nodes = list(names)
    rng.shuffle(nodes)
    stop = min(len(nodes), rng.randint(2, 4 if multifurcating else 3))   # children of the root
    while len(nodes) > stop:
        k = rng.randint(2, min(4, len(nodes) - stop + 1)) if multifurcating else 2
        picked = [nodes.pop(rng.randrange(len(nodes))) for _ in range(k)]
        nodes.append([(c, ":%g" % (rng.randint(1, 99) / 100.0), "") for c in picked])
    return [(c, ":%g" % (rng.randint(1, 99) / 100.0), "") for c in nodes]


def random_tree_sets(n, rng, multifurcating=False):
    """The non-trivial sets of a random tree over n leaves, each on a random side."""
    names = ["t%05d" % k for k in range(n)]
    index = {s: k for k, s in enumerate(names)}
    full = (1 << n) - 1
    return [s ^ full if rng.random() < 0.5 else s for s in nontrivial_sets(random_tree(names, rng, multifurcating), index)]


def labels_of(text):
    """{leaf set below a labelled node (as the node has it): label text} of a labelled newick line, and the sorted leaf names."""
    root = parse(text)
    names = sorted(leaves(root))
    index = {s: k for k, s in enumerate(names)}
    out = {}

    def walk(node):
        for kid, _, lab in node:
            if not isinstance(kid, str):
                walk(kid)
                if lab != "":
                    out[leaf_set(kid, index)] = lab

    walk(root)
    return out, names


def to_words(sets, n):
    """Sets as rows of (n + 63) // 64 little-endian 64-bit words."""
    words = (n + 63) // 64
    return [[(s >> (64 * w)) & ((1 << 64) - 1) for w in range(words)] for s in sets]
