"""The independent statement of --topology in python / numpy float64: the plan of joins a fixed topology gives (reference
src/TreeNJ.cpp:31-130 as build_topo_plan in host/bionj.cpp restates it) and BioNJ's join record when the pairs come from such a
plan (TreeNJ.cpp:158-179: the pair is taken from the plan, the criterion is not evaluated).  tests/test_cpu_topology.py pins both
to the host loop and to the goldens of the reference binary (tests/golden/topology.json); tests/test_gpu_topology.py holds
pgm_bionj_plan to them.

A join with a known pair needs two column sums only.  column_sum is bionj_ref.column_sums for one column: the four accumulators
are np.add.accumulate over every fourth element (accumulate adds in index order), so a join costs O(dim) here as well."""
import os
import random

import numpy as np

import batch_util as bu
import gen
from bionj_ref import JOIN_DTYPE, MIN_DIST, MIN_VAR, _clamp_low


# ---- newick: topologies only ----------------------------------------------------------------------------------------------------
def parse_newick(text):
    """The topology of a newick string: a leaf is its name, an internal node the list of its children.  Branch lengths and
    supports are skipped."""
    pos = [0]
    text = "".join(text.split())

    def node():
        if text[pos[0]] == "(":
            pos[0] += 1
            kids = [node()]
            while text[pos[0]] == ",":
                pos[0] += 1
                kids.append(node())
            assert text[pos[0]] == ")", text[pos[0]:pos[0] + 20]
            pos[0] += 1
            out = kids
        else:
            s = pos[0]
            while text[pos[0]] not in ",:();":
                pos[0] += 1
            out = text[s:pos[0]]
        while text[pos[0]] not in ",);":   # support and branch length
            pos[0] += 1
        return out

    t = node()
    assert text[pos[0]] == ";"
    return t


def format_topology(t, length="1"):
    """newick of a topology with the same branch length on every edge (the driver's reader wants one; the values are ignored)."""
    def rec(x):
        return x if isinstance(x, str) else "(" + ",".join(rec(c) + ":" + length for c in x) + ")"
    return rec(t) + ";"


def leaves(t):
    return [t] if isinstance(t, str) else [l for c in t for l in leaves(c)]


def swap_children(t, rng, p=0.5):
    """The same tree with the children reversed at a random subset of its internal nodes."""
    if isinstance(t, str):
        return t
    kids = [swap_children(c, rng, p) for c in t]
    return kids[::-1] if rng.random() < p else kids


def ladder(names):
    """((((a,b),c),d),...)"""
    t = [names[0], names[1]]
    for x in names[2:]:
        t = [t, x]
    return t


def ladder_far(names):
    """(a,(b,(c,(...,(y,z)))))"""
    t = [names[-2], names[-1]]
    for x in names[-3::-1]:
        t = [x, t]
    return t


def balanced(names):
    if len(names) == 1:
        return names[0]
    h = (len(names) + 1) // 2
    return [balanced(names[:h]), balanced(names[h:])]


def random_tree(names, rng):
    """A random binary tree: two random clusters are joined, in random child order, until one is left."""
    pool = list(names)
    while len(pool) > 1:
        a = pool.pop(rng.randrange(len(pool)))
        b = pool.pop(rng.randrange(len(pool)))
        pool.insert(rng.randrange(len(pool) + 1), [a, b])
    return pool[0]


# ---- the plan -------------------------------------------------------------------------------------------------------------------
class TopologyError(ValueError):
    pass


def build_topo_plan(seqs_order, topo):
    """[(index1, index2)] in reduced indices, index1 < index2: one entry per internal node of `topo` (a parsed topology) that has
    sequences of seqs_order below both children, in the order the reference's work list visits the nodes: first the nodes all of
    whose children are leaves, in pre-order of the file, then every node when its last child has been visited (first in, first out).
    A leaf that is no sequence has no index; a node with one such child passes the other child's index up."""
    index_of = {name: i for i, name in enumerate(seqs_order)}
    kids, parent, name = [], [], []   # nodes numbered in pre-order

    stack = [(topo, -1)]   # (no recursion: a ladder is as deep as it has leaves)
    while stack:
        t, p = stack.pop()
        k = len(kids)
        kids.append([])
        parent.append(p)
        name.append(t if isinstance(t, str) else None)
        if p >= 0:
            kids[p].append(k)
        if not isinstance(t, str):
            stack.extend((c, k) for c in reversed(t))
    held = {k: index_of.get(name[k]) for k in range(len(kids)) if not kids[k]}   # node -> reduced index of its cluster (None: none)
    present = set(name[k] for k in held)
    for s in seqs_order:
        if s not in present:
            raise TopologyError('sequence "%s"is missing in given topology' % s)
    for k in range(len(kids)):
        if kids[k] and len(kids[k]) != 2:
            raise TopologyError("node with %d children" % len(kids[k]))
    ready = {k: sum(1 for c in kids[k] if not kids[c]) for k in range(len(kids)) if kids[k]}
    work = [k for k in sorted(ready) if ready[k] == len(kids[k])]
    plan = []
    while work:
        k = work.pop(0)
        i1, i2 = held.pop(kids[k][0]), held.pop(kids[k][1])
        if i1 is None:
            held[k] = i2
        elif i2 is None:
            held[k] = i1
        else:
            i1, i2 = min(i1, i2), max(i1, i2)
            plan.append((i1, i2))
            held[k] = i1
            for m in held:
                if held[m] is not None and held[m] > i2:
                    held[m] -= 1
        p = parent[k]
        if p >= 0:
            ready[p] += 1
            if ready[p] == len(kids[p]):
                work.append(p)
    return plan


# ---- the joins ------------------------------------------------------------------------------------------------------------------
def column_sum(x, j):
    """Sum of column j of a dim x dim matrix, x its dim elements, as eigen_column_sum adds it (dim >= 4)."""
    dim = x.shape[0]
    start = (j * dim) & 1
    end2 = start + ((dim - start) // 4) * 4
    end = start + ((dim - start) // 2) * 2
    acc = [np.add.accumulate(x[start + q:end2:4])[-1] for q in range(4)]
    a0 = acc[0] + acc[2]
    a1 = acc[1] + acc[3]
    if end > end2:
        a0 = a0 + x[end2]
        a1 = a1 + x[end2 + 1]
    res = a0 + a1
    for k in range(0, start):
        res = res + x[k]
    for k in range(end, dim):
        res = res + x[k]
    return res


def bionj_joins_plan(D, V, plan):
    """(joins, final_d, info) like bionj_ref.bionj_joins, the pair of join s taken from plan[s] (len(plan) >= n - 3: what is left
    of the plan when three clusters remain is not used)."""
    D = np.array(D, dtype=np.float64)
    V = np.array(V, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n) and V.shape == (n, n) and n >= 4 and len(plan) >= n - 3
    D = _clamp_low(D, MIN_DIST)
    V = _clamp_low(V, MIN_VAR)
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(V, 0.0)
    act = np.arange(n)
    joins = np.zeros(n - 3, dtype=JOIN_DTYPE)
    info = dict(lambda_at_0=0, lambda_at_1=0)
    fresh = -1
    with np.errstate(all="ignore"):
        for step, dim in enumerate(range(n, 3, -1)):
            if fresh >= 0:   # the row / column the previous join wrote, from its column
                af = act[fresh]
                others = act[np.arange(dim) != fresh]
                d = _clamp_low(D[others, af], MIN_DIST)
                v = _clamp_low(V[others, af], MIN_VAR)
                D[others, af] = d
                D[af, others] = d
                V[others, af] = v
                V[af, others] = v
            index1, index2 = plan[step]
            assert 0 <= index1 < index2 < dim
            a1, a2 = act[index1], act[index2]
            s1 = column_sum(D[act, a1], index1)
            s2 = column_sum(D[act, a2], index2)
            d12 = D[a1, a2]
            dist1 = (d12 + (s1 - s2) / (np.float64(dim) - 2.0)) / 2.0
            dist1 = MIN_DIST if dist1 < MIN_DIST else dist1
            dist1 = d12 if d12 < dist1 else dist1
            dist2 = D[a2, a1] - dist1
            dist2 = MIN_DIST if dist2 < MIN_DIST else dist2
            diffs = V[a2, act] - V[a1, act]
            vsum = np.add.accumulate(np.concatenate([[0.0], diffs]))[-1]
            v12 = V[a1, a2]
            lam = np.float64(0.5) + vsum / (np.float64(2 * (dim - 2)) * v12)
            if np.isnan(lam):
                lam = np.float64(0.5)
            else:   # std::min(std::max(0.0, lambda), 1.0)
                info["lambda_at_0"] += int(lam < 0.0)
                info["lambda_at_1"] += int(lam > 1.0)
                lam = lam if np.float64(0.0) < lam else np.float64(0.0)
                lam = np.float64(1.0) if np.float64(1.0) < lam else lam
            keep = np.arange(dim) != index2
            rest = act[keep]
            nd = lam * (D[a1, rest] - dist1) + (1.0 - lam) * (D[a2, rest] - dist2)
            nv = lam * V[a1, rest] + (1.0 - lam) * V[a2, rest] - lam * (1.0 - lam) * v12
            own = rest == a1
            nd = np.where(own, 0.0, nd)
            nv = np.where(own, 0.0, nv)
            D[a1, rest] = nd
            D[rest, a1] = nd
            V[a1, rest] = nv
            V[rest, a1] = nv
            act = rest
            fresh = index1
            joins[step] = (index1, index2, dist1, dist2)
    return joins, D[np.ix_(act, act)].copy(), info


# ---- the plans of tests/test_gpu_topology.py -------------------------------------------------------------------------------------
PLANS = ["ladder", "far", "balanced", "random"]


def plan(kind, n, seed=0):
    """n - 1 pairs over n clusters: the ladder from the front (always (0, 1)), the ladder from the far end (index2 = dim - 1), a
    balanced tree, a seeded random tree."""
    ids = ["%06d" % i for i in range(n)]   # (no sequences: the rows of the matrix are the names)
    if kind == "ladder":
        t = ladder(ids)
    elif kind == "far":
        t = ladder_far(ids)
    elif kind == "balanced":
        t = balanced(ids)
    else:
        t = random_tree(ids, random.Random(31 * n + seed))
    return build_topo_plan(ids, t)


def read_plan_joins(joins):
    return [(int(j["index1"]), int(j["index2"])) for j in joins]


# ---- the --batch lists of tests/test_cpu_topology.py and tests/test_gpu_topology.py ----------------------------------------------
def _write(path, text):
    with open(str(path), "w") as f:
        f.write(text)
    return str(path)


def topology_families(d, sizes=(3, 5, 8, 13, 24, 4, 9)):
    """Families and a line of options for each: plain, with a guide tree, with a topology, with both."""
    rng = random.Random(77)
    fams = []
    for k, n in enumerate(sizes):
        fa = _write(os.path.join(str(d), "fam%02d.fa" % k), gen.fasta(gen.gen(n, rng.randint(50, 200), 900 + k)))
        names = ["seq%04d" % i for i in range(n)]
        topo = tree = None
        if k % 4 in (2, 3) or k == 0:
            topo = _write(os.path.join(str(d), "fam%02d.topo" % k), format_topology(random_tree(names + (["other"] if k == 2 else []), rng)) + "\n")
        if k % 4 in (1, 3):
            tree = _write(os.path.join(str(d), "fam%02d.nwk" % k), format_topology(random_tree(names, rng), "0.1") + "\n")
        fams.append((fa, tree, topo))
    return fams


def batch_against_solo(exe, solo_exe, fams, opts, d, env=None, solo_env=None):
    outs = [os.path.join(str(d), "b%02d.out" % i) for i in range(len(fams))]
    lst = os.path.join(str(d), "fams.list")
    with open(lst, "w") as f:
        for (fa, tree, topo), o in zip(fams, outs):
            f.write("\t".join([fa, o] + ([tree or "", topo] if topo else [tree] if tree else [])) + "\n")
    r = bu.run(exe, ["--batch", lst, "--stats"] + list(opts), env)
    solo = [bu.run(solo_exe, list(opts) + (["-t", tree] if tree else []) + (["--topology", topo] if topo else []) + [fa], solo_env).stdout for fa, tree, topo in fams]
    bu.assert_identical(outs, solo)
    return bu.stats_of(r.stderr)
