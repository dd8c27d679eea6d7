"""`--bootstrap_taxa` on the MI355X: pgm_transfer_taxa against the loops of tests/taxa_ref.py (exact integers, every output preset
to garbage) over the shapes around the 64-set tiles and the 32- and 64-bit words, its contents (a set twice, ties across tiles, a
set and its complement, thresholds of 0 and 2^32 - 1, a replicate only the clamp reaches, a full last word and tail bits), more than one tile of
leaves and chunk of replicates in the count kernel, phi against pgm_transfer_min, repeated and mixed calls, every rejection, and the product driver with PGM_DEVICE_TRANSFER=1 against the
CPU oracle driver, all files byte for byte.  Every driver run is a child process under a time limit of its own."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import batch_util as bu
import taxa_ref as X
import test_cpu_taxa as TX
import test_cpu_transfer as TC
import test_gpu_transfer as TG
import transfer_ref as T

pytestmark = pytest.mark.gpu
P = TG.P
GARBAGE = 0xDEADBEEF
NONE = X.NONE
COUNTS = TG.COUNTS


def device_taxa(ctx, n, ref, thr, reps):
    """ctx.transfer_taxa on Python integer sets, every output preset to garbage: (phi, arg, moved, counted)."""
    off = np.concatenate([[0], np.cumsum([len(r) for r in reps])]).astype(np.uint32)
    out = tuple(np.full(s, GARBAGE, np.uint32) for s in ((len(ref), len(reps)), (len(ref), len(reps)), (len(ref), n), (len(ref),)))
    got = ctx.transfer_taxa(n, TG.words_of(ref, n), np.array(thr, np.uint32), off, TG.words_of([s for r in reps for s in r], n), out)
    assert all(g is o for g, o in zip(got, out))
    return out


def check(ctx, n, ref, thr, reps, what):
    got = device_taxa(ctx, n, ref, thr, reps)
    want = X.taxa_matrices(n, ref, thr, reps)
    for name, g, w in zip(("phi", "arg", "moved", "counted"), got, want):
        w = np.array(w, np.uint32).reshape(g.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())
    assert np.array_equal(got[0], TG.device_phi(ctx, n, ref, reps)), (what, "phi of pgm_transfer_min")
    return got


def thresholds(kind, ref, n, rng):
    if kind == "zero": return [0] * len(ref)
    if kind == "all": return [0xFFFFFFFF] * len(ref)
    return [rng.randint(0, max(0, T.p_of(a, n) - 1)) for a in ref]          # around the values phi takes


@pytest.mark.parametrize("nleaves", [4, 5, 63, 64, 65, 128, 129, 200])
def test_transfer_taxa_equals_the_python_loop_over_the_shapes(ctx, nleaves):
    rng = random.Random(9100 + nleaves)
    case = 0
    for nref in (1, 63, 64, 65, 130):
        for nrep in (1, 3):
            kind = "tree" if case % 2 == 0 else "bits"
            counts = [COUNTS[(case + 2 * k) % len(COUNTS)] for k in range(nrep)]   # mixed within one call; every count with either kind over the loop
            ref = TG.make_sets(kind, nleaves, nref, rng, True)
            reps = [TG.make_sets("bits" if kind == "tree" and k % 2 else kind, nleaves, c, rng, False) for k, c in enumerate(counts)]
            thr = thresholds(("mixed", "all", "zero")[case % 3], ref, nleaves, rng)
            check(ctx, nleaves, ref, thr, reps, (nleaves, nref, nrep, kind, counts))
            case += 1
    # every replicate size in one call, every pair with a set counted
    ref = TG.make_sets("bits", nleaves, 65, rng, True)
    reps = [TG.make_sets("tree" if k % 2 else "bits", nleaves, c, rng, False) for k, c in enumerate(COUNTS)]
    _, arg, moved, counted = check(ctx, nleaves, ref, [0xFFFFFFFF] * 65, reps, (nleaves, "all counts"))
    assert np.all(arg[:, 0] == NONE) and np.all(counted <= len(COUNTS) - 1)             # (the replicate without a set names none)


@pytest.mark.parametrize("nleaves,nrep", [(256, 256), (257, 257), (300, 520)])
def test_more_than_one_tile_of_leaves_and_chunk_of_replicates(ctx, nleaves, nrep):
    """The count kernel walks the leaves 256 at a time and stages the replicates 256 at a time: one and two tiles of leaves, one,
    two and three chunks of replicates, with sets near enough to the reference sets that most pairs are counted."""
    n = nleaves
    rng = random.Random(4000 + n)
    ref = TG.bit_sets(n, 3, rng, True)
    reps = []
    for r in range(nrep):
        near = [ref[(r + k) % 3] ^ sum(1 << b for b in {rng.randrange(n) for _ in range(rng.randint(0, 3))}) ^ (((1 << n) - 1) * (k & 1)) for k in range(1 + r % 3)]
        reps.append(near + TG.bit_sets(n, r % 2, rng, False))
    phi, arg, moved, counted = check(ctx, n, ref, [2, 0xFFFFFFFF, 0], reps, (n, nrep))
    last = 256 * ((nrep - 1) // 256)                                                                # the first replicate of the last chunk
    assert (arg[1, last:] != NONE).any() and counted[1] == (arg[1] != NONE).sum() and counted[2] <= counted[0] <= counted[1]
    assert moved[1, 256 * ((n - 1) // 256):].sum() > 0 and moved[0].sum() > 0 and moved[2].sum() == 0   # moved leaves in the last tile too


@pytest.mark.parametrize("nleaves", [5, 64, 128, 200])
def test_contents(ctx, nleaves):
    n = nleaves
    rng = random.Random(177 + n)
    full = (1 << n) - 1
    ALL = 0xFFFFFFFF
    ref = TG.make_sets("tree", n, 70, rng, True) if n > 5 else [0b00011, 0b01100, 0b10001]
    others = TG.bit_sets(n, 66, rng, False)
    # a set present twice at different indices, in different tiles: the lowest index wins, and nothing moves
    reps = [others + ref + others[:5] + ref, ref[::-1] + others]
    phi, arg, moved, counted = check(ctx, n, ref, [0] * len(ref), reps, "a set twice")
    assert np.all(phi == 0) and np.all(moved == 0) and np.all(counted == 2)
    first = [min(k for k, b in enumerate(reps[0]) if b in (a, a ^ full)) for a in ref]
    assert arg[:, 0].tolist() == first and arg[:, 1].tolist() == [len(reps[0]) + min(k for k, b in enumerate(reps[1]) if b in (a, a ^ full)) for a in ref]
    # equal-distance sets with different T in different tiles of one replicate: the first one's taxa are counted
    if n >= 64:
        a = sum(1 << k for k in range(4, 24))
        near = [a ^ (1 << 30), a ^ (1 << 40), (a ^ (1 << 50)) ^ full]                       # each one leaf from a: leaves 30, 40, 50
        far = [s for s in TG.bit_sets(n, 200, rng, False) if X.moved_set(a, s, n)[0] > 1]
        for order, leaf in (((0, 1, 2), 30), ((1, 2, 0), 40), ((2, 0, 1), 50)):
            rep = far[:70] + [near[order[0]]] + far[70:140] + [near[order[1]]] + far[140:150] + [near[order[2]]]
            phi, arg, moved, counted = check(ctx, n, [a], [ALL], [rep], ("tie", order))
            assert phi[0, 0] == 1 and arg[0, 0] == 70 and counted[0] == 1 and moved[0].tolist() == [int(t == leaf) for t in range(n)]
    # a set and its complement: the same moved taxa (the other orientation of T)
    phi, arg, moved, counted = check(ctx, n, ref, [ALL] * len(ref), [others, [s ^ full for s in others]], "complemented replicate")
    flipped = device_taxa(ctx, n, [s ^ full for s in ref], [ALL] * len(ref), [others, [s ^ full for s in others]])
    for g, w in zip(flipped, (phi, arg, moved, counted)):
        assert np.array_equal(g, w)
    assert moved.sum() == sum(int(phi[e, r]) for e in range(len(ref)) for r in range(2) if arg[e, r] != NONE)   # |T| = d
    # thresholds: 0 counts only present sets, 2^32 - 1 every pair with a set
    phi_all, arg_all, _, counted_all = check(ctx, n, ref, [ALL] * len(ref), [others + ref[:3], others], "thr all")
    phi0, arg0, moved0, counted0 = check(ctx, n, ref, [0] * len(ref), [others + ref[:3], others], "thr 0")
    assert np.all(moved0 == 0) and np.array_equal(counted0, ((phi0 == 0) & (arg0 != NONE)).sum(axis=1)) and np.all(counted0[:3] >= 1)
    assert np.array_equal(phi0, phi_all) and np.array_equal(arg0[:, 1], arg_all[:, 1])        # the threshold changes neither phi nor arg
    assert counted_all.tolist() == (arg_all != NONE).sum(axis=1).tolist()
    # a replicate that only the clamp reaches: NONE, not counted, whatever the threshold
    small = [0b11, 0b111 << (n - 3), full ^ 0b1001, 1, full ^ (1 << (n - 1))]
    if n >= 64:
        far3 = [sum(1 << k for k in range(n) if (k >> j) & 1) for j in range(3)]            # about half the leaves, a few from any small set
        phi, arg, moved, counted = check(ctx, n, small, [ALL] * 5, [far3, [], far3 * 30], "clamp")
        assert np.all(arg == NONE) and np.all(counted == 0) and np.all(moved == 0) and phi[:, 0].tolist() == [1, 2, 1, 0, 0]
    else:
        phi, arg, moved, counted = check(ctx, n, small, [ALL] * 5, [[], []], "clamp")
        assert np.all(arg == NONE) and np.all(counted == 0) and np.all(moved == 0)
    # the last word full and tail bits: sets of the highest leaves, their complements, the full set as a replicate set
    top = [full ^ 0b11, (full >> 1) ^ full | 1 << (n - 2), full ^ (1 << (n // 2))]
    phi, arg, moved, counted = check(ctx, n, top, [ALL] * 3, [top[:2], [s ^ full for s in top], TG.bit_sets(n, 64, rng, False) + [full], [full, 0]], "full last word")
    b = top[1] | 1 << (n - 3)                                                              # the two highest leaves and leaf n - 3: T = {n - 3}, either way
    phi, arg, moved, counted = check(ctx, n, [top[1]], [ALL], [[b], [b ^ full]], "tail bits")
    assert phi.tolist() == [[1, 1]] and arg.tolist() == [[0, 1]] and counted.tolist() == [2] and moved[0].tolist() == [2 * int(t == n - 3) for t in range(n)]


def test_repeated_and_mixed_calls(ctx):
    rng = random.Random(15)
    big_ref = TG.tree_sets(200, 130, rng)
    big_reps = [TG.tree_sets(200, 130, rng), TG.bit_sets(200, 65, rng, False), TG.tree_sets(200, 64, rng)]
    thr = [0xFFFFFFFF] * 130
    a = check(ctx, 200, big_ref, thr, big_reps, "large")
    b = device_taxa(ctx, 200, big_ref, thr, big_reps)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                 # two calls, one result
    small_ref = [0b00011, 0b01100]
    check(ctx, 5, small_ref, [1, 1], [[0b00110], []], "small after large")   # sees nothing of the large call's buffers
    check(ctx, 65, TG.bit_sets(65, 3, rng, True), [40] * 3, [TG.bit_sets(65, 2, rng, False)], "small, two words")
    TG.check(ctx, 200, big_ref, big_reps, "transfer_min between")           # the other entry shares the scratch buffers
    c = device_taxa(ctx, 200, big_ref, thr, big_reps)
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    got = ctx.transfer_taxa(5, TG.words_of(small_ref, 5), [1, 1], np.array([0, 1, 1], np.uint32), TG.words_of([0b00111], 5))   # (outputs allocated by the binding)
    assert all(g.dtype == np.uint32 for g in got)
    assert [g.tolist() for g in got] == [[[1, 1], [1, 1]], [[0, NONE], [NONE, NONE]], [[0, 0, 1, 0, 0], [0, 0, 0, 0, 0]], [1, 0]]
    with pytest.raises(ValueError):
        ctx.transfer_taxa(5, TG.words_of(small_ref, 5), [1], np.array([0, 1, 1], np.uint32), TG.words_of([0b00111], 5))


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    n, nref, nrep = 70, 3, 2
    rng = random.Random(16)
    ref = TG.words_of(TG.bit_sets(n, nref, rng, True), n)
    rep = TG.words_of(TG.bit_sets(n, 5, rng, False), n)
    off = np.array([0, 2, 5], np.uint32)
    thr = np.array([5, 0, 0xFFFFFFFF], np.uint32)
    outs = [np.full(s, GARBAGE, np.uint32) for s in ((nref, nrep), (nref, nrep), (nref, n), (nref,))]
    f = pg.lib.pgm_transfer_taxa
    args = [ctx.handle, n, nref, P(ref, C.c_uint64), P(thr, C.c_uint32), nrep, P(off, C.c_uint32), P(rep, C.c_uint64)] + [P(a, C.c_uint32) for a in outs]
    bad = []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 3, 4, 6, 7, 8, 9, 10, 11):                               # null pointers (rep: the call has sets)
        call({k: None})
    for k, v in ((1, 3), (1, 0), (2, 0), (5, 0)):                         # nleaves < 4, nref == 0, nrep == 0
        call({k: v})
    call({2: 0x10000, 5: 0x10000})                                        # nref * nrep beyond 32 bits (refused before any set is read)
    call({1: 0x10000, 2: 0x10000})                                        # nref * nleaves beyond 32 bits
    call({1: 0x80000000, 2: 1})                                           # nleaves beyond 2^31 - 1
    for o in ([1, 2, 5], [0, 3, 2], [0, 6, 5]):                           # rep_off not from 0, not ascending
        o = np.array(o, np.uint32)
        call({6: P(o, C.c_uint32)})
    high = ref.copy(); high[1, 1] |= np.uint64(1 << 6)                    # leaf 70 of 70 in a reference set
    call({3: P(high, C.c_uint64)})
    high_rep = rep.copy(); high_rep[4, 1] |= np.uint64(1 << 63)           # ... in the last replicate set
    call({7: P(high_rep, C.c_uint64)})
    empty = ref.copy(); empty[2, :] = 0                                   # a reference set with p == 0: empty, full
    call({3: P(empty, C.c_uint64)})
    fullset = ref.copy(); fullset[0, 0] = np.uint64(0xFFFFFFFFFFFFFFFF); fullset[0, 1] = np.uint64(0x3F)
    call({3: P(fullset, C.c_uint64)})
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    assert all(np.all(a == GARBAGE) for a in outs)                        # nothing was launched, nothing written
    # with no sets at all rep may be null, and the context is as good as before
    sets = [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in ref]
    rsets = [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in rep]
    none = np.zeros(nrep + 1, np.uint32)
    a = list(args); a[6] = P(none, C.c_uint32); a[7] = None
    assert f(*a) == 0
    assert outs[0].tolist() == [[T.p_of(s, n) - 1] * nrep for s in sets] and np.all(outs[1] == NONE) and np.all(outs[2] == 0) and np.all(outs[3] == 0)
    assert f(*args) == 0
    want = X.taxa_matrices(n, sets, thr.tolist(), [rsets[:2], rsets[2:]])
    assert [o.tolist() for o in outs] == list(want)


# ---- the driver -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    return TC.families(tmp_path_factory.mktemp("taxa_fams"))


@pytest.mark.parametrize("n", [24, 70])
@pytest.mark.parametrize("cutoff", ["0.3", "0.99"])
def test_driver_equals_the_oracle_driver(exe, oracle_build, fams, tmp_path, n, cutoff):
    env = dict(os.environ, PGM_DEVICE_TRANSFER="1")
    got = TX.run_taxa(exe, fams[n], tmp_path, "hip", ["-i", "0"], cutoff=cutoff, env=env)
    ref = TX.run_taxa(os.path.join(oracle_build, "pgmsa_oracle"), fams[n], tmp_path, "ref", ["-i", "0"], cutoff=cutoff)
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    for k in ("out", "tbe", "trees", "taxa", "edges", "stdout"):
        assert getattr(got, k) == getattr(ref, k) and len(getattr(got, k)) > 0, k
    st = got.stats
    assert st["bootstrap_taxa_calls"] >= 1 and st["bootstrap_taxa_kernel_ms"] > 0 and "PGM_DEVICE_TRANSFER" in st["switches"]
    host = TX.run_taxa(exe, fams[n], tmp_path, "host", ["-i", "0"], cutoff=cutoff, env=dict(os.environ, PGM_HOST_TRANSFER="1"))
    assert (host.out, host.tbe, host.trees, host.taxa, host.edges) == (got.out, got.tbe, got.trees, got.taxa, got.edges)
    assert host.stats["bootstrap_taxa_kernel_ms"] == 0
    if n == 70:
        assert sum(TX.check_against_python(got, 70, cutoff)["moved"]) > 0   # (not a comparison of zeros)


def test_default_route_by_size(exe, fams, tmp_path):
    """Without a switch the host loop runs below kTransferDeviceMin = 256 taxa and the device from there on; either way the files
    are the Python statement's."""
    import gen
    small = TX.run_taxa(exe, fams[24], tmp_path, "small", ["-T", "-i", "0"], n=4)
    assert small.stats["bootstrap_taxa_calls"] == 1 and small.stats["bootstrap_taxa_kernel_ms"] == 0
    TX.check_against_python(small, 24, n=4)
    fa = str(tmp_path / "n256.fa")
    with open(fa, "w") as f:
        f.write(gen.fasta(gen.gen(256, 60, 99, sub=0.1)))
    large = TX.run_taxa(exe, fa, tmp_path, "large", ["-T", "-i", "0"], n=4)
    assert large.stats["bootstrap_taxa_calls"] == 1 and large.stats["bootstrap_taxa_kernel_ms"] > 0 and large.stats["switches"] == ""
    TX.check_against_python(large, 256, n=4)
