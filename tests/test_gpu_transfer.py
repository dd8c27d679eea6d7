"""`--bootstrap_tbe` on the MI355X: pgm_transfer_min against the double loop of tests/transfer_ref.py (exact integers) over the
shapes around the 64-set tiles and the 64-bit words, its contents (garbage in the output, sets that are present, complemented
inputs, the clamp, p = 1, a full last word), repeated and mixed calls, every rejection, and the product driver with
PGM_DEVICE_TRANSFER=1 against the CPU oracle driver, all three files byte for byte.  Every driver run is a child process under a
time limit of its own."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import batch_util as bu
import test_cpu_transfer as TC
import transfer_ref as T

pytestmark = pytest.mark.gpu
P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
GARBAGE = 0xDEADBEEF


def words_of(sets, n):
    return np.array(T.to_words(sets, n), np.uint64).reshape(len(sets), (n + 63) // 64)


def device_phi(ctx, n, ref, reps):
    """ctx.transfer_min on Python integer sets, the output preset to garbage."""
    off = np.concatenate([[0], np.cumsum([len(r) for r in reps])]).astype(np.uint32)
    phi = np.full((len(ref), len(reps)), GARBAGE, np.uint32)
    got = ctx.transfer_min(n, words_of(ref, n), off, words_of([s for r in reps for s in r], n), phi)
    assert got is phi
    return phi


def check(ctx, n, ref, reps, what):
    phi = device_phi(ctx, n, ref, reps)
    want = np.array(T.phi_matrix(n, ref, reps), np.uint32).reshape(len(ref), len(reps))
    assert np.array_equal(phi, want), (what, np.argwhere(phi != want)[:5].tolist())
    return phi


def tree_sets(n, count, rng):
    """`count` non-trivial sets of random trees over n leaves, binary and multifurcating in turn (a tree has at most n - 3)."""
    out = []
    k = 0
    while len(out) < count:
        out += T.random_tree_sets(n, rng, multifurcating=bool(k % 2))
        k += 1
        if n < 4 or (k > 4 and not out):
            break
    return out[:count]


def bit_sets(n, count, rng, proper):
    """`count` random bit sets that are the sets of no tree; proper: neither empty nor full (what a reference set must be)."""
    out = []
    while len(out) < count:
        s = rng.getrandbits(n)
        if not proper or 0 < T.popcount(s) < n:
            out.append(s)
    return out


def make_sets(kind, n, count, rng, proper):
    if kind == "tree" and n > 4:   # (4 leaves: one bipartition a tree; too few to fill a tile)
        return tree_sets(n, count, rng)
    return bit_sets(n, count, rng, proper)


COUNTS = [0, 1, 63, 64, 65, 130]   # sets of one replicate: none, fewer than a tile, a tile, more than one tile


@pytest.mark.parametrize("nleaves", [4, 5, 63, 64, 65, 128, 129, 200])
def test_transfer_min_equals_the_python_loop_over_the_shapes(ctx, nleaves):
    rng = random.Random(9000 + nleaves)
    case = 0
    for nref in (1, 63, 64, 65, 130):
        for nrep in (1, 3):
            kind = "tree" if case % 2 == 0 else "bits"
            counts = [COUNTS[(case + 2 * k) % len(COUNTS)] for k in range(nrep)]   # mixed within one call; every count with either kind over the loop
            ref = make_sets(kind, nleaves, nref, rng, True)
            reps = [make_sets("bits" if kind == "tree" and k % 2 else kind, nleaves, c, rng, False) for k, c in enumerate(counts)]
            check(ctx, nleaves, ref, reps, (nleaves, nref, nrep, kind, counts))
            case += 1
    # every replicate size once more as a call of its own, then all of them in one call
    ref = make_sets("bits", nleaves, 65, rng, True)
    reps = [make_sets("tree" if k % 2 else "bits", nleaves, c, rng, False) for k, c in enumerate(COUNTS)]
    for r in reps:
        check(ctx, nleaves, ref, [r], (nleaves, "alone", len(r)))
    check(ctx, nleaves, ref, reps, (nleaves, "all counts"))


@pytest.mark.parametrize("nleaves", [5, 64, 128, 200])
def test_contents(ctx, nleaves):
    n = nleaves
    rng = random.Random(77 + n)
    full = (1 << n) - 1
    # reference sets that a replicate holds (on either side) give 0 there and only there
    ref = make_sets("tree", n, 70, rng, True) if n > 5 else [0b00011, 0b01100, 0b10001]
    others = bit_sets(n, 66, rng, False)
    reps = [others + ref[::2], others, [s ^ full for s in ref[1::2]] + others[:3], []]
    phi = check(ctx, n, ref, reps, "present sets")
    assert np.all(phi[0::2, 0] == 0) and np.all(phi[1::2, 2] == 0)
    want_zero = np.array([[any(b in (a, a ^ full) for b in r) for r in reps] for a in ref])
    assert np.array_equal(phi == 0, want_zero | np.array([[T.p_of(a, n) == 1] * len(reps) for a in ref]))
    # every input set complemented: the same phi
    flipped = device_phi(ctx, n, [s ^ full for s in ref], [[s ^ full for s in r] for r in reps])
    assert np.array_equal(flipped, phi)
    half = device_phi(ctx, n, ref, [[s ^ full for s in r] for r in reps])
    assert np.array_equal(half, phi)
    # a replicate whose sets are all far from small reference sets: the clamp p - 1; a set with p = 1: 0
    small = [0b11, 0b111 << (n - 3), full ^ 0b1001, 1, full ^ (1 << (n - 1))]
    if n >= 64:
        far = [sum(1 << k for k in range(n) if (k >> j) & 1) for j in range(3)]   # about half the leaves, a few from any small set
        phi = check(ctx, n, small, [far, [], far * 30], "clamp")
        want = np.array([[T.p_of(a, n) - 1] * 3 for a in small], np.uint32)
        assert np.array_equal(phi, want) and list(want[:, 0]) == [1, 2, 1, 0, 0]
    else:
        phi = check(ctx, n, small, [[], []], "clamp")
        assert [list(r) for r in phi] == [[1, 1], [1, 1], [1, 1], [0, 0], [0, 0]]
    # the last word full: sets that hold the highest leaves, and the complement of a pair
    top = [full ^ 0b11, (full >> 1) ^ full | 1 << (n - 2), full ^ (1 << (n // 2))]
    check(ctx, n, top, [top[:2], [s ^ full for s in top], bit_sets(n, 64, rng, False) + [full]], "full last word")


def test_repeated_and_mixed_calls(ctx):
    rng = random.Random(5)
    big_ref = tree_sets(200, 130, rng)
    big_reps = [tree_sets(200, 130, rng), bit_sets(200, 65, rng, False), tree_sets(200, 64, rng)]
    a = check(ctx, 200, big_ref, big_reps, "large")
    b = device_phi(ctx, 200, big_ref, big_reps)
    assert np.array_equal(a, b)                                           # two calls, one result
    small_ref = [0b00011, 0b01100]
    check(ctx, 5, small_ref, [[0b00110], []], "small after large")        # sees nothing of the large call's buffers
    check(ctx, 65, bit_sets(65, 3, rng, True), [bit_sets(65, 2, rng, False)], "small, two words")
    c = device_phi(ctx, 200, big_ref, big_reps)
    assert np.array_equal(a, c)
    got = ctx.transfer_min(5, words_of(small_ref, 5), np.array([0, 1, 1], np.uint32), words_of([0b00110], 5))   # (output allocated by the binding)
    assert got.dtype == np.uint32 and got.tolist() == [[1, 1], [1, 1]]
    with pytest.raises(ValueError):
        ctx.transfer_min(5, words_of(small_ref, 5), np.array([0, 1], np.uint32), words_of([0b00110], 5), np.zeros((2, 2), np.uint32))


def test_invalid_arguments(ctx):
    import prographmsa_amd as pg
    n, nref, nrep = 70, 3, 2
    rng = random.Random(6)
    ref = words_of(bit_sets(n, nref, rng, True), n)
    rep = words_of(bit_sets(n, 5, rng, False), n)
    off = np.array([0, 2, 5], np.uint32)
    phi = np.full((nref, nrep), GARBAGE, np.uint32)
    f = pg.lib.pgm_transfer_min
    args = [ctx.handle, n, nref, P(ref, C.c_uint64), nrep, P(off, C.c_uint32), P(rep, C.c_uint64), P(phi, C.c_uint32)]
    bad = []

    def call(changes):
        a = list(args)
        for k, v in changes.items():
            a[k] = v
        bad.append((sorted(changes), f(*a)))

    for k in (0, 3, 5, 6, 7):                                             # null pointers (rep: the call has sets)
        call({k: None})
    for k, v in ((1, 3), (1, 0), (2, 0), (4, 0)):                         # nleaves < 4, nref == 0, nrep == 0
        call({k: v})
    call({2: 0x10000, 4: 0x10000})                                        # nref * nrep beyond 32 bits (refused before any set is read)
    for o in ([1, 2, 5], [0, 3, 2], [0, 6, 5]):                           # rep_off not from 0, not ascending
        o = np.array(o, np.uint32)
        call({5: P(o, C.c_uint32)})
    high = ref.copy(); high[1, 1] |= np.uint64(1 << 6)                    # leaf 70 of 70 in a reference set
    call({3: P(high, C.c_uint64)})
    high_rep = rep.copy(); high_rep[4, 1] |= np.uint64(1 << 63)           # ... in the last replicate set
    call({6: P(high_rep, C.c_uint64)})
    empty = ref.copy(); empty[2, :] = 0                                   # a reference set with p == 0: empty, full
    call({3: P(empty, C.c_uint64)})
    fullset = ref.copy(); fullset[0, 0] = np.uint64(0xFFFFFFFFFFFFFFFF); fullset[0, 1] = np.uint64(0x3F)
    call({3: P(fullset, C.c_uint64)})
    assert all(rc == pg.PGM_ERR_INVALID for _, rc in bad), bad
    assert np.all(phi == GARBAGE)                                         # nothing was launched, nothing written
    # with no sets at all rep may be null, and the context is as good as before
    none = np.zeros(nrep + 1, np.uint32)
    assert f(ctx.handle, n, nref, P(ref, C.c_uint64), nrep, P(none, C.c_uint32), None, P(phi, C.c_uint32)) == 0
    sets = [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in ref]
    assert phi.tolist() == [[T.p_of(s, n) - 1] * nrep for s in sets]
    assert f(*args) == 0
    rsets = [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in rep]
    assert phi.tolist() == T.phi_matrix(n, sets, [rsets[:2], rsets[2:]])


# ---- the driver -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    import prographmsa_amd as pg
    assert os.path.exists(pg.PGMSA_PATH), "product driver not built"
    return pg.PGMSA_PATH


@pytest.fixture(scope="module")
def fams(tmp_path_factory):
    return TC.families(tmp_path_factory.mktemp("transfer_fams"))


@pytest.mark.parametrize("n", [13, 70])
@pytest.mark.parametrize("opts", [[], ["-m"]], ids=["default", "m"])
def test_driver_equals_the_oracle_driver(exe, oracle_build, fams, tmp_path, n, opts):
    env = dict(os.environ, PGM_DEVICE_TRANSFER="1")
    got = TC.run_tbe(exe, fams[n], tmp_path, "hip", ["-i", "0"] + opts, env=env)
    ref = TC.run_tbe(os.path.join(oracle_build, "pgmsa_oracle"), fams[n], tmp_path, "ref", ["-i", "0"] + opts)
    assert got.stats["backend"] == "hip" and ref.stats["backend"] == "oracle"
    assert got.out == ref.out and got.tbe == ref.tbe and got.trees == ref.trees and got.stdout == ref.stdout
    assert len(got.tbe) > 0 and got.trees.count("\n") == TC.N
    st = got.stats
    assert st["bootstrap_transfer_calls"] >= 1 and st["bootstrap_transfer_kernel_ms"] > 0 and "PGM_DEVICE_TRANSFER" in st["switches"]
    host = TC.run_tbe(exe, fams[n], tmp_path, "host", ["-i", "0"] + opts, env=dict(os.environ, PGM_HOST_TRANSFER="1"))
    assert (host.out, host.tbe, host.trees) == (got.out, got.tbe, got.trees) and host.stats["bootstrap_transfer_kernel_ms"] == 0


def test_default_route_by_size(exe, fams, tmp_path):
    """Without a switch the host loop runs below kTransferDeviceMin = 256 taxa and the device from there on; either way the file
    is the Python statement's."""
    import gen
    small = TC.run_tbe(exe, fams[24], tmp_path, "small", ["-T", "-i", "0"], n=4)
    assert small.stats["bootstrap_transfer_calls"] == 1 and small.stats["bootstrap_transfer_kernel_ms"] == 0
    TC.check_against_python(small, 24, n=4)
    fa = str(tmp_path / "n256.fa")
    with open(fa, "w") as f:
        f.write(gen.fasta(gen.gen(256, 60, 99, sub=0.1)))
    large = TC.run_tbe(exe, fa, tmp_path, "large", ["-T", "-i", "0"], n=4)
    assert large.stats["bootstrap_transfer_calls"] == 1 and large.stats["bootstrap_transfer_kernel_ms"] > 0 and large.stats["switches"] == ""
    TC.check_against_python(large, 256, n=4)
