"""Lattices of DISCONNECTED PIECES with known region sizes (plain numpy, no GPU): a chain seeded in a piece of n atoms grows to exactly
that piece and stays there, so its group count ceil(n / 8) and with it the workgroups ceil(groups / 4) that take part in its post-hop passes are
known per chain -- and differ between the chains of one call.  tests/test_piece_lattices.py states the conditions the GPU tests rely on
(tests/test_gpu_batch_composition.py, tests/test_gpu_post_hop_forms.py); the problems those tests run are defined HERE, once, so that the
conditions are checked on the very lattices that run on the GPU.

The problem dict has the shape of test_gpu_spmm_random.random_problem: one atom type, nmax = 0, random blocks per (slot, type).
  * general form: inside a piece a ring (k +- 1) plus random chords; the neighbour table is symmetric (k lists n <=> n lists k), every atom uses at
    most `nslots` slots (slot 1 is the atom itself), every seventh atom keeps two slots free and spreads its neighbours over all slots (absent
    neighbours: 0 entries in front of the count); the operator is NOT Hermitian (the block belongs to the slot, and the slots of k -> n and n -> k
    are unrelated);
  * hermitian = True: every piece is a regular ring with the neighbours k +- d, d in HERMITIAN_OFFSETS, slot 2 j + 2 the step +d_j and slot 2 j + 3
    its reverse; block(slot of -d) = block(slot of +d)^H, on-site block and lsham Hermitian; every 11th +d_1 bond is cut in both directions
    (absent neighbours).  The library's Hermiticity check passes and the Gram fold of the SpMM epilogue is eligible.
"""
import numpy as np

HERMITIAN_OFFSETS = (1, 5, 17, 43)


def _scatter_row(rng, nbrs, nslots, spread):
    """One row of nn: column 0 the count (own slot included), columns 1 .. count - 1 the neighbours, 0 = absent."""
    row = np.zeros(nslots + 1, np.int32)
    nbrs = list(nbrs)
    if spread:                                       # neighbours at random slots, zeros in between, every slot counted
        pos = np.sort(rng.permutation(nslots - 1)[:len(nbrs)]) + 1
        row[0] = nslots
        for q, n in zip(pos, nbrs):
            row[q] = n
    else:
        row[0] = len(nbrs) + 1
        row[1:len(nbrs) + 1] = nbrs
    return row


def _chord_piece(rng, base, n, nslots):
    """Adjacency (1-based global atom numbers) of one piece: ring + random chords, symmetric, at most nslots - 1 neighbours per atom and
    nslots - 3 for every seventh atom."""
    cap = np.full(n, nslots - 1)
    cap[::7] = max(2, nslots - 3)
    cap = np.minimum(cap, n - 1)
    adj = [set() for _ in range(n)]

    def link(a, b):
        if a != b and b not in adj[a] and len(adj[a]) < cap[a] and len(adj[b]) < cap[b]:
            adj[a].add(b); adj[b].add(a)
    for k in range(n):                               # the ring first: it keeps the piece connected
        link(k, (k + 1) % n)
    pairs = rng.integers(0, n, (6 * n * nslots, 2))
    for a, b in pairs:
        link(int(a), int(b))
    return [[base + 1 + m for m in rng.permutation(sorted(s))] for s in adj]


def pieces_problem(rng, sizes, nslots=9, hoh=False, hermitian=False, collinear=True):
    sizes = tuple(int(s) for s in sizes)
    kk = sum(sizes)
    nn = np.zeros((kk, nslots + 1), np.int32, order="F")
    base = 0
    for n in sizes:
        if hermitian:
            offs = HERMITIAN_OFFSETS[:(nslots - 1) // 2]
            assert n > 2 * max(offs) + 1, "ring too short for distinct +-d neighbours"
            for k in range(n):
                nn[base + k, 0] = 2 * len(offs) + 1
                for j, d in enumerate(offs):
                    fwd_cut = j == 0 and k % 11 == 3                 # the bond k -> k + 1 ...
                    back_cut = j == 0 and (k - 1) % n % 11 == 3      # ... and its reverse (k + 1) -> k
                    nn[base + k, 2 * j + 1] = 0 if fwd_cut else base + 1 + (k + d) % n
                    nn[base + k, 2 * j + 2] = 0 if back_cut else base + 1 + (k - d) % n
        else:
            for k, nbrs in enumerate(_chord_piece(rng, base, n, nslots)):
                nn[base + k] = _scatter_row(rng, nbrs, nslots, spread=(k % 7 == 0))
        base += n
    if not hermitian:
        nn[kk - 1, 0] = nslots                                       # at least one atom uses every slot

    def blocks():
        a = (rng.standard_normal((18, 18, nslots, 1)) + 1j * rng.standard_normal((18, 18, nslots, 1))) * 0.2
        if collinear:                                                # hopping blocks of a collinear magnet: no spin-flip part
            a[:9, 9:] = 0
            a[9:, :9] = 0
        if hermitian:
            a[:, :, 0, 0] = 0.5 * (a[:, :, 0, 0] + a[:, :, 0, 0].conj().T)
            for s in range(1, nslots - 1, 2):
                a[:, :, s + 1, 0] = a[:, :, s, 0].conj().T           # H(n -> k) = H(k -> n)^H
        return np.asfortranarray(a)

    def onsite():
        a = (rng.standard_normal((18, 18, 1)) + 1j * rng.standard_normal((18, 18, 1))) * 0.1
        if hermitian:
            a[:, :, 0] = 0.5 * (a[:, :, 0] + a[:, :, 0].conj().T)
        return np.asfortranarray(a)

    p = dict(nn=nn, iz=np.ones(kk, np.int32), nmax=0, hoh=int(hoh), nsp=2, ee=blocks(), lsham=onsite())
    if hoh:
        p["eeo"] = blocks()
        p["enim"] = onsite()
    return p


def neighbours(nn, k):
    """1-based neighbours of the 1-based atom k (absent entries left out)."""
    row = nn[k - 1]
    return [int(n) for n in row[1:row[0]] if n]


def region_counts(nn, seed, nlevels):
    """Breadth-first search: counts[l] = atoms within l hops of the 1-based atom `seed`, l = 0 .. nlevels."""
    seen = np.zeros(nn.shape[0] + 1, bool)
    seen[seed] = True
    front, counts = [seed], [1]
    for _ in range(nlevels):
        nxt = []
        for k in front:
            for n in neighbours(nn, k):
                if not seen[n]:
                    seen[n] = True
                    nxt.append(n)
        front = nxt
        counts.append(counts[-1] + len(nxt))
    return np.array(counts)


def region_atoms(nn, seed):
    """Every atom that can be reached from `seed` (1-based, sorted)."""
    seen = {seed}
    front = [seed]
    while front:
        front = [n for k in front for n in neighbours(nn, k) if n not in seen and not seen.add(n)]
    return sorted(seen)


def piece_bounds(sizes):
    """(first, last) 1-based atom of every piece."""
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(edges[i]) + 1, int(edges[i + 1])) for i in range(len(sizes))]


def workgroups(natoms):
    """Workgroups that take part in a post-hop pass over `natoms` atoms: groups of 8 atoms, four groups (waves) per workgroup."""
    groups = -(-natoms // 8)
    return -(-groups // 4)


def max_condition(b2_b):
    """Largest condition number over the matrices b2_b(:,:,level,chain) (the 'comparable' rule of tools/fuzz_recursion.py)."""
    worst = 1.0
    for l in range(b2_b.shape[2]):
        for c in range(b2_b.shape[3]):
            m = b2_b[:, :, l, c]
            ev = np.linalg.eigvalsh(0.5 * (m + m.conj().T))
            worst = max(worst, ev.max() / max(abs(ev.min()), 1e-300))
    return worst


# ---- the problems of the GPU tests ----------------------------------------------------------------------------------------------
EMIN, EMAX = -60.0, 60.0          # Chebyshev window of the random operators (as tests/test_gpu_spmm_random.py)

# batch composition: four pieces whose saturated workgroup counts are 12, 25, 38 and 51; one seed per piece (its first atom)
BATCH_SIZES = (384, 771, 1203, 1603)
BATCH_WORKGROUPS = {384: 12, 771: 25, 1203: 38, 1603: 51}
BATCH_LLD = 9
BATCH_SEEDS = {"s%d" % BATCH_WORKGROUPS[n]: lo for n, (lo, hi) in zip(BATCH_SIZES, piece_bounds(BATCH_SIZES))}
BATCH_RNG = 20263


def batch_problem(hoh=False):
    return pieces_problem(np.random.default_rng(BATCH_RNG + int(hoh)), BATCH_SIZES, hoh=hoh)


# post-hop forms: one piece of kk atoms, chains seeded at its first and last atom
ONE_PIECE_KK = (7, 8, 9, 33, 230, 260, 1100)
ONE_PIECE_RNG = 5150


def one_piece_lld(kk):
    return 3 if kk <= 9 else 5


def one_piece_llds(kk, hoh):
    """The depths the one-piece lattice runs at: four plain hops leave the 1100-atom piece at 31 workgroups, so it also runs two levels deeper."""
    return (one_piece_lld(kk), 7) if kk == 1100 and not hoh else (one_piece_lld(kk),)


def one_piece_problem(kk, hoh=False):
    return pieces_problem(np.random.default_rng(ONE_PIECE_RNG + 2 * kk + int(hoh)), (kk,), hoh=hoh)


def one_piece_seeds(kk):
    return np.array([1, kk], np.int32)


def round_robin_seeds(kk, nchains):
    return (np.arange(nchains, dtype=np.int32) % kk) + 1


# Hermitian ring lattices (Gram fold): one ring, and two rings of different length in one call
HERMITIAN_CASES = {"ring260": (260,), "rings203_330": (203, 330)}
HERMITIAN_LLD = 6
HERMITIAN_RNG = 909


def hermitian_problem(name):
    return pieces_problem(np.random.default_rng(HERMITIAN_RNG + len(name)), HERMITIAN_CASES[name], hermitian=True)


def hermitian_seeds(name):
    return np.array([lo for lo, hi in piece_bounds(HERMITIAN_CASES[name])] + [sum(HERMITIAN_CASES[name])], np.int32)


# sat_pct: the larger piece holds 77 % of the lattice; the chain of the smaller piece never reaches that share
TWO_PIECE_SIZES = (200, 60)
TWO_PIECE_LLD = 5
TWO_PIECE_RNG = 4711


def two_piece_problem():
    return pieces_problem(np.random.default_rng(TWO_PIECE_RNG), TWO_PIECE_SIZES)


def two_piece_seeds():
    return np.array([1, 201, 100], np.int32)
