"""Digests built for an edge of the dedupe index: every digest's home slot, and its whole 64-bit fold, is chosen, not met by chance
(the index's counterpart of lz_inputs.py, hash_inputs.py and cdc_inputs.py).

Pure Python plus numpy, fixed seeds: no GPU, no ctypes, no library.

THE ONE COPY OF DEVICE CODE IN THE SUITE.  mix64 / fold below restate `mix64` and `fold` of compute_war_amd/csrc/dedupe_kernels.hip
(constants included) and cap_of restates `dedupe_cap` of cw_dedupe.hip.  fold is a splitmix64 chain, invertible in the last word:
for any W - 1 leading words and any target T the last word is unmix64(T - GOLD) ^ fold(leading words), so a digest can be put on
any home slot of any capacity and any number of distinct digests can share one full fold.  The copy is used ONLY to aim inputs and
to check slot positions (slots_after, check_export_order).  What ref, new_idx, n_new, n_found or the count should be is never
taken from it: those come from the dict model of test_gpu_dedupe_lifecycle.py.  If the kernel's fold changes, the calibration test
at the head of test_gpu_dedupe_inputs.py fails and says so.

A digest is a tuple of W Python ints (u64 words, as the kernels load them: little endian); rows() packs a list of them into the
uint8[n, 8 W] array the calls take.  CASES is the catalogue: name -> Case.  A case is a schedule of calls on one index (each
cw_dev_dedupe with a `base`, or cw_dev_dedupe_insert with `values`), the `absent` queries that must miss, each with the way it
collides (`absent_claims`), the structure the case was built for (`claims`) and the edge `tags` it covers.  test_dedupe_inputs.py
establishes on the CPU that every case is what it claims; test_gpu_dedupe_inputs.py runs them.

Families: A placement (all homes distinct: every slot is exact), B chains (one home, pairwise different folds), C full 64-bit fold
collisions, D merging chains, E chains and collisions across calls, F special digests and batch tails."""
from __future__ import annotations

import random
import zlib
from dataclasses import dataclass

import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
MUL1, MUL2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
INV1, INV2 = pow(MUL1, -1, 1 << 64), pow(MUL2, -1, 1 << 64)
TILE = 256                                  # slots per export tile (kThreads)
MISS = M64                                  # CW_DEDUPE_MISS: never a value
ALGS = {2: "skein", 4: "sha256mb", 8: "skein512"}
WIDTHS = (2, 4, 8)


# ---- the fold copy ------------------------------------------------------------------------------------------------------
def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * MUL1) & M64
    z = ((z ^ (z >> 27)) * MUL2) & M64
    return z ^ (z >> 31)


def _unshift(y: int, s: int) -> int:
    """x with x ^ (x >> s) == y."""
    x, t = y, y >> s
    while t:
        x ^= t
        t >>= s
    return x


def unmix64(z: int) -> int:
    z = (_unshift(z, 31) * INV2) & M64
    z = (_unshift(z, 27) * INV1) & M64
    return _unshift(z, 30)


def fold(words) -> int:
    h = GOLD
    for w in words:
        h = (mix64(h ^ w) + GOLD) & M64
    return h


def cap_of(max_entries: int) -> int:
    cap = 2
    while cap < 2 * max_entries:
        cap <<= 1
    return cap


# ---- builders -------------------------------------------------------------------------------------------------------------
def finish(lead, T: int) -> tuple:
    """The digest with the leading words `lead` and fold T."""
    return tuple(lead) + (unmix64((T - GOLD) & M64) ^ fold(lead),)


def digest(W: int, T: int, rng) -> tuple:
    return finish([rng.getrandbits(64) for _ in range(W - 1)], T)


def home_fold(slot: int, cap: int, rng) -> int:
    """A random fold whose home slot at `cap` is `slot`."""
    return (rng.getrandbits(64) & ~(cap - 1) & M64) | slot


def with_home(W: int, slot: int, cap: int, rng) -> tuple:
    return digest(W, home_fold(slot, cap, rng), rng)


def same_fold(W: int, T: int, k: int, rng) -> list:
    out = []
    while len(out) < k:
        d = digest(W, T, rng)
        if d not in out:
            out.append(d)
    return out


def chain(W: int, s: int, cap: int, L: int, rng) -> list:
    """L digests with home s at `cap` and pairwise different folds.  Member i has fold bit log2(cap) = i & 1 and the bit above
    = (i >> 1) & 1: at 2 cap the even members stay on s and the odd ones move to s + cap, at 4 cap the chain splits in four."""
    k = cap.bit_length() - 1
    seen, out = set(), []
    for i in range(L):
        while True:
            T = s | ((i & 3) << k) | ((rng.getrandbits(64) << (k + 2)) & M64)
            if T not in seen:
                break
        seen.add(T)
        out.append(digest(W, T, rng))
    return out


def rows(ds, W: int) -> np.ndarray:
    """uint8[n, 8 W] of a list of digests."""
    a = np.array([list(d) for d in ds], dtype="<u8").reshape(-1, W)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, 8 * W)


def words(r) -> list:
    """The digests of a uint8[n, 8 W] array, as tuples of ints."""
    r = np.ascontiguousarray(r, dtype=np.uint8)
    return [tuple(t) for t in r.view("<u8").tolist()]


def _digests(x) -> list:
    return words(x) if isinstance(x, np.ndarray) else [tuple(d) for d in x]


def homes(ds, cap: int) -> list:
    return [fold(d) & (cap - 1) for d in _digests(ds)]


# ---- slot positions --------------------------------------------------------------------------------------------------------
def slots_after(ds, cap: int) -> set:
    """The occupied slots once the (distinct) digests are in a table of `cap` slots with linear probing, in whatever order: the
    digests per home slot, swept once round the table with the overflow carried along (a slot is occupied when a digest is at
    home there or one is carried in)."""
    per_home = [0] * cap
    for h in homes(ds, cap):
        per_home[h] += 1
    assert sum(per_home) < cap
    carry = 0
    for s in range(cap):                    # what wraps from slot cap - 1 into slot 0
        carry = max(carry + per_home[s] - 1, 0)
    occupied = set()
    for s in range(cap):
        carry += per_home[s]
        if carry:
            occupied.add(s)
            carry -= 1
    return occupied


def check_export_order(exported, cap: int, exact: bool = False) -> list:
    """The export's order is ascending slot order: entry i sits at the i-th occupied slot.  Asserts the invariant of linear probing
    for every entry -- every slot of the cyclic range [home, own slot) is occupied -- which holds whoever won a race inside a
    cluster.  exact: all homes are distinct, so the export is in ascending home order, exactly.  Returns the slots."""
    ds = _digests(exported)
    assert len(set(ds)) == len(ds), "the export holds a digest twice"
    hs = homes(ds, cap)
    occ = sorted(slots_after(ds, cap))
    assert len(occ) == len(ds)
    if exact:
        assert len(set(hs)) == len(hs), "exact order asked for digests that share a home"
        bad = [i for i in range(len(ds)) if hs[i] != occ[i]]
        assert not bad, f"entry {bad[0]} of the export has home {hs[bad[0]]}, the {bad[0]}-th occupied slot is {occ[bad[0]]}"
        return occ
    before = np.zeros(cap + 1, np.int64)    # occupied slots below s
    before[np.asarray(occ, np.int64) + 1] = 1
    before = np.cumsum(before)
    for i, (h, s) in enumerate(zip(hs, occ)):
        inside = before[s] - before[h] if h <= s else before[cap] - before[h] + before[s]
        assert inside == (s - h) % cap, f"entry {i} of the export: home {h}, slot {s}, and a slot of [home, slot) is empty"
    return occ


# ---- the catalogue -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Call:
    digests: np.ndarray                     # uint8[n, 8 W]
    base: int | None = None                 # cw_dev_dedupe
    values: np.ndarray | None = None        # cw_dev_dedupe_insert: uint64[n]


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    W: int
    max_entries: int
    calls: tuple
    absent: np.ndarray                      # uint8[k, 8 W]
    absent_claims: tuple                    # per absent row: ("home", s) | ("fold", T) | ("word", d, w) | ("twin", d, w) |
    #                                         ("inside", slot) | ("free", slot) | ("any",); d is a stored digest
    claims: tuple                           # what the stored digests were built for (test_dedupe_inputs.py lists the kinds)
    tags: frozenset
    note: str

    @property
    def alg(self) -> str:
        return ALGS[self.W]

    @property
    def db(self) -> int:
        return 8 * self.W

    @property
    def cap(self) -> int:
        return cap_of(self.max_entries)

    def stored(self) -> list:
        """The distinct digests of all calls, in the order of their first appearance."""
        seen, out = set(), []
        for c in self.calls:
            for d in words(c.digests):
                if d not in seen:
                    seen.add(d)
                    out.append(d)
        return out


CASES: dict = {}


def ZERO(W: int) -> tuple:
    return (0,) * W


def ONES(W: int) -> tuple:
    return (M64,) * W


def _rng(name: str):
    return random.Random(zlib.crc32(name.encode()))


def _add(name, family, W, max_entries, calls, absent, claims, tags, note):
    assert name not in CASES, name
    ds = [d for d, _ in absent]
    CASES[name] = Case(name, family, W, max_entries, tuple(calls), rows(ds, W), tuple(c for _, c in absent), tuple(claims),
                       frozenset(tags), note)


def _shuffled(ds, rng) -> list:
    ds = list(ds)
    rng.shuffle(ds)
    return ds


def _near(stored, W, rng) -> list:
    """Per stored digest and word w a digest that differs in word w only, and per stored digest a twin of the SAME fold that
    differs in one leading word and the last."""
    out = []
    for i, d in enumerate(stored):
        for w in range(W):
            e = list(d)
            e[w] ^= 1 << rng.randrange(64)
            out.append((tuple(e), ("word", d, w)))
        w = i % (W - 1)
        lead = list(d[:-1])
        lead[w] ^= 1 << rng.randrange(64)
        out.append((finish(lead, fold(d)), ("twin", d, w)))
    return out


def _absent_at(W, cap, kind, slots, rng) -> list:
    return [(with_home(W, s, cap, rng), (kind, s)) for s in slots]


def _family_a(W):
    # a run of 256 distinct homes across the tile edge of a two-tile table
    name = f"A_run_W{W}"
    rng = _rng(name)
    cap = 512
    ds = [with_home(W, s, cap, rng) for s in range(128, 384)]
    absent = _absent_at(W, cap, "inside", (128, 255, 256, 383), rng) + _absent_at(W, cap, "free", (0, 127, 384, 511), rng)
    _add(name, "A", W, 256, [Call(rows(_shuffled(ds, rng), W), base=7)], absent,
         [("homes_distinct",), ("occupied", tuple(range(128, 384)))], {"tile_edge_run"},
         "homes 128..383 of 512 slots, shuffled, one call: a run across the tile edge, every slot exact")
    # tile 1 wholly full, entries in the first and last slot of other tiles, the other tiles otherwise empty
    name = f"A_tile_W{W}"
    rng = _rng(name)
    cap = 1024
    occ = (0, 255) + tuple(range(256, 512)) + (512, 1023)
    ds = [with_home(W, s, cap, rng) for s in occ]
    absent = _absent_at(W, cap, "inside", (0, 255, 256, 511, 512, 1023), rng) + _absent_at(W, cap, "free", (1, 254, 513, 1022), rng)
    _add(name, "A", W, 512, [Call(rows(_shuffled(ds, rng), W), base=1 << 40)], absent,
         [("homes_distinct",), ("occupied", occ), ("full_tile", 1)], {"full_tile", "tile_first_last_slot"},
         "1024 slots: tile 1 full (homes 256..511) plus slots 0, 255, 512, 1023")
    # tables smaller than a tile, filled to max_entries, an entry in the last slot
    for m, occ in ((1, (1,)), (2, (0, 3)), (3, (0, 4, 7))):
        name = f"A_cap{cap_of(m)}_W{W}"
        rng = _rng(name)
        cap = cap_of(m)
        ds = [with_home(W, s, cap, rng) for s in occ]
        free = [s for s in range(cap) if s not in occ]
        absent = _absent_at(W, cap, "inside", occ, rng) + _absent_at(W, cap, "free", free, rng)
        _add(name, "A", W, m, [Call(rows(_shuffled(ds, rng), W), base=3)], absent, [("homes_distinct",), ("occupied", occ)],
             {f"cap{cap}"}, f"max_entries {m}: {cap} slots, filled to max_entries, slot {cap - 1} occupied")


CHAIN_LENGTHS = (2, 64, 65, 256, "full")
CHAIN_HOMES = ("0", "1", "mid", "cap-2", "cap-1", "cap-halfL")


def _family_b(W):
    for L_ in CHAIN_LENGTHS:
        max_entries = 1024 if L_ == "full" else 512
        cap = cap_of(max_entries)
        L = max_entries if L_ == "full" else L_
        done = set()
        for s_ in CHAIN_HOMES:
            s = {"0": 0, "1": 1, "mid": cap // 2, "cap-2": cap - 2, "cap-1": cap - 1, "cap-halfL": cap - L // 2}[s_]
            if s in done:                   # (L = 2: cap - L/2 is cap - 1)
                continue
            done.add(s)
            name = f"B_L{L_}_s{s_}_W{W}"
            rng = _rng(name)
            ds = chain(W, s, cap, L, rng)
            absent = _absent_at(W, cap, "home", [s] * 8, rng) + _near(ds, W, rng)
            tags = {f"chain_{L_}", f"chain_home_{s_}"}
            claims = [("chain", s, rows(ds, W)), ("cluster", s, L)]
            if s + L > cap:
                tags.add("chain_wraps")
                claims.append(("wrap",))
            _add(name, "B", W, max_entries, [Call(rows(_shuffled(ds, rng), W), base=11)], absent, claims, tags,
                 f"{L} digests of pairwise different folds on home {s} of {cap} slots"
                 + (": the whole table is one cluster of cap/2 slots" if L_ == "full" else ""))


COLLISION_SIZES = (2, 64, 65, 300)


def _family_c(W):
    for K in COLLISION_SIZES:
        name = f"C_K{K}_W{W}"
        rng = _rng(name)
        max_entries = 1024
        T = rng.getrandbits(64)
        ds = same_fold(W, T, K + 8, rng)
        ds, more = ds[:K], ds[K:]
        batch = []
        for i in range(K):                  # d0, d1 d0, d2 d1, ...: followers and leaders of one fold side by side in a wave
            batch.append(ds[i])
            if i:
                batch.append(ds[i - 1])
        _add(name, "C", W, max_entries, [Call(rows(batch, W), base=1 << 20)], [(d, ("fold", T)) for d in more] + _near(ds, W, rng),
             [("collide", T, rows(ds, W)), ("cluster", T & (cap_of(max_entries) - 1), K)], {f"collide_{K}"},
             f"{K} distinct digests of one 64-bit fold, interleaved with duplicates of each other")


def _family_d(W):
    max_entries, L = 512, 64
    cap = cap_of(max_entries)
    for kind, gap, s, wraps in (("adjacent", 1, 100, False), ("adjacent", 1, cap - L, True), ("touch", L, 200, False),
                                ("touch", L, cap - L - L // 2, True)):
        name = f"D_{kind}_s{s}_W{W}"
        rng = _rng(name)
        a, b = chain(W, s, cap, L, rng), chain(W, (s + gap) % cap, cap, L, rng)
        inside = [(s + k) % cap for k in (L // 2, L - 1, L, 3 * L // 2, 2 * L - 1)]
        absent = _absent_at(W, cap, "inside", inside, rng) + _absent_at(W, cap, "free", [(s + 2 * L) % cap, (s - 1) % cap], rng)
        claims = [("chain", s, rows(a, W)), ("chain", (s + gap) % cap, rows(b, W)), ("cluster", s, 2 * L)]
        tags = {f"merge_{kind}"}
        if wraps:
            claims.append(("wrap",))
            tags.add("merge_wraps")
        _add(name, "D", W, max_entries, [Call(rows(_shuffled(a + b, rng), W), base=1 << 50)], absent, claims, tags,
             f"two chains of {L} on homes {s} and {(s + gap) % cap} of {cap} slots: one cluster of {2 * L}")


def _family_e(W):
    name = f"E_calls_W{W}"
    rng = _rng(name)
    max_entries = 512
    cap = cap_of(max_entries)
    s, L, K = 300, 64, 64
    T = home_fold(700, cap, rng)
    ch, co = chain(W, s, cap, L, rng), same_fold(W, T, K + 8, rng)
    co, spare = co[:K], co[K:]
    more_home = [with_home(W, s, cap, rng) for _ in range(8)]
    one = _shuffled(ch[:L // 2] + co[:K // 2], rng)
    two = _shuffled(ch[L // 2:] + co[K // 2:] + ch[:16] + co[:16] + ch[L // 2:L // 2 + 16] + co[K // 2:K // 2 + 16], rng)
    new3 = more_home[:4] + spare[:4]
    three = _shuffled(ch[::3] + co[::3] + new3 + new3, rng)
    values = np.array([rng.randrange(MISS) for _ in three], np.uint64)
    absent = [(d, ("home", s)) for d in more_home[4:]] + [(d, ("fold", T)) for d in spare[4:]] + _near(ch + co, W, rng)
    _add(name, "E", W, max_entries, [Call(rows(one, W), base=1000), Call(rows(two, W), base=1 << 33), Call(rows(three, W), values=values)],
         absent, [("chain", s, rows(ch, W)), ("collide", T, rows(co, W)), ("across_calls",)], {"across_calls"},
         "half a chain and half a collision set committed by call 1; call 2 walks COMMITTED mismatches, PENDING mismatches, then "
         "a match; call 3 inserts with explicit values")


TAILS = (1, 63, 64, 65, 255, 256, 257)


def _family_f(W):
    name = f"F_special_W{W}"
    rng = _rng(name)
    sp = [ZERO(W), ONES(W), digest(W, 0, rng), digest(W, 0, rng), digest(W, M64, rng), digest(W, M64, rng)]
    absent = [(digest(W, 0, rng), ("fold", 0)), (digest(W, M64, rng), ("fold", M64)), (digest(W, fold(ZERO(W)), rng), ("fold", fold(ZERO(W)))),
              (digest(W, fold(ONES(W)), rng), ("fold", fold(ONES(W))))] + _near(sp, W, rng)
    _add(name, "F", W, 16, [Call(rows(sp + sp[::-1], W), base=5)], absent,
         [("digest", 0, "zero"), ("digest", 1, "ones"), ("digest", 2, "fold0"), ("digest", 3, "fold0"), ("digest", 4, "foldmax"),
          ("digest", 5, "foldmax")], {"zero", "ones", "fold0", "foldmax"},
         "the all-zero and the all-ones digest, two digests of fold 0 and two of fold 2^64 - 1, each twice")
    for n in TAILS:
        name = f"F_tail{n}_W{W}"
        rng = _rng(name)
        ds = [tuple(rng.getrandbits(64) for _ in range(W)) for _ in range(n - 1)] + [ZERO(W)]
        absent = [(ONES(W), ("any",)), (digest(W, fold(ZERO(W)), rng), ("fold", fold(ZERO(W))))] + \
                 [(tuple(1 << b if w == v else 0 for v in range(W)), ("any",)) for w in range(W) for b in (0, 63)]
        _add(name, "F", W, 512, [Call(rows(ds, W), base=9), Call(rows([ZERO(W), ds[0], ZERO(W)], W), base=1 << 30)], absent,
             [("tail", n)], {f"tail_{n}"},
             f"a batch of {n} whose last valid lane holds the all-zero digest (the lanes beyond n are given zeros); then it is a hit")
    name = f"F_zero_first_W{W}"
    rng = _rng(name)
    batch = []
    for _ in range(65):                     # 0, r, 0, r, ..., 0: 131 lanes, the zero digest first and in every wave
        batch += [ZERO(W), tuple(rng.getrandbits(64) for _ in range(W))]
    batch.append(ZERO(W))
    _add(name, "F", W, 512, [Call(rows(batch, W), base=2)], [(ONES(W), ("any",))], [("zero_first", 66)], {"zero_first_repeated"},
         "the all-zero digest as the first entry of a batch of 131 and 65 times more")


for _W in WIDTHS:
    _family_a(_W)
    _family_b(_W)
    _family_c(_W)
    _family_d(_W)
    _family_e(_W)
    _family_f(_W)


def family(letter: str, W: int | None = None) -> list:
    return [n for n, c in CASES.items() if c.family == letter and W in (None, c.W)]
