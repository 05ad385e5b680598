"""Chunker inputs built for an edge: buffers whose candidate positions are chosen, not met by chance (the chunker's counterpart of
lz_inputs.py and hash_inputs.py).

Pure Python plus numpy, fixed seeds: no GPU, no ctypes, no library.  The gear table is a parameter of the chunker, and with a
degenerate gear the candidate class of every position -- none (N), mask_l only (L), both masks (B) -- is decided by two bytes:

* scheme "hi": gear[1] = 2^63, gear[2] = 2^62, gear[3] = 2^62 + 2^63, mask_s = 2^63 | 2^62, mask_l = 2^63.  Both masks have a zero
  low word (the scan's high-word-only variant).  H(i) = gear[b[i]] + 2 gear[b[i-1]]: the previous byte carries 2^63 when it is 2 or 3.
* scheme "lo": gear[1] = 1, gear[2] = 2, mask_s = 3, mask_l = 1 (the two-word variant).  The previous byte carries 2 when it is 1.
* the delay gear: gear[7] = 1, mask_s = mask_l = 1 << k.  Bit k of H(i) is b[i-k] == 7, so a buffer of 7s with lone other bytes at
  positions p has candidates at p + k (and at the positions below k, where the window is not full; they lie below min_size).

emit() turns a class sequence into bytes, chain() is the cut chain over candidate arrays from any start (the second half of
cdc_model.chunk, stated again), and CASES is the table: name -> Case.  A cut x means a candidate at position x - 1; m, a, M are
min, normal and max size, z = c + min(a, r), e = c + min(M, r), S the segment, off the source address mod 16.
test_cdc_inputs.py establishes from the models that every case reaches the edge it names; test_gpu_cdc_inputs.py runs them."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import cdc_model as CM
import streams_model as SM

N, L, B = 0, 1, 2                     # candidate classes: none, mask_l only, both masks
SMALL = (64, 256, 1024)
PARAM_SETS = (SMALL, (64, 64, 1024), (64, 1024, 1024), (64, 64, 64), (100, 300, 700))
SCHEMES = ("hi", "lo")
C0 = 777                              # a first cut that is no multiple of 64
# The resolve's segment when CW_CDC_SEGMENT is not set: cdc_segment_bytes() in cdc_kernels.hip gives 256 KiB rounded up to a multiple
# of max_size, which for max_size 1024 is 256 KiB itself.  The "_sdef" rows of family E sit on the edges of THIS value: if that
# default changes, change it here too (streams_model.SEGMENTS holds the same for max_size 8192).
DEFAULT_SEGMENT = 256 << 10
OFFS = (0, 5, 15)

_BYTE = {"hi": np.array([[1, 0], [2, 3], [0, 1]], np.uint8),   # [wanted class][carry] -> byte
         "lo": np.array([[1, 1], [2, 0], [0, 2]], np.uint8)}
_CARRIES = {"hi": L, "lo": N}         # the class whose bytes carry into the next position (hi: 2 and 3; lo: 1)


def scheme_params(scheme: str, sizes=SMALL) -> dict:
    gear = np.zeros(256, np.uint64)
    if scheme == "hi":
        gear[1], gear[2], gear[3] = 1 << 63, 1 << 62, (1 << 62) | (1 << 63)
        return CM.params(*sizes, (1 << 63) | (1 << 62), 1 << 63, gear=gear)
    gear[1], gear[2] = 1, 2
    return CM.params(*sizes, 3, 1, gear=gear)


def emit(classes, scheme: str, sizes=SMALL):
    """(bytes as uint8 array, params): position i of the bytes has candidate class classes[i] under the scheme's gear and masks."""
    k = np.asarray(classes, np.uint8)
    carry = np.zeros(len(k), np.intp)
    carry[1:] = k[:-1] == _CARRIES[scheme]
    return _BYTE[scheme][k, carry], scheme_params(scheme, sizes)


def delay_params(k: int, sizes=SMALL) -> dict:
    gear = np.zeros(256, np.uint64)
    gear[7] = 1
    return CM.params(*sizes, 1 << k, 1 << k, gear=gear)


def delay(n: int, lone, k: int, sizes=SMALL):
    """(bytes, params, candidate positions): 7s with other bytes at `lone`; the candidates are lone + k and the positions below k."""
    data = np.full(n, 7, np.uint8)
    lone = np.asarray(sorted(lone), np.int64)
    data[lone] = 0
    cands = np.union1d(np.arange(min(k, n)), lone + k)
    return data, delay_params(k, sizes), cands[cands < n]


def classes_of(data, p: dict) -> np.ndarray:
    """The candidate class of every position, from the model's window hash (3: mask_s only, which no built input has)."""
    H = CM.window_hash(np.asarray(data, np.uint8), CM._gear(p))
    s, l = (H & np.uint64(p["mask_s"])) == 0, (H & np.uint64(p["mask_l"])) == 0
    return np.where(s & l, B, np.where(l, L, np.where(s, 3, N))).astype(np.uint8)


def candidates(classes):
    """(cs, cl): the sorted candidate cuts of mask_s and of mask_l for a class sequence (a both-position is in each)."""
    k = np.asarray(classes)
    return np.flatnonzero(k == B) + 1, np.flatnonzero((k == B) | (k == L)) + 1


def chain(cs, cl, n: int, p: dict, start: int = 0, final: bool = True, stop: int | None = None) -> list[int]:
    """The cut chain over the candidate cuts cs (mask_s) and cl (mask_l) of an n-byte stream, from the cut `start` (to the first cut
    at or past `stop`, when given)."""
    m, A, M = p["min"], p["avg"], p["max"]
    cuts, c = [start], start
    while not ((c == n) if final else (c + M > n)) and (stop is None or c < stop):
        r = n - c
        if r <= m:
            c = n
        else:
            e, z = c + min(M, r), c + min(A, r)
            i = np.searchsorted(cs, c + m)
            if i < len(cs) and cs[i] < z:
                c = int(cs[i])
            else:
                j = np.searchsorted(cl, z)
                c = int(cl[j]) if j < len(cl) and cl[j] < e else e
        cuts.append(c)
    return cuts


def unmerged_segments(cs, cl, n: int, p: dict, S: int, cuts) -> list[int]:
    """The segments g >= 1 below n in which the true chain `cuts` shares no cut with the segment's own chain from g * S."""
    true = np.asarray(cuts, np.int64)
    out = []
    for g in range(1, (n - 1) // S + 1 if n else 0):
        lo, hi = g * S, (g + 1) * S
        inside = true[np.searchsorted(true, lo):np.searchsorted(true, hi)]
        own = [c for c in chain(cs, cl, n, p, start=lo, stop=hi) if c < hi]
        if not np.intersect1d(inside, own).size:
            out.append(g)
    return out


def longest_row(segments) -> int:
    best = run = 0
    prev = None
    for g in segments:
        run = run + 1 if prev is not None and g == prev + 1 else 1
        best, prev = max(best, run), g
    return best


def noise_classes(n: int, seed: int) -> np.ndarray:
    """Seeded classes at about the density of text under small masks: one both-candidate in 128 positions, one mask_l-only in 43."""
    return np.random.default_rng(seed).choice(np.array([N, L, B], np.uint8), n, p=[1 - 1 / 32, 1 / 32 - 1 / 128, 1 / 128])


@dataclass
class Case:
    """One row of the table.  The bytes are built when first asked for (`data`, `classes`): the table itself costs an import little,
    whatever a test run selects."""
    family: str
    n: int                            # the length in bytes
    params: dict
    raw: np.ndarray | None = None     # the bytes themselves (default-gear and delay-gear cases) ...
    make: object = None               # ... or what builds the classes to emit (a callable without arguments) ...
    base: object = None               # ... or the case whose bytes these are (family G: inputs of other families cut into streams)
    sizes: tuple = SMALL
    segs: tuple = (None,)             # CW_CDC_SEGMENT values to run at (None = not set)
    edge: str = ""
    finals: tuple = (True,)
    shifts: tuple = OFFS              # source addresses mod 16 to run at
    scheme: str | None = None
    cands: np.ndarray | None = None   # delay-gear cases: the candidate positions asked for
    has: tuple = ()                   # cuts the model's final = True chain holds ...
    hasnt: tuple = ()                 # ... and does not hold
    prog: tuple | None = None         # (cut, stride, count): exactly `count` (None: at least two) differences of `stride` from `cut` on
    ends: tuple | None = None         # family G: the stream ends
    lone: int | None = None           # family D: the lone position, and off (shifts[0]); lone + off is the virtual position
    virtual: int | None = None
    body: int = 0                     # family D: where the built body begins (behind the noise-class prefix)
    note: dict | None = None

    @functools.cached_property
    def classes(self):
        """Emitted cases: the classes asked for (uint8, read-only); None for the others."""
        if self.base is not None:
            return self.base.classes
        if self.make is None:
            return None
        k = _ro(np.asarray(self.make(), np.uint8))
        assert len(k) == self.n, (len(k), self.n)
        return k

    @functools.cached_property
    def data(self):
        """The bytes (uint8, read-only)."""
        if self.base is not None:
            return self.base.data
        return self.raw if self.raw is not None else _ro(emit(self.classes, self.scheme, self.sizes)[0])


CASES: dict[str, Case] = {}


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _tag(sizes):
    return "%d-%d-%d" % tuple(sizes)


def _add(name, family, classes, scheme, sizes=SMALL, n=None, **kw):
    """An emitted case: `classes` is the class sequence, or (with n, for the large inputs) a callable that builds it when asked."""
    assert name not in CASES, name
    if callable(classes):
        make = classes
    else:
        k, n = _ro(np.asarray(classes, np.uint8)), len(classes)
        make = lambda: k  # noqa: E731
    CASES[name] = Case(family, n, scheme_params(scheme, sizes), make=make, sizes=tuple(sizes), scheme=scheme, **kw)


def _sizes_params(sizes):
    return dict(min=sizes[0], avg=sizes[1], max=sizes[2])


def _reached(k, sizes, T, final=True):
    return T in chain(*candidates(k), len(k), _sizes_params(sizes), final=final)


def _force(k, sizes, T):
    """Makes T a cut of the chain over the classes k: a both-candidate at T, and where the chain would pass it by (it lies within
    min_size of the cut before it) another one a few hundred bytes in front."""
    k[T - 1] = B
    for d in (0, 300, 500, 200, 400, 600, 150, 450):
        if d:
            if T - d - 1 < 0 or k[T - d - 1] != N:
                continue
            k[T - d - 1] = B
        if _reached(k, sizes, T):
            return
        if d:
            k[T - d - 1] = N
    raise AssertionError(("cannot reach", T))


def _lead(n, sizes, c0):
    """n positions without a candidate, behind a both-cut at c0 that the chain from 0 takes (c0 = 0: none)."""
    k = np.full(n, N, np.uint8)
    if c0:
        if c0 > sizes[2]:
            k[c0 - 477 - 1] = B        # (100, 300, 700): 300, then 777
        k[c0 - 1] = B
        assert _reached(k, sizes, c0), (sizes, c0)
    return k


# ---- A. the cut rule ----------------------------------------------------------------------------------------------------------
def _family_a():
    for sizes in PARAM_SETS:
        m, a, M = sizes
        for c in (0, C0):
            if c and m == M:          # every cut is a multiple of 64
                continue
            z, e = c + a, c + M
            rows = [
                ("both_at_min-1", [(c + m - 1, B)], [e], [c + m - 1], True, "a both-cut at c+m-1 is ignored"),
                ("both_at_min", [(c + m, B)], [c + m], [], True, "a both-cut at c+m is taken"),
                ("both_at_min+1", [(c + m + 1, B)], [c + m + 1], [], m + 1 < M, "a both-cut at c+m+1 is taken"),
                ("both_at_z-1", [(z - 1, B)], [z - 1], [], a > m, "a both-cut at z-1 is taken"),
                ("l_at_z-1_then_l", [(z - 1, L), (z + 10, L)], [z + 10], [z - 1], M - a > 10, "an l-only cut at z-1 is not taken, a later one is"),
                ("l_at_z", [(z, L)], [z], [], a < M, "an l-only cut at z is taken"),
                ("both_at_z", [(z, B)], [z], [], a < M, "a both-cut at z is taken"),
                ("l_at_z-1_and_e-1", [(z - 1, L), (e - 1, L)], [e - 1], [z - 1], a < M, "l-only cuts at z-1 and e-1: e-1 is taken"),
                ("l_at_e-1", [(e - 1, L)], [e - 1], [], a < M, "an l-only cut at e-1 is taken"),
                ("l_at_e-1_normal_is_max", [(e - 1, L)], [e], [e - 1], a == M and m < M, "a == M: e-1 = z-1 is in the mask_s range"),
                ("both_at_e", [(e, B)], [e], [], True, "a candidate at e is the forced cut"),
                ("nothing", [], [e], [], True, "no candidate: the cut is forced"),
                ("l_early_both_later", [(c + m + 5, L), (c + m + 20, B)], [c + m + 20], [c + m + 5], a > m + 20,
                 "an l-only cut early in the small region loses to a later both-cut"),
            ]
            for row, places, has, hasnt, sense, edge in rows:
                if not sense:
                    continue
                for scheme in SCHEMES:
                    k = _lead(c + 3 * M + 50, sizes, c)
                    for x, klass in places:
                        k[x - 1] = klass
                    _add(f"A_{row}_c{c}_{_tag(sizes)}_{scheme}", "A", k, scheme, sizes, segs=(None, M), edge=edge,
                         has=tuple(has) + ((c,) if c else ()), hasnt=tuple(hasnt))


# ---- B. tails -----------------------------------------------------------------------------------------------------------------
def _family_b():
    m, a, M = SMALL
    for scheme in SCHEMES:
        for t in (1, m - 1, m, m + 1, a - 1, a, a + 1, M - 1, M, M + 1):
            for cand in (False, True):
                k = _lead(C0 + t, SMALL, C0)
                if cand:
                    k[-1] = B
                _add(f"B_tail{t}_{'cand' if cand else 'bare'}_{scheme}", "B", k, scheme, finals=(True, False), has=(C0, C0 + t),
                     edge=f"{t} bytes behind the cut at {C0}" + (", a both-candidate at n-1" if cand else ""))
        _add(f"B_n0_{scheme}", "B", np.zeros(0, np.uint8), scheme, finals=(True, False), edge="n = 0")
        for klass in (N, B):
            _add(f"B_n1_{'cand' if klass else 'bare'}_{scheme}", "B", np.array([klass], np.uint8), scheme, finals=(True, False), has=(1,),
                 edge="n = 1")


# ---- C. runs ------------------------------------------------------------------------------------------------------------------
PERIOD = 700


def periodic_both(n):
    """One both-cut every 700 bytes in a buffer without other candidates."""
    k = np.full(n, N, np.uint8)
    k[PERIOD - 1::PERIOD] = B
    return k


def periodic_hole(n):
    """One non-candidate every 700 bytes (positions = 699 mod 700) in an l-only buffer behind a both-cut at 777.  The true chain is
    777 + 256 j (= 1 mod 4, while a cut sees a hole only when it is = 444 mod 700, = 0 mod 4); a segment's own chain starts at a
    multiple of 1024 and steps by 256 or, across a hole, 257: it keeps its phase against the true chain and never lands on it."""
    k = np.full(n, L, np.uint8)
    k[PERIOD - 1::PERIOD] = N
    k[:C0] = N
    k[C0 - 1] = B
    return k


def _family_c():
    m, a, M = SMALL
    for scheme in SCHEMES:
        for kk in (1, 2, 17):
            for d in (-1, 0, 1):
                run = kk * m + d
                for entry in ("exact", "late"):
                    s = C0 + m - 1 + (entry == "late")              # the run's first position
                    k = _lead(s + run + 3 * M, SMALL, C0)
                    k[s:s + run] = B
                    if entry == "exact":                            # the first cut in the run is c + m: the m-step progression
                        steps = (m + run - 1) // m
                        kw = dict(has=(C0, C0 + steps * m), hasnt=(C0 + (steps + 1) * m,), prog=(C0, m, steps))
                    else:                                           # the first cut is c + m + 1: one step, then the progression
                        steps = (run - 1) // m
                        kw = dict(has=(C0, C0 + m + 1), hasnt=(C0 + m,), prog=(C0 + m + 1, m, steps) if steps else None)
                    _add(f"C_allboth_{kk}m{d:+d}_{entry}_{scheme}", "C", k, scheme, segs=(None, M), finals=(True, False),
                         edge=f"an all-both run of {run} entered {'at c+m' if entry == 'exact' else 'one byte late'}", **kw)
        k = _lead(C0 + m - 1 + 40 * m + 13, SMALL, C0)
        k[C0 + m - 1:] = B
        _add(f"C_allboth_to_n_{scheme}", "C", k, scheme, segs=(None, M), finals=(True, False), has=(C0,), prog=(C0, m, None),
             edge="an all-both run that reaches n: (n - M - cut) / m + 1 binds")
        for ender in (B, L):
            for kk in (1, 2, 9):
                for d in (-1, 0, 1):
                    E = C0 + kk * M + d
                    k = _lead(E + 2 * M + 100, SMALL, C0)
                    k[E - 1] = ender
                    if d < 0:
                        kw = dict(has=(C0, E), hasnt=(C0 + kk * M,), prog=(C0, M, kk - 1) if kk > 1 else None)
                    elif d == 0:
                        kw = dict(has=(C0, E), prog=(C0, M, kk + 2))
                    else:
                        kw = dict(has=(C0, C0 + kk * M), hasnt=(E,), prog=(C0, M, kk + 2))
                    _add(f"C_free_{kk}M{d:+d}_{'both' if ender == B else 'l'}_{scheme}", "C", k, scheme, segs=(None, M), finals=(True, False),
                         edge=f"a candidate-free run ended by a {'both' if ender == B else 'l-only'}-cut at c+{kk}M{d:+d}", **kw)
        for kk in (1, 2, 9):
            for d in (-1, 0, 1):
                steps = kk - 1 if d < 0 else kk
                _add(f"C_free_to_n_{kk}M{d:+d}_{scheme}", "C", _lead(C0 + kk * M + d, SMALL, C0), scheme, segs=(None, M), finals=(True, False),
                     has=(C0,), prog=(C0, M, steps) if steps else None, edge=f"a candidate-free run that reaches n = c+{kk}M{d:+d}")
        for sizes in (SMALL, (64, 64, 1024)):
            A = sizes[1]
            k = np.full(C0 + 50 * A + 7, L, np.uint8)
            k[:C0] = N
            k[C0 - 1] = B
            _add(f"C_all_l_{_tag(sizes)}_{scheme}", "C", k, scheme, sizes, segs=(None, M), finals=(True, False), has=(C0,), prog=(C0, A, 50),
                 edge="an all-l-only run: every chunk is a bytes" + (" by the map-3 progression" if A == sizes[0] else ", one step each"))
        n = 300 << 10
        _add(f"C_periodic_both_{scheme}", "C", functools.partial(periodic_both, n), scheme, n=n, finals=(True, False), has=(PERIOD, 2 * PERIOD), prog=(0, PERIOD, None),
             edge="one both-cut every 700 bytes over 300 KiB")
        _add(f"C_periodic_hole_{scheme}", "C", functools.partial(periodic_hole, n), scheme, n=n, finals=(True, False), has=(C0,), prog=(C0, a, None),
             edge="one non-candidate every 700 bytes in an l-only buffer: chains keep their phase")


# ---- D. bitmap words and summaries --------------------------------------------------------------------------------------------
PREFIX = 3001
VIRTUAL = (63, 64, 4095, 4096, 262143, 262144)
LEVEL3 = (16777215, 16777216)


def lone_classes(v, off, fill, lone_class):
    """A buffer of class `fill` with one position of class `lone_class` at v - off; behind a 3001-byte noise-class prefix when v lies
    past it, so that the chain enters the run at an odd phase.  Returns (classes, where the built body begins)."""
    pos = v - off
    k = np.full(pos + 1 + 3 * SMALL[2] + 77, fill, np.uint8)
    body = 0
    if pos > PREFIX + 1000:
        k[:PREFIX] = noise_classes(PREFIX, 21)
        body = PREFIX
    k[pos] = lone_class
    return k, body


def lone_at_end(v, off, lone_class):
    """A lone candidate at v - off in a candidate-free buffer that ends 5 bytes behind it, so that every search that runs to n ends in
    the word of v -- for v the first bit of a summary group, the group's first word.  The chain comes in M-steps from a both-cut T
    whose lattice T + j M passes the lone cut x by two bytes (x + 2 <= n): the progression has to stop one step short and take x,
    M - 2 behind the cut before it; a search that misses the candidate in that last word steps over it.  Returns (classes, T)."""
    M = SMALL[2]
    x = v - off + 1
    T = (x + 2) % M + 2 * M
    k = np.full(x + 5, N, np.uint8)
    _force(k, SMALL, T)
    k[x - 1] = lone_class
    assert (x + 2 - T) % M == 0 and _reached(k, SMALL, x) and not _reached(k, SMALL, x + 2)
    return k, T


def _classes_only(build, *args):
    return build(*args)[0]


def lone_body(v, off):
    """Where lone_classes' built body begins, and its length."""
    return (PREFIX if v - off > PREFIX + 1000 else 0), v - off + 1 + 3 * SMALL[2] + 77


def _family_d():
    M = SMALL[2]
    for scheme in SCHEMES:
        for v in (4096, 262144):
            for off in OFFS:
                for klass in (B, L):
                    c0 = (v - off + 3) % M + 2 * M
                    k = functools.partial(_classes_only, lone_at_end, v, off, klass)
                    _add(f"D_lone_{'both' if klass == B else 'l'}_end_v{v}_off{off}_{scheme}", "D", k, scheme, n=v - off + 6, segs=(None, 3 * M + 1),
                         shifts=(off,),
                         finals=(True, False), lone=v - off, virtual=v, body=c0, has=(c0, v - off + 1), hasnt=(v - off + 3,),
                         prog=(c0, M, (v - off + 3 - c0) // M - 1),
                         edge=f"a lone candidate at virtual position {v}, the first bit of a group, in the last word of the buffer")
        for v in VIRTUAL:
            for off in OFFS:
                for klass in (B, L):
                    body, n = lone_body(v, off)
                    k = functools.partial(_classes_only, lone_classes, v, off, N, klass)
                    _add(f"D_lone_{'both' if klass == B else 'l'}_v{v}_off{off}_{scheme}", "D", k, scheme, n=n, segs=(None, 3 * M + 1), shifts=(off,),
                         lone=v - off, virtual=v, body=body, edge=f"a lone candidate at virtual position {v}")
                for sizes in (SMALL, (64, 64, 1024)):
                    body, n = lone_body(v, off)
                    k = functools.partial(_classes_only, lone_classes, v, off, B, N)
                    _add(f"D_hole_v{v}_off{off}_{_tag(sizes)}_{scheme}", "D", k, scheme, sizes, n=n, segs=(None, 3 * M + 1), shifts=(off,),
                         lone=v - off, virtual=v, body=body,
                         edge=f"a lone non-candidate at virtual position {v} in an all-both buffer (map {2 if sizes[0] < sizes[1] else 3})")


# the level-3 inputs, 16 MiB each and the only ones above 4.5 MiB: both shapes at both positions, each shape at both offsets
LEVEL3_ROWS = (("lone", 16777215, 0), ("lone", 16777216, 15), ("hole", 16777215, 15), ("hole", 16777216, 0))


@functools.lru_cache(None)
def level3_case(shape: str, v: int, off: int) -> Case:
    if shape == "lone" and v == LEVEL3[1]:       # the buffer ends in the first word of the second 16 MiB group
        make, body, n = functools.partial(_classes_only, lone_at_end, v, off, B), (v - off + 3) % SMALL[2] + 2 * SMALL[2], v - off + 6
    else:
        make = functools.partial(_classes_only, lone_classes, v, off, N if shape == "lone" else B, B if shape == "lone" else N)
        body, n = lone_body(v, off)
    scheme = "hi" if shape == "lone" else "lo"
    return Case("D3", n, scheme_params(scheme), make=make, segs=(None,), shifts=(off,), scheme=scheme, lone=v - off, virtual=v, body=body,
                has=(v - off + 1,) if body != PREFIX else (),
                edge=f"level 3: a lone {'candidate' if shape == 'lone' else 'non-candidate'} at virtual position {v}")


# ---- E. segments --------------------------------------------------------------------------------------------------------------
SEGMENTS = {"sM": SMALL[2], "s3M1": 3 * SMALL[2] + 1, "sdef": DEFAULT_SEGMENT}


def _e_cut(S, T):
    k = np.full(3 * S + 100, N, np.uint8)
    _force(k, SMALL, T)
    return k


def _e_spec_exit(S):
    k = _lead(4 * S + 100, SMALL, C0)
    for g in range(3):
        k[(g + 1) * S - 500 - 1] = B
        k[(g + 1) * S - 1] = B
    return k


def _e_late_unmerged(n):
    k = periodic_both(n)
    k[PERIOD * 6200:] = L
    return k


def _family_e():
    m, a, M = SMALL
    for stag, S in SEGMENTS.items():
        segs = (None if stag == "sdef" else S,)
        for scheme in SCHEMES:
            for g in (1, 2):
                for d in (-1, 0, 1):
                    _add(f"E_cut_{g}S{d:+d}_{stag}_{scheme}", "E", functools.partial(_e_cut, S, g * S + d), scheme, n=3 * S + 100, segs=segs, has=(g * S + d,), edge=f"a true cut at {g}S{d:+d}")
            _add(f"E_spec_exit_{stag}_{scheme}", "E", functools.partial(_e_spec_exit, S), scheme, n=4 * S + 100, segs=segs, has=(C0,), note=dict(S=S, spec_exit=(0, 1, 2)),
                 edge="the chains from 0, S and 2S first cut past their segment at exactly (g+1)S")
            for nn, name in ((S - 1, "S-1"), (S, "S"), (S + 1, "S+1"), (5 * S, "5S")):
                _add(f"E_n_{name}_{stag}_{scheme}", "E", functools.partial(noise_classes, nn, 31), scheme, n=nn, segs=segs, finals=(True, False),
                     edge=f"n = {name}: the last segment starts at n or one byte either side")
            _add(f"E_open_5S+100_{stag}_{scheme}", "E", functools.partial(noise_classes, 5 * S + 100, 32), scheme, n=5 * S + 100, segs=segs, finals=(False,),
                 edge="final = 0: the chain ends inside a segment, the later ones come out empty")
    for scheme in SCHEMES:
        n = 300 << 10
        _add(f"E_periodic_hole_sM_{scheme}", "E", functools.partial(periodic_hole, n), scheme, n=n, segs=(M,), has=(C0,), prog=(C0, a, None),
             note=dict(S=M, unmerged_row=64), edge="more than 64 unmerged segments in a row, walked one step at a time")
        _add(f"E_periodic_both_sM_{scheme}", "E", functools.partial(periodic_both, n), scheme, n=n, segs=(M,), has=(PERIOD,), prog=(0, PERIOD, None),
             note=dict(S=M, unmerged_row=0), edge="one both-cut every 700 bytes: every segment's chain lands on the true one")
        n = 9 << 19
        _add(f"E_periodic_hole_4608seg_{scheme}", "E", functools.partial(periodic_hole, n), scheme, n=n, segs=(M,), has=(C0,), prog=(C0, a, None),
             note=dict(S=M, nseg=4096), edge="4.5 MiB at S = 1024: more than 4096 segments, all unmerged")
        # both-cuts every 700 bytes (every segment merges), then an l-only run entered at 700 * 6200 = 32 mod 256: the first unmerged
        # segment lies past 4096, where the fix-up's search for it reaches in its second stride
        _add(f"E_late_unmerged_{scheme}", "E", functools.partial(_e_late_unmerged, n), scheme, n=n, segs=(M,), has=(PERIOD * 6200, PERIOD * 6200 + a), note=dict(S=M, first_unmerged=4096),
             prog=(PERIOD * 6200, a, None), edge="the first unmerged segment is past segment 4096: the search's second stride finds it")
        for pre in (0, 33):
            k = np.full(pre + 20 * 1030 + 17, B, np.uint8)
            k[:pre] = N
            _add(f"E_capacity_pre{pre}_{scheme}", "E", k, scheme, segs=(1030,), finals=(True, False), note=dict(S=1030, capacity=(1030 + m - 1) // m),
                 edge="all-both at S = 1030: a segment's lists hold ceil(S / m) cuts of cap = S / m + 2")


# ---- F. scan ------------------------------------------------------------------------------------------------------------------
DEFAULT_SMALL = CM.params(*SMALL, CM.top_bits(10), CM.top_bits(6))
BOTH_WORDS = CM.params(*SMALL, 0xF0000000000000F0, 0x8000000000000001)
SPAN_EDGES = (4095, 4096, 4097, 8191, 8192, 8193)
WINDOW_K = (0, 1, 31, 32, 62, 63)


def _delay_case(name, n, probes, k, **kw):
    """A delay-gear case whose candidates at `probes` are all cuts of the chain: where the chain would pass one by, a candidate a few
    hundred bytes in front of it sets the chain up."""
    cset = set()
    p = _sizes_params(SMALL)

    def cuts():
        c = np.asarray(sorted(cset), np.int64) + 1
        return chain(c, c, n, p)

    for q in sorted(probes):
        cset.add(q)
        for d in (0, 300, 500, 200, 400, 600, 150, 450):
            if d:
                if q - d - k < 0 or any(abs(q - d - o) < 70 for o in cset):
                    continue
                cset.add(q - d)
            if q + 1 in cuts():
                break
            if d:
                cset.discard(q - d)
        else:
            raise AssertionError(("cannot reach", name, q))
    assert all(q + 1 in cuts() for q in probes), name
    lone = [q - k for q in cset]
    assert min(lone) >= 0
    data, params, cands = delay(n, lone, k)
    assert name not in CASES
    CASES[name] = Case("F", n, params, raw=_ro(data), cands=_ro(cands), has=tuple(q + 1 for q in sorted(probes)), **kw)


def _family_f():
    src = np.random.default_rng(41).integers(0, 256, 64 << 10, dtype=np.uint8)
    H = CM.window_hash(src)
    ok = (H & np.uint64(DEFAULT_SMALL["mask_l"])) == 0
    for nv in SPAN_EDGES:
        for off in (0, 1, 15):
            n = nv - off
            s = int(np.flatnonzero(ok[n - 1:])[0])                  # the first slice start with a candidate at its position n - 1
            CASES[f"F_span_{nv}_off{off}_default"] = Case("F", n, DEFAULT_SMALL, raw=_ro(src[s:s + n]), finals=(False,), shifts=(off,),
                                                          note=dict(candidate_at_end=True), edge=f"n + off = {nv}, default gear, noise")
            rng = np.random.default_rng(nv * 16 + off)
            at, probes = 100, []
            while at < n - 500:
                probes.append(at)
                at += int(rng.integers(100, 400))
            CASES[f"F_span_{nv}_off{off}_delay"] = _delay_span(n, probes + [n - 1], 33, off, nv)      # the high-word-only scan
            CASES[f"F_span_{nv}_off{off}_delay31"] = _delay_span(n, probes + [n - 1], 31, off, nv)    # the two-word scan
    for k in WINDOW_K:
        for off in (0, 5):
            # a lone byte at B - 1 (its candidate lies k - 1 past the edge) and at B - k (its candidate is the edge's first position), B
            # virtual: a lane edge, a wavefront edge (position 0 of the second span), and the same in later spans
            last = [B_ - 1 - off + k for B_ in (320, 4096, 12288)]
            first = [B_ - off for B_ in (1344, 8192, 16384)]
            _delay_case(f"F_window_k{k}_off{off}", 17000, last + first, k, finals=(True,), shifts=(off,),
                        note=dict(k=k), edge=f"delay {k}: lone bytes whose candidates lie across a lane or wavefront edge")
    noise = np.random.default_rng(42).integers(0, 256, 64 << 10, dtype=np.uint8)
    CASES["F_both_words"] = Case("F", len(noise), BOTH_WORDS, raw=_ro(noise), finals=(True, False), edge="both words of both masks are tested")
    # a low word in one mask only: the high-word-only variant must not be chosen on the strength of the other mask
    CASES["F_low_word_in_mask_l"] = Case("F", len(noise), dict(DEFAULT_SMALL, mask_l=BOTH_WORDS["mask_l"]), raw=_ro(noise), finals=(True, False),
                                         edge="mask_s has a zero low word, mask_l has not")
    CASES["F_low_word_in_mask_s"] = Case("F", len(noise), dict(DEFAULT_SMALL, mask_s=CM.top_bits(10) | 0xF0), raw=_ro(noise), finals=(True, False),
                                         edge="mask_l has a zero low word, mask_s has not")


def _delay_span(n, cand_positions, k, off, nv):
    lone = [q - k for q in cand_positions if q - k >= 0]
    data, params, cands = delay(n, lone, k)
    return Case("F", n, params, raw=_ro(data), cands=_ro(cands), finals=(False,), shifts=(off,), note=dict(candidate_at_end=True),
                edge=f"n + off = {nv}, delay gear")


# ---- G. streams ---------------------------------------------------------------------------------------------------------------
def _family_g():
    m, a, M = SMALL
    S = M
    segs = (M, None)
    for scheme in SCHEMES:
        k = _lead(C0 + m + 2000, SMALL, C0)
        k[C0 + 30 - 1] = B
        k[C0 + m + 300 - 1] = B
        _add(f"G_end_at_min_{scheme}", "G", k, scheme, segs=segs, ends=(C0 + m, len(k)), has=(C0, C0 + m), hasnt=(C0 + 30,),
             edge="a stream end at c+m: the remainder is one chunk")
        k = _lead(C0 + m + 1 + 2000, SMALL, C0)
        k[C0 + m - 1] = B
        _add(f"G_one_byte_chunk_{scheme}", "G", k, scheme, segs=segs, ends=(C0 + m + 1, len(k)), has=(C0, C0 + m, C0 + m + 1),
             edge="a stream end at c+m+1 behind a both-cut at c+m: a 1-byte chunk")
        k = _lead(C0 + 300 + 2000, SMALL, C0)
        k[C0 + 300 - 1] = B
        _add(f"G_end_on_candidate_{scheme}", "G", k, scheme, segs=segs, ends=(C0 + 300, len(k)), has=(C0, C0 + 300),
             edge="a stream end exactly on a candidate")
        ends = (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 50)
        _add(f"G_segment_edges_allboth_{scheme}", "G", np.full(ends[-1], B, np.uint8), scheme, segs=segs, ends=ends, has=ends,
             edge="stream ends at gS-1, gS, gS+1 inside an all-both run")
        _add(f"G_segment_edges_free_{scheme}", "G", np.full(ends[-1], N, np.uint8), scheme, segs=segs, ends=ends, has=ends,
             edge="stream ends at gS-1, gS, gS+1 inside a candidate-free run")
        ends = (1000,) + tuple(range(1001, 1301)) + (3300,)
        _add(f"G_300_one_byte_streams_{scheme}", "G", np.full(3300, B, np.uint8), scheme, segs=segs, ends=ends, has=ends,
             edge="300 one-byte streams inside an all-both run")
        _add(f"G_open_within_max_{scheme}", "G", noise_classes(5000, 33), scheme, segs=segs, ends=(1500, 4500, 5000), has=(1500, 4500),
             edge="the open last stream starts within M of n: it stops at its start")
    # the inputs of families A to C, and of family E at S = M, cut into three streams
    for name, c in list(CASES.items()):
        if c.family in "ABC" or (c.family == "E" and c.segs == (M,)):
            n = c.n
            if n < 3:
                continue
            CASES["G_split_" + name] = Case("G", n, c.params, base=c, sizes=c.sizes, segs=(M,), shifts=(5,), scheme=c.scheme,
                                            ends=(n // 3, 2 * n // 3 + 1, n), note=dict(of=c.family), edge="cut into three streams: " + c.edge)


_family_a()
_family_b()
_family_c()
_family_d()
_family_e()
_family_f()
_family_g()


def family(f: str) -> list[str]:
    return [name for name, c in CASES.items() if c.family == f]


def streams_of(c: Case) -> list[bytes]:
    raw = c.data.tobytes()
    return [raw[a:b] for a, b in zip((0,) + tuple(c.ends[:-1]), c.ends)]


@functools.lru_cache(None)
def model(name: str, final: bool = True) -> list[int]:
    """cdc_model.chunk of a case, computed once."""
    c = CASES[name]
    return CM.chunk(c.data, c.params, final=final)


@functools.lru_cache(None)
def model_level3(shape: str, v: int, off: int) -> list[int]:
    c = level3_case(shape, v, off)
    return CM.chunk(c.data, c.params)


@functools.lru_cache(None)
def model_streams(name: str):
    """streams_model.chunk_streams of a family G case, computed once: (offsets, first)."""
    c = CASES[name]
    return SM.chunk_streams(streams_of(c), c.params)
