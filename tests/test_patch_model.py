"""tests/patch_model.py against ``cdc_model.chunk(edited)``: the restart / window / resync rule of cw_store_patch gives exactly the
cuts of the whole edited stream, on seeded edits over random, all-zero and periodic streams, and every class of outcome the rule
distinguishes is reached."""
import numpy as np
import pytest

import cdc_model as CM
import patch_model as PM

P256, P8K = CM.default_params(256), CM.default_params(8192)   # 64 / 256 / 2048 and 2048 / 8192 / 65536
SIZES = (0, 1, 63, 64, 65, 300, 2048, 2049, 5000, 20000)


def stream(kind: str, n: int, rng) -> bytes:
    if kind == "zero":
        return bytes(n)
    if kind == "periodic":
        return (bytes(range(7, 7 + 37)) * (n // 37 + 1))[:n]
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def edits_of(old: bytes, cuts, rng):
    """Edits at 0, at n, at and around every kind of cut, inside the first and the last chunk; removals of 0, 1, some and to the end;
    inserts of 0 .. 5000 bytes."""
    n = len(old)
    first, last = cuts[1] if len(cuts) > 1 else 0, cuts[-2] if len(cuts) > 1 else 0
    inner = cuts[len(cuts) // 2]
    at = {0, n, first, last, inner, first // 2, (last + n) // 2, max(first - 1, 0), min(first + 1, n), max(inner - 1, 0), min(inner + 1, n),
          max(n - 1, 0)} | {int(v) for v in rng.integers(0, n + 1, 3)}
    for a in sorted(at):
        removes = {0, min(1, n - a), n - a, int(rng.integers(0, n - a + 1)), min(int(rng.integers(0, 700)), n - a)}
        for r in sorted(removes):
            for m in {0, 1, int(rng.integers(2, 300)), int(rng.integers(300, 5001))} if r in (0, n - a) else {0, int(rng.integers(1, 5001))}:
                yield a, r, rng.integers(0, 256, m, dtype=np.uint8).tobytes()


def check(old, cuts, p, a, r, ins, lookahead=0):
    j, t, s, got, attempts = PM.patch(old, cuts, p, a, r, ins, lookahead)
    want = CM.chunk(PM.edited(old, a, r, ins), p)
    assert got == want, (len(old), a, r, len(ins), lookahead)
    k = len(cuts) - 1
    assert 0 <= j <= max(k - 1, 0) and 0 <= s <= k and len(got) - 1 == j + t + (k - s)
    return j, t, s, got, attempts


@pytest.mark.parametrize("kind", ["random", "zero", "periodic"])
@pytest.mark.parametrize("p", [P256, P8K], ids=["p256", "p8192"])
def test_the_spliced_cuts_are_the_cuts_of_the_edited_stream(kind, p):
    rng = np.random.default_rng(sum(map(ord, kind)) + p["avg"])
    done = 0
    for n in SIZES:
        old = stream(kind, n, rng)
        cuts = CM.chunk(old, p)
        for a, r, ins in edits_of(old, cuts, rng):
            check(old, cuts, p, a, r, ins, lookahead=int(rng.choice([0, 0, 1, 3 * p["max"]])))
            done += 1
    assert done >= 500      # six cases: a few thousand edits in all


def test_every_class_of_outcome_is_reached():
    rng = np.random.default_rng(99)
    rand = stream("random", 20000, rng)
    cuts = CM.chunk(rand, P256)
    k, n = len(cuts) - 1, len(rand)
    assert k > 40
    # resync at the first window cut at or behind the edit's end, in the first window, which is not final
    j, t, s, got, attempts = check(rand, cuts, P256, cuts[5] + 3, 2, b"xyz")
    assert attempts == 1 and j == 5 and s < k and PM.window_end(cuts, cuts[5] + 5, 4 * 2048) < n
    assert got[j + t] >= cuts[5] + 6 and (t == 1 or got[j + t - 1] < cuts[5] + 6)
    # resync after one doubling: zeros never resynchronise, the random bytes behind them do at their first cut
    mixed = bytes(6000) + rand[:14000]
    mcuts = CM.chunk(mixed, P256)
    assert mcuts[:3] == [0, 2048, 4096]
    j, t, s, got, attempts = check(mixed, mcuts, P256, 0, 0, b"\x01", lookahead=1)
    assert attempts == 2 and j == 0 and s < len(mcuts) - 1 and got[t] - 1 == mcuts[s] and t == 3
    assert check(mixed, mcuts, P256, 0, 0, b"\x01")[4] == 1       # (the default lookahead reaches the random bytes at once)
    # growth to the end of the stream: all-zero data with a one-byte insert
    zeros = bytes(20000)
    zcuts = CM.chunk(zeros, P256)
    j, t, s, got, attempts = check(zeros, zcuts, P256, 0, 0, b"\x00", lookahead=1)
    assert attempts == 4        # (windows to 4096, 8192, 16384 and the end)
    assert s == len(zcuts) - 1 and j + t == len(got) - 1 and got[-1] == 20001
    # a final first window
    j, t, s, got, attempts = check(rand, cuts, P256, cuts[k - 2], 1, b"")
    assert attempts == 1 and PM.window_end(cuts, cuts[k - 2] + 1, 4 * 2048) == n
    # K == 0, and an empty result
    assert check(b"", [0], P256, 0, 0, b"hello")[:4] == (0, 1, 0, [0, 5])
    assert check(b"", [0], P256, 0, 0, b"")[:4] == (0, 0, 0, [0])
    assert check(rand, cuts, P256, 0, n, b"")[3] == [0]
    # a no-op edit and a replacement by identical bytes return the old cuts
    for a, r in ((0, 0), (n, 0), (cuts[7], 0), (cuts[7] + 1, 0), (cuts[7] - 5, 900), (0, n), (n - 1, 1)):
        assert check(rand, cuts, P256, a, r, rand[a:a + r])[3] == cuts
    # an append restarts in the last chunk, whose end the end of the stream forced
    j, t, s, got, attempts = check(rand, cuts, P256, n, 0, rand[:3000])
    assert j == k - 1 and s == k


def test_resync_is_the_device_steps_rule():
    """``resync``: the smallest t >= 1 at or behind new_from whose shifted cut is an old cut; index 0 never matches."""
    old = [0, 10, 20, 30]
    assert PM.resync([0, 10, 20], old, 0, 0, False) == (0, 1, 1, 10, 1)
    assert PM.resync([0, 10, 20], old, 11, 0, False) == (0, 2, 2, 20, 2)
    assert PM.resync([0, 5, 7], old, 0, 0, False) == (1, 0, 0, 0, 0)
    assert PM.resync([0, 5, 7], old, 0, 0, True) == (1, 0, 0, 0, 2)
    assert PM.resync([0, 5, 7], old, 0, 3, False) == (0, 2, 1, 7, 2)
    assert PM.resync([0], [0], 0, 0, True) == (1, 0, 0, 0, 0)
    assert PM.resync([3, 9], [2], 0, (1 << 64) - 7, False) == (0, 1, 0, 9, 1)      # a shift that wraps
