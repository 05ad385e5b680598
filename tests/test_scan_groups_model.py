"""The LZ4 span scan's group schedule, restated in Python and checked against the serial probe schedule (no GPU needed).

The kernel (lz4_scan_span_kernel, lz4_kernel.hip) runs one batch of 64 lanes per schedule GROUP q = (k + 62) >> 6: lane L of group q is
probe k = 64 q - 62 + L at position group_base(q) + q * L.  After chunk c of a block has been staged (the ring then holds chunks c - 1
and c) it runs every group not yet run whose last position + 4 lies at or below the end of chunk c; the block's last group, the only
partial one beside group 0, runs when the block is finished.  Before that, the rule was: after chunk c, every probe at a position below
c * 4 KiB; the rest at the end."""
import pytest

CHUNK = 4096
SIZES = [4096, 8192, 16384, 32768, 65536]
GROUPS = {65536: 46, 32768: 33, 16384: 24, 8192: 17, 4096: 12}


def scan_probes(n):
    """lz4_launch's scan_probes(): the number of probes of a no-match walk over n bytes."""
    if n < 13:
        return 0
    limit = n - 11
    k, p, step, nb = 0, 1, 1, 64
    while p + step <= limit:
        p += step
        step = nb >> 6
        nb += 1
        k += 1
    return k


def probe_pos(k):
    q = (k + 62) >> 6
    return q * (k + 31 - 32 * q) + 1 + (1 if k else 0)


def group_base(q):
    return q * (32 * q - 31) + 2


def group_end(end, qlast):
    """groups q < qlast whose last position + 4 lies at or below end (the kernel's binary search on 32 q^2 + 32 q + 6 <= end)"""
    lo, hi = 0, qlast
    while lo < hi:
        mid = (lo + hi) >> 1
        if 32 * mid * mid + 32 * mid + 6 <= end:
            lo = mid + 1
        else:
            hi = mid
    return lo


def group_schedule(n):
    """[(stage, q, [(lane, position), ...])] in the order the kernel runs them; stage = chunk just staged, n // CHUNK = at the end."""
    nprobes = scan_probes(n)
    nchunks = n // CHUNK
    qlast = (nprobes + 61) >> 6
    out, qnext = [], 0

    def partial(stage, q):
        left = min(64, nprobes + 62 - 64 * q)
        lanes = range(62 if q == 0 else 0, left)
        out.append((stage, q, [(L, (q * L + group_base(q)) if q else L - 61) for L in lanes]))

    for c in range(nchunks):
        if c == 0 and qlast:
            partial(0, 0)
            qnext = 1
        qe = group_end(min((c + 1) * CHUNK, n), qlast)
        for q in range(qnext, qe):
            out.append((c, q, [(L, group_base(q) + q * L) for L in range(64)]))
        qnext = max(qnext, qe)
    assert qnext == qlast, "every full group has run once the last chunk is staged"
    if nprobes:
        partial(nchunks, qlast)
    return out


def serial_stage(pos, n):
    """the stage at which the rule 'after chunk c: every probe below c * 4 KiB, the rest at the end' runs the probe at pos"""
    return min(pos // CHUNK + 1, n // CHUNK)


@pytest.mark.parametrize("n", SIZES)
def test_groups_visit_the_serial_positions_in_order(n):
    nprobes = scan_probes(n)
    sched = group_schedule(n)
    visited = [p for _, _, lanes in sched for _, p in lanes]
    assert visited == [probe_pos(k) for k in range(nprobes)]
    # lanes ascend inside a group, groups ascend, and lane L of group q is probe 64 q - 62 + L
    ks = [64 * q - 62 + L for _, q, lanes in sched for L, _ in lanes]
    assert ks == list(range(nprobes))
    assert [q for _, q, _ in sched] == list(range(len(sched)))


@pytest.mark.parametrize("n", SIZES)
def test_group_counts(n):
    sched = group_schedule(n)
    assert len(sched) == GROUPS[n]
    # only the first and the last group are partial
    assert [q for _, q, lanes in sched if len(lanes) != 64] == sorted({0, len(sched) - 1})


@pytest.mark.parametrize("n", SIZES)
def test_every_group_runs_inside_the_ring_and_no_later_than_before(n):
    nchunks = n // CHUNK
    for stage, q, lanes in group_schedule(n):
        first, last = lanes[0][1], lanes[-1][1]
        c = min(stage, nchunks - 1)  # the newest chunk in the ring when the group runs (at the end: the block's last)
        assert first >= max(c - 1, 0) * CHUNK, (n, q)  # chunk c - 1 is the oldest byte the ring still holds
        assert last + 4 <= (c + 1) * CHUNK, (n, q)     # nothing reaches into a chunk that is not staged yet
        assert stage <= serial_stage(last, n), (n, q, stage)
        # a full group is narrower than a chunk
        assert last - first < CHUNK

