"""Costs of the guard stripes on one GPU.

--gib GiB of the tiled corpus of tools/restore_probe.py (1 MiB segments, a stamp every 1 KiB, no duplicate segments) ingested as
--streams streams of equal length into one cw.ChunkStore (Skein-512, LZ4), as tools/scrub_probe.py does.  Then, in one session:

  a  update    one cw_dev_store_guard_update over all stored bytes into a zeroed guard at group = 4, 16 and 64 (stripe 65536), beside
               a device-to-device hipMemcpyAsync of the same bytes, which also moves every byte once; the sides alternate;
  b  queued    the update behind a 64 KiB ChunkStore.append and behind a 256 MiB ChunkStore.ingest of new bytes: the call alone on
               the store with its guard set aside, then the update it would have queued, each synchronised;
  c  check     cw_dev_store_guard_check of the whole store (group 16);
  d  repair    a byte changed in every hundredth stored chunk (the pattern of tools/scrub_probe.py): scrub + repair_local, verify
               on; then the chunks it could not repair are healed, the same damage is done again, and scrub + repair_from a peer
               that the streams were replicated to runs over it.  One run each.  Afterwards the store must scrub clean.

Wall clock around synchronised calls: one warm-up, the median of --reps rounds for a and c.  Prints one JSON object (and writes it
to --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compute_war_amd as cw  # noqa: E402
from tools.restore_probe import tiled_corpus  # noqa: E402

STRIPE = 65536


def note(text):
    print(text, file=sys.stderr, flush=True)   # progress: the run takes minutes


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(configs, reps):
    """(median ms, the runs) of every configuration: one warm-up each, then reps rounds over all of them"""
    times = {name: [] for name in configs}
    for fn in configs.values():
        wall(fn)
    for _ in range(reps):
        for name, fn in configs.items():
            times[name].append(wall(fn))
    return {name: statistics.median(t) for name, t in times.items()}, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=36)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-peer", action="store_true", help="leave the repair_from leg out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    st = torch.cuda.current_stream().cuda_stream
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    seg = 1 << 20
    per = max(1, int(args.gib * (1 << 30)) // seg // args.streams)      # segments per stream
    n_s, n = per * seg, per * seg * args.streams
    extra = (256 << 20) + (1 << 20)
    p = cw.CdcParams.default(8192)
    cap = p.max_offsets(n_s) * args.streams + p.max_offsets(extra) + 4096
    nseg = (n + extra) // seg
    src = tiled_corpus(nseg * seg)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    src.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    host = src.cpu().numpy()
    del src, stamps
    stream_bytes = lambda s: host[s * n_s:(s + 1) * n_s]  # noqa: E731
    idx = cw.DedupeIndex("skein512", 1 << 20)
    A = cw.ChunkStore(idx, "lz4", p, n + extra, cap)
    recipes = [A.ingest(stream_bytes(s)) for s in range(args.streams)]
    used = A.used()
    res = {"bytes": n, "streams": args.streams, "hash": "skein512", "codec": "lz4", "stripe": STRIPE, "stored_bytes": used,
           "chunks": sum(len(x.refs) for x in recipes)}
    note(f"ingested {n} bytes, {used} stored")

    # a. the full update beside a copy of the same bytes
    copy_to = torch.empty(used, dtype=torch.uint8, device="cuda")
    result = torch.zeros(4, dtype=torch.int64, device="cuda")
    guards = {}
    for G in (4, 16, 64):
        size = cw.store_guard_bytes(A.store_bytes, STRIPE, G)
        guards[G] = (torch.zeros(size, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), size)

    def update(G):
        guard, covered, size = guards[G]

        def run():
            guard.zero_()
            covered.zero_()
            torch.cuda.synchronize()
            t = time.perf_counter()
            cw.dev_store_guard_update(A.d_store.data_ptr(), A.store_bytes, A.d_used.data_ptr(), covered.data_ptr(), STRIPE, G, guard.data_ptr(), size,
                                      result.data_ptr(), st)
            torch.cuda.synchronize()
            run.ms.append((time.perf_counter() - t) * 1e3)
        run.ms = []
        return run

    def copy():
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = hip.hipMemcpyAsync(copy_to.data_ptr(), A.d_store.data_ptr(), used, 3, st)   # hipMemcpyDeviceToDevice
            torch.cuda.synchronize()
            run.ms.append((time.perf_counter() - t) * 1e3)
            assert rc == 0, rc
        run.ms = []
        return run

    sides = {"copy": copy(), **{f"update_g{G}": update(G) for G in guards}}
    alternate(sides, args.reps)
    assert result.cpu().numpy().view(np.uint64).tolist() == [0, 0, used, used] and (copy_to == A.d_store[:used]).all()
    for name, run in sides.items():
        ms = statistics.median(run.ms[1:])                                  # (the first is the warm-up)
        res[f"{name}_ms"], res[f"{name}_runs_ms"], res[f"{name}_GBps"] = ms, run.ms[1:], used / ms / 1e6
    for G in guards:
        res[f"update_g{G}_vs_copy"] = res[f"update_g{G}_GBps"] / res["copy_GBps"]
    note("; ".join(f"{name} {res[name + '_ms']:.2f} ms ({res[name + '_GBps']:.0f} GB/s)" for name in sides))
    del copy_to

    # the store's own guard from here on: group 16, taken over from leg a
    A.stripe, A.group = STRIPE, 16
    A.d_guard, A.d_covered, A._fold_result = guards[16][0], guards[16][1], result
    del guards[4], guards[64]
    assert A.protected_bytes() == used and A.guard_check() == (0, [])

    # c. the check
    bad, res4 = torch.zeros(A.d_guard.numel() // STRIPE, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    t, runs = alternate({"check": lambda: cw.dev_store_guard_check(A.d_store.data_ptr(), A.store_bytes, A.d_covered.data_ptr(), STRIPE, 16,
                                                                    A.d_guard.data_ptr(), A.d_guard.numel(), bad.data_ptr(), res4.data_ptr(), st)}, args.reps)
    assert res4.cpu().numpy().view(np.uint64).tolist()[2] == 0
    res["check_g16_ms"], res["check_g16_runs_ms"], res["check_g16_GBps"] = t["check"], runs["check"], used / t["check"] / 1e6
    note(f"check {t['check']:.2f} ms")

    # the peer, before anything else is appended
    B = b_idx = None
    if not args.no_peer:
        b_idx = cw.DedupeIndex("skein512", 1 << 20)
        B = cw.ChunkStore(b_idx, "lz4", p, n, 2 * cap, dir_base=1 << 32)
        A.replicate_to(B, recipes)

    # b. the queued update behind two appending calls
    fresh = host[n:n + extra]

    def behind(call):
        guard, A.d_guard = A.d_guard, None            # the call alone
        box = {}
        t_call = wall(lambda: box.update(out=call()))
        A.d_guard = guard
        before = A.protected_bytes()
        t_update = wall(A._fold)
        folded = A.protected_bytes() - before
        assert A.protected_bytes() == A.used() and folded > 0
        return box["out"], t_call, t_update, folded

    for warm in (True, False):                        # (the first edit of a session allocates the context's buffers)
        piece = fresh[(0 if warm else 1) * 65536:][:65536]
        _, t_call, t_update, folded = behind(lambda: A.append(recipes[-1], piece))
    res.update({"append_64KiB_ms": t_call, "append_64KiB_update_ms": t_update, "append_64KiB_folded_bytes": folded})
    _, t_call, t_update, folded = behind(lambda: A.ingest(fresh[1 << 20:]))
    res.update({"ingest_256MiB_ms": t_call, "ingest_256MiB_update_ms": t_update, "ingest_256MiB_folded_bytes": folded})
    note(f"append 64 KiB {res['append_64KiB_ms']:.2f} ms + update {res['append_64KiB_update_ms']:.3f} ms; ingest 256 MiB "
         f"{res['ingest_256MiB_ms']:.1f} ms + update {res['ingest_256MiB_update_ms']:.3f} ms")
    assert A.guard_check() == (0, [])

    # d. one damaged byte in every hundredth stored chunk of the streams
    d = A.d_dir.cpu().numpy().view(cw.LOC_DTYPE)
    named = np.unique(np.concatenate([x.refs for x in recipes])).astype(np.int64)
    hurt = named[::100]
    at = torch.from_numpy((d["pos"][hurt] + d["stored"][hurt] // 2).astype(np.int64)).cuda()
    original = A.d_store[at].clone()

    def damage():
        A.d_store[at] = original ^ 0x5C
        torch.cuda.synchronize()

    damage()
    box = {}
    t_scrub = wall(lambda: box.update(report=A.scrub()))
    found = len(box["report"].damaged)                # (a changed byte that decodes to the same bytes is no damage: rare, and counted)
    assert set(box["report"].damaged.tolist()) <= set(hurt.tolist()) and found > 0.9 * len(hurt), (found, len(hurt))
    t_local = wall(lambda: box.update(out=A.repair_local(box["report"])))
    out = box["out"]
    res.update({"repair_edited_chunks": len(hurt), "repair_damaged_chunks": found, "repair_scrub_ms": t_scrub, "repair_local_ms": t_local,
                **{f"repair_local_{k}": len(v) for k, v in out.items()}})
    note(f"repair_local of {found} chunks: scrub {t_scrub:.0f} ms + repair_local {t_local:.0f} ms; " + ", ".join(f"{k} {len(v)}" for k, v in out.items()))
    # (a damaged chunk the scrub did not find can spoil a neighbour's rebuild: such a chunk is `failed`, rare, and counted)
    assert sum(len(v) for v in out.values()) == found and not out["unprotected"] and not out["no_digest"] and len(out["failed"]) <= len(hurt) - found
    A.d_store[at] = original                          # heal what it could not
    torch.cuda.synchronize()
    assert A.scrub().clean and A.guard_check() == (0, [])
    if B is not None:
        damage()
        report = A.scrub()
        t_from = wall(lambda: box.update(out=A.repair_from(B, report)))
        assert len(box["out"]["repaired"]) == len(report.damaged) and A.scrub().clean
        res.update({"repair_from_ms": t_from, "repair_from_repaired": len(box["out"]["repaired"]), "repair_local_vs_from": t_from / t_local})
        note(f"repair_from of {len(report.damaged)} chunks: {t_from:.0f} ms")
        b_idx.close()
    assert A.restore(recipes[0], verify=True) == stream_bytes(0).tobytes()
    idx.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
