"""Costs of the dual guard on one GPU, beside the single guard's in the same session.

The store of tools/guard_probe.py: --gib GiB of the tiled corpus ingested as --streams streams of equal length into one cw.ChunkStore
(Skein-512, LZ4).  Then, in one session:

  a  update    one cw_dev_store_guard2_update over all stored bytes into zeroed guards at group = 4, 16 and 64 (stripe 65536), beside
               cw_dev_store_guard_update of the same bytes and a device-to-device hipMemcpyAsync of them; the sides alternate;
  c  check     cw_dev_store_guard2_check and cw_dev_store_guard_check of the whole store (group 16), alternating;
  b  queued    behind a 64 KiB ChunkStore.append and behind a 256 MiB ChunkStore.ingest of new bytes: the call alone on the store with
               its guards set aside, then the single update it would have queued (into a copy of P and of the cursor) and the dual
               update, each synchronised;
  d  repair    a byte changed in every hundredth stored chunk: scrub + repair_local on the parity-2 store -- how many chunks it
               mends, how many of them needed Q, how many stay collided; the damage again and repair_local with Q set aside (the
               parity-1 run); the damage again and repair_from a peer the streams were replicated to.  One run each, the store healed
               between them; afterwards it must scrub clean.

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
from tools.guard_probe import STRIPE, alternate, note, wall  # noqa: E402
from tools.restore_probe import tiled_corpus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=36)
    ap.add_argument("--reps", type=int, default=5)
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
           "chunks": sum(len(x.refs) for x in recipes), "reps": args.reps}
    note(f"ingested {n} bytes, {used} stored")
    zeros = lambda k, dtype=torch.int64: torch.zeros(k, dtype=dtype, device="cuda")  # noqa: E731
    words = lambda t: t.cpu().numpy().view(np.uint64).tolist()  # noqa: E731

    # a. the full updates beside a copy of the same bytes
    copy_to = torch.empty(used, dtype=torch.uint8, device="cuda")
    result = zeros(4)
    guards = {}
    for G in (4, 16, 64):
        size = cw.store_guard_bytes(A.store_bytes, STRIPE, G)
        guards[G] = dict(size=size, single=zeros(size, torch.uint8), p=zeros(size, torch.uint8), q=zeros(size, torch.uint8), covered=zeros(1),
                         covered2=zeros(1))

    def timed(prepare, call):
        def run():
            prepare()
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            run.ms.append((time.perf_counter() - t) * 1e3)
        run.ms = []
        return run

    def single(G):
        g = guards[G]
        return timed(lambda: (g["single"].zero_(), g["covered"].zero_()),
                     lambda: cw.dev_store_guard_update(A.d_store.data_ptr(), A.store_bytes, A.d_used.data_ptr(), g["covered"].data_ptr(), STRIPE, G,
                                                       g["single"].data_ptr(), g["size"], result.data_ptr(), st))

    def dual(G):
        g = guards[G]
        return timed(lambda: (g["p"].zero_(), g["q"].zero_(), g["covered2"].zero_()),
                     lambda: cw.dev_store_guard2_update(A.d_store.data_ptr(), A.store_bytes, A.d_used.data_ptr(), g["covered2"].data_ptr(), STRIPE, G,
                                                        g["p"].data_ptr(), g["q"].data_ptr(), g["size"], result.data_ptr(), st))

    def copy():
        rc = hip.hipMemcpyAsync(copy_to.data_ptr(), A.d_store.data_ptr(), used, 3, st)       # hipMemcpyDeviceToDevice
        assert rc == 0, rc

    sides = {"copy": timed(lambda: None, copy)}
    for G in guards:
        sides[f"update_g{G}"], sides[f"update2_g{G}"] = single(G), dual(G)
    alternate(sides, args.reps)
    assert words(result) == [0, 0, used, used] and (copy_to == A.d_store[:used]).all()
    for G, g in guards.items():
        assert (g["p"] == g["single"]).all() and g["q"].any()                                # P is the single guard's, bit for bit
    for name, run in sides.items():
        ms = statistics.median(run.ms[1:])                                  # (the first is the warm-up)
        res[f"{name}_ms"], res[f"{name}_runs_ms"], res[f"{name}_GBps"] = ms, run.ms[1:], used / ms / 1e6
    for G in guards:
        res[f"update_g{G}_vs_copy"] = res[f"update_g{G}_GBps"] / res["copy_GBps"]
        res[f"update2_g{G}_vs_copy"] = res[f"update2_g{G}_GBps"] / res["copy_GBps"]
        res[f"update2_g{G}_vs_update"] = res[f"update2_g{G}_ms"] / res[f"update_g{G}_ms"]
    note("; ".join(f"{name} {res[name + '_ms']:.3f} ms ({res[name + '_GBps']:.0f} GB/s)" for name in sides))
    del copy_to

    # the store's own guards from here on: group 16, parity 2, taken over from leg a
    A.stripe, A.group = STRIPE, 16
    A.d_guard, A.d_guard_q, A.d_covered, A._fold_result = guards[16]["p"], guards[16]["q"], guards[16]["covered2"], result
    single_p, single_covered = guards[16]["single"], guards[16]["covered"]
    size = guards[16]["size"]
    del guards
    assert A.protected_bytes() == used and A.guard_check(detail=True) == (0, [], [])

    # c. the checks
    bad, res4 = zeros(size // STRIPE, torch.int32), zeros(4)
    t, runs = alternate({
        "check": lambda: cw.dev_store_guard_check(A.d_store.data_ptr(), A.store_bytes, A.d_covered.data_ptr(), STRIPE, 16, A.d_guard.data_ptr(), size,
                                                  bad.data_ptr(), res4.data_ptr(), st),
        "check2": lambda: cw.dev_store_guard2_check(A.d_store.data_ptr(), A.store_bytes, A.d_covered.data_ptr(), STRIPE, 16, A.d_guard.data_ptr(),
                                                    A.d_guard_q.data_ptr(), size, bad.data_ptr(), res4.data_ptr(), st)}, args.reps)
    assert words(res4)[2] == 0
    for name in ("check", "check2"):
        res[f"{name}_g16_ms"], res[f"{name}_g16_runs_ms"], res[f"{name}_g16_GBps"] = t[name], runs[name], used / t[name] / 1e6
    res["check2_g16_vs_check"] = t["check2"] / t["check"]
    note(f"check {t['check']:.3f} ms, check2 {t['check2']:.3f} ms")

    # the peer, before anything else is appended
    B = b_idx = None
    if not args.no_peer:
        b_idx = cw.DedupeIndex("skein512", 1 << 20)
        B = cw.ChunkStore(b_idx, "lz4", p, n, 2 * cap, dir_base=1 << 32)
        A.replicate_to(B, recipes)

    # b. the queued updates behind two appending calls
    fresh = host[n:n + extra]

    def behind(call):
        held, A.d_guard, A.d_guard_q = (A.d_guard, A.d_guard_q), None, None            # the call alone
        box = {}
        t_call = wall(lambda: box.update(out=call()))
        A.d_guard, A.d_guard_q = held
        before = A.protected_bytes()
        t_single = wall(lambda: cw.dev_store_guard_update(A.d_store.data_ptr(), A.store_bytes, A.d_used.data_ptr(), single_covered.data_ptr(), STRIPE,
                                                          16, single_p.data_ptr(), size, res4.data_ptr(), st))
        t_dual = wall(A._fold)
        folded = A.protected_bytes() - before
        assert A.protected_bytes() == A.used() and folded > 0 and words(res4)[3] == folded
        return t_call, t_single, t_dual, folded

    for warm in (True, False):                        # (the first edit of a session allocates the context's buffers)
        piece = fresh[(0 if warm else 1) * 65536:][:65536]
        t_call, t_single, t_dual, folded = behind(lambda: A.append(recipes[-1], piece))
    res.update({"append_64KiB_ms": t_call, "append_64KiB_update_ms": t_single, "append_64KiB_update2_ms": t_dual, "append_64KiB_folded_bytes": folded})
    t_call, t_single, t_dual, folded = behind(lambda: A.ingest(fresh[1 << 20:]))
    res.update({"ingest_256MiB_ms": t_call, "ingest_256MiB_update_ms": t_single, "ingest_256MiB_update2_ms": t_dual,
                "ingest_256MiB_folded_bytes": folded})
    note(f"append 64 KiB {res['append_64KiB_ms']:.2f} ms + update {res['append_64KiB_update_ms']:.3f} / {res['append_64KiB_update2_ms']:.3f} ms; "
         f"ingest 256 MiB {res['ingest_256MiB_ms']:.1f} ms + update {res['ingest_256MiB_update_ms']:.3f} / {res['ingest_256MiB_update2_ms']:.3f} ms")
    assert A.guard_check() == (0, []) and (single_p == A.d_guard).all()

    # d. one damaged byte in every hundredth stored chunk of the streams
    d = A.d_dir.cpu().numpy().view(cw.LOC_DTYPE)
    named = np.unique(np.concatenate([x.refs for x in recipes])).astype(np.int64)
    hurt = named[::100]
    at = torch.from_numpy((d["pos"][hurt] + d["stored"][hurt] // 2).astype(np.int64)).cuda()
    original = A.d_store[at].clone()

    def damage():
        A.d_store[at] = original ^ 0x5C
        torch.cuda.synchronize()

    def heal():
        A.d_store[at] = original
        torch.cuda.synchronize()
        assert A.scrub().clean and A.guard_check() == (0, [])

    box = {}
    for parity in (2, 1):
        damage()
        t_scrub = wall(lambda: box.update(report=A.scrub()))
        found = len(box["report"].damaged)            # (a changed byte that decodes to the same bytes is no damage: rare, and counted)
        assert set(box["report"].damaged.tolist()) <= set(hurt.tolist()) and found > 0.9 * len(hurt), (found, len(hurt))
        held, A.d_guard_q = A.d_guard_q, (A.d_guard_q if parity == 2 else None)
        t_local = wall(lambda: box.update(out=A.repair_local(box["report"])))
        A.d_guard_q = held
        out, key = box["out"], "repair_local2" if parity == 2 else "repair_local"
        res.update({"repair_edited_chunks": len(hurt), "repair_damaged_chunks": found, "repair_scrub_ms": t_scrub, f"{key}_ms": t_local,
                    f"{key}_paired": A.last_repair["paired"], **{f"{key}_{k}": len(v) for k, v in out.items()}})
        note(f"parity {parity}: repair_local of {found} chunks: scrub {t_scrub:.0f} ms + repair_local {t_local:.0f} ms; "
             + ", ".join(f"{k} {len(v)}" for k, v in out.items()) + f", paired {A.last_repair['paired']}")
        # (a damaged chunk the scrub did not find can spoil a neighbour's rebuild: such a chunk is `failed`, rare, and counted)
        assert sum(len(v) for v in out.values()) == found and not out["unprotected"] and not out["no_digest"]
        heal()                                        # what it could not mend
    res["repair_local2_vs_local"] = res["repair_local2_ms"] / res["repair_local_ms"]
    if B is not None:
        damage()
        report = A.scrub()
        t_from = wall(lambda: box.update(out=A.repair_from(B, report)))
        assert len(box["out"]["repaired"]) == len(report.damaged) and A.scrub().clean
        res.update({"repair_from_ms": t_from, "repair_from_repaired": len(box["out"]["repaired"]), "repair_local2_vs_from": res["repair_local2_ms"] / t_from})
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
