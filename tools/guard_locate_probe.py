"""Costs of locating damage from the guard's syndromes on one GPU, beside the calls it builds on, in the same session (DESIGN.md
section 31).

The store of tools/guard_probe.py: --gib GiB of the tiled corpus ingested as --streams streams of equal length into one cw.ChunkStore
(Skein-512, LZ4), protected with stripe 65536, group 16 and both syndromes; the parity-1 sides set Q aside.  Then, in one session:

  a  locate    cw_dev_store_guard_locate / cw_dev_store_guard2_locate beside cw_dev_store_guard_check / cw_dev_store_guard2_check,
               alternating, on the clean store, with 16 damaged chunks and with a byte changed in every hundredth chunk;
  b  heal      ChunkStore.heal() beside the path there was before it, a full scrub() + repair_local(), alternating, for both damage
               patterns at parity 1 and 2: what each takes, and the suspects, cleared and repaired chunks of the heal.  The store's
               bytes are put back between the runs; afterwards it must scrub clean.

Wall clock around synchronised calls: one warm-up, the median of --reps rounds.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compute_war_amd as cw  # noqa: E402
from tools.guard_probe import STRIPE, alternate, note, wall  # noqa: E402
from tools.restore_probe import tiled_corpus  # noqa: E402

GROUP = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=36)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    st = torch.cuda.current_stream().cuda_stream
    seg = 1 << 20
    per = max(1, int(args.gib * (1 << 30)) // seg // args.streams)      # segments per stream
    n_s, n = per * seg, per * seg * args.streams
    p = cw.CdcParams.default(8192)
    cap = p.max_offsets(n_s) * args.streams + 4096
    nseg = n // seg
    src = tiled_corpus(nseg * seg)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    src.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    host = src.cpu().numpy()
    del src, stamps
    stream_bytes = lambda s: host[s * n_s:(s + 1) * n_s]  # noqa: E731
    idx = cw.DedupeIndex("skein512", 1 << 20)
    A = cw.ChunkStore(idx, "lz4", p, n, cap)
    A.protect(STRIPE, GROUP, parity=2)
    recipes = [A.ingest(stream_bytes(s)) for s in range(args.streams)]
    used = A.used()
    res = {"bytes": n, "streams": args.streams, "hash": "skein512", "codec": "lz4", "stripe": STRIPE, "group": GROUP, "stored_bytes": used,
           "chunks": sum(len(x.refs) for x in recipes), "reps": args.reps}
    note(f"ingested {n} bytes, {used} stored")
    assert A.protected_bytes() == used and A.guard_check(detail=True) == (0, [], [])
    zeros = lambda k, dtype=torch.int64: torch.zeros(k, dtype=dtype, device="cuda")  # noqa: E731
    words = lambda t: t.cpu().numpy().view(np.uint64).tolist()  # noqa: E731
    size = A.d_guard.numel()

    d = A.d_dir.cpu().numpy().view(cw.LOC_DTYPE)
    named = np.unique(np.concatenate([x.refs for x in recipes])).astype(np.int64)
    patterns = {"16": named[len(named) // 32::len(named) // 16][:16], "dense": named[::100]}

    class Damage:
        def __init__(self, hurt):
            self.hurt = hurt
            self.at = torch.from_numpy((d["pos"][hurt] + d["stored"][hurt] // 2).astype(np.int64)).cuda()
            self.original = A.d_store[self.at].clone()

        def do(self):
            A.d_store[self.at] = self.original ^ 0x5C
            torch.cuda.synchronize()

        def undo(self):
            A.d_store[self.at] = self.original
            torch.cuda.synchronize()

    # a. locate beside check
    bad, res4, res8, suspect = zeros(size // STRIPE, torch.int32), zeros(4), zeros(8), zeros(A.dir_entries, torch.int32)
    front = (A.d_store.data_ptr(), A.store_bytes)
    geo = (A.d_covered.data_ptr(), STRIPE, GROUP)
    dirs = (A.d_dir.data_ptr(), A.dir_base, A.dir_entries)
    sides = {
        "check": lambda: cw.dev_store_guard_check(*front, *geo, A.d_guard.data_ptr(), size, bad.data_ptr(), res4.data_ptr(), st),
        "check2": lambda: cw.dev_store_guard2_check(*front, *geo, A.d_guard.data_ptr(), A.d_guard_q.data_ptr(), size, bad.data_ptr(), res4.data_ptr(), st),
        "locate": lambda: cw.dev_store_guard_locate(*front, *dirs, *geo, A.d_guard.data_ptr(), size, suspect.data_ptr(), res8.data_ptr(), st),
        "locate2": lambda: cw.dev_store_guard2_locate(*front, *dirs, *geo, A.d_guard.data_ptr(), A.d_guard_q.data_ptr(), size, suspect.data_ptr(),
                                                      res8.data_ptr(), st)}
    for state in ("clean", "16", "dense"):
        dmg = None if state == "clean" else Damage(patterns[state])
        if dmg:
            dmg.do()
        t, runs = alternate(sides, args.reps)
        totals = words(res8)                                               # (of the last call: locate2)
        assert totals[0] == 0 and (totals[2] == 0) == (dmg is None)
        for name in sides:
            res[f"{name}_{state}_ms"], res[f"{name}_{state}_runs_ms"] = t[name], runs[name]
        res[f"locate_{state}_vs_check"], res[f"locate2_{state}_vs_check2"] = t["locate"] / t["check"], t["locate2"] / t["check2"]
        res[f"locate2_{state}_totals"] = dict(zip(("groups", "dirty_cells", "located_cells", "ambiguous_cells", "suspects", "unprotected"), totals[1:7]))
        note(f"{state}: check {t['check']:.3f} / {t['check2']:.3f} ms, locate {t['locate']:.3f} / {t['locate2']:.3f} ms; {res[f'locate2_{state}_totals']}")
        if dmg:
            dmg.undo()

    # b. heal beside a full scrub + repair_local
    box = {}
    held_q = A.d_guard_q
    for state in ("16", "dense"):
        dmg = Damage(patterns[state])
        for parity in (1, 2):
            A.d_guard_q = held_q if parity == 2 else None

            def parent():
                dmg.do()
                box["t"] = wall(lambda: box.update(parent=A.repair_local(A.scrub())))
                dmg.undo()                                                  # what it could not mend

            def heal():
                dmg.do()
                box["t"] = wall(lambda: box.update(heal=A.heal()))
                dmg.undo()

            times = {"parent": [], "heal": []}
            for rep in range(args.reps + 1):                               # the first round is the warm-up
                for name, fn in (("parent", parent), ("heal", heal)):
                    fn()
                    if rep:
                        times[name].append(box["t"])
            A.d_guard_q = held_q
            key = f"p{parity}_{state}"
            t_parent, t_heal, out = statistics.median(times["parent"]), statistics.median(times["heal"]), box["heal"]
            res.update({f"scrub_repair_{key}_ms": t_parent, f"scrub_repair_{key}_runs_ms": times["parent"], f"heal_{key}_ms": t_heal,
                        f"heal_{key}_runs_ms": times["heal"], f"heal_{key}_vs_scrub_repair": t_heal / t_parent,
                        f"heal_{key}_edited_chunks": len(dmg.hurt), f"heal_{key}_windows": out["windows"], f"heal_{key}_groups_left": out["groups_left"],
                        f"scrub_repair_{key}_repaired": len(box["parent"]["repaired"]),
                        **{f"heal_{key}_{k}": len(out[k]) for k in ("suspects", "located", "ambiguous", "cleared", "repaired", "collided", "failed")}})
            note(f"parity {parity}, {state}: scrub + repair_local {t_parent:.1f} ms, heal {t_heal:.1f} ms ({t_heal / t_parent:.3f}); "
                 f"{len(out['suspects'])} suspects, {len(out['cleared'])} cleared, {len(out['repaired'])} repaired, {out['windows']} windows")
    assert A.scrub().clean and A.guard_check() == (0, [])
    assert A.restore(recipes[0], verify=True) == stream_bytes(0).tobytes()
    idx.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
