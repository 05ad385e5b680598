"""The whole chunk store in plain Python, and the life-cycle scripts that run on it and on ``cw.ChunkStore``.

``Store`` is ``restore_model.Model`` (blob, directory, ``values`` keyed by content) with what ``ChunkStore`` keeps beside its buffers:
``base``, ``dir_base``, the directory's size, ``store_bytes``, ``max_entries``, the live named streams (name -> bytes, refs, cuts) and,
once ``protect`` has been called, the guard: (stripe, group, parity, P, Q or None, covered), kept by guard_model / guard2_model's
``update``, read by their ``check`` and ``rebuild``.
Every method mirrors a ``ChunkStore`` call and composes the model of that call -- it restates none of them -- and returns a dict with
``code``: 0, or the CwError code of a refusal, after which nothing has changed where the header says nothing changes.  A refused
one-shot ``ingest`` / ``ingest_many`` leaves the index as it was, too.  The module never imports the package under test.

A script is a list of steps ``(op, args)`` over named stores and named streams, built deterministically (the seeds are in this file)
by running the model, so that counts a step needs -- the window chunks of the next patch, the stored chunks K -- are the model's.
``scripts(oracle, alg)`` returns them; ``run`` is the one interpreter of a step on the model, which the builder, the model test and the
GPU test share.  A recipe is either current or wholly stale in these scripts (``renumber`` moves to another ``dir_base``), so the
model refuses a call on a stale recipe by restoring the whole recipe, not only the positions the call reads."""
from __future__ import annotations

import functools
import os

import numpy as np

import account_model as AM
import cdc_model as CM
import compose_model as XM
import delta_model as DM
import guard2_model as G2
import guard_model as G1
import ingest_model as IM
import patch_model as PM
import read_model as RD
import renumber_model as RN
import replicate_model as RP
import restore_model as RM
import scrub_model as SM
import store_gc_model as GM
import streams_ingest_model as SIM

P = XM.P                                         # 64 / 256 / 2048
NONE = XM.NONE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corpus", "canterbury")


class Stream:
    def __init__(self, data: bytes, refs, cuts):
        self.bytes, self.refs, self.cuts = bytes(data), [int(r) for r in refs], [int(c) for c in cuts]
        assert len(self.cuts) == len(self.refs) + 1

    def chunks(self):
        return [self.bytes[a:b] for a, b in zip(self.cuts[:-1], self.cuts[1:])]


def ok(**kw):
    return dict(code=0, **kw)


class Guard:
    """What ``protect`` keeps: (stripe, group, parity, P, Q or None, covered).  A fresh one is all zero with its cursor at 0."""

    def __init__(self, stripe, group, parity, store_bytes):
        size = G1.guard_bytes(max(store_bytes, 1), stripe, group)
        assert size and parity in (1, 2) and (parity == 1 or G2.geometry_ok(stripe, group)), (stripe, group, parity)
        self.stripe, self.group, self.parity, self.covered = stripe, group, parity, 0
        self.P, self.Q = np.zeros(size, np.uint8), np.zeros(size, np.uint8) if parity == 2 else None

    def state(self):
        return self.stripe, self.group, self.parity, self.P.tobytes(), None if self.Q is None else self.Q.tobytes(), self.covered


def _folds(method):
    """A Store method that mirrors an appending ChunkStore method: it ends, refused or not, with one guard update."""
    @functools.wraps(method)
    def appending(self, *args, **kwargs):
        try:
            return method(self, *args, **kwargs)
        finally:
            self._fold()
    return appending


class Store:
    def __init__(self, oracle, alg, store_bytes, dir_entries, dir_base=0, max_entries=1 << 14, p=P):
        self.m = RM.Model(oracle, alg, store_bytes, dir_entries, dir_base)
        self.p, self.base, self.max_entries = p, dir_base, max_entries
        self.streams, self.stale = {}, {}
        self.made = set()                        # the contents of every stream made since the last compact, and of the kept ones
        self.hurt = set()                        # the values ``corrupt`` has flipped a byte of and no repair has replaced
        self.last_patch = self.last_compose = self.last_repair = None
        self.guard = None                        # a Guard while the store is protected
        self.flipped = set()                     # what has been flipped since the last ``protect`` and not put back: stored positions, and
        #                                          (which, at) of the guard -- while it is empty, the guard is exact

    # ---- state ------------------------------------------------------------------------------------------------------------------
    @property
    def dir_base(self):
        return self.m.dir_base

    @property
    def dir_entries(self):
        return len(self.m.directory)

    @property
    def store_bytes(self):
        return self.m.store_bytes

    @property
    def used(self):
        return len(self.m.blob)

    def stored_chunks(self) -> int:
        return int(RN.nonzero(self.m.directory).sum())

    def holes(self) -> int:
        """the all-zero entries below ``base``"""
        return self.base - self.dir_base - int(RN.nonzero(self.m.directory[:self.base - self.dir_base]).sum())

    def snapshot(self):
        return (bytes(self.m.blob), self.m.directory.tobytes(), tuple(sorted(self.m.values.items())), self.base, self.dir_base, self.dir_entries,
                self.store_bytes, tuple(sorted((n, tuple(s.refs), tuple(s.cuts)) for n, s in self.streams.items())),
                None if self.guard is None else self.guard.state())

    def _get(self, name):
        return self.streams[name] if name in self.streams else self.stale[name]

    def _restores(self, s: Stream) -> bool:
        got = RM.restore(self.m.blob, self.store_bytes, self.m.directory, self.dir_base, s.refs, s.cuts, s.cuts[-1], self.m.decode())
        return all(st == 0 for st, _ in got)

    def _make(self, name, data, refs, cuts):
        self.streams[name] = Stream(data, refs, cuts)
        self.stale.pop(name, None)
        self.made.update(self.streams[name].chunks())

    def _admit(self, k: int, nbytes: int):
        """cw_store_ingest's admission of a piece of k chunks that consumes nbytes: None, or the refusal"""
        if len(self.m.values) + k > self.max_entries:
            return dict(code=-5, why="index")
        if k and not (self.dir_base <= self.base and self.base + k <= self.dir_base + self.dir_entries):
            return dict(code=-5, why="directory")
        if self.used + nbytes > self.store_bytes:
            return dict(code=-5, why="store")
        return None

    # ---- the guard --------------------------------------------------------------------------------------------------------------
    def _stored(self):
        return np.frombuffer(bytes(self.m.blob), np.uint8)

    def protect(self, stripe=65536, group=16, parity=1):
        """a fresh guard, also over one that is there, and one fold of [0, used)"""
        self.guard = Guard(stripe, group, parity, self.store_bytes)
        self.flipped = set()
        self._fold()
        return ok()

    def _fold(self):
        g = self.guard
        if g is None:
            return
        if g.Q is None:
            result, g.covered = G1.update(g.P, self._stored(), self.store_bytes, self.used, g.covered, g.stripe, g.group)
        else:
            result, g.covered = G2.update(g.P, g.Q, self._stored(), self.store_bytes, self.used, g.covered, g.stripe, g.group)
        assert result[0] == 0 and g.covered == self.used, result

    def guard_check(self, detail=True):
        g = self.guard
        if g.Q is None:
            result, bits = G1.check(g.P, self._stored(), self.store_bytes, g.covered, g.stripe, g.group)
        else:
            result, bits = G2.check(g.P, g.Q, self._stored(), self.store_bytes, g.covered, g.stripe, g.group)
        assert result[0] == 0
        which = np.nonzero(bits)[0].tolist()
        return ok(count=result[2], groups=which, bits=bits[which].tolist())

    def corrupt_guard(self, which, at):
        """not a ChunkStore call: byte ``at`` of P (which = 0) or Q (1) is flipped"""
        (self.guard.P, self.guard.Q)[which][at] ^= 0xFF
        self.flipped ^= {(which, at)}
        return ok(at=at)

    def repair_local(self, damaged, verify=True):
        g = self.guard
        damaged = sorted(set(int(v) for v in damaged))
        self.last_repair = dict(paired=0)
        out = dict(repaired=[], collided=[], unprotected=[], failed=[], no_digest=[])
        if not damaged:
            return ok(**out, paired=0)
        if damaged[0] < self.dir_base or damaged[-1] >= self.dir_base + self.dir_entries:
            return dict(code=-2)
        by_value = {v: c for c, v in self.m.values.items()}
        out["no_digest"] = [v for v in damaged if v not in by_value]
        if g.Q is None:
            result, status, payload, locs = G1.rebuild(self._stored(), self.store_bytes, self.m.directory, self.dir_base, g.covered, g.stripe, g.group,
                                                       g.P, damaged, 1 << 62)
        else:
            result, status, payload, locs = G2.rebuild(self._stored(), self.store_bytes, self.m.directory, self.dir_base, g.covered, g.stripe, g.group,
                                                       g.P, g.Q, damaged, 1 << 62)
            self.last_repair = dict(paired=result[4])
        assert result[0] == 0
        held = [(k, v) for k, v in enumerate(damaged) if v in by_value]
        out["collided"] = [v for k, v in held if status[k] == G1.COLLIDES]
        out["unprotected"] = [v for k, v in held if status[k] == G1.UNPROTECTED]
        # the rebuilt ones in ascending pos: good when the payload decodes to the content the index holds, and not in front of the end
        # of the good one before it
        rebuilt = sorted((int(self.m.directory[v - self.dir_base]["pos"]), k, v) for k, v in held if status[k] == G1.REBUILT)
        end = 0
        for pos, k, v in rebuilt:
            at, stored, word = (int(x) for x in locs[k])
            good = pos >= end
            if good and verify:
                want = by_value[v]
                (st, piece), = RM.restore(payload, len(payload), locs, 0, [k], [0, len(want)], len(want), self.m.decode())
                good = st == 0 and piece == want
            if good:
                self.m.blob[pos:pos + stored] = payload[at:at + stored].tobytes()
                self.flipped -= set(range(pos, pos + stored))
                end = pos + stored
            out["repaired" if good else "failed"].append(v)
        out["repaired"].sort()
        out["failed"].sort()
        self.hurt -= set(out["repaired"])
        return ok(**out, paired=self.last_repair["paired"])

    # ---- ingest -----------------------------------------------------------------------------------------------------------------
    def _one_shot(self, data: bytes, cuts):
        """ONE fused call and ONE cw_dev_store_chunks: (refs, new, stored bytes), or the refusal with the index put back"""
        before = dict(self.m.values)
        refs, new, verdict, total = self.m.ingest(data, cuts, self.base)
        assert len(self.m.values) <= self.max_entries
        if verdict:
            self.m.values = before
            return dict(code=-5, why="store" if verdict == 1 else "directory", needed=total)
        self.base += len(cuts) - 1
        return refs, new, total

    @_folds
    def ingest(self, name, data):
        cuts = CM.chunk(data, self.p) if len(data) else [0]
        got = self._one_shot(data, cuts)
        if isinstance(got, dict):
            return got
        self._make(name, data, got[0], cuts)
        return ok(new_chunks=len(got[1]), stored_bytes=got[2])

    @_folds
    def ingest_many(self, names, datas):
        data, cuts, first = XM.join([bytes(d) for d in datas], self.p)
        got = self._one_shot(data, cuts)
        if isinstance(got, dict):
            return got
        for f, (name, d) in enumerate(zip(names, datas)):
            a, b = first[f], first[f + 1]
            self._make(name, d, got[0][a:b], [c - cuts[a] for c in cuts[a:b + 1]])
        return ok(new_chunks=len(got[1]), stored_bytes=got[2])

    @_folds
    def ingest_stream(self, name, data, piece):
        r = IM.ingest(self.m, data, self.p, piece, self.base, self.max_entries)
        self.base += r.nchunks
        self._make(name, data[:r.consumed], r.refs, r.offsets)
        return dict(code=-5 if r.refused else 0, why=r.refused, run=r, stats=r.stats)

    @_folds
    def ingest_many_stream(self, names, datas, piece):
        r = SIM.ingest_streams(self.m, [bytes(d) for d in datas], self.p, piece, self.base, self.max_entries)
        self.base += r.nchunks
        whole, partial = r.recipes()
        for name, d, (refs, cuts) in zip(names, datas, whole):
            self._make(name, d, refs, cuts)
        if partial is not None:
            self._make(names[r.streams_done], datas[r.streams_done][:partial[1][-1]], *partial)
        return dict(code=-5 if r.refused else 0, why=r.refused, run=r, stats=r.stats)

    # ---- edits ------------------------------------------------------------------------------------------------------------------
    @_folds
    def patch(self, src, dst, a, r, ins, lookahead=0, dry=False):
        """``dry``: only the plan (j, t, s, cuts), nothing changes"""
        old = self._get(src)
        if not self._restores(old):
            return dict(code=-2)
        j, t, s, cuts, attempts = PM.patch(old.bytes, old.cuts, self.p, a, r, ins, lookahead)
        new = PM.edited(old.bytes, a, r, ins)
        lo, hi = cuts[j], cuts[j + t]
        plan = dict(j=j, t=t, s=s, window=(lo, hi), attempts=attempts)
        refused = self._admit(t, hi - lo)
        if dry or refused:
            return dict(refused or ok(), **plan)
        refs, fresh, verdict, total = self.m.ingest(new[lo:hi], [c - lo for c in cuts[j:j + t + 1]], self.base)
        assert verdict == 0, "an admitted append was refused"
        self.base += t
        self._make(dst, new, old.refs[:j] + refs + old.refs[s:], cuts)
        self.last_patch = dict(window_chunks=t, new_chunks=len(fresh), stored_bytes=total)
        return ok(**plan, **self.last_patch)

    @_folds
    def _compose(self, dst, sources, ops, payload, lookahead=0):
        srcs = [self._get(n) for n in sources]
        if not all(self._restores(s) for s in srcs):
            return dict(code=-2)
        a, cuts, first, refs_a = b"", [0], [0], []
        for s in srcs:
            cuts += [len(a) + c for c in s.cuts[1:]]
            a += s.bytes
            refs_a += s.refs
            first.append(len(cuts) - 1)
        if not ops:
            self._make(dst, b"", [], [0])
            self.last_compose = dict(rebuilt_chunks=0, new_chunks=0, stored_bytes=0)
            return ok(**self.last_compose)
        got = XM.compose(a, cuts, first, ops, payload, self.p, lookahead)
        b, bcuts, kept = got["bytes"], got["cuts"], got["kept"]
        t = got["stats"]["rebuilt_chunks"]
        refused = self._admit(t, got["stats"]["rebuilt_bytes"])
        if refused:
            return refused
        # ONE commit: the extents back to back, rebuilt chunk i of the call in B order
        data, rcuts = b"", [0]
        for lo, hi, _ in got["extents"]:
            i = bcuts.index(lo)
            while bcuts[i] < hi:
                rcuts.append(len(data) + bcuts[i + 1] - lo)
                i += 1
            data += b[lo:hi]
        assert len(rcuts) - 1 == t
        refs, fresh, verdict, total = self.m.ingest(data, rcuts, self.base)
        assert verdict == 0, "an admitted append was refused"
        self.base += t
        it = iter(refs)
        out = [refs_a[kept[x]] if x in kept else next(it) for x in bcuts[:-1]]
        assert next(it, None) is None
        self._make(dst, b, out, bcuts)
        self.last_compose = dict(rebuilt_chunks=t, new_chunks=len(fresh), stored_bytes=total)
        return ok(kept=kept, cuts=bcuts, stats=got["stats"], **self.last_compose)

    def compose(self, dst, parts, lookahead=0):
        """parts: (name, offset, length) or bytes, as ``ChunkStore.compose`` takes them"""
        sources, where, tiled = [], {}, []
        for part in parts:
            if isinstance(part, tuple):
                name, off, n = part
                if name not in where:
                    where[name] = sum(len(self._get(s).bytes) for s in sources)
                    sources.append(name)
                tiled.append(("copy", where[name] + off, n))
            else:
                tiled.append(("new", bytes(part)))
        ops, payload = XM.tile(tiled)
        return self._compose(dst, sources, ops, payload, lookahead)

    def concat(self, dst, names):
        return self.compose(dst, [(n, 0, len(self._get(n).bytes)) for n in names])

    def edit(self, src, dst, edits):
        parts, at, n = [], 0, len(self._get(src).bytes)
        for o, r, d in sorted(edits, key=lambda e: (e[0], e[1])):
            parts += [(src, at, o - at), d]
            at = o + r
        return self.compose(dst, parts + [(src, at, n - at)])

    def apply_delta(self, old, dst, ops, payload):
        return self._compose(dst, [old], [tuple(int(v) for v in o) for o in ops], payload)

    # ---- compact, renumber --------------------------------------------------------------------------------------------------------
    def _mark(self, names):
        live, outside = np.zeros(self.dir_entries, np.uint32), 0
        for n in names:
            live, outside = GM.mark(self._get(n).refs, self.dir_base, self.dir_entries, live, outside)
        return live, outside

    def compact(self, keep, store_bytes=None):
        live, outside = self._mark(keep)
        new_bytes = self.store_bytes if store_bytes is None else store_bytes
        verdict, result, blob, new_dir = GM.compact(self.m.blob, self.store_bytes, self.m.directory, live, new_bytes)
        if verdict == 2 or outside:
            return dict(code=-2)
        if verdict:
            return dict(code=-5, needed=result[1])
        before, count = self.used, len(self.m.values)
        dropped = {c for c, v in self.m.values.items() if c not in GM.retain(self.m.values, live, self.dir_base, self.dir_entries)}
        self.m.values = GM.retain(self.m.values, live, self.dir_base, self.dir_entries)
        self.m.blob, self.m.directory, self.m.store_bytes = bytearray(blob), new_dir, new_bytes
        self.streams = {n: s for n, s in self.streams.items() if n in keep}
        self.stale = {}
        self.made = {c for s in self.streams.values() for c in s.chunks()}
        if self.guard is not None:                                         # every kept byte moved: a fresh guard over the new store
            self.protect(self.guard.stripe, self.guard.group, self.guard.parity)
        return ok(kept=result[2], dropped=result[3], bytes_before=before, bytes_after=result[1], removed=count - len(self.m.values),
                  dropped_contents=dropped)

    def renumber(self, keep, dir_entries=None, dir_base=None):
        n, old_base = self.dir_entries, self.dir_base
        new_base = old_base if dir_base is None else dir_base
        K = self.stored_chunks()
        new_entries = max(n, K) if dir_entries is None else dir_entries
        if new_entries < max(K, 1):
            return dict(code=-5, needed=K)
        result, new_dir, d_from, d_to = RN.renumber(self.m.directory, old_base, None, new_base, new_base, new_entries, K)
        assert result[0] == 0 and result[1] == K
        out = {}
        for name in keep:
            out[name], missing = RP.translate(self._get(name).refs, d_from, d_to)
            if missing:
                return dict(code=-2, missing=missing)
        keys = list(self.m.values)
        res, vals = RN.revalue([self.m.values[k] for k in keys], d_from, d_to, K, K, old_base, n)
        if res[0]:
            return dict(code=-2, stale=res[2])
        self.m.values = dict(zip(keys, vals))
        self.m.directory, self.m.dir_base, self.base = new_dir, new_base, result[2]
        for name, s in list(self.streams.items()):
            if name in out:
                s.refs = out[name]
            else:
                self.stale[name] = self.streams.pop(name)
        return ok(K=K)

    # ---- reading ----------------------------------------------------------------------------------------------------------------
    def restore(self, name):
        s = self._get(name)
        got = RM.restore(self.m.blob, self.store_bytes, self.m.directory, self.dir_base, s.refs, s.cuts, s.cuts[-1], self.m.decode())
        if any(st for st, _ in got):
            return dict(code=-2)
        return ok(bytes=b"".join(piece for _, piece in got))

    def read_ranges(self, name, ranges):
        s = self._get(name)
        to, placed = 0, []
        for off, n in ranges:
            placed.append((off, n, to))
            to += n
        got = RD.read(self.m.blob, self.store_bytes, self.m.directory, self.dir_base, s.refs, s.cuts, placed, to, self.m.decode())
        if any(st for st, _ in got):
            return dict(code=-2)
        return ok(bytes=[piece for _, piece in got])

    def diff(self, old, new):
        a, b = self._get(old), self._get(new)
        got = DM.diff(a.refs, a.cuts, b.refs, b.cuts, self.dir_base, self.dir_entries)
        assert got["verdict"] == 0
        return ok(ops=got["ops"], src=got["src"], totals=got["totals"][1:], payload=DM.payload_of(b.bytes, got["ops"]))

    def account(self, names, flag=None):
        refs, first = [], [0]
        for n in names:
            refs += self._get(n).refs
            first.append(len(refs))
        verdict, streams, refcount, owner, totals = AM.account(refs, first, self.m.directory, self.dir_base, flag)
        assert verdict == 0
        return ok(streams=streams, refcount=refcount, owner=owner, totals=totals[1:])

    # ---- scrub, repair ------------------------------------------------------------------------------------------------------------
    def corrupt(self, value, at):
        """not a ChunkStore call: stored byte ``at`` of the chunk ``value`` is flipped"""
        pos, stored, _ = (int(v) for v in self.m.directory[value - self.dir_base])
        assert 0 <= at < stored
        self.m.blob[pos + at] ^= 0xFF
        self.flipped ^= {pos + at}
        self.hurt.add(value)
        return ok(pos=pos + at)

    def corrupt_unlisted(self, value, at, keep):
        """``corrupt`` of a chunk that none of the streams ``keep`` names, so a ``scrub(keep=keep)`` does not report it"""
        assert all(value not in self._get(n).refs for n in keep), value
        return self.corrupt(value, at)

    def scrub(self, keep=None):
        live = None if keep is None else self._mark(keep)[0]
        held = SM.digests_by_value((c, v) for c, v in self.m.values.items())       # in a Model the digest of a chunk is its content
        status = SM.statuses(self.m.blob, self.store_bytes, self.m.directory, self.dir_base, live, held, self.m.decode(), lambda piece: piece)
        damaged = [self.dir_base + int(i) for i in np.nonzero((status >= 1) & (status <= 3))[0]]
        self.last_scrub = damaged
        return ok(status=status, damaged=damaged)

    def affected(self, names, status):
        flag = ((status >= 1) & (status <= 3)).astype(np.uint32)
        streams = self.account(names, flag)["streams"]
        return ok(affected=[(i, int(a["flagged_positions"]), int(a["flagged_bytes"])) for i, a in enumerate(streams) if a["flagged_positions"] > 0])

    @_folds
    def repair_from(self, peer: "Store", damaged):
        by_value = {v: c for c, v in self.m.values.items()}
        out = dict(repaired=[], unavailable=[], no_digest=[])
        want = []
        for v in sorted(set(damaged)):
            if v not in by_value:
                out["no_digest"].append(v)
                continue
            there = peer.m.values.get(by_value[v])
            idx = None if there is None else there - peer.dir_base
            here = int(self.m.directory[v - self.dir_base]["raw"]) & RM.LEN_MASK
            fits = idx is not None and 0 <= idx < peer.dir_entries and GM.sound(peer.m.directory[idx], peer.store_bytes) and \
                (not 1 <= here <= 65536 or here == int(peer.m.directory[idx]["raw"]) & RM.LEN_MASK)
            if fits:
                status, piece = RM.restore(peer.m.blob, peer.store_bytes, peer.m.directory, peer.dir_base, [there], [0, len(by_value[v])],
                                           len(by_value[v]), peer.m.decode())[0]
                fits = status == 0 and piece == by_value[v]
            (want if fits else out["unavailable"]).append((v, there) if fits else v)
        if not want:
            return ok(**out)
        verdict, _, payload, locs = RP.export_chunks(peer.m.blob, peer.store_bytes, peer.m.directory, peer.dir_base, [t for _, t in want], 1 << 62)
        assert verdict == 0
        if self.used + len(payload) > self.store_bytes:
            return dict(code=-5, needed=len(payload))
        verdict, _, blob, entries = SM.replace_chunks(payload, len(payload), locs, [v for v, _ in want], self.used, self.store_bytes, self.m.directory,
                                                      self.dir_base)
        assert verdict == 0
        self.m.blob += blob
        for idx, e in entries.items():
            self.m.directory[idx] = e
        out["repaired"] = [v for v, _ in want]
        self.hurt -= set(out["repaired"])
        return ok(**out)

    # ---- bundles ----------------------------------------------------------------------------------------------------------------
    def replicate_to(self, other: "Store", names, as_names, negotiate=True):
        try:
            return self._replicate_to(other, names, as_names, negotiate)
        finally:
            other._fold()                                                  # import_bundle appends on the receiving store

    def _replicate_to(self, other: "Store", names, as_names, negotiate):
        recipes = [self._get(n).refs for n in names]
        bundle = RP.export_bundle(self.m, recipes, other.m.values if negotiate else None)
        lacks = [k for k, d in enumerate(bundle["digests"]) if d not in other.m.values]
        n = len(bundle["values"])
        if len(other.m.values) + len(lacks) > other.max_entries:
            return dict(code=-5, why="index")
        if n and other.base + n > other.dir_base + other.dir_entries:
            return dict(code=-5, why="directory")
        if other.used + sum(int(bundle["locs"][k]["stored"]) for k in lacks) > other.store_bytes:
            return dict(code=-5, why="store")
        out, new = RP.import_bundle(other.m, bundle, other.base, recipes)
        other.base += n
        for name, as_name, refs in zip(names, as_names, out):
            other._make(as_name, self._get(name).bytes, refs, self._get(name).cuts)
        return ok(carried=len(bundle["carried"]), listed=n, new=len(new))


def run(stores: dict, op: str, args: dict):
    """One step on the model: the stores by name, the step's arguments by keyword (``store`` defaults to "P")."""
    args = dict(args)
    s = stores[args.pop("store", "P")]
    if op in ("save_load", "restore_many_stream"):                       # the model has no file and one restore
        return ok(bytes=[s.restore(n)["bytes"] for n in args.get("names", [])])
    if op == "replicate_to":
        return s.replicate_to(stores[args.pop("to")], **args)
    if op == "repair_from":
        return s.repair_from(stores[args.pop("peer")], s.scrub()["damaged"])
    if op == "repair_local":                                             # of the store's last scrub, which may have had a ``keep``
        return s.repair_local(s.last_scrub, **args)
    if op == "affected":
        return s.affected(args["names"], s.scrub()["status"])
    if op == "delta_round_trip":
        d = s.diff(args["old"], args["new"])
        return dict(d, plain=DM.apply(s._get(args["old"]).bytes, d["payload"], d["ops"]),
                    inside=s.apply_delta(args["old"], args["dst"], d["ops"], d["payload"]))
    return getattr(s, op)(**args)


# ---- the scripts -----------------------------------------------------------------------------------------------------------------
def noise(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def alice():
    with open(os.path.join(GOLDEN, "alice29.txt"), "rb") as f:
        return f.read()


ROOMY = dict(store_bytes=1 << 20, dir_entries=640, dir_base=7, max_entries=1 << 12)


class Script:
    """A script while it is built: the steps, and the model they have run on so far."""

    def __init__(self, name, oracle, alg, **specs):
        self.name, self.specs, self.steps, self.notes = name, specs or dict(P=ROOMY), [], {}
        self.stores = new_stores(oracle, alg, self.specs)

    def do(self, op, expect=0, **args):
        got = run(self.stores, op, args)
        assert got["code"] == expect, (self.name, len(self.steps), op, got["code"], got.get("why"), expect)
        self.steps.append((op, dict(args), expect))
        return got

    def note(self, key, value=None):
        """what the step just added has to reach: checked by the model test"""
        self.notes.setdefault(key, []).append((len(self.steps) - 1, value))

    def done(self):
        return dict(name=self.name, specs=self.specs, steps=self.steps, notes=self.notes)


def new_stores(oracle, alg, specs):
    return {n: Store(oracle, alg, **kw) for n, kw in specs.items()}


def _edit_after_compact(O, alg):
    s = Script("edit_after_compact", O, alg)
    a = alice()[:30000] + noise(1, 10000)
    ed = dict(a=20000, r=100, ins=noise(2, 3000))
    s.do("ingest", name="A", data=a)
    first = s.do("patch", src="A", dst="B", **ed)
    gone = s.do("compact", keep=["A"])
    s.note("dropped", (gone["dropped_contents"], first["new_chunks"]))
    again = s.do("patch", src="A", dst="B", **ed)
    s.note("rebuilt", again["new_chunks"])
    s.do("compose", dst="C", parts=[("A", 1000, 15000), noise(3, 2000), ("B", 18000, 10000), b"tail" * 50])
    s.do("scrub")
    s.do("account", names=["A", "B", "C"])
    s.do("restore_many_stream", names=["A", "B", "C"])
    return s.done()


def _edit_after_renumber(O, alg):
    s = Script("edit_after_renumber", O, alg)
    a, b = alice()[40000:65000] + noise(4, 8000), noise(5, 20000) + alice()[70000:80000]
    s.do("ingest", name="A", data=a)
    s.do("ingest", name="S", data=b)
    s.do("patch", src="A", dst="A2", a=12000, r=300, ins=noise(6, 1500))
    # holes: whole chunks of S inserted at a cut of A2 are chunked as they were in S, so the window is all duplicates
    S, A2 = s.stores["P"].streams["S"], s.stores["P"].streams["A2"]
    dup = s.do("patch", src="A2", dst="A3", a=A2.cuts[40], r=0, ins=S.bytes[S.cuts[5]:S.cuts[9]])
    assert dup["new_chunks"] == 0 and dup["t"] == 4 and s.stores["P"].holes() >= 4
    nxt = dict(a=5000, r=50, ins=noise(7, 700))
    t = s.do("patch", src="A3", dst="A4", dry=True, **nxt)["t"]
    s.steps.pop()                                                          # (the dry run only sized the directory)
    K = s.stores["P"].stored_chunks()
    s.do("renumber", keep=["A3", "S"], dir_entries=K + t, dir_base=5000)
    s.note("room", t)
    for stale in ("A", "A2"):
        s.do("patch", expect=-2, src=stale, dst="X", **nxt)
        s.do("compose", expect=-2, dst="X", parts=[(stale, 100, 9000), b"new"])
        s.do("read_ranges", expect=-2, name=stale, ranges=[(10, 500)])
        s.do("restore", expect=-2, name=stale)
    s.do("patch", src="A3", dst="A4", **nxt)
    s.note("full")
    last = dict(src="A4", dst="A5", a=20000, r=0, ins=noise(8, 40))
    s.do("patch", expect=-5, **last)
    s.note("refused", "directory")
    s.do("renumber", keep=["A3", "A4", "S"], dir_entries=K + t + 64)
    s.do("patch", **last)
    s.do("account", names=["A3", "A4", "A5", "S"])
    return s.done()


def _refused_ingest(O, alg, many: bool):
    name = "refused_ingest_then_on[%s]" % ("ingest_many" if many else "ingest")
    probe = Store(O, alg, **ROOMY)
    s0 = alice()[:16000] + noise(10, 4000)
    probe.ingest("S0", s0)
    used0, x = probe.used, noise(11, 24000)                                # noise is stored raw: X takes 24000 bytes
    xc = CM.chunk(x, P)
    tight = dict(ROOMY, store_bytes=used0 + 16000)
    s = Script(name, O, alg, a=ROOMY, b=tight, c=tight)

    def put(store, names, datas, expect=0):
        if many:
            return s.do("ingest_many", expect, store=store, names=names, datas=datas)
        return s.do("ingest", expect, store=store, name=names[0], data=b"".join(datas))

    half = xc[len(xc) // 2]
    split = lambda d, at: [d[:at], d[at:]] if many else [d]  # noqa: E731
    # (a) a directory that is exactly full
    put("a", ["S0"], [s0])
    K = s.stores["a"].stored_chunks()
    s.do("renumber", store="a", keep=["S0"], dir_entries=K)
    s.note("full")
    put("a", ["X", "X2"], split(x, 9000), expect=-5)
    s.note("refused", "directory")
    s.do("renumber", store="a", keep=["S0"], dir_entries=K + 4 * len(xc))
    put("a", ["X", "X2"], split(x, 9000))
    put("a", ["Y", "Y2"], split(x[:half] + noise(12, 9000), 5000))         # about half of X's chunks
    # (b) refused for store bytes, then a prefix that fits, with nothing in between
    put("b", ["S0"], [s0])
    put("b", ["X", "X2"], split(x, 9000), expect=-5)
    s.note("refused", "store")
    put("b", ["Y", "Y2"], split(x[:half], 5000))
    # (c) refused for store bytes, a compact into a larger store, then the same again
    put("c", ["S0"], [s0])
    put("c", ["X", "X2"], split(x, 9000), expect=-5)
    s.note("refused", "store")
    s.do("compact", store="c", keep=["S0"], store_bytes=used0 + 40000)
    put("c", ["X", "X2"], split(x, 9000))
    for st in "abc":
        s.do("scrub", store=st)
    return s.done()


def _duplicates(O, alg):
    s = Script("duplicates", O, alg)
    block = noise(20, 3000)
    d = alice()[:6000] + block * 5 + bytes(14000) + alice()[90000:98000]
    s.do("ingest", name="D", data=d)
    D = s.stores["P"].streams["D"]
    zero = bytes(P["max"])
    run_ = [i for i, c in enumerate(D.chunks()) if c == zero]
    assert len(run_) >= 4 and len(set(D.refs)) < len(D.refs)
    s.do("account", names=["D"])
    got = s.do("patch", src="D", dst="D2", a=D.cuts[run_[1]], r=0, ins=zero * 3)
    s.note("all_duplicates", 3)
    assert got["t"] == 3 and got["new_chunks"] == 0
    s.do("patch", src="D2", dst="D3", a=6000 + 3000, r=0, ins=block)       # one more repetition, inside the repeated block
    s.do("account", names=["D", "D2", "D3"])
    s.do("renumber", keep=["D", "D2", "D3"])
    s.note("renumbered")
    s.do("account", names=["D", "D2", "D3"])
    s.do("edit", src="D3", dst="D4", edits=[(100, 10, b"x" * 10), (20000, 0, zero)])
    s.do("scrub")
    return s.done()


def _peers(O, alg):
    s = Script("peers", O, alg, P=ROOMY, Q=dict(ROOMY, dir_base=1000))
    a = alice()[100000:125000] + noise(30, 9000)
    s.do("ingest", name="A", data=a)
    s.do("replicate_to", to="Q", names=["A"], as_names=["A"])
    edits = [(300, 40, noise(31, 900)), (9000, 0, b"inserted " * 30), (20000, 2500, b""), (len(a), 0, noise(32, 1200))]
    s.do("edit", store="Q", src="A", dst="B", edits=edits)
    s.note("edits", edits)
    back = s.do("replicate_to", store="Q", to="P", names=["B"], as_names=["B"])
    s.note("negotiated", (back["carried"], back["listed"]))
    s.do("diff", old="A", new="B")
    s.do("delta_round_trip", old="A", new="B", dst="B2")
    s.do("account", names=["A", "B", "B2"])
    s.do("scrub", store="Q")
    return s.done()


def _repair_then_edit(O, alg):
    s = Script("repair_then_edit", O, alg, P=ROOMY, Q=dict(ROOMY, dir_base=300))
    a = alice()[20000:38000] + b"lorem ipsum dolor sit amet " * 150 + noise(40, 12000)
    s.do("ingest", name="A", data=a)
    s.do("replicate_to", to="Q", names=["A"], as_names=["A"], negotiate=False)
    Pm, A = s.stores["P"], s.stores["P"].streams["A"]
    is_raw = lambda v: bool(int(Pm.m.directory[v - Pm.dir_base]["raw"]) & RM.RAW)  # noqa: E731
    first = lambda want: next(j for j in range(20, len(A.refs)) if is_raw(A.refs[j]) == want and A.refs.index(A.refs[j]) == j)  # noqa: E731
    jc, jr = first(False), first(True)
    for j in (jc, jr):
        stored = int(Pm.m.directory[A.refs[j] - Pm.dir_base]["stored"])
        s.do("corrupt", value=A.refs[j], at=stored // 2)
    s.do("scrub")
    s.note("damaged", sorted((A.refs[jc], A.refs[jr])))
    s.do("affected", names=["A"])
    s.note("affected", 2)
    s.do("repair_from", peer="Q")
    s.do("scrub")
    s.note("clean")
    for n, j in (("A2", jc), ("A3", jr)):                                  # the window begins with the replaced chunk
        s.do("patch", src="A", dst=n, a=A.cuts[j] + 5, r=3, ins=noise(41 + j, 200))
        s.note("window_reads", (A.cuts[j], A.cuts[j + 1]))
    s.do("compact", keep=["A", "A2", "A3"])
    s.do("renumber", keep=["A", "A2", "A3"])
    s.do("scrub")
    s.do("account", names=["A", "A2", "A3"])
    return s.done()


def _streamed_and_reloaded(O, alg):
    s = Script("streamed_and_reloaded", O, alg)
    a = alice()[5000:30000] + bytes(5000) + noise(50, 12000)
    piece = next(pc for pc in range(6001, 6400, 7) if cut_in_carry(a, pc))
    s.do("ingest_stream", name="A", data=a, piece=piece)
    s.note("cut_in_carry", piece)
    three = [noise(51, 9000) + a[1000:4000], alice()[60000:72000], a[20000:33000]]
    s.do("ingest_many_stream", names=["S1", "S2", "S3"], datas=three, piece=7001)
    s.do("patch", src="A", dst="A2", a=15000, r=700, ins=noise(52, 2500))
    s.do("save_load", names=["A", "A2", "S1", "S2", "S3"])
    got = s.do("compose", dst="C", parts=[("A2", 2000, 20000), noise(53, 1500), ("S2", 500, 9000), ("S1", 0, 4000)])
    cuts, kept = got["cuts"], got["kept"]
    edges = [x for i, x in enumerate(cuts[1:-1], 1) if (cuts[i - 1] in kept) != (x in kept) and 300 <= x <= cuts[-1] - 301]
    assert len(edges) >= 3
    ranges = [r for x in edges for r in ((x - 1, 2), (x, 1), (x - 1, 1), (x + 1, 300), (x - 300, 299), (x - 300, 301))]
    s.do("read_ranges", name="C", ranges=ranges)
    s.note("edges", edges)
    s.do("compact", keep=["A2", "C", "S3"])
    s.do("renumber", keep=["A2", "C", "S3"])
    s.do("restore_many_stream", names=["A2", "C", "S3"])
    s.do("read_ranges", name="C", ranges=ranges)
    s.do("account", names=["A2", "C", "S3"])
    return s.done()


def cut_in_carry(data, piece) -> bool:
    """a piece of the streamed ingest whose first cut lies inside the carry in front of it"""
    r = SIM.chain([data], P, piece)
    return any(len(q["cuts"]) > 1 and q["cuts"][1] < carry for carry, q in zip(r.carries, r.log))


# ---- the guarded scripts ---------------------------------------------------------------------------------------------------------
S = G1.S                                                                   # 65536
GUARDED = dict(store_bytes=1 << 20, dir_entries=4096, dir_base=7, max_entries=1 << 13)
PARTIAL = ("ingest_stream", "ingest_many_stream")                          # a refusal of these may leave a prefix behind


def _fill(s, store, names, seed, G, n=60000):
    """Noise streams, stored raw, until ``used`` has passed G * S."""
    for k, name in enumerate(names):
        s.do("ingest", store=store, name=name, data=noise(seed + k, n))
    m = s.stores[store]
    assert m.used > G * S and m.used == n * len(names), (s.name, m.used)


def _extents(m):
    """(pos, stored, value) of every stored chunk, in ascending pos"""
    d = m.m.directory
    return sorted((int(d[i]["pos"]), int(d[i]["stored"]), m.dir_base + int(i)) for i in np.nonzero(RN.nonzero(d))[0])


def _chunk_at(ext, p):
    return next((v for pos, stored, v in ext if pos <= p < pos + stored), None)


def _kind(pos, stored, G, S=S):
    """where an extent lies: inside one stripe, across a stripe boundary inside a group, or across a group boundary"""
    if pos // (G * S) != (pos + stored - 1) // (G * S):
        return "group"
    return "stripe" if pos // S != (pos + stored - 1) // S else "inside"


def _pairs(m, G, kinds, S=S, spread=20000):
    """One pair (a, b, q) per kind: a of that kind, b the chunk over the column of a's first byte in the next member of a's group
    (in the one before it, from the last member), q that byte of b.  The pairs share no chunk, and the inside ones lie apart."""
    ext, out, taken, last = _extents(m), [], set(), -spread
    for kind in kinds:
        for pos, stored, a in ext:
            q = pos + S if pos // S % G < G - 1 else pos - S
            b = _chunk_at(ext, q) if 0 <= q < m.used else None
            if _kind(pos, stored, G, S) != kind or b is None or {a, b} & taken or a == b or (kind == "inside" and pos < last + spread):
                continue
            out.append((a, b, q))
            taken |= {a, b}
            last = pos if kind == "inside" else last
            break
        else:
            raise AssertionError(f"no {kind} pair in the built store")
    return out


def _owner(m, value):
    """(stream, position) of a live recipe that names the value"""
    return next((n, st.refs.index(value)) for n, st in sorted(m.streams.items()) if value in st.refs)


def _damage(s, store, pairs):
    """a's middle byte and b's byte over the column of a's first one, of every pair"""
    m = s.stores[store]
    for a, b, q in pairs:
        pa, na = (int(v) for v in m.m.directory[a - m.dir_base][["pos", "stored"]])
        s.do("corrupt", store=store, value=a, at=na // 2)
        s.do("corrupt", store=store, value=b, at=q - int(m.m.directory[b - m.dir_base]["pos"]))
    return sorted(v for a, b, _ in pairs for v in (a, b))


def _scrub_and_repair(s, store, victims, keep=None):
    s.do("scrub", store=store, keep=keep)
    s.note("reports", victims)
    return s.do("repair_local", store=store)


def _guarded_pairs(O, alg):
    G = 2
    s = Script("guarded_pairs", O, alg, P=dict(GUARDED, store_bytes=5 * G * S))
    s.do("protect", stripe=S, group=G, parity=2)
    names = ["N0", "N1", "N2", "N3", "N4"]
    _fill(s, "P", names, 100, G)
    m = s.stores["P"]
    pairs = _pairs(m, G, ["stripe", "group", "inside", "inside", "inside"])
    assert len(pairs) >= 4 and len({v for a, b, _ in pairs for v in (a, b)}) == 2 * len(pairs)
    victims = _damage(s, "P", pairs)
    _scrub_and_repair(s, "P", victims)
    s.note("all_paired", len(pairs))
    s.do("scrub")
    s.note("clean")
    s.do("guard_check")
    name, j = _owner(m, pairs[0][0])                                       # the window begins with a repaired chunk
    st = m.streams[name]
    s.do("patch", src=name, dst="E", a=st.cuts[j] + 5, r=3, ins=noise(110, 200))
    s.note("window_reads", (st.cuts[j], st.cuts[j + 1]))
    before = m.guard.state()[:3] + (len(m.guard.P),)
    s.do("compact", keep=names[1:] + ["E"], store_bytes=1 << 20)           # N0 goes: every kept byte moves, into 8 groups
    s.note("fresh_guard", before)
    for keep in (None, names[1:] + ["E"]):
        if keep:
            s.do("renumber", keep=keep, dir_base=3000)
        again = _pairs(m, G, ["inside", "group"] if keep else ["stripe", "inside"])
        victims = _damage(s, "P", again)
        _scrub_and_repair(s, "P", victims)
        s.note("all_paired", len(again))
        s.do("scrub")
        s.note("clean")
    s.do("restore_many_stream", names=names[1:] + ["E"])
    return s.done()


def _guarded_triple(O, alg):
    G = 3
    s = Script("guarded_triple", O, alg, P=GUARDED, Q=dict(GUARDED, dir_base=1000))
    s.do("protect", stripe=S, group=G, parity=2)
    s.do("protect", store="Q")                                             # the peer under ChunkStore.protect()'s own geometry
    names = ["N0", "N1", "N2", "N3"]
    _fill(s, "P", names, 200, G)
    s.do("replicate_to", to="Q", names=names, as_names=names)
    m, W = s.stores["P"], G * S
    ext = _extents(m)
    a, three = next((v, [v, _chunk_at(ext, pos + S), _chunk_at(ext, pos + 2 * S)]) for pos, n, v in ext if pos > 3000 and _kind(pos, n, G) == "inside")
    assert len(set(three)) == 3 and None not in three
    pa = int(m.m.directory[a - m.dir_base]["pos"])
    alone = next(v for pos, n, v in ext if pos > W + 1000 and _kind(pos, n, G) == "inside")
    for k, v in enumerate(three):                                          # one column of group 0, in members 0, 1 and 2
        s.do("corrupt", value=v, at=pa + k * S - int(m.m.directory[v - m.dir_base]["pos"]))
    s.do("corrupt", value=alone, at=0)
    s.do("scrub")
    s.note("reports", sorted(three + [alone]))
    s.do("repair_local")
    s.note("repair", dict(repaired=[alone], collided=sorted(three), unprotected=[], failed=[], no_digest=[], paired=0))
    s.do("scrub")
    s.note("reports", sorted(three))
    s.do("repair_from", peer="Q")
    s.do("scrub")
    s.note("clean")
    s.do("guard_check")                                                    # the old bytes stay, damaged, until a compact
    s.note("guard_check", dict(count=1, groups=[0], bits=[3]))
    s.do("compact", keep=names)
    s.do("guard_check")
    s.note("guard_check", dict(count=0, groups=[], bits=[]))
    s.do("restore_many_stream", names=names)
    return s.done()


def _guard_is_damaged(O, alg):
    G = 2
    s = Script("guard_is_damaged", O, alg, A=GUARDED, B=dict(GUARDED, dir_base=500))
    names = ["N0", "N1", "N2"]
    for store, parity in (("A", 1), ("B", 2)):
        s.do("protect", store=store, stripe=S, group=G, parity=parity)
        _fill(s, store, names, 300, G)
        m = s.stores[store]
        (a, b, q), = _pairs(m, G, ["inside"])
        pa, na = (int(v) for v in m.m.directory[a - m.dir_base][["pos", "stored"]])
        assert pa + na <= S and q == pa + S
        column = pa + 1                                                    # group 0: the guard byte of a's second byte
        # 1. a alone, and a P byte of its column
        s.do("corrupt", store=store, value=a, at=na // 2)
        s.do("corrupt_guard", store=store, which=0, at=column)
        _scrub_and_repair(s, store, [a])
        s.note("repair", dict(repaired=[], collided=[], unprotected=[], failed=[a], no_digest=[], paired=0))
        s.note("nothing_changed")
        s.do("guard_check", store=store)
        s.note("guard_check", dict(count=1, groups=[0], bits=[1 if parity == 1 else 3]))
        s.do("corrupt_guard", store=store, which=0, at=column)             # the guard byte put back: now it rebuilds
        got = s.do("repair_local", store=store)
        assert got["repaired"] == [a]
        # 2. a pair, and a Q byte of the column where it meets
        if parity == 2:
            victims = _damage(s, store, [(a, b, q)])
            s.do("corrupt_guard", store=store, which=1, at=q % S)
            got = _scrub_and_repair(s, store, victims)
            s.note("some_failed", victims)
            if len(got["failed"]) == 2:
                s.note("nothing_changed")
            s.do("corrupt_guard", store=store, which=1, at=q % S)
            s.do("scrub", store=store)
            s.do("repair_local", store=store)
            s.do("scrub", store=store)
            s.note("clean")
        # 3. a, and a chunk of its column that the scrub was not asked about: N1 is not kept
        assert _owner(m, a)[0] == "N0" and _owner(m, b)[0] == "N1"
        s.do("corrupt", store=store, value=a, at=na // 2)
        s.do("corrupt_unlisted", store=store, value=b, at=q - int(m.m.directory[b - m.dir_base]["pos"]), keep=["N0", "N2"])
        _scrub_and_repair(s, store, [a], keep=["N0", "N2"])
        s.note("repair", dict(repaired=[], collided=[], unprotected=[], failed=[a], no_digest=[], paired=0))
        s.note("nothing_changed")
        _scrub_and_repair(s, store, sorted([a, b]))                         # a whole scrub names both: two in one column
        s.note("repair", dict(repaired=[a, b], collided=[], unprotected=[], failed=[], no_digest=[], paired=2) if parity == 2 else
               dict(repaired=[], collided=sorted([a, b]), unprotected=[], failed=[], no_digest=[], paired=0))
    return s.done()


def _protect_over_damage(O, alg):
    G = 2
    s = Script("protect_over_damage", O, alg, P=GUARDED, Q=dict(GUARDED, dir_base=1000))
    names = ["N0", "N1", "N2"]
    _fill(s, "P", names, 400, G)
    s.do("replicate_to", to="Q", names=names, as_names=names)
    s.do("protect", stripe=S, group=G, parity=1)                            # late, on a store that is not empty
    m = s.stores["P"]
    pair, = _pairs(m, G, ["inside"])
    victims = _damage(s, "P", [pair])
    _scrub_and_repair(s, "P", victims)
    s.note("repair", dict(repaired=[], collided=victims, unprotected=[], failed=[], no_digest=[], paired=0))
    s.do("protect", stripe=S, group=G, parity=2)                            # over the damage: the new guards hold it
    s.do("guard_check")
    s.note("guard_check", dict(count=0, groups=[], bits=[]))
    _scrub_and_repair(s, "P", victims)
    s.note("repair", dict(repaired=[], collided=[], unprotected=[], failed=victims, no_digest=[], paired=2))
    s.note("nothing_changed")
    s.do("repair_from", peer="Q")
    s.do("scrub")
    s.note("clean")
    s.do("protect", stripe=1 << 17, group=G, parity=2)                      # a second geometry
    s.do("ingest", name="N3", data=noise(410, 60000))
    pair, = _pairs(m, G, ["inside"], S=1 << 17)
    victims = _damage(s, "P", [pair])
    _scrub_and_repair(s, "P", victims)
    s.note("repair", dict(repaired=victims, collided=[], unprotected=[], failed=[], no_digest=[], paired=2))
    s.do("scrub")
    s.note("clean")
    s.do("restore_many_stream", names=names + ["N3"])
    return s.done()


def _guarded_refusals(O, alg):
    G = 2
    names = ["N0", "N1", "N2"]
    small, large = dict(a=20000, r=1, ins=b"x"), dict(a=30000, r=0, ins=noise(510, 4000))
    parts = lambda n: [("N0", 100, 3000), noise(511, n), ("N1", 200, 2500)]  # noqa: E731

    def probe():                                                            # a store with all the room, to count on
        m = Store(O, alg, **GUARDED)
        for k, name in enumerate(names):
            m.ingest(name, noise(500 + k, 60000))
        return m
    K, used = probe().stored_chunks(), probe().used
    t = [probe().patch("N0", "X", dry=True, **kw)["t"] for kw in (small, large)] + [probe().compose("X", parts(n))["rebuilt_chunks"] for n in (10, 4000)]
    few, many = max(t[0], t[2]), min(t[1], t[3])                            # the window chunks of the small calls and of the large ones
    assert few < many and K == len(probe().m.values), t
    tight = dict(GUARDED, store_bytes=used + 50000)
    s = Script("guarded_refusals", O, alg, D=dict(GUARDED, max_entries=K + few), T=tight)
    # D: the directory, then the index
    s.do("protect", store="D", stripe=S, group=G, parity=1)
    _fill(s, "D", names, 500, G)
    s.do("renumber", store="D", keep=names, dir_entries=K)
    s.note("full")
    s.do("patch", expect=-5, store="D", src="N0", dst="X", **small)
    s.note("refused", "directory")
    s.do("compose", expect=-5, store="D", dst="X", parts=parts(10))
    s.note("refused", "directory")
    s.do("renumber", store="D", keep=names, dir_entries=K + 64)
    s.do("patch", expect=-5, store="D", src="N0", dst="X", **large)
    s.note("refused", "index")
    s.do("compose", expect=-5, store="D", dst="X", parts=parts(4000))
    s.note("refused", "index")
    s.do("patch", store="D", src="N0", dst="X", **small)
    s.do("guard_check", store="D")
    # T: the store's bytes, one-shot and part-way
    s.do("protect", store="T", stripe=S, group=G, parity=2)
    _fill(s, "T", names, 500, G)
    s.do("ingest", expect=-5, store="T", name="Y", data=noise(520, 55000))
    s.note("refused", "store")
    got = s.do("ingest_stream", expect=-5, store="T", name="Y", data=noise(521, 60000), piece=7001)
    s.note("part_way", got["run"].consumed)
    got = s.do("ingest_many_stream", expect=-5, store="T", names=["Z0", "Z1", "Z2"], datas=[noise(522 + k, n) for k, n in enumerate((1200, 5000, 2500))], piece=2100)
    assert got["run"].recipes()[1] is not None, "no stream was cut"
    s.note("part_way", got["run"].consumed)
    s.do("guard_check", store="T")
    m = s.stores["T"]
    pair, = _pairs(m, G, ["inside"])
    victims = _damage(s, "T", [pair])
    s.do("save_load", store="T", names=[])                                  # a snapshot of a damaged store
    _scrub_and_repair(s, "T", victims)                                       # in the loaded store, from the loaded guards
    s.note("repair", dict(repaired=victims, collided=[], unprotected=[], failed=[], no_digest=[], paired=2))
    s.do("scrub", store="T")
    s.note("clean")
    s.do("restore_many_stream", store="T", names=names + ["Y", "Z0", "Z1"])
    return s.done()


BUILDERS = (_edit_after_compact,_edit_after_renumber, lambda O, alg: _refused_ingest(O, alg, False), lambda O, alg: _refused_ingest(O, alg, True),
            _duplicates, _peers, _repair_then_edit, _streamed_and_reloaded, _guarded_pairs, _guarded_triple, _guard_is_damaged, _protect_over_damage,
            _guarded_refusals)
NAMES = ("edit_after_compact", "edit_after_renumber", "refused_ingest_then_on[ingest]", "refused_ingest_then_on[ingest_many]", "duplicates", "peers",
         "repair_then_edit", "streamed_and_reloaded", "guarded_pairs", "guarded_triple", "guard_is_damaged", "protect_over_damage",
         "guarded_refusals")
UNGUARDED = NAMES[:8]                                                      # these run once more under ``protected``
_BUILT = {}


def script(oracle, alg, name):
    """One script for one codec (stored sizes differ between the codecs, and so do the store sizes that refuse), built once."""
    if (alg, name) not in _BUILT:
        _BUILT[alg, name] = BUILDERS[NAMES.index(name)](oracle, alg)
    return _BUILT[alg, name]


def scripts(oracle, alg):
    return [script(oracle, alg, name) for name in NAMES]


FLAVOUR = dict(lz4=dict(stripe=65536, group=3, parity=1), lzf=dict(stripe=65536, group=2, parity=2))


def protected(sc, alg):
    """The script with ``protect`` as the first step on every store, one flavour per codec; the notes move with their steps."""
    first = [("protect", dict(store=n, **FLAVOUR[alg]), 0) for n in sc["specs"]]
    notes = {key: [(i + len(first), value) for i, value in hits] for key, hits in sc["notes"].items()}
    return dict(name=sc["name"] + "+guard", specs=sc["specs"], steps=first + sc["steps"], notes=notes)
