"""cw_dev_cdc_streams_part, cw_dev_ingest_commit_streams and cw_store_ingest_streams in plain Python.

``chunk_part`` is the chunker with an open last stream: the complete streams by streams_model.chunk_streams, the open one by
cdc_model.chunk(final=False).  ``pieces`` is the piecewise loop: the concatenation goes through in pieces of ``piece`` fresh bytes
(raised to max_size) plus the carry; each piece takes the stream ends not yet taken that lie at or before its end, and when the last
of them is not the piece's end its own length is one more end and its last stream stays open.  ``chain`` commits the pieces into one
recipe with its stream index (``commit_streams``); ``ingest_streams`` does the same into a restore_model.Model with ingest_model's
admission, so a refused piece ends the run and leaves everything as the pieces before it left it."""
from __future__ import annotations

import cdc_model as CM
import ingest_model as IM
import restore_model as RM
import streams_model as SM


def chunk_part(part: bytes, ends, final: bool, p: dict):
    """(offsets[0..K], first[0..nstreams]) of one piece whose streams end at ``ends`` (the last = len(part))."""
    assert list(ends) == sorted(ends) and (not ends or ends[-1] == len(part))
    streams = [part[a:b] for a, b in zip([0] + list(ends[:-1]), ends)]
    if final:
        return SM.chunk_streams(streams, p)
    offsets, first = SM.chunk_streams(streams[:-1], p)
    s = ends[-2] if len(ends) > 1 else 0
    first[-1] = len(offsets) - 1                      # the open stream's first chunk: K when nothing of it is consumed
    offsets += [s + c for c in CM.chunk(part[s:], p, final=False)[1:]]
    return offsets, first + [len(offsets) - 1]


def pieces(streams, p: dict, piece: int):
    """The pieces of a run, one dict each: the piece's bytes, its rebased ends, final, its cuts and stream index, and the arguments
    of its commit (origin, first_stream, skip_first)."""
    data = b"".join(bytes(s) for s in streams)
    gends, total, P = SM.ends_of(streams), sum(len(s) for s in streams), IM.piece_bytes(p, piece)
    done, taken, open_ = 0, 0, False
    for i in range((total + P - 1) // P):
        end = min(total, (i + 1) * P)
        part, t = data[done:end], 0
        while taken + t < len(gends) and gends[taken + t] <= end:
            t += 1
        ends = [e - done for e in gends[taken:taken + t]]
        final = t > 0 and gends[taken + t - 1] == end
        if not final:
            ends.append(len(part))
        cuts, first = chunk_part(part, ends, final, p)
        yield dict(index=i, origin=done, end=end, carry=i * P - done, part=part, ends=ends, final=final, cuts=cuts, first=first, took=t,
                   first_stream=taken, skip_first=open_, open_consumed=None if final else cuts[-1] - (ends[-2] if len(ends) > 1 else 0))
        done, taken, open_ = done + cuts[-1], taken + t, not final
    assert done == total and taken == len(gends) and not open_ or total == 0


def commit_streams(ref, offsets, n, n_new, store_result, stream_off, rec_ref, rec_off, rec_count, rec_cap, stats, stream_first, nstreams_piece,
                   first_stream, skip_first, rec_first, first_cap):
    """cw_dev_ingest_commit_streams on lists: ingest_model.commit, verdict 3 when the piece's streams leave the stream index, and
    rec_first[first_stream + f] = rec_count + stream_first[f] for skip_first <= f < nstreams_piece.  Returns (verdict, rec_count)."""
    refused = (store_result is not None and store_result[0]) or rec_count + n + 1 > rec_cap
    if not refused and first_stream + nstreams_piece > first_cap:
        return 3, rec_count
    verdict, count = IM.commit(ref, offsets, n, n_new, store_result, stream_off, rec_ref, rec_off, rec_count, rec_cap, stats)
    if verdict == 0:
        for f in range(int(skip_first), nstreams_piece):
            rec_first[first_stream + f] = rec_count + stream_first[f]
    return verdict, count


class Run(IM.Run):
    """What one cw_store_ingest_streams call returns, plus what the tests assert about its pieces."""

    def __init__(self, nstreams):
        super().__init__()
        self.nstreams, self.first, self.streams_done, self.log = nstreams, [0] * (nstreams + 1), nstreams, []

    def finish(self, rec_first, taken, open_):
        """The host's part of the stream index: behind the entries the pieces wrote, the stream that was not begun (or the end) and
        the entry behind it."""
        written = taken + int(open_)
        self.first = rec_first[:written] + [self.nchunks] * (min(taken + 1, self.nstreams) + 1 - written)
        self.streams_done = taken

    def recipes(self):
        """Per complete stream (refs, cuts rebased to 0), and the recipe of the stream that was cut (or None)."""
        cut = lambda a, b: (self.refs[a:b], [c - self.offsets[a] for c in self.offsets[a:b + 1]]) if b > a else ([], [0])  # noqa: E731
        done = self.streams_done
        whole = [cut(a, b) for a, b in zip(self.first[:done], self.first[1:done + 1])]
        partial = cut(self.first[done], self.first[done + 1]) if done + 1 < len(self.first) and self.first[done + 1] > self.first[done] else None
        return whole, partial


def chain(streams, p: dict, piece: int) -> Run:
    """The pieces committed one after the other, with no store behind them: the cuts and the stream index of the whole run."""
    r = Run(len(streams))
    total = sum(len(s) for s in streams)
    if total == 0:
        return r
    cap = total // p["min"] + len(streams) + 1
    rec_ref, rec_off, rec_first, count, taken, open_ = [0] * cap, [0] * cap, [None] * (len(streams) + 1), 0, 0, False
    for q in pieces(streams, p, piece):
        k = len(q["cuts"]) - 1
        v, count = commit_streams([0] * k, q["cuts"], k, 0, None, q["origin"], rec_ref, rec_off, count, cap, [0] * 5, q["first"], len(q["ends"]),
                                  q["first_stream"], q["skip_first"], rec_first, len(streams) + 1)
        assert v == 0
        r.log.append(q)
        r.carries.append(q["carry"])
        taken, open_ = taken + q["took"], not q["final"]
    r.refs, r.offsets = rec_ref[:count], rec_off[:count + 1]
    r.finish(rec_first, taken, open_)
    return r


def ingest_streams(m: RM.Model, streams, p: dict, piece: int, base: int, max_entries=None) -> Run:
    """The streamed ingest of ``streams`` into the model ``m``: ingest_model.ingest's admission and statistics, per piece."""
    r = Run(len(streams))
    total = sum(len(s) for s in streams)
    if total == 0:
        return r
    cap = total // p["min"] + len(streams) + 1
    rec_ref, rec_off, rec_first, count, taken, open_, stats = [0] * cap, [0] * cap, [None] * (len(streams) + 1), 0, 0, False, [0] * 5
    for q in pieces(streams, p, piece):
        cuts = q["cuts"]
        k, consumed, base_k, used = len(cuts) - 1, cuts[-1], base + count, len(m.blob)
        if k and not (m.dir_base <= base_k and base_k + k <= m.dir_base + len(m.directory)):
            r.refused = "directory"
        elif used + consumed > m.store_bytes:
            r.refused = "store"
        elif max_entries is not None and len(m.values) + k > max_entries:
            r.refused = "index"
        if r.refused:
            break
        refs, new, verdict, stored = m.ingest(q["part"], cuts, base_k)
        assert verdict == 0, "an admitted append was refused"
        v, count = commit_streams(refs, cuts, k, len(new), [0, stored], q["origin"], rec_ref, rec_off, count, cap, stats, q["first"], len(q["ends"]),
                                  q["first_stream"], q["skip_first"], rec_first, len(streams) + 1)
        assert v == 0
        r.log.append(q)
        r.carries.append(q["carry"])
        r.pieces.append(dict(chunks=k, new=len(new), consumed=consumed, stored=stored, used_before=used,
                             inner_dups=sum(1 for j, v_ in enumerate(refs) if base_k <= v_ != base_k + j)))
        taken, open_ = taken + q["took"], not q["final"]
    r.refs, r.offsets = rec_ref[:count], rec_off[:count + 1]
    r.stats = dict(zip(("bytes", "chunks", "new_chunks", "stored_bytes", "pieces"), stats))
    r.finish(rec_first, taken, open_)
    return r
