"""What the pipelined ingest of many host streams costs on one GPU.

One warm-up, the median of --reps runs with the configurations alternating.

  cdc       cw_dev_cdc_streams over --gib GiB of cw_dev_gen_random data (cw_cdc_default_params(8192)) as one stream, as streams of 64 KiB
            and as streams of 4 KiB (device events).  With --parent-lib (the parent commit's libcwhc.so) each library runs in child
            processes of its own, alternating, through plain ctypes: the kernels gained a runtime branch, and the claim to check is that
            the difference lies inside the parent's own run-to-run spread.
  ingest    cw_store_ingest_streams over --gib GiB of the tiled corpus (tools/ingest_probe.py's: every chunk is new) in page-locked
            memory, LZ4, as one span, as 64 Ki-byte spans and as 4 Ki-byte spans, against cw_store_ingest of the same bytes; and, reported
            apart, as 64 KiB spans scattered in pageable memory (the staged gather: a host memcpy on the critical path).  Wall time of
            the C call alone, each run into a fresh index and an empty store.
  many      ChunkStore.ingest_many_stream of --files corpus slices of 4 to 64 KiB (LZ4, Skein-512, cw_cdc_default_params(1024)) against
            ingest_many and a loop of ingest_stream, and of --big-files slices against ingest_many alone (wall time with uploads).

Prints one JSON object and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(configs, reps, timer):
    times = {name: [] for name in configs}
    for fn in configs.values():
        timer(fn)
    for _ in range(reps):
        for name, fn in configs.items():
            times[name].append(timer(fn))
    return times


# ---- cdc: one library through plain ctypes (a child process per library and round) ---------------------------------------------------
class Params(C.Structure):
    _fields_ = [("min_size", C.c_uint32), ("normal_size", C.c_uint32), ("max_size", C.c_uint32), ("reserved", C.c_uint32),
                ("mask_s", C.c_uint64), ("mask_l", C.c_uint64), ("gear", C.c_void_p)]


def cdc_child(lib_path, n, reps):
    L = C.CDLL(lib_path)
    vp, sz = C.c_void_p, C.c_size_t
    L.cw_init.argtypes, L.cw_cdc_default_params.argtypes = [C.c_int], [vp, C.c_uint32]
    L.cw_dev_gen_random.argtypes = [C.c_uint64, C.c_uint64, sz, sz, vp, vp]
    L.cw_dev_cdc.argtypes = [vp, vp, sz, C.c_int, vp, sz, vp, vp]
    L.cw_dev_cdc_streams.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp]
    assert L.cw_init(0) == 0
    st = torch.cuda.current_stream().cuda_stream
    p = Params()
    L.cw_cdc_default_params(C.byref(p), 8192)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert L.cw_dev_gen_random(7, 0, n // 4096, 4096, src.data_ptr(), st) == 0
    z = lambda count: torch.zeros(count, dtype=torch.int64, device="cuda")  # noqa: E731
    shapes = {"one_stream": n, "streams_64k": 64 << 10, "streams_4k": 4 << 10}
    most = n // min(shapes.values())
    cap = n // p.min_size + most + 1
    offs, k, first, result = z(cap), z(1), z(most + 1), z(1)
    ends = {name: torch.arange(1, n // size + 1, dtype=torch.int64, device="cuda") * size for name, size in shapes.items()}
    torch.cuda.synchronize()

    def single():
        assert L.cw_dev_cdc(C.byref(p), src.data_ptr(), n, 1, offs.data_ptr(), cap, k.data_ptr(), st) == 0

    def streams(name):
        def run():
            e = ends[name]
            assert L.cw_dev_cdc_streams(C.byref(p), src.data_ptr(), n, e.data_ptr(), e.numel(), offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(),
                                        result.data_ptr(), st) == 0
        return run

    configs = {"dev_cdc": single}
    configs.update({name: streams(name) for name in shapes})
    t = alternate(configs, reps, event_ms)
    chunks = {}
    for name, fn in configs.items():
        fn()
        torch.cuda.synchronize()
        chunks[name] = int(k.item())
    print(json.dumps({"ms": t, "chunks": chunks}))


def probe_cdc(n, reps, rounds, parent_lib, res):
    import compute_war_amd as cw
    libs = {"new": cw.lib_path()}
    if parent_lib:
        libs = {"parent": parent_lib, "new": cw.lib_path()}
    runs = {who: {} for who in libs}
    for _ in range(rounds):
        for who, path in libs.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cdc-child", path, "--bytes", str(n), "--reps", str(reps)],
                                 capture_output=True, text=True, check=True, timeout=300).stdout
            got = json.loads(out.strip().splitlines()[-1])
            for name, v in got["ms"].items():
                runs[who].setdefault(name, []).append(statistics.median(v))
            res[f"cdc_{who}_chunks"] = got["chunks"]
    for who, per in runs.items():
        for name, v in per.items():
            res[f"cdc_{who}_{name}_ms"], res[f"cdc_{who}_{name}_ms_rounds"] = statistics.median(v), v
    if parent_lib:
        for name in runs["new"]:
            pv, nv = runs["parent"][name], runs["new"][name]
            res[f"cdc_{name}_new_minus_parent_ms"] = statistics.median(nv) - statistics.median(pv)
            res[f"cdc_{name}_parent_spread_ms"] = max(pv) - min(pv)
            res[f"cdc_{name}_inside_parent_spread"] = abs(statistics.median(nv) - statistics.median(pv)) <= max(pv) - min(pv)
        assert res["cdc_new_chunks"] == res["cdc_parent_chunks"]


# ---- ingest: cw_store_ingest_streams over the tiled corpus --------------------------------------------------------------------------
def probe_ingest(n, reps, res):
    import compute_war_amd as cw
    from tools.restore_probe import tiled_corpus
    L = cw.lib()
    p = cw.CdcParams.default(8192)
    seg = 1 << 20
    nseg = n // seg
    h_src = L.cw_host_alloc(n)
    assert h_src
    src = torch.from_numpy(np.ctypeslib.as_array(C.cast(h_src, C.POINTER(C.c_uint8)), shape=(n,)))
    dev = tiled_corpus(n).view(nseg, seg)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    dev.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    src.copy_(dev.view(-1))
    torch.cuda.synchronize()
    del dev, stamps
    torch.cuda.empty_cache()
    # the same bytes as 64 KiB spans 64 bytes apart in pageable memory
    span, gap = 64 << 10, 64
    pageable = np.empty(n + (n // span) * gap, np.uint8)
    pageable.reshape(n // span, span + gap)[:, :span] = src.numpy().reshape(n // span, span)

    shapes = {"one_span": n, "spans_64k": 64 << 10, "spans_4k": 4 << 10}
    most = n // min(shapes.values())
    cap = p.max_offsets_streams(n, most)
    z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")  # noqa: E731
    store, used, directory = torch.empty(n, dtype=torch.uint8, device="cuda"), z(1, torch.int64), z(2 * cap, torch.int64)
    triple = cw.Store(store.data_ptr(), n, used.data_ptr(), directory.data_ptr(), 0, cap)
    refs, offs, first = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(most + 1, np.uint64)
    spans = {}
    for name, size in shapes.items():
        count = n // size
        spans[name] = (np.arange(count, dtype=np.uint64) * np.uint64(size) + np.uint64(h_src), np.full(count, size, np.uint64))
    spans["pageable_64k"] = (np.arange(n // span, dtype=np.uint64) * np.uint64(span + gap) + np.uint64(pageable.ctypes.data),
                             np.full(n // span, span, np.uint64))
    state = {}

    def fresh():
        if state.get("idx"):
            state["idx"].close()
        state["idx"] = cw.DedupeIndex("skein512", 1 << 22)
        used.zero_()
        directory.zero_()
        torch.cuda.synchronize()

    def one():
        fresh()
        t = time.perf_counter()
        rc, r, c, consumed, stats = cw.store_ingest(state["idx"], p, "lz4", triple, h_src, n, 0)
        state["ms"] = (time.perf_counter() - t) * 1e3
        assert rc == 0 and consumed == n
        state["one_chunks"] = len(r)

    def many(name):
        ptrs, lens = spans[name]

        def run():
            fresh()
            k, consumed, done, stats = C.c_size_t(0), C.c_uint64(0), C.c_size_t(0), cw.IngestStats()
            t = time.perf_counter()
            rc = L.cw_store_ingest_streams(state["idx"]._x(), C.byref(p), 0, C.byref(triple), ptrs.ctypes.data, lens.ctypes.data, len(lens), 0,
                                           refs.ctypes.data, offs.ctypes.data, cap, first.ctypes.data, C.byref(k), C.byref(consumed), C.byref(done),
                                           C.byref(stats))
            state["ms"] = (time.perf_counter() - t) * 1e3
            assert rc == 0 and consumed.value == n and done.value == len(lens), (rc, L.cw_last_error())
            state[name + "_chunks"] = int(k.value)
        return run

    def timed(fn):   # the call times itself: the fresh index and the emptied store are no part of it
        fn()
        return state["ms"]

    configs = {"store_ingest": one}
    configs.update({name: many(name) for name in spans})
    t = alternate(configs, reps, timed)
    assert state["one_span_chunks"] == state["one_chunks"]
    base = statistics.median(t["store_ingest"])
    res["ingest_bytes"] = n
    for name, v in t.items():
        med = statistics.median(v)
        res[f"ingest_{name}_ms"], res[f"ingest_{name}_ms_runs"], res[f"ingest_{name}_GBps"] = med, v, n / med / 1e6
        res[f"ingest_{name}_over_store_ingest"] = med / base
        if name != "store_ingest":
            res[f"ingest_{name}_chunks"], res[f"ingest_{name}_spans"] = state[name + "_chunks"], len(spans[name][1])
    res["ingest_store_ingest_spread_ms"] = max(t["store_ingest"]) - min(t["store_ingest"])
    state["idx"].close()
    L.cw_host_free(h_src)


# ---- many: the Python forms over corpus slices ---------------------------------------------------------------------------------------
def probe_many(files, big_files, reps, res):
    import compute_war_amd as cw
    names = sorted(os.listdir(os.path.join(ROOT, "tests", "golden", "corpus", "canterbury")))
    text = b"".join(open(os.path.join(ROOT, "tests", "golden", "corpus", "canterbury", f), "rb").read() for f in names)
    rng = np.random.default_rng(16)
    p = cw.CdcParams.default(1024)

    def slices(count):
        out = []
        for _ in range(count):
            n = int(rng.integers(4 << 10, (64 << 10) + 1))
            at = int(rng.integers(0, len(text) - n))
            out.append(text[at:at + n])
        return out

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for tag, count, with_loop in (("many", files, True), ("big", big_files, False)):
        datas = slices(count)
        total = sum(len(d) for d in datas)
        entries = p.max_offsets_streams(total, count)
        state = {}

        def fresh():
            if state.get("idx"):
                state["idx"].close()
            state["idx"] = cw.DedupeIndex("skein512", entries)
            state["cs"] = cw.ChunkStore(state["idx"], "lz4", p, total + (1 << 20), entries)

        def timed(key, fn):
            def run():
                fresh()
                state.setdefault(key, []).append(wall_ms(lambda: state.__setitem__(key + "_out", fn())))
            return run

        configs = {"stream": timed("stream", lambda: state["cs"].ingest_many_stream(datas)),
                   "many": timed("many", lambda: state["cs"].ingest_many(datas))}
        if with_loop:
            configs["loop"] = timed("loop", lambda: [state["cs"].ingest_stream(d) for d in datas])
        alternate(configs, reps, lambda fn: fn())
        for other in [k for k in configs if k != "stream"]:
            assert all(a.refs.tolist() == b.refs.tolist() and a.offsets.tolist() == b.offsets.tolist()
                       for a, b in zip(state["stream_out"], state[other + "_out"])), other
        res[f"{tag}_files"], res[f"{tag}_bytes"], res[f"{tag}_pieces"] = count, total, state["cs"].last_stats and state["cs"].last_stats["pieces"]
        res[f"{tag}_chunks"] = sum(len(r.refs) for r in state["stream_out"])
        for key in configs:
            runs = state[key][1:]
            res[f"{tag}_{key}_ms"], res[f"{tag}_{key}_ms_runs"] = statistics.median(runs), runs
        state["idx"].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--big-files", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="child processes per library of the cdc probe")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default="cdc,ingest,many")
    ap.add_argument("--cdc-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--bytes", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_streams_ingest_probe.json"))
    args = ap.parse_args()
    if args.cdc_child:
        return cdc_child(args.cdc_child, args.bytes, args.reps)
    n = int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20)
    res = {"bytes": n, "reps": args.reps}
    only = args.only.split(",")
    if "cdc" in only:
        probe_cdc(n, args.reps, args.rounds, args.parent_lib, res)   # (before this process opens the device)
    import compute_war_amd as cw
    cw.init(0)
    if "ingest" in only:
        probe_ingest(n, args.reps, res)
        torch.cuda.empty_cache()
    if "many" in only:
        probe_many(args.files, args.big_files, args.reps, res)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
