"""What chunking many streams in one call costs and saves on one GPU.

Device events around the calls, one warm-up, the median of --reps runs with the configurations alternating.

  cdc       cw_dev_cdc_streams against cw_dev_cdc over the same --gib GiB of cw_dev_gen_random data (cw_cdc_default_params(8192)):
            as one stream, as streams of 64 KiB and as streams of 4 KiB.  Reported: ms, GB/s and the ratio to cw_dev_cdc.
  ingest    ChunkStore.ingest_many of --files corpus slices of 4 to 64 KiB (LZ4, Skein-512, cw_cdc_default_params(1024)) against a
            loop of ChunkStore.ingest over them, each into a fresh index and store (wall time: both include their uploads).  Reported:
            both times and the per-call cost the difference implies.

Prints one JSON object and writes it to --out."""
import argparse
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


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(configs, reps, timer):
    times = {name: [] for name in configs}
    for fn in configs.values():
        timer(fn)
    for _ in range(reps):
        for name, fn in configs.items():
            times[name].append(timer(fn))
    return times


def probe_cdc(n, reps, res):
    st = torch.cuda.current_stream().cuda_stream
    p = cw.CdcParams.default(8192)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    cw.dev_gen_random(7, 0, n // 4096, 4096, src.data_ptr(), st)
    z = lambda count: torch.zeros(count, dtype=torch.int64, device="cuda")  # noqa: E731
    shapes = {"one_stream": n, "streams_64k": 64 << 10, "streams_4k": 4 << 10}
    most = n // min(shapes.values())
    cap = p.max_offsets_streams(n, most)
    offs, k, first, result = z(cap), z(1), z(most + 1), z(1)
    ends = {name: torch.arange(1, n // size + 1, dtype=torch.int64, device="cuda") * size for name, size in shapes.items()}
    torch.cuda.synchronize()

    def single():
        cw.dev_cdc(p, src.data_ptr(), n, True, offs.data_ptr(), cap, k.data_ptr(), st)

    def streams(name):
        def run():
            e = ends[name]
            cw.dev_cdc_streams(p, src.data_ptr(), n, e.data_ptr(), e.numel(), offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(), result.data_ptr(), st)
        return run

    configs = {"dev_cdc": single}
    configs.update({name: streams(name) for name in shapes})
    t = alternate(configs, reps, event_ms)
    chunks = {}
    for name, fn in configs.items():
        fn()
        torch.cuda.synchronize()
        chunks[name] = int(k.item())
        assert name == "dev_cdc" or int(result.item()) == 0
    assert chunks["one_stream"] == chunks["dev_cdc"]
    base = statistics.median(t["dev_cdc"])
    for name, v in t.items():
        med = statistics.median(v)
        res[f"cdc_{name}_ms"], res[f"cdc_{name}_ms_runs"], res[f"cdc_{name}_GBps"] = med, v, n / med / 1e6
        res[f"cdc_{name}_chunks"] = chunks[name]
        if name != "dev_cdc":
            res[f"cdc_{name}_streams"] = int(ends[name].numel())
            res[f"cdc_{name}_over_dev_cdc"] = med / base


def probe_ingest(files, reps, res):
    names = sorted(os.listdir(os.path.join(ROOT, "tests", "golden", "corpus", "canterbury")))
    text = b"".join(open(os.path.join(ROOT, "tests", "golden", "corpus", "canterbury", f), "rb").read() for f in names)
    rng = np.random.default_rng(16)
    datas = []
    for _ in range(files):
        n = int(rng.integers(4 << 10, (64 << 10) + 1))
        at = int(rng.integers(0, len(text) - n))
        datas.append(text[at:at + n])
    total = sum(len(d) for d in datas)
    p = cw.CdcParams.default(1024)
    entries = p.max_offsets_streams(total, files)
    state = {}

    def fresh():
        if state.get("idx"):
            state["idx"].close()
        state["idx"] = cw.DedupeIndex("skein512", entries)
        state["cs"] = cw.ChunkStore(state["idx"], "lz4", p, total + (1 << 20), entries)

    def timed(fn, key):
        def run():
            fresh()
            state.setdefault(key, []).append(wall_ms(fn))
        return run

    def many():
        state["many"] = state["cs"].ingest_many(datas)

    def loop():
        state["loop"] = [state["cs"].ingest(d) for d in datas]

    alternate({"many": timed(many, "many_ms"), "loop": timed(loop, "loop_ms")}, reps, lambda fn: fn())
    assert all(a.refs.tolist() == b.refs.tolist() and a.offsets.tolist() == b.offsets.tolist() for a, b in zip(state["many"], state["loop"]))
    state["idx"].close()
    many_runs, loop_runs = state["many_ms"][1:], state["loop_ms"][1:]
    m, lo = statistics.median(many_runs), statistics.median(loop_runs)
    res.update(ingest_files=files, ingest_bytes=total, ingest_chunks=sum(len(r.refs) for r in state["many"]),
               ingest_many_ms=m, ingest_many_ms_runs=many_runs, ingest_loop_ms=lo, ingest_loop_ms_runs=loop_runs,
               ingest_loop_over_many=lo / m, ingest_per_call_ms=(lo - m) / files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_streams_probe.json"))
    args = ap.parse_args()
    cw.init(0)
    res = {"bytes": int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20), "reps": args.reps}
    probe_cdc(res["bytes"], args.reps, res)
    torch.cuda.empty_cache()
    probe_ingest(args.files, args.reps, res)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
