#!/usr/bin/env python3
"""Generate tests/golden/* from the reference tree (run in the build container only).

What it writes (all DATA -- inputs and expected outputs, no reference source text):

* skein_kat_{512,256}.json   -- vectors taken verbatim from the reference's NIST KAT files
                                reference_code/skein/KAT_MCT/{ShortMsgKAT,LongMsgKAT}_{512,256}.txt
                                (every byte-aligned short message, a sample of bit-granular ones,
                                every 8th long message) and MonteCarlo_{512,256}.txt (seed + first MDs).
* skein_ref_blocks.json      -- digests of 4096 / 65536-byte blocks (sizes no KAT reaches) and of
                                Skein-256-128 (a variant no KAT covers) computed by oracle/_ref =
                                the reference's Optimized_64bit/skein.c + skein_block.c compiled
                                where they lie (oracle/Makefile target `ref`).
* skein_ref_live.json        -- oracle/_ref's digests of the fresh inputs of
                                tests/test_oracle_skein.py::test_live_reference_build_when_present
                                (Skein-512-512/-256/-160, Skein-256-128), so that the test also runs
                                where oracle/_ref cannot be built (`--live` writes only this file).
* survey_anchors.json        -- the reference outputs SURVEY.md 8(c) / BASELINE.md section 2 recorded
                                (LZ4 1.8.2 / liblzf sizes, SHA-256 of outputs, corpus ratios).
* corpus/canterbury/*        -- the reference's dataset/canterbury files (data the reference's own
                                run_tests feed to the path: src/hashandcompress/run_tests:17).
* codec_regress.json         -- per-block compressed size + SHA-256 from THIS repo's oracle over the
                                corpus (regression values; pinned to the reference only through
                                survey_anchors.json -- "parity unpinned by the reference itself").
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference"
KAT = f"{REF}/reference_code/skein/KAT_MCT"
OUT = f"{ROOT}/tests/golden"

import numpy as np  # noqa: E402

import oracle as O  # noqa: E402


def parse_kat(path):
    recs, cur = [], {}
    for line in open(path):
        line = line.strip()
        if line.startswith("Len = "):
            cur = {"len": int(line[6:])}
        elif line.startswith("Msg = "):
            cur["msg"] = line[6:].lower()
        elif line.startswith("MD = "):
            cur["md"] = line[5:].lower()
            recs.append(cur)
    return recs


def parse_mct(path, keep=12):
    seed, mds = None, []
    for line in open(path):
        line = line.strip()
        if line.startswith("Seed = "):
            seed = line[7:].lower()
        elif line.startswith("MD = "):
            mds.append(line[5:].lower())
    return {"seed": seed, "md": mds[:keep]}


def skein_kats(bits):
    short = parse_kat(f"{KAT}/ShortMsgKAT_{bits}.txt")
    long_ = parse_kat(f"{KAT}/LongMsgKAT_{bits}.txt")
    keep_short = [r for r in short if r["len"] % 8 == 0 or r["len"] < 72 or r["len"] % 61 == 0]
    keep_long = long_[::8] + [long_[-1]]
    # messages are stored padded to whole bytes; trim to ceil(len/8) bytes (Len=0 is stored as "00")
    for r in keep_short + keep_long:
        r["msg"] = r["msg"][: 2 * ((r["len"] + 7) // 8)]
    return {
        "source": f"reference_code/skein/KAT_MCT/ShortMsgKAT_{bits}.txt, LongMsgKAT_{bits}.txt, MonteCarlo_{bits}.txt",
        "variant": f"Skein-{512 if bits == 512 else 256}-{bits}",
        "short": keep_short, "long": keep_long,
        "montecarlo": parse_mct(f"{KAT}/MonteCarlo_{bits}.txt"),
    }


def seeded_block(seed, n, kind):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "text":  # low-entropy
        return rng.integers(97, 101, n, dtype=np.uint8).tobytes()
    if kind == "zero":
        return bytes(n)
    if kind == "pattern":  # SURVEY 8(c) anchor input
        return bytes(((i * 131 + (i >> 8)) & 0xFF) for i in range(n))
    raise ValueError(kind)


def ref_blocks():
    assert O.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    recs = []
    for n in (4096, 65536, 64, 65, 128, 1, 0, 8192, 12345):
        for kind, seed in (("random", 1), ("random", 2), ("text", 3), ("zero", 0), ("pattern", 0)):
            d = seeded_block(seed, n, kind)
            recs.append({
                "n": n, "kind": kind, "seed": seed,
                "skein512_512": O.ref_skein512(d, 512).hex(),
                "skein256_128": O.ref_skein256(d, 128).hex(),
                "skein256_256": O.ref_skein256(d, 256).hex(),
            })
    return {"source": "oracle/_ref/libskein_ref.so = reference_code/skein/Optimized_64bit/{skein.c,skein_block.c} "
                      "compiled in place; inputs regenerated by tools/make_golden.py:seeded_block",
            "blocks": recs}


SURVEY_ANCHORS = {
    "source": "SURVEY.md 8(c) session anchors + BASELINE.md section 2 (outputs of the reference's liblz4.a v1.8.2 / "
              "liblzf.a / Optimized_64bit skein, recorded by the survey; the archives themselves are never run here)",
    "anchors": [
        {"input": "zero", "n": 4096, "skein512_prefix": "9bdfbffee6dc08117ae9c04ed72bf19c",
         "skein256_128": "4f9eaecfeb124af5fd75ed83099f678b", "lz4": 26, "lzf": 54},
        {"input": "zero", "n": 65536, "skein512_prefix": "546ad3bfcfb68f8c3f6bba7691ff5a34",
         "skein256_128": "1fbfa0b477fb9e493aaddd3cd4f1e397", "lz4": 267, "lzf": 753},
        {"input": "pattern", "n": 65536, "skein512_prefix": "b74d5d38d00a1d63b79228d7358002f3",
         "skein256_128": "8cdad38e595ec88c91d93f2f81ec70af", "lz4": 2699, "lzf": 3307},
        {"input": "alice29", "n": 4096, "skein512_prefix": "1cb13eb86b55535b206c28be36cbae0a",
         "skein256_128": "4159727875aebb36b49ca87786a9ddf8", "lz4": 3044, "lzf": 2809},
        {"input": "alice29", "n": 65536, "skein512_prefix": "7f6256b16d9172cf57d03f05d0f0f91d",
         "skein256_128": "78c690e49fe4c62df9d96afe9b0f58dd", "lz4": 39618, "lzf": 36641,
         "lz4_sha256": "4fc3554d1b84881b07f4ec8729a54aa9d9c74120e9543b4a926d40af50f66c06",
         "lzf_sha256": "94937e9983ca50494f16327c892f65c773423e4af553992d41177c6651b47734"},
    ],
    # whole 64 KiB blocks of every file of the corpus, chunked at `block`
    "corpus_ratios": [
        {"corpus": "canterbury", "block": 4096, "lz4": 1.9776, "lzf": 2.0374},
        {"corpus": "canterbury", "block": 65536, "lz4": 2.2890, "lzf": 2.3396},
        {"corpus": "canterbury-large", "block": 4096, "lz4": 1.4933, "lzf": 1.6064},
        {"corpus": "canterbury-large", "block": 65536, "lz4": 1.9313, "lzf": 1.9295},
    ],
    "random_64k_lz4_size": 65794,
}


def skein_tree_kats():
    """Tree-mode vectors of the reference's golden KAT file (Skein-256 and Skein-512 states; byte-granular messages)."""
    import re
    txt = open(f"{KAT}/skein_golden_kat.txt").read()
    out = []
    for blk in txt.split("--------------------------------"):
        m = re.search(r":Skein-(\d+):\s+(\d+)-bit hash, msgLen =\s*(\d+) bits\. Tree: leaf=([0-9A-Fa-f]+), node=([0-9A-Fa-f]+), maxLevels=([0-9A-Fa-f]+)", blk)
        if not m or m[1] not in ("256", "512"):
            continue
        bits = int(m[3])
        assert bits % 8 == 0
        msg_part = blk[blk.index("Message data:") + len("Message data:"):blk.index("Result:")]
        res_part = blk[blk.index("Result:") + len("Result:"):]
        hx = lambda t: "".join(re.findall(r"\b[0-9A-Fa-f]{2}\b", t)).lower()
        msg, res = hx(msg_part) if bits else "", hx(res_part)
        assert len(msg) == bits // 4 and len(res) == (int(m[2]) + 7) // 8 * 2, (m[0], len(msg), len(res))
        out.append({"state_bits": int(m[1]), "hash_bits": int(m[2]), "leaf": int(m[4], 16), "node": int(m[5], 16),
                    "max_level": int(m[6], 16), "msg": msg, "digest": res})
    return {"source": "reference_code/skein/KAT_MCT/skein_golden_kat.txt (tree vectors, Skein-256 / Skein-512)", "vectors": out}


def corpus_files(name):
    d = f"{REF}/dataset/{name}"
    return [(f, open(f"{d}/{f}", "rb").read()) for f in sorted(os.listdir(d))]


def codec_regress():
    """Per-block size + sha256 of the oracle's LZ4/LZF output over canterbury (both block sizes),
    plus corpus totals for canterbury-large (whose files are too big to commit)."""
    out = {"source": "this repo's oracle (regression values; reference-pinned only via survey_anchors.json)",
           "blocks": [], "totals": []}
    for corpus in ("canterbury", "canterbury-large"):
        for bs in (4096, 65536):
            tin = t4 = tf = 0
            for fname, data in corpus_files(corpus):
                whole = len(data) // 65536 * 65536
                for o in range(0, whole, bs):
                    b = data[o:o + bs]
                    c4, cf = O.lz4_compress(b), O.lzf_compress(b)
                    tin += bs
                    t4 += len(c4)
                    tf += len(cf) if cf else bs
                    if corpus == "canterbury" and (bs == 65536 or (o // bs) % 16 == 0):
                        out["blocks"].append({
                            "file": fname, "offset": o, "n": bs,
                            "lz4": len(c4), "lz4_sha256": hashlib.sha256(c4).hexdigest(),
                            "lzf": len(cf), "lzf_sha256": hashlib.sha256(cf).hexdigest(),
                        })
            out["totals"].append({"corpus": corpus, "block": bs, "in": tin, "lz4": t4, "lzf": tf})
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    O.build()
    for bits in (512, 256):
        json.dump(skein_kats(bits), open(f"{OUT}/skein_kat_{bits}.json", "w"), indent=0)
    json.dump(ref_blocks(), open(f"{OUT}/skein_ref_blocks.json", "w"), indent=0)
    json.dump(skein_tree_kats(), open(f"{OUT}/skein_kat_tree.json", "w"), indent=0)
    json.dump(SURVEY_ANCHORS, open(f"{OUT}/survey_anchors.json", "w"), indent=1)
    dst = f"{OUT}/corpus/canterbury"
    os.makedirs(dst, exist_ok=True)
    for fname, data in corpus_files("canterbury"):
        with open(f"{dst}/{fname}", "wb") as f:
            f.write(data)
    json.dump(codec_regress(), open(f"{OUT}/codec_regress.json", "w"), indent=0)
    print("golden fixtures written to", OUT)


LIVE_SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4096, 65536, 70001)


def ref_live():
    assert O.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    recs = []
    for n in LIVE_SIZES:
        d = seeded_block(n + 7, n, "random")
        recs.append({"n": n, "kind": "random", "seed": n + 7,
                     **{f"skein512_{bits}": O.ref_skein512(d, bits).hex() for bits in (512, 256, 160)},
                     "skein256_128": O.ref_skein256(d, 128).hex()})
    return {"source": "oracle/_ref/libskein_ref.so (see skein_ref_blocks.json); inputs regenerated by tools/make_golden.py:seeded_block",
            "blocks": recs}


def skein_internals():
    """Round-by-round Threefish states of the reference's skein_golden_kat_short_internals.txt (generated by the reference's
    SKEIN_DEBUG build, skein.h:246-254): every Threefish-256 / -512 call record of the file = tweak, key words, input block
    and the states after the initial key injection, each round and each key injection, in file order."""
    import re
    path = os.path.join(REF, "reference_code", "skein", "KAT_MCT", "skein_golden_kat_short_internals.txt")
    text = open(path, newline="").read().replace("\r\n", "\n")   # the file has DOS line ends
    recs = []
    words = lambda s: [int(w.replace(".", ""), 16) for w in re.findall(r"[0-9A-F]{8}\.[0-9A-F]{8}", s)]
    for m in re.finditer(r":Threefish-(256|512):  encryption \+ plaintext feedforward \(round-by-round\):\n(.*?)(?=\n:Threefish-\d+:  encryption|\n:Skein-|\Z)", text, re.S):
        bits, body = int(m.group(1)), m.group(2)
        nw = bits // 64
        tweak = words(re.search(r"Tweak:\n(.*?)\n  Key words", body, re.S).group(1))
        key = words(re.search(r"Key words:\n(.*?)\n  Tweak schedule", body, re.S).group(1))
        block = words(re.search(r"Input block \(words\):\n(.*?)\n  Input block \(bytes\)", body, re.S).group(1))
        states = [words(x.split("\n:")[0]) for x in body.split("]=\n")[1:]]   # the words between "]=" and the next ":" line
        if len(key) != nw or len(block) != nw or len(states) < 91 or any(len(s) != nw for s in states[:91]):
            continue
        recs.append({"state_words": nw, "tweak": tweak, "key": key, "block_words": block, "states": states[:91]})
        if len(recs) >= 12:
            break
    return {"source": "reference_code/skein/KAT_MCT/skein_golden_kat_short_internals.txt (the reference's own round-by-round dump), "
                      "first Threefish-256/-512 call records; states = after the initial key injection, then after each round / "
                      "key injection in execution order (91 per call)",
            "calls": recs}


if __name__ == "__main__":
    if "--internals" in sys.argv:   # only the round-by-round fixture (the other fixtures are unchanged)
        with open(f"{OUT}/skein_internals.json", "w") as f:
            json.dump(skein_internals(), f)
        print("wrote skein_internals.json")
    elif "--live" in sys.argv:      # only the live-input fixture
        O.build()
        with open(f"{OUT}/skein_ref_live.json", "w") as f:
            json.dump(ref_live(), f, indent=0)
        print("wrote skein_ref_live.json")
    else:
        main()
