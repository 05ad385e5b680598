"""The launch plans of the LZ4 / LZF compressors (csrc/launch_plan.h), read through cw_plan_describe without a device, and one GPU
test that the launch functions enqueue what the plan says."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden


def _cases():
    return load_golden("launch_names_parent.json")


def _describe(cw, c):
    with cw.tuned(**c["knobs"]):
        return cw.plan_describe(c["alg"], c["block_bytes"], c["nblocks"], c["src_misalign"], c["dst_misalign"])


def test_plan_names_equal_what_the_parent_commit_launched():
    """launch_names_parent.json: profile_kernels()["codec"] after one dev_compress call per case, recorded on an MI355X from the commit
    BEFORE the launch functions were split into plan and enqueue (every parser knob set of test_gpu_round3 at five block sizes, the
    CW_LZ4_MODE / CW_LZF_MODE variants, sizes below the parsers' floors, misaligned sources and slots, and one block below and exactly
    at every default threshold).  Line 1 of the plan's description must be that string, for every case."""
    import compute_war_amd as cw
    cases = _cases()
    assert len(cases) == 198
    for c in cases:
        assert _describe(cw, c).split("\n")[0] == c["names"], c


def _pin_line(cw, c):
    """One line per case: the case, then cw_plan_describe's whole output with its newlines written as " | "."""
    tag = f"{c['alg']} {c['nblocks']} x {c['block_bytes']} src+{c['src_misalign']} dst+{c['dst_misalign']} " + " ".join(f"{k}={v}" for k, v in c["knobs"].items())
    return tag.rstrip() + " => " + _describe(cw, c).rstrip("\n").replace("\n", " | ")


def test_plan_dump_is_pinned():
    """launch_plans.txt: cw_plan_describe's whole output (description + every field of the plan) for the same cases, one case per line.
    This file was recorded from the plan code itself, after the names above had shown it equal to the parent: it is a regression pin
    for later work on the policy -- a change of any grid, threshold, reserve or workspace size shows up as a diff of this file -- not
    evidence of equivalence with the parent."""
    import compute_war_amd as cw
    with open(os.path.join(GOLDEN, "launch_plans.txt")) as f:
        want = f.read().split("\n")[:-1]
    cases = _cases()
    assert len(want) == len(cases)
    for c, w in zip(cases, want):
        got = _pin_line(cw, c)
        if got != w:
            g, p = got.split(" | "), w.split(" | ")
            diff = [(a, b) for a, b in zip(g, p) if a != b] or [(g[len(p):], p[len(g):])]
            raise AssertionError(f"{g[0]}: (got, pinned) {diff}")


def test_plan_describe_refuses_what_the_launch_refuses():
    import compute_war_amd as cw
    L = cw.lib()
    buf = bytearray(8192)
    import ctypes as C
    b = (C.c_char * len(buf)).from_buffer(buf)
    for alg, bs, nb in ((cw.COMP_LZ4, 0, 72), (cw.COMP_LZ4, 65537, 72), (cw.COMP_LZF, 65537, 72), (cw.COMP_LZ4, 4096, 1 << 32), (cw.COMP_NONE, 4096, 72)):
        assert L.cw_plan_describe(alg, bs, nb, 0, 0, b, len(buf)) != 0, (alg, bs, nb)
    assert L.cw_plan_describe(cw.COMP_LZ4, 4096, 72, 0, 0, b, 16) != 0      # buffer too small
    assert L.cw_plan_describe(cw.COMP_LZF, 4096, 1 << 32, 0, 0, b, len(buf)) == 0


# ---- the launch follows the plan (GPU) ----------------------------------------------------------------------------------------
FOLLOW_KNOBS = [
    dict(),
    dict(CW_LZ4_LANES=1),
    dict(CW_LZ4_VTAB=0, CW_LZ4_LANES=0, CW_LZ4_PARSE="fp", CW_LZ4_HEADW=32),
    dict(CW_LZF_LANES=1, CW_LZF_ROUND=5, CW_LANES_RESERVE=10),
    dict(CW_LZ4_MODE="cut"),
]
NBLOCKS = 72


@pytest.fixture(scope="module")
def sweep(oracle):
    """72 blocks of test_gpu_round3's sweep data per block size, and the oracle's output for each: computed once, never modified."""
    from test_gpu_round3 import _sweep_data
    blob = _sweep_data() * 4
    out = {}
    for bs in (65536, 4096, 1000):
        data = blob[:NBLOCKS * bs]
        blocks = [data[i * bs:(i + 1) * bs] for i in range(NBLOCKS)]
        out[bs] = (data, {"lz4": [oracle.lz4_compress(b) for b in blocks], "lzf": [oracle.lzf_compress(b) for b in blocks]})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", FOLLOW_KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "default")
@pytest.mark.parametrize("bs", [65536, 4096, 1000])
@pytest.mark.parametrize("comp", ["lz4", "lzf"])
def test_launch_follows_the_plan(sweep, comp, bs, knobs):
    """What the launch reports it enqueued is line 1 of the plan for the call's actual alignment, sizes and payloads equal the
    oracle's, and a second identical call (warm workspaces) gives the same of both."""
    import torch
    import compute_war_amd as cw
    cw.init(0)
    data, want = sweep[bs][0], sweep[bs][1][comp]
    s = torch.cuda.current_stream().cuda_stream
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    stride = (cw.compress_bound(comp, bs) + 15) // 16 * 16
    with cw.tuned(**knobs):
        planned = cw.plan_describe(comp, bs, NBLOCKS, (src.data_ptr() | bs) & 15, 0).split("\n")[0]
        for _ in range(2):
            dst = torch.zeros(NBLOCKS * stride, dtype=torch.uint8, device="cuda")
            sizes = torch.zeros(NBLOCKS, dtype=torch.int32, device="cuda")
            assert (dst.data_ptr() | stride) & 15 == 0
            cw.dev_compress(comp, src.data_ptr(), bs, NBLOCKS, dst.data_ptr(), stride, sizes.data_ptr(), s)
            torch.cuda.synchronize()
            assert cw.profile_kernels()["codec"] == planned
            assert [int(z) for z in sizes.cpu().numpy().astype(np.uint32)] == [len(e) for e in want], (planned,)
            slots = dst.view(NBLOCKS, stride).cpu().numpy()
            for i, e in enumerate(want):
                assert slots[i, :len(e)].tobytes() == e, (i, planned)
