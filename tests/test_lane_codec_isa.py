"""CPU-side checks of the lane-per-block codecs as compiled for gfx950 (no GPU needed).

The fixed-size lane kernels and the kernels over content-defined chunks run one loop each (csrc/lane_codec.h) over a source / table
pair.  A lane kernel's speed is its number of resident chains, so sharing the loop must cost no registers: every kernel has no
scratch, no spills, and no more VGPRs than it had with its own copy of the loop (a block length that became a lane value in a
fixed-size kernel shows here first).  Each helper the copies came with is defined exactly once."""
import os
import re

import pytest

from conftest import ROOT
from test_fused_isa import _assert_no_scratch, _compile, _field, _kernel_meta, _one

CSRC = os.path.join(ROOT, "compute_war_amd", "csrc")

# (file, kernel, template arguments as mangled): .vgpr_count of the commit before the loops were shared, hipcc -O3 -std=c++17
VGPRS_BEFORE = {
    ("lz4_kernel.hip", "lz4_lanes_kernel", "ILi0E"): 60,
    ("lz4_kernel.hip", "lz4_lanes_kernel", "ILi1E"): 60,
    ("lz4_kernel.hip", "lz4_lanes_kernel", "ILi2E"): 60,
    ("lzf_kernel.hip", "lzf_lanes_kernel", "ILb0E"): 50,
    ("lzf_kernel.hip", "lzf_lanes_kernel", "ILb1E"): 50,
    ("decompress_kernels.hip", "decompress_lanes_kernel", "ILi0E"): 38,
    ("decompress_kernels.hip", "decompress_lanes_kernel", "ILi1E"): 34,
    ("chunk_codec_kernels.hip", "lz4_chunks_kernel", ""): 70,
    ("chunk_codec_kernels.hip", "lzf_chunks_kernel", ""): 52,
    ("chunk_codec_kernels.hip", "decompress_chunks_kernel", "ILi0E"): 32,
    ("chunk_codec_kernels.hip", "decompress_chunks_kernel", "ILi1E"): 32,
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return {name: _compile(tmp_path_factory, name) for name in sorted({f for f, _, _ in VGPRS_BEFORE})}


@pytest.mark.parametrize("file,kernel,targs", list(VGPRS_BEFORE), ids=["%s%s" % (k, t) for _, k, t in VGPRS_BEFORE])
def test_lane_kernels_keep_their_registers(asm, file, kernel, targs):
    name = _one(asm[file], kernel, kernel + targs)
    _assert_no_scratch(asm[file], name)
    vgprs = _field(_kernel_meta(asm[file])[name], ".vgpr_count")
    print(name, "VGPRs", vgprs, "before", VGPRS_BEFORE[file, kernel, targs])
    assert vgprs <= VGPRS_BEFORE[file, kernel, targs], (name, vgprs)


@pytest.mark.parametrize("helper", ["store_upto16", "lane_copy_match", "lane_copy_literals", "lane_put_len", "win_at", "lzf_slot",
                                    "lz4_lane_run", "lzf_lane_run", "lane_decode"])
def test_each_shared_helper_is_defined_once(helper):
    defs = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(CSRC, f)).read()
            defs += [f for _ in re.finditer(r"^[^\n/]*__device__[^\n;(]*\b%s\(" % helper, text, flags=re.M)]
    assert defs == ["lane_codec.h"], (helper, defs)
