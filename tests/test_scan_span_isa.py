"""CPU-side checks of the LZ4 span scan as compiled for gfx950 (no GPU needed): no scratch and no spills, a register budget no
larger than before the probe schedule and the aligned literal stores, and aligned 16-byte nontemporal stores on the literal path of
the 16-byte-aligned variant."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

VGPR_BUDGET = 117  # lz4_scan_span_kernel before the per-n probe schedule and the aligned literal stores


def _kernel_blocks(asm):
    """{kernel symbol: its code} of the device assembly (each kernel runs from its label to .Lfunc_end)."""
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.M | re.S)}


def _kernel_meta(asm):
    """{kernel symbol: its metadata entry}"""
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def _field(entry, key):
    return int(re.search(re.escape(key) + r":\s+(\d+)", entry).group(1))


@pytest.fixture(scope="module")
def lz4_asm(tmp_path_factory):
    src = os.path.join(ROOT, "compute_war_amd", "csrc", "lz4_kernel.hip")
    out = str(tmp_path_factory.mktemp("asm") / "lz4.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True)
    return open(out).read()


def _span(asm, aligned):
    tag = "ILb1E" if aligned else "ILb0E"
    names = [k for k in _kernel_meta(asm) if "lz4_scan_span_kernel" in k and tag in k]
    assert len(names) == 1, names
    return names[0]


@pytest.mark.parametrize("aligned", [True, False])
def test_span_scan_has_no_scratch_and_keeps_its_register_budget(lz4_asm, aligned):
    name = _span(lz4_asm, aligned)
    e = _kernel_meta(lz4_asm)[name]
    assert _field(e, ".private_segment_fixed_size") == 0, name
    assert _field(e, ".vgpr_spill_count") == 0, name
    assert _field(e, ".sgpr_spill_count") == 0, name
    assert _field(e, ".vgpr_count") <= VGPR_BUDGET, (name, _field(e, ".vgpr_count"))
    body = _kernel_blocks(lz4_asm)[name]
    assert not re.search(r"\b(scratch|buffer)_(load|store)", body), name


def test_aligned_span_scan_stores_the_literal_run_as_aligned_lines(lz4_asm):
    body = _kernel_blocks(lz4_asm)[_span(lz4_asm, True)]
    stores = re.findall(r"^\s*global_store_dwordx4 [^\n]*", body, flags=re.M)
    nt = [s for s in stores if s.rstrip().endswith(" nt")]
    # 16 chunks per span x 4 pieces, unrolled over the three register sets, plus the header lines
    assert len(nt) >= 12, stores
    # the aligned variant computes each line from the ring: no store sits at the header's 2-byte shift
    for s in nt:
        off = re.search(r"offset:(-?\d+)", s)
        assert off is None or int(off.group(1)) % 16 == 0, s
    assert "v_alignbyte_b32" in body
    # the block's last 2 bytes
    assert re.search(r"global_store_short", body)
