"""CPU-side checks of the two kernels of the fused hash + LZ4 step as compiled for gfx950 (no GPU needed).

Span scan (both variants): no scratch, no spills, and no more VGPRs than before the probes were batched by schedule group.
Skein slice kernel, the mask-free instantiation that runs every slice but a hash's last: its loop holds no v_cndmask_b32 (no
prefetched line is masked), the cipher's instructions as before, the line still requested in one piece between the rounds of its two
halves and waited for behind them, four waves per SIMD, no spills, no scratch."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

# lz4_scan_span_kernel<true> / <false> with the chunk-cut probe batches (the commit before the group schedule)
SPAN_VGPRS_BEFORE = {True: 99, False: 114}
# per loop iteration = one 128-byte line = two Threefish-512 or four Threefish-256 calls
# (v_xor_b32, v_alignbit_b32, v_lshl_add_u64), counted in the masked kernel before the split
CIPHER_COUNTS = {8: (1216, 1152, 940)}


def _compile(tmp_path_factory, name):
    src = os.path.join(ROOT, "compute_war_amd", "csrc", name)
    out = str(tmp_path_factory.mktemp("asm") / (name + ".s"))
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True)
    return open(out).read()


@pytest.fixture(scope="module")
def lz4_asm(tmp_path_factory):
    return _compile(tmp_path_factory, "lz4_kernel.hip")


@pytest.fixture(scope="module")
def skein_asm(tmp_path_factory):
    return _compile(tmp_path_factory, "skein_kernels.hip")


def _kernel_blocks(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.M | re.S)}


def _kernel_meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def _field(entry, key):
    return int(re.search(re.escape(key) + r":\s+(\d+)", entry).group(1))


def _one(asm, *parts):
    names = [k for k in _kernel_meta(asm) if all(p in k for p in parts)]
    assert len(names) == 1, (parts, names)
    return names[0]


def _assert_no_scratch(asm, name):
    e = _kernel_meta(asm)[name]
    assert _field(e, ".private_segment_fixed_size") == 0, name
    assert _field(e, ".vgpr_spill_count") == 0, name
    assert _field(e, ".sgpr_spill_count") == 0, name
    assert not re.search(r"\b(scratch|buffer)_(load|store)", _kernel_blocks(asm)[name]), name


def _loops(body):
    """every loop of a kernel body as its list of instruction lines: from a label to the last backward branch to it"""
    lines = body.splitlines()
    label_at = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    ends = {}
    for i, l in enumerate(lines):
        m = re.match(r"^\s+s_cbranch_\w+ (\.LBB\d+_\d+)", l) or re.match(r"^\s+s_branch (\.LBB\d+_\d+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            ends[m.group(1)] = i
    return [[l.strip() for l in lines[label_at[lab]:end + 1] if re.match(r"^\s+[a-z]", l)] for lab, end in ends.items()]


def _count(loop, op):
    return sum(1 for l in loop if l.split()[0].startswith(op))


@pytest.mark.parametrize("aligned", [True, False])
def test_span_scan_keeps_its_registers(lz4_asm, aligned):
    name = _one(lz4_asm, "lz4_scan_span_kernel", "ILb1E" if aligned else "ILb0E")
    _assert_no_scratch(lz4_asm, name)
    vgprs = _field(_kernel_meta(lz4_asm)[name], ".vgpr_count")
    assert vgprs <= SPAN_VGPRS_BEFORE[aligned], (name, vgprs)


def test_four_word_slices_stay_masked(skein_asm):
    """Skein-256 keeps the masked kernel for every slice: hipcc moves a quarter of the mask-free kernel's line request to the top of
    the loop (the line would be fetched in two parts), so that instantiation is not built."""
    assert [k for k in _kernel_meta(skein_asm) if "skein_slice_kernel" in k and "ILi4E" in k] == [_one(skein_asm, "skein_slice_kernel", "ILi4ELb1ELb0E")]


@pytest.mark.parametrize("nw", [8])
def test_interior_skein_slices_run_a_mask_free_loop(skein_asm, nw):
    interior = _one(skein_asm, "skein_slice_kernel", "ILi%dELb1ELb1E" % nw)
    masked = _one(skein_asm, "skein_slice_kernel", "ILi%dELb1ELb0E" % nw)
    _assert_no_scratch(skein_asm, interior)
    _assert_no_scratch(skein_asm, masked)
    for name in (interior, masked):
        assert _field(_kernel_meta(skein_asm)[name], ".vgpr_count") <= 112, name  # four waves per SIMD

    def main_loop(name):
        loops = _loops(_kernel_blocks(skein_asm)[name])
        assert loops, name
        return max(loops, key=lambda lp: _count(lp, "v_xor_b32"))

    loop, ref = main_loop(interior), main_loop(masked)
    assert _count(loop, "v_cndmask_b32") == 0, [l for l in loop if l.startswith("v_cndmask")]
    assert _count(ref, "v_cndmask_b32") > 0  # the last slice still masks what lies past the message
    ops = ("v_xor_b32", "v_alignbit_b32", "v_lshl_add_u64")
    cipher, cipher_ref = [_count(loop, op) for op in ops], [_count(ref, op) for op in ops]
    # the masked kernel is the one counted before the split: over the whole kernel, where the 64-bit adds include the tweak and
    # address arithmetic around the cipher (4 of the 940 lie outside the loop)
    whole_ref = tuple(len(re.findall(r"^\s+%s" % op, _kernel_blocks(skein_asm)[masked], flags=re.M)) for op in ops)
    if nw in CIPHER_COUNTS:
        assert whole_ref == CIPHER_COUNTS[nw], whole_ref
        assert tuple(cipher[:2]) == CIPHER_COUNTS[nw][:2], cipher
    # rotates and xors are the cipher's alone: identical.  The 64-bit adds are the cipher's (per call 72 rounds x NW/2 MIX adds and
    # 19 key injections x NW words = 440 for 8 words, 220 for 4; 880 per 128-byte line either way) plus tweak and address arithmetic,
    # of which the interior loop needs less (no "last step" / "output transform" cases): never more than the masked loop has.
    assert cipher[:2] == cipher_ref[:2], (cipher, cipher_ref)
    assert 880 <= cipher[2] <= cipher_ref[2], (cipher, cipher_ref)

    def vm_waits(lp):
        return [(i, int(re.search(r"vmcnt\((\d+)\)", l).group(1))) for i, l in enumerate(lp) if l.startswith("s_waitcnt") and "vmcnt" in l]

    loads = [i for i, l in enumerate(loop) if l.startswith("global_load_dwordx")]
    assert sum(4 * int(loop[i].split()[0][len("global_load_dwordx"):]) for i in loads) == 128, [loop[i] for i in loads]  # one line
    # the whole next line is requested together, between the rounds of the two halves ...
    assert not any(l.startswith(("v_xor_b32", "v_alignbit_b32")) for l in loop[loads[0]:loads[-1]])
    assert _count(loop[:loads[0]], "v_xor_b32") >= cipher[0] // 3
    # ... and waited for only behind the rounds of the second half: the loop ends with nothing outstanding, so a wait at its top
    # (the first iteration's) finds nothing to wait for later on
    after = [(i, n) for i, n in vm_waits(loop) if i > loads[-1]]
    assert after and after[-1][1] == 0, vm_waits(loop)
    assert _count(loop[loads[-1]:after[0][0]], "v_xor_b32") >= cipher[0] // 3, vm_waits(loop)
    assert _count(loop[after[0][0]:], "v_xor_b32") <= 2 * nw  # (the last call's feed-forward of its message words)
    if nw == 8:
        assert [n for _, n in vm_waits(ref)] == [3, 0], vm_waits(ref)
