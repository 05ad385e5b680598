"""What test_guard_abi.py and test_guard2_abi.py ask of guard_kernels.hip compiled for gfx950: the file holds the kernels they expect,
each once, none of them uses scratch memory or spills, and none holds more registers than the two files it was merged from."""
import os
import re
import subprocess

from conftest import ROOT

HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950"]
KERNELS = 17  # 6 templates over Dual in both instantiations, 3 kernels that both parities run, 2 that only the dual guard runs

# By the name pattern in the merged file -- `ILb0E` is the Dual = false instantiation and stands for the single guard's kernel,
# `ILb1E` for the dual guard's -- the .vgpr_count of the kernel before the merge: measured with the command above on the single and
# the dual guard's own files (guard_fold .. rebuild_finish, guard2_fold .. rebuild2_finish).
VGPRS_BEFORE = {"guard_fold_kernelILb0E": 64, "guard_compare_kernelILb0E": 56, "guard_check_finish_kernelILb0E": 14, "rebuild_count_kernelE": 24,
                "rebuild_scatter_kernelE": 26, "rebuild_status_kernelILb0E": 25, "rebuild_copy_kernelILb0E": 22, "rebuild_finish_kernelILb0E": 6,
                "guard_fold_kernelILb1E": 63, "guard_compare_kernelILb1E": 62, "guard_check_finish_kernelILb1E": 15, "rebuild_status_kernelILb1E": 32,
                "rebuild2_fill_kernelE": 10, "rebuild2_pair_kernelE": 42, "rebuild_copy_kernelILb1E": 36, "rebuild_finish_kernelILb1E": 8}
SINGLE = ("guard_fold_kernelILb0E", "guard_update_finish_kernelE", "guard_compare_kernelILb0E", "guard_check_finish_kernelILb0E", "rebuild_count_kernelE",
          "rebuild_scatter_kernelE", "rebuild_status_kernelILb0E", "rebuild_copy_kernelILb0E", "rebuild_finish_kernelILb0E")
DUAL = ("guard_fold_kernelILb1E", "guard_update_finish_kernelE", "guard_compare_kernelILb1E", "guard_check_finish_kernelILb1E", "rebuild_count_kernelE",
        "rebuild_scatter_kernelE", "rebuild_status_kernelILb1E", "rebuild2_fill_kernelE", "rebuild2_pair_kernelE", "rebuild_copy_kernelILb1E",
        "rebuild_finish_kernelILb1E")
assert len(set(SINGLE) | set(DUAL)) == KERNELS and set(VGPRS_BEFORE) == (set(SINGLE) | set(DUAL)) - {"guard_update_finish_kernelE"}


def vgpr_bound(before):
    """A merged kernel may hold 4 registers more than its counterpart did -- the allocator's noise when code is reordered -- but never
    so many that fewer wavefronts fit.  A gfx950 SIMD has 512 registers per lane for its wavefronts of 64, hands them out in eights
    and holds at most 8 wavefronts: the occupancy step of a kernel is the largest count that still fits as many wavefronts as
    `before` did.  Every kernel of the table holds at most 64 registers, 8 wavefronts, so the step of each is 64."""
    waves = min(8, 512 // (-(-before // 8) * 8))
    step = 512 // waves // 8 * 8
    return min(before + 4, step)


assert all(vgpr_bound(v) == min(v + 4, 64) for v in VGPRS_BEFORE.values())


def lds_bytes(entry):
    return int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1))


def compiled(tmp_path, names):
    """The metadata of the kernels `names`, in that order, after every assertion above."""
    out = str(tmp_path / "guard_kernels.s")
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", "guard_kernels.hip"), "-o", out], check=True, capture_output=True)
    asm = open(out).read()
    meta = {}
    for e in re.split(r"\n  - ", asm[asm.index("amdhsa.kernels"):]):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            meta[m.group(1)] = e
    assert len(meta) == KERNELS, sorted(meta)
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    found = []
    for name in names:
        hits = [e for k, e in meta.items() if re.search(r"\d" + name, k)]
        assert len(hits) == 1, name
        if name in VGPRS_BEFORE:
            vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", hits[0]).group(1))
            print(f"{name}: {vgprs} VGPRs, {VGPRS_BEFORE[name]} before, at most {vgpr_bound(VGPRS_BEFORE[name])}")
            assert vgprs <= vgpr_bound(VGPRS_BEFORE[name]), (name, vgprs)
        found.append(hits[0])
    return found
