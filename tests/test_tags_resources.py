"""The tag kernel's resources, from the compiler's own report (no GPU needed).

`tag_filters_kernel` keeps a lane's row bounds of its four 64-row groups in registers (an array indexed by an unrolled
loop counter); indexed by a runtime value that array would move to scratch.  The kernel is compiled alone, device side
only, with the library's flags and `-Rpass-analysis=kernel-resource-usage`, as tests/test_encode_resources.py does
(DESIGN.md section 4 records the figures)."""
import re
import subprocess

from cphnsw_mi355x import build as b


def test_tag_kernel_has_no_scratch_and_no_spills(tmp_path):
    src = tmp_path / "tags_only.hip"
    src.write_text('#include "device_tags.h"\n')
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [b._hipcc()] + flags + ["-I", b.CSRC, "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "tags_only.o"),
                                  "-Rpass-analysis=kernel-resource-usage"]
    log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    got, name = {}, None
    keys = r"Function Name|TotalSGPRs|VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]"
    for line in log.splitlines():
        m = re.search(r"remark:.*?\s(" + keys + r"): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
        elif name and "tag_filters_kernel" in name:
            got[m.group(1)] = int(m.group(2))
    print("tag_filters_kernel:", got)
    assert got, log[-2000:]
    assert got["VGPRs Spill"] == 0 and got["ScratchSize [bytes/lane]"] == 0, got
    assert got["SGPRs Spill"] == 0, got
    assert got["LDS Size [bytes/block]"] <= 160 * 1024 // 3, got          # three blocks of four waves share a CU's 160 KiB
