"""The register budget of the exhaustive int8 rescoring scan, from the compiler's own report (no GPU needed).

csrc/device_rescore_i8_all.h is compiled alone, device side only, with the library's flags and
`-Rpass-analysis=kernel-resource-usage`, as test_rescore_int8_resources.py does.  rescore_i8_all_scan_kernel holds eight
32x32 int32 accumulators per wave: it may use no scratch and spill no VGPR.  The numbers found are recorded in DESIGN.md
section 4.  Only the compiler's remarks are read.
"""
import re
import subprocess

from cphnsw_mi355x import build as b

KERNELS = ("rescore_i8_all_pack_kernel", "rescore_i8_all_scan_kernel", "rescore_i8_all_select_kernel")
FIELDS = "Function Name|VGPRs|AGPRs|VGPRs Spill|ScratchSize \\[bytes/lane\\]|Occupancy \\[waves/SIMD\\]|LDS Size \\[bytes/block\\]"


def test_rescore_all_kernels_use_no_scratch(tmp_path):
    src = tmp_path / "rescore_i8_all_only.hip"
    src.write_text('#include "device_rescore_i8_all.h"\n')
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [b._hipcc()] + flags + ["-I", b.CSRC, "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "rescore_i8_all_only.o"),
                                  "-Rpass-analysis=kernel-resource-usage"]
    log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    got, name = {}, None
    for line in log.splitlines():
        m = re.search(r"remark:.*?\s(" + FIELDS + r"): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
        elif name and any(re.search(r"\d" + kn + "E", name) for kn in KERNELS):
            got.setdefault(name, {})[m.group(1)] = int(m.group(2))
    for name, g in sorted(got.items()):
        print(name, g)
    assert len(got) == 3, (sorted(got), log[-2000:])
    for name, g in got.items():
        assert g["VGPRs Spill"] == 0 and g["ScratchSize [bytes/lane]"] == 0, (name, g)
