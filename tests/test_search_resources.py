"""The register budget of the benchmark's search kernel, from the compiler's own report (no GPU needed).

`search_kernel<4, 128, true>` -- 4-bit codes, D = 128, probe first: the launch a C2 step consists of -- runs six waves
per SIMD, which takes 80 VGPRs or fewer; it has carried 8 spilled VGPRs and a frame of 68 bytes per lane since the
upper-layer descent moved into the encoder, all of them outside the expansion loop (`scripts/loop_reloads.py` on the
assembly shows that; this test reads the resource remarks only).  The instantiation is compiled alone, device side
only, with the library's flags and `-Rpass-analysis=kernel-resource-usage`; the rows of all
instantiations in the library build are in `profiles/issue_diet.md`.
"""
import re
import subprocess

from cphnsw_mi355x import build as b

KERNEL = "_ZN3cph13search_kernelILi4ELi128ELb1ELb0ELb0EEEvNS_10SearchArgsE"


def test_search_kernel_c2_keeps_six_waves_and_its_frame(tmp_path):
    src = tmp_path / "search_one.hip"
    src.write_text('#include "device_search.h"\n'
                   "template __global__ void cph::search_kernel<4, 128, true, false, false>(cph::SearchArgs);\n")
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [b._hipcc()] + flags + ["-I", b.CSRC, "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "search_one.o"),
                                  "-Rpass-analysis=kernel-resource-usage"]
    log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    got, name = {}, None
    for line in log.splitlines():
        m = re.search(r"remark:.*?\s(Function Name|VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
        elif name == KERNEL:
            got[m.group(1)] = int(m.group(2))
    print("search_kernel<4,128,true>:", got)
    assert got, log[-2000:]
    assert got["VGPRs"] <= 80, got
    assert got["Occupancy [waves/SIMD]"] >= 6, got
    assert got["VGPRs Spill"] <= 8, got
    assert got["ScratchSize [bytes/lane]"] <= 68, got
