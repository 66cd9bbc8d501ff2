"""The query encoder's register budget, from the compiler's own report (no GPU needed).

An `encode_kernel` wave runs next to a full house of `search_kernel<4,128>` waves, which are allocated 80 VGPRs each
(6 per SIMD).  At 80 or fewer it takes exactly the registers one search wave frees; above, it displaces two.  The
kernel is compiled alone, device side only, with the library's flags and `-Rpass-analysis=kernel-resource-usage`
(DESIGN.md section 4); the figures of the full library build are in `profiles/descent_hops.md`.
"""
import os
import re
import subprocess

from cphnsw_mi355x import build as b


def test_encode_kernel_fits_a_search_waves_registers(tmp_path):
    src = tmp_path / "encode_only.hip"
    src.write_text('#include "device_encode.h"\n')
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [b._hipcc()] + flags + ["-I", b.CSRC, "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "encode_only.o"),
                                  "-Rpass-analysis=kernel-resource-usage"]
    log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    got, name = {}, None
    for line in log.splitlines():
        m = re.search(r"remark:.*?\s(Function Name|VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
        elif name and "encode_kernel" in name:
            got[m.group(1)] = int(m.group(2))
    print("encode_kernel:", got)
    assert got, log[-2000:]
    assert got["VGPRs"] <= 80, got
    assert got["VGPRs Spill"] == 0 and got["ScratchSize [bytes/lane]"] == 0, got
    assert got["Occupancy [waves/SIMD]"] >= 6, got
