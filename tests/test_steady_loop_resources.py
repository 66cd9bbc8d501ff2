"""Register budgets of the search kernel's other probe-first instantiations, from the compiler's own report (no GPU needed).

The expansion loop's body is compiled twice where that pays (general and steady loop, csrc/device_search.h); neither
the second copy nor the edits that came with it may cost the kernels that sit on their register limit a register or a
wave.  `tests/test_search_resources.py` holds `<4,128,true>`; here `<4,1024,true>` (C3), `<2,128,true>` and
`<1,128,true>` are compiled alone, device side only, with the library's flags and
`-Rpass-analysis=kernel-resource-usage`, and held to the figures they had before the loop was split
(profiles/steady_loop.md): 159 VGPRs / 3 waves per SIMD, 78 / 6 and 79 / 6.
"""
import re
import subprocess

import pytest

from cphnsw_mi355x import build as b

CEILINGS = {(4, 1024): (159, 3), (2, 128): (78, 6), (1, 128): (79, 6)}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("steady_res")
    src = tmp / "search_three.hip"
    src.write_text('#include "device_search.h"\n' + "".join(
        f"template __global__ void cph::search_kernel<{bw}, {sd}, true, false, false>(cph::SearchArgs);\n"
        for bw, sd in CEILINGS))
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [b._hipcc()] + flags + ["-I", b.CSRC, "--cuda-device-only", "-c", str(src), "-o", str(tmp / "search_three.o"),
                                  "-Rpass-analysis=kernel-resource-usage"]
    log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    got, name = {}, None
    for line in log.splitlines():
        m = re.search(r"remark:.*?\s(Function Name|VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
        elif name is not None:
            got.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert got, log[-2000:]
    return got


@pytest.mark.parametrize("bw,sd", sorted(CEILINGS))
def test_probe_first_instantiation_keeps_its_registers_and_waves(usage, bw, sd):
    kernel = f"_ZN3cph13search_kernelILi{bw}ELi{sd}ELb1ELb0ELb0EEEvNS_10SearchArgsE"
    vgprs, waves = CEILINGS[(bw, sd)]
    got = usage[kernel]
    print(f"search_kernel<{bw},{sd},true>:", got)
    assert got["VGPRs"] <= vgprs, got
    assert got["Occupancy [waves/SIMD]"] >= waves, got
