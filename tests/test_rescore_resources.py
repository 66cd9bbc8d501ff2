"""The register budget of the two-stage search kernels, from the compiler's own report (no GPU needed).

The four kernels of csrc/device_rescore.h -- rescore_rows_kernel and rescore_rows_in_kernel, each for float16 and float32
storage -- are compiled alone, device side only, with the library's flags and `-Rpass-analysis=kernel-resource-usage`.  None
may use scratch or spill a VGPR; the occupancy found is recorded in DESIGN.md section 4.  Only the compiler's remarks are
read.
"""
import re
import subprocess

from cphnsw_mi355x import build as b

KERNELS = ("rescore_rows_kernel", "rescore_rows_in_kernel")


def test_rescore_kernels_use_no_scratch(tmp_path):
    src = tmp_path / "rescore_only.hip"
    src.write_text('#include "device_rescore.h"\n'
                   "template __global__ void cph::rescore_rows_kernel<false>(cph::RescoreArgs);\n"
                   "template __global__ void cph::rescore_rows_kernel<true>(cph::RescoreArgs);\n"
                   "template __global__ void cph::rescore_rows_in_kernel<false>(const float*, uint64_t, uint64_t, const uint32_t*, "
                   "cph::RescoreStore, uint8_t*, float*, unsigned long long*);\n"
                   "template __global__ void cph::rescore_rows_in_kernel<true>(const float*, uint64_t, uint64_t, const uint32_t*, "
                   "cph::RescoreStore, uint8_t*, float*, unsigned long long*);\n")
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [b._hipcc()] + flags + ["-I", b.CSRC, "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "rescore_only.o"),
                                  "-Rpass-analysis=kernel-resource-usage"]
    log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    got, name = {}, None
    for line in log.splitlines():
        m = re.search(r"remark:.*?\s(Function Name|VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
        elif name and any(kn in name for kn in KERNELS):
            got.setdefault(name, {})[m.group(1)] = int(m.group(2))
    for name, g in sorted(got.items()):
        print(name, g)
    assert len(got) == 4 and all(sum(kn in name for name in got) == 2 for kn in KERNELS), (sorted(got), log[-2000:])
    for name, g in got.items():
        assert g["VGPRs Spill"] == 0 and g["ScratchSize [bytes/lane]"] == 0, (name, g)
