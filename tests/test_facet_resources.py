"""The facet kernels' resources, from the compiler's own report (no GPU needed).

`facet_counts_kernel` keeps a thread's 32 codes in registers (an array indexed by an unrolled loop counter; indexed by a
runtime value it would move to scratch), and its on-chip instantiations hold the LDS histograms whose size fixes how many
workgroups a CU can hold.  csrc/device_facets.h is compiled alone, device side only, with the library's flags and
`-Rpass-analysis=kernel-resource-usage`, as tests/test_tags_resources.py does (DESIGN.md section 4 records the figures)."""
import re
import subprocess

from cphnsw_mi355x import build as b

LDS_PER_CU = 160 * 1024
BLOCKS_PER_CU = 4            # device_facets.h: kFacetBlocksPerCu, the residency the on-chip bin limit was chosen for


def test_facet_kernels_have_no_scratch_no_spills_and_fit_their_lds(tmp_path):
    src = tmp_path / "facets_only.hip"
    src.write_text('#include "device_facets.h"\n'
                   "static_assert(cph::kFacetBlocksPerCu == %d, \"the test and the header disagree\");\n"
                   "static_assert(cph::kFacetLdsBins * 4 * cph::kFacetBlocksPerCu <= %d, \"bins x blocks exceed a CU's LDS\");\n"
                   % (BLOCKS_PER_CU, LDS_PER_CU))
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [b._hipcc()] + flags + ["-I", b.CSRC, "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "facets_only.o"),
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
            got[name] = {}
        elif name:
            got[name][m.group(1)] = int(m.group(2))
    counting = {k: v for k, v in got.items() if "facet_counts_kernel" in k}
    top = {k: v for k, v in got.items() if "facet_top_kernel" in k}
    for k, v in {**counting, **top}.items():
        print(k, v)
    assert len(counting) == 4 and len(top) == 1, log[-2000:]         # dense / tags x on-chip / global, and the selection
    for k, v in {**counting, **top}.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] <= LDS_PER_CU // BLOCKS_PER_CU, (k, v)
    assert sorted(v["LDS Size [bytes/block]"] for v in counting.values())[:2] == [0, 0]      # the global path holds no LDS
