"""Register budgets, loop cleanliness and the square root of the two flagship search kernels after the estimator's
diet (csrc/device_fastscan.h: sqrt_in_range and the static-D forms of lower_bounds_split / stage2_est_only), from the
compiler's remarks and the listing only (no GPU needed).

`<4,128,true>` (C2) and `<4,1024,true>` (C3) are each compiled alone, device side only, with the library's flags.  Each
keeps its waves per SIMD (6 and 3), has no more spilled VGPRs than before (7 and 0), and `scripts/loop_reloads.py`
finds no scratch operation inside either copy of its expansion loop.  The generic square root's pre-scale by 2^32
(the literal 0x4f800000, once per loop copy before) is gone from the listing of `<4,128,true>`
(profiles/estimator_valu.md).
"""
import os
import re
import subprocess
import sys

import pytest

from cphnsw_mi355x import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (BW, SD): (waves per SIMD at least, spilled VGPRs at most)
BOUNDS = {(4, 128): (6, 7), (4, 1024): (3, 0)}


@pytest.fixture(scope="module", params=sorted(BOUNDS))
def alone(request, tmp_path_factory):
    bw, sd = request.param
    tmp = tmp_path_factory.mktemp(f"est_res_{bw}_{sd}")
    src = tmp / "search_one.hip"
    src.write_text('#include "device_search.h"\n'
                   f"template __global__ void cph::search_kernel<{bw}, {sd}, true, false, false>(cph::SearchArgs);\n")
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    lst = tmp / "search_one.s"
    cmd = [b._hipcc()] + flags + ["-I", b.CSRC, "--cuda-device-only", "-S", "-gline-tables-only", str(src), "-o", str(lst),
                                  "-Rpass-analysis=kernel-resource-usage"]
    log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    got = {}
    for line in log.splitlines():
        m = re.search(r"remark:.*?\s(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if m:
            got[m.group(1)] = int(m.group(2))
    assert got, log[-2000:]
    return (bw, sd), got, str(lst)


def test_keeps_waves_and_spills(alone):
    (bw, sd), got, _ = alone
    waves, spilled = BOUNDS[(bw, sd)]
    print(f"search_kernel<{bw},{sd},true>:", got)
    assert got["Occupancy [waves/SIMD]"] >= waves, got
    assert got["VGPRs Spill"] <= spilled, got


def test_no_scratch_operation_inside_the_expansion_loops(alone):
    (bw, sd), _, lst = alone
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "loop_reloads.py"), lst],
                         capture_output=True, text=True, check=True).stdout
    print(out)
    counts = [int(x) for x in re.findall(r"in-loop scratch ops: (\d+)", out)]
    assert counts == [0], out
    text = open(lst).read()
    assert len(re.findall(r"=>\s+This Loop Header: Depth=2", text)) >= 2


def test_square_root_has_no_prescale(alone):
    _, _, lst = alone          # (in both listings)
    text = open(lst).read()
    assert "v_sqrt_f32" in text
    assert "0x4f800000" not in text
