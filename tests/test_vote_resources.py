"""Wave votes as mask algebra (csrc/device_search.h: ballot_and / lanes_below; the call sites in
csrc/device_search_expansion.inc), from the compiler's remarks and the listing only (no GPU needed).

`<4,128,true>` (C2) and `<4,1024,true>` (C3) are each compiled alone, device side only, with the library's flags, the
way tests/test_estimator_resources.py does.  The usual steady expansion of `<4,128,true>` is walked with
scripts/isa_trace.py and the decisions of profiles/vote_masks_isa_trace.json (profiles/vote_masks.md, section 2):

* no `v_cndmask_b32 v, 0, 1, s[..]` / `v_cmp_ne_u32 .., 0, v` pair is left on the path (the parent had seven);
* no 64-bit vector compare is left on the path (the parent had the two capacity tests);
* the path's vector instructions: 215 (the parent: 236), 494 issued in all (the parent: 506);
* the whole listing of `<4,128,true>` holds 39 `v_cndmask .., 0, 1` (the parent: 91; what is left sits in the
  spilled-beam routines, which keep their votes), that of `<4,1024,true>` 39.

Waves and spills as in the existing resource tests: 6 and 3 waves per SIMD, at most 7 and 0 spilled VGPRs, no
scratch operation inside either copy of the expansion loop.
"""
import json
import os
import re
import subprocess
import sys

import pytest

from cphnsw_mi355x import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (BW, SD): (waves per SIMD at least, spilled VGPRs at most, `v_cndmask .., 0, 1` in the whole listing at most)
BOUNDS = {(4, 128): (6, 7, 39), (4, 1024): (3, 0, 39)}
PATH_VALU, PATH_TOTAL = 215, 494           # the usual steady expansion of <4,128,true>; the parent: 236, 506
ZERO_ONE = re.compile(r"v_cndmask_b32_e64 v\d+, 0, 1, (s\[\d+:\d+\]|vcc)")


@pytest.fixture(scope="module", params=sorted(BOUNDS))
def alone(request, tmp_path_factory):
    bw, sd = request.param
    tmp = tmp_path_factory.mktemp(f"vote_res_{bw}_{sd}")
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


def _walk(lst):
    """The usual steady expansion of <4,128,true>: (isa_trace's summary line, the instructions executed)."""
    dec = os.path.join(ROOT, "profiles", "vote_masks_isa_trace.json")
    start = json.load(open(dec))["start"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_trace.py"), lst, start, dec, "-v"],
                         capture_output=True, text=True, check=True).stdout
    assert "(default)" not in out, "a branch on the path has no decision:\n" + out[-3000:]
    insts = [l.split(None, 1)[1] for l in out.splitlines() if l.startswith(".LBB")]
    summary = re.search(r"total (\d+)\s+SALU (\d+)\s+VALU (\d+)", out)
    return tuple(int(x) for x in summary.groups()), insts


def test_keeps_waves_and_spills(alone):
    (bw, sd), got, lst = alone
    waves, spilled, _ = BOUNDS[(bw, sd)]
    print(f"search_kernel<{bw},{sd},true>:", got)
    assert got["Occupancy [waves/SIMD]"] >= waves, got
    assert got["VGPRs Spill"] <= spilled, got
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "loop_reloads.py"), lst],
                         capture_output=True, text=True, check=True).stdout
    counts = [int(x) for x in re.findall(r"in-loop scratch ops: (\d+)", out)]
    assert counts == [0], out


def test_zero_one_materialisations_in_the_listing(alone):
    (bw, sd), _, lst = alone
    n = len(ZERO_ONE.findall(open(lst).read()))
    print(f"search_kernel<{bw},{sd},true>: v_cndmask .., 0, 1 in the listing:", n)
    assert n <= BOUNDS[(bw, sd)][2], n          # (the parent: 91 in <4,128,true>)


def test_usual_steady_path(alone):
    (bw, sd), _, lst = alone
    if (bw, sd) != (4, 128):
        return      # the decisions file walks <4,128,true>; <4,1024,true> is held by the two tests above
    (total, salu, valu), insts = _walk(lst)
    print("usual steady expansion: total", total, "SALU", salu, "VALU", valu)
    # no vote goes through 0 / 1 in a VGPR
    for inst in insts:
        assert not ZERO_ONE.match(inst), inst
        assert not re.match(r"v_cmp_\w+_u64", inst), inst
    assert valu <= PATH_VALU, (total, salu, valu)
    assert total <= PATH_TOTAL, (total, salu, valu)
