"""Build-time guard for the head of k_ffn_ws (csrc/ffn.hip): between the first barrier and the first matrix
instruction -- A(t0) and the start of GEMM1(t0) -- the shipped code waits for no W2 fragment.  W2 is the last group of 16
loads in front of the first barrier; vector loads return in issue order, so `s_waitcnt vmcnt(N)` behind k later loads
leaves W2 in flight exactly when N >= k + 16.  A compiler that moves the bias loads behind W2 again, or a join of two
paths with different load counts, brings such a wait back: same results, a slower launch, and nothing else would notice.
Checked on the table forms at 128 x 256 (the Block launches of the frame; the plain forms branch on the owner list in this
stretch).  Reads the code objects inside libmssvt_hip.so; needs no GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mfma_hazard_check as hz  # noqa: E402

LIB = os.path.join(ROOT, "mssvt_amd", "lib", "libmssvt_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(hz.LLVM_BIN, "llvm-objdump")), reason="no llvm-objdump")

W2_LOADS = 16


def waits_covering_w2(instrs):
    """[(vmcnt, later loads)] of the waits between the first s_barrier and the first matrix instruction that cover a W2 load."""
    first_barrier = next(i for i, ins in enumerate(instrs) if ins.mnem == "s_barrier")
    first_mfma = next(i for i, ins in enumerate(instrs) if ins.mnem.startswith("v_mfma"))
    assert first_barrier < first_mfma
    bad, later = [], 0
    for ins in instrs[first_barrier:first_mfma]:
        if ins.mnem.startswith("global_load") or ins.mnem.startswith("buffer_load"):
            later += 1
        m = re.search(r"vmcnt\((\d+)\)", ins.ops) if ins.mnem == "s_waitcnt" else None
        if m and int(m.group(1)) < later + W2_LOADS:
            bad.append((int(m.group(1)), later))
    return bad


def test_finder_sees_a_wait_that_covers_w2_and_none_when_it_is_counted():
    def listing(wait):
        body = ["global_load_dwordx4 v[%d:%d], v[2:3], off" % (4 * k + 8, 4 * k + 11) for k in range(16)]
        body += ["s_barrier"] + ["global_load_dwordx4 v[%d:%d], v[4:5], off" % (4 * k + 80, 4 * k + 83) for k in range(6)]
        body += [wait, "v_mfma_f32_16x16x32_f16 v[40:43], v[44:47], v[48:51], 0"]
        lines = ["0000000000000000 <k>:"]
        for n, text in enumerate(body + ["s_endpgm"]):
            lines.append("\t%-58s // %012X: 00000000" % (text, 4 * n))
        return hz.parse_disassembly("\n".join(lines) + "\n")["k"]
    assert waits_covering_w2(listing("s_waitcnt vmcnt(8) lgkmcnt(3)")) == [(8, 6)]
    assert waits_covering_w2(listing("s_waitcnt vmcnt(21)")) == [(21, 6)]
    assert waits_covering_w2(listing("s_waitcnt vmcnt(22)")) == []
    assert waits_covering_w2(listing("s_waitcnt lgkmcnt(0)")) == []


def test_no_wait_covers_w2_before_the_first_gemm1():
    assert os.path.exists(LIB), "build() first"
    found = {}
    for elf in hz.code_objects(LIB):
        for name, instrs in hz.parse_disassembly(hz.disassemble(elf)).items():
            if "k_ffn_wsILi128ELi256ELb1E" in name:  # <128, 256, TABBED = true, ..>
                found[name] = instrs
    assert len(found) == 6, sorted(found)  # three table forms x host / device row count
    for name, instrs in found.items():
        assert waits_covering_w2(instrs) == [], name
