"""Build-time guard for k_attn_kvh's software pipeline (csrc/block_attn.hip): between the loads a window
iteration issues for the NEXT windows (rows, first Q' piece, metadata, work-order entry) and the first matrix instruction
of its passes, the shipped code waits for no vector-memory load.  The source keeps the wave-uniform metadata words in
vector registers by a device the compiler is free to see through one day; a compiler that copies them to scalar
registers behind their loads again puts `s_waitcnt vmcnt(..)` there and drains the prefetch every window -- same results,
a slower kernel, and nothing else would notice.  Reads the code objects inside libmssvt_hip.so; needs no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mfma_hazard_check as hz  # noqa: E402

LIB = os.path.join(ROOT, "mssvt_amd", "lib", "libmssvt_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(hz.LLVM_BIN, "llvm-objdump")), reason="no llvm-objdump")

H16 = "v_mfma_f32_16x16x32_f16"


def _is_vmem_load(ins):
    return ins.mnem.startswith("buffer_load") or ins.mnem.startswith("global_load")


def window_loop(instrs):
    """The instructions of the outermost loop: the backward branch that spans the most code."""
    addr = {ins.addr: i for i, ins in enumerate(instrs)}
    back = [(ins.addr - ins.target, addr[ins.target], i) for i, ins in enumerate(instrs)
            if ins.target is not None and ins.target <= ins.addr and ins.target in addr]
    assert back, "no loop"
    _, lo, hi = max(back)
    return instrs[lo:hi + 1]


def waits_between_prefetch_and_first_pass(instrs):
    """[s_waitcnt vmcnt operands] between the last load of the iteration's prefetch cluster and the next K = 32 fp16 matrix
    instruction.  The cluster starts at the first run of four 16-byte buffer loads in the loop (the rows of a window: two
    key tiles x Cg / 16 pieces, four at Cg = 32) and takes in every load of the 100 instructions behind it."""
    loop = window_loop(instrs)
    rows = [i for i, ins in enumerate(loop) if ins.mnem == "buffer_load_dwordx4"]
    start = next(rows[k] for k in range(len(rows) - 3) if rows[k + 3] - rows[k] < 30)
    last = max(i for i in range(start, min(start + 100, len(loop))) if _is_vmem_load(loop[i]))
    first_pass = next(i for i in range(last, len(loop)) if loop[i].mnem.startswith(H16))
    return [ins.ops for ins in loop[last:first_pass] if ins.mnem == "s_waitcnt" and "vmcnt" in ins.ops]


def flagship_kernels():
    out = {}
    for elf in hz.code_objects(LIB):
        for name, instrs in hz.parse_disassembly(hz.disassemble(elf)).items():
            if "k_attn_kvh" in name and name.endswith("ELi2ELb1EEv8AttnPack"):  # <.., KT = 2, QP = true>
                out[name] = instrs
    return out


def test_finder_sees_a_wait_behind_the_prefetch_and_none_when_it_is_gone():
    def listing(wait):
        body = ["buffer_load_dwordx4 v[%d:%d], v1, s[4:7], 0 offen" % (4 * k + 8, 4 * k + 11) for k in range(8)]
        body += ["global_load_dword v60, v2, s[8:9]"] + ([wait] if wait else []) + ["v_readfirstlane_b32 s20, v61"]
        body += [H16 + " v[40:43], v[44:47], v[48:51], 0", "s_cbranch_scc1 65000"]
        lines = ["0000000000000000 <k>:", "\t%-58s // %012X: 00000000" % ("v_mov_b32_e32 v0, 0", 0)]
        for n, text in enumerate(body):
            tail = " <k+0x4>" if text.startswith("s_cbranch") else ""
            lines.append("\t%-58s // %012X: 00000000%s" % (text, 4 * (n + 1), tail))
        lines.append("\t%-58s // %012X: 00000000" % ("s_endpgm", 4 * (len(body) + 1)))
        return hz.parse_disassembly("\n".join(lines) + "\n")["k"]
    assert waits_between_prefetch_and_first_pass(listing("s_waitcnt vmcnt(3)")) == ["vmcnt(3)"]
    assert waits_between_prefetch_and_first_pass(listing("s_waitcnt lgkmcnt(0)")) == []
    assert waits_between_prefetch_and_first_pass(listing(None)) == []


def test_no_vector_memory_wait_between_a_windows_prefetch_and_its_first_pass():
    assert os.path.exists(LIB), "build() first"
    kernels = flagship_kernels()
    assert kernels, "k_attn_kvh<.., 2, true> not found in the library"
    for name, instrs in kernels.items():
        assert waits_between_prefetch_and_first_pass(instrs) == [], name
