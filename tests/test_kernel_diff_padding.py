"""tools/kernel_diff.py and the padding behind a symbol: a kernel that was the section's last symbol is followed, once
kernels are added behind it, by alignment padding. llvm-objdump folds a run of zero bytes into "...", but prints a
single zero dword as the instruction it decodes to (encoding 00000000). Neither is code of the symbol."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_diff  # noqa: E402

HEAD = ["", "dev.co:\tfile format elf64-amdgpu", "", "Disassembly of section .text:", ""]
LAST = ["\tglobal_store_dwordx4 v[4:5], v[0:3], off                   // 0000002EDAEC: DC7C8000 007F0004",
        "\ts_endpgm                                                   // 0000002EDAF4: BF810000",
        "\ts_branch 62224                                             // 0000002EDAF8: BF82F310 <_Z1kPf+0x63c>"]
PAD = "\tv_cndmask_b32_e32 v0, s0, v0, vcc                          // 0000002EDAFC: 00000000"
NEXT = ["0000000000000b00 <_Z3newPf>:", "\ts_endpgm                                                   // 000000000B00: BF810000", ""]


def test_one_zero_dword_of_padding_is_no_code():
    a = "\n".join(HEAD + ["00000000002e0000 <_Z1kPf>:"] + LAST + [""])
    b = "\n".join(HEAD + ["00000000002e0000 <_Z1kPf>:"] + LAST + [PAD, ""] + NEXT)
    assert kernel_diff.compare(a, b) == (2, [("_Z3newPf", "missing in A")])


def test_padding_runs_and_single_dwords_mix():
    b = "\n".join(HEAD + ["00000000002e0000 <_Z1kPf>:"] + LAST + [PAD, "\t...", ""] + NEXT)
    assert kernel_diff.symbols(b)["_Z1kPf"] == kernel_diff.symbols("\n".join(HEAD + ["00000000002e0000 <_Z1kPf>:"] + LAST))["_Z1kPf"]


def test_a_changed_last_instruction_still_counts():
    a = "\n".join(HEAD + ["00000000002e0000 <_Z1kPf>:"] + LAST + [""])
    b = "\n".join(HEAD + ["00000000002e0000 <_Z1kPf>:"] + LAST[:2] + [""])
    n, diffs = kernel_diff.compare(a, b)
    assert n == 1 and len(diffs) == 1 and "3 / 2 instructions" in diffs[0][1]
