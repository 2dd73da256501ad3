"""tools/kernel_diff.py: the symbol-by-symbol comparison of two libraries' device code, on synthetic disassembly
(the form llvm-objdump -d prints for a gfx950 code object) and metadata notes (llvm-readelf --notes)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_diff  # noqa: E402


def _dis(base, body_k, with_helper=True):
    """Two symbols (three with the helper) laid out from address base."""
    lines = ["", "dev.co:\tfile format elf64-amdgpu", "", "Disassembly of section .text:", ""]
    addr = base
    syms = [("_Z1kPf", body_k), ("_Z1gPf", ["s_waitcnt lgkmcnt(0)", "s_endpgm"])]
    if with_helper:
        syms.append(("__helper", ["v_mov_b32_e32 v0, 0", "s_setpc_b64 s[30:31]"]))
    for name, body in syms:
        lines.append(f"{addr:016x} <{name}>:")
        for text in body:
            lines.append(f"\t{text:58s} // {addr:012X}: BF8CC07F" + (f" <{name}+0x8>" if "cbranch" in text else ""))
            addr += 4
        lines.append("")
    return "\n".join(lines)


BODY = ["s_load_dword s3, s[0:1], 0x14", "s_cbranch_execz 1", "v_add_u32_e32 v0, s2, v0", "s_endpgm"]


def _notes(vgprs_k, lds_k=0):
    def entry(name, vgprs, lds):
        return "\n".join([
            "  - .agpr_count:     0",
            "    .args:",
            "      - .address_space:  global",
            "        .name:           out",  # an argument's name, deeper than the kernel's own keys
            "        .offset:         0",
            f"    .group_segment_fixed_size: {lds}",
            f"    .name:           {name}",
            "    .private_segment_fixed_size: 0",
            "    .sgpr_count:     25",
            "    .sgpr_spill_count: 0",
            f"    .symbol:         {name}.kd",
            f"    .vgpr_count:     {vgprs}",
            "    .vgpr_spill_count: 0",
        ])
    return "\n".join(["Displaying notes found in: .note", "    AMDGPU Metadata:", "        ---", "amdhsa.kernels:",
                      entry("_Z1kPf", vgprs_k, lds_k), entry("_Z1gPf", 4, 0), "amdhsa.target:   amdgcn-amd-amdhsa--gfx950",
                      "amdhsa.version:", "  - 1", "  - 2", "..."])


def test_address_comments_do_not_count():
    # the same code linked at another address: every symbol identical, helper functions included
    n, diffs = kernel_diff.compare(_dis(0x2E200, BODY), _dis(0x31000, BODY), _notes(12), _notes(12))
    assert (n, diffs) == (3, [])


def test_branch_targets_count():
    a = _dis(0x2E200, BODY)
    n, diffs = kernel_diff.compare(a, a.replace("<_Z1kPf+0x8>", "<_Z1kPf+0xc>"))
    assert n == 3 and [s for s, _ in diffs] == ["_Z1kPf"]


def test_changed_instruction_is_reported_under_its_symbol():
    changed = BODY[:2] + ["v_add_u32_e32 v1, s2, v0"] + BODY[3:]
    n, diffs = kernel_diff.compare(_dis(0x2E200, BODY), _dis(0x2E200, changed), _notes(12), _notes(12))
    assert n == 3 and len(diffs) == 1
    sym, what = diffs[0]
    assert sym == "_Z1kPf"
    assert "first difference at #2" in what and "v_add_u32_e32 v0, s2, v0" in what and "v_add_u32_e32 v1, s2, v0" in what


def test_added_instruction_is_reported():
    n, diffs = kernel_diff.compare(_dis(0x2E200, BODY), _dis(0x2E200, BODY[:3] + ["s_nop 0"] + BODY[3:]))
    assert [s for s, _ in diffs] == ["_Z1kPf"] and "4 / 5 instructions" in diffs[0][1]


def test_symbol_on_one_side_only_is_reported():
    a, b = _dis(0x2E200, BODY), _dis(0x2E200, BODY, with_helper=False)
    assert kernel_diff.compare(a, b) == (3, [("__helper", "missing in B")])
    assert kernel_diff.compare(b, a) == (3, [("__helper", "missing in A")])


def test_resource_fields_count():
    a = _dis(0x2E200, BODY)
    n, diffs = kernel_diff.compare(a, a, _notes(12, 1024), _notes(16, 2048))
    assert n == 3 and [s for s, _ in diffs] == ["_Z1kPf"]
    assert "vgpr_count 12 / 16" in diffs[0][1] and "group_segment_fixed_size 1024 / 2048" in diffs[0][1]


def test_resources_reads_the_kernels_own_keys():
    r = kernel_diff.resources(_notes(12, 1024))
    assert sorted(r) == ["_Z1gPf", "_Z1kPf"]  # not the argument named "out"
    assert r["_Z1kPf"] == {"agpr_count": "0", "group_segment_fixed_size": "1024", "private_segment_fixed_size": "0",
                           "sgpr_count": "25", "sgpr_spill_count": "0", "vgpr_count": "12", "vgpr_spill_count": "0"}
