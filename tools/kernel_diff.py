#!/usr/bin/env python3
"""Symbol-by-symbol comparison of the device code of two built librt4.so: the check of a refactoring that must
not change the device code by one instruction (on the CPU; no GPU needed).

For every symbol of the device code object (not only the trace kernels) the instruction text is compared with
the absolute address comments stripped; the `<sym+0x..>` branch targets stay. For every kernel the resource
fields of the code object's metadata note are compared too: VGPR, SGPR and AGPR counts, LDS size
(group_segment_fixed_size), private segment size and the spill counts.

Usage: python tools/kernel_diff.py [--arch gfxNNN] A.so B.so
Prints each differing or missing symbol, then `identical N of N`; exit status 1 if any differs.
The code object is taken out of each library as tools/codegen_check.py does it ($ROCM_LLVM_BIN)."""
import re
import subprocess
import sys
import tempfile

import codegen_check

ADDR_COMMENT = re.compile(r"//\s*[0-9A-Fa-f]+:\s*")
RESOURCES = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
             "vgpr_spill_count", "sgpr_spill_count")


def symbols(dis):
    """{symbol: [instruction text, ...]} of a disassembly (llvm-objdump -d), address comments stripped."""
    out, cur = {}, None
    for ln in dis.splitlines():
        m = codegen_check.HEAD.match(ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.strip() and not ln.startswith("Disassembly of section"):
            cur.append(" ".join(ADDR_COMMENT.sub("// ", ln).split()))
    # objdump prints "..." for the zero bytes that pad a symbol up to the next one: every symbol ends with it except
    # the section's last, which is another symbol once kernels are added behind it. Padding after the code is no code.
    # A single zero dword of padding is not folded into "...": objdump decodes it (v_cndmask_b32 v0, s0, v0, vcc,
    # encoding 00000000). No symbol's code ends in it: the last instruction is s_endpgm or a branch.
    for text in out.values():
        while text and (text[-1] == "..." or text[-1].endswith("// 00000000")):
            text.pop()
    return out


def resources(notes):
    """{kernel: {field: value}} from the AMDGPU metadata note (llvm-readelf --notes): the RESOURCES fields of each
    entry of amdhsa.kernels (the keys at the entries' own indentation; their .args lie deeper)."""
    out, cur, key = {}, None, None
    for ln in notes.splitlines():
        if ln.startswith("amdhsa.kernels:"):
            key = re.compile(r"^  (- |  )\.(\w+):\s*(.*)$")
            continue
        if key is None:
            continue
        if ln and not ln.startswith(" "):  # the next top-level key of the note
            key = None
            continue
        m = key.match(ln)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if m.group(2) == "name":
            out[m.group(3)] = cur
        elif m.group(2) in RESOURCES:
            cur[m.group(2)] = m.group(3)
    return out


def compare(dis_a, dis_b, notes_a="", notes_b=""):
    """(symbols compared, [(symbol, what differs), ...]) of two disassemblies and, when given, the two metadata
    notes. A symbol on one side only is reported as missing; a symbol whose text differs is reported with its first
    differing instruction; a kernel whose resource fields differ is reported with them."""
    a, b = symbols(dis_a), symbols(dis_b)
    ra, rb = resources(notes_a), resources(notes_b)
    diffs = []
    for s in sorted(set(a) | set(b)):
        if s not in a or s not in b:
            diffs.append((s, "missing in " + ("A" if s not in a else "B")))
            continue
        what = []
        if a[s] != b[s]:
            k = next((k for k, (x, y) in enumerate(zip(a[s], b[s])) if x != y), min(len(a[s]), len(b[s])))
            x, y = (t[k] if k < len(t) else "(end)" for t in (a[s], b[s]))
            what.append(f"{len(a[s])} / {len(b[s])} instructions, first difference at #{k}: {x}  |  {y}")
        if ra.get(s) != rb.get(s):
            fa, fb = ra.get(s) or {}, rb.get(s) or {}
            what.append("resources: " + ", ".join(f"{f} {fa.get(f)} / {fb.get(f)}" for f in RESOURCES
                                                  if fa.get(f) != fb.get(f)))
        if what:
            diffs.append((s, "; ".join(what)))
    return len(set(a) | set(b)), diffs


def read(lib, arch="gfx950"):
    """(disassembly, metadata notes) of a library's device code object."""
    with tempfile.TemporaryDirectory() as d:
        co = codegen_check.code_object(lib, d, arch)
        notes = subprocess.run([f"{codegen_check.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        return codegen_check.disassemble_object(co), notes


if __name__ == "__main__":
    argv = sys.argv[1:]
    arch = "gfx950"
    if "--arch" in argv:
        at = argv.index("--arch")
        arch = argv[at + 1]
        del argv[at:at + 2]
    if len(argv) != 2:
        sys.exit(__doc__)
    (dis_a, notes_a), (dis_b, notes_b) = read(argv[0], arch), read(argv[1], arch)
    n, diffs = compare(dis_a, dis_b, notes_a, notes_b)
    for s, what in diffs:
        print(f"{s}: {what}")
    print(f"identical {n - len(diffs)} of {n}")
    sys.exit(1 if diffs or n == 0 else 0)
