#!/usr/bin/env python3
"""How the hot loops of a gfx950 listing (make asm UNIT=...) lie in memory: for every innermost loop of at least 300 VALU
instructions, how many of its instructions cross a 16-, 32- and 64-byte boundary.  Most of a calm loop is 8-byte encodings
(v_pk_*); a 4-byte one (v_rcp_f32, v_add_f32_e32, SALU) in front shifts every 8-byte instruction after it across the
boundaries until the next 4-byte one shifts them back.  An observation, not an established mechanism: over the builds of
one session (profiles/r10_calm_runs_ab.txt section 4) the calm loops with 35 - 37 such crossings of 16-byte boundaries ran
the headline batch 5 - 8 % faster than those with 80 - 143, but those builds also differ in instruction order.  Runs on
the build box: assembles the listing (clang, local labels kept) and reads the addresses back (llvm-objdump).

usage: isa_fetch_straddles.py file.s [rocm-llvm-bin-dir]"""
import os
import re
import subprocess
import sys
import tempfile

src = sys.argv[1]
llvm = sys.argv[2] if len(sys.argv) > 2 else "/opt/rocm/llvm/bin"
with tempfile.TemporaryDirectory() as tmp:
    obj = os.path.join(tmp, "listing.o")
    subprocess.check_call([os.path.join(llvm, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950",
                           "-Wa,-L", "-c", src, "-o", obj])
    dis = subprocess.check_output([os.path.join(llvm, "llvm-objdump"), "-d", obj]).decode().splitlines()

kernels, items, label = [], None, None
for line in dis:
    m = re.match(r'^[0-9a-f]+ <(.*)>:', line)
    if m:
        label = m.group(1)
        if label.startswith("_ZN5grail") and "synth_kernel" in label:
            items = []
            kernels.append((label, items))
        continue
    m = re.match(r'^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*((?:[0-9A-Fa-f]{8}\s*)+)', line)
    if m and items is not None:
        items.append((int(m.group(3), 16), 4 * len(m.group(4).split()), m.group(1), m.group(2), label))
        label = None

for ki, (name, ins) in enumerate(kernels):
    loops = []
    for i, x in enumerate(ins):
        if x[2].startswith("s_cbranch"):
            m = re.search(r'(\.LBB[0-9_]+)', x[3])
            head = [q for q in range(i, -1, -1) if m and ins[q][4] == m.group(1)]
            if head:
                loops.append((head[0], i))
    inner = [lp for lp in loops if not any(o is not lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
    print("kernel", ki, re.sub(r'.*synth_kernelI', 'synth_kernel<', name)[:80])
    for a, b in inner:
        body = ins[a:b + 1]
        valu = sum(1 for x in body if x[2].startswith("v_"))
        if valu < 300:
            continue
        cross = [sum(1 for x in body if x[0] // n != (x[0] + x[1] - 1) // n) for n in (16, 32, 64)]
        short = sum(1 for x in body if x[1] == 4)
        stores = ",".join(sorted(set(x[2] for x in body if x[2].startswith(("ds_write", "global_store"))))) or "-"
        print("   loop %-10s valu %4d, %4d instructions (%3d of 4 bytes), %5d bytes, stores %-22s crossing 16 / 32 / 64 bytes: %3d / %3d / %3d"
              % (ins[a][4], valu, len(body), short, body[-1][0] + body[-1][1] - body[0][0], stores, cross[0], cross[1], cross[2]))
