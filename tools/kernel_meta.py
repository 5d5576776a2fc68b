#!/usr/bin/env python3
"""Per-kernel resource usage of a built liblbk8s.so (or of one unit's object file), read from its
gfx950 code objects (no rebuild): VGPRs, AGPRs, SGPRs, spills, scratch and LDS bytes.

    python tools/kernel_meta.py exp/liblbk8s_x.so [name-substring ...]

--code adds, per kernel, the instruction count and a hash of its normalised disassembly, so two
builds can be compared kernel by kernel (the same source in another unit must give the same code).
The normalisation is two rules: the padding after the kernel's last instruction is dropped (the
run of `s_nop 0` / `...` the last function of a code object gets), and the literals of the
s_add_u32 / s_addc_u32 pair that directly follows an s_getpc_b64, on its registers, are masked (pc-relative addresses of read-only
tables, which move with the unit's layout).  --json prints the rows as one JSON list.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("name", "vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size")


def normalised(lines):
    """The instructions of one kernel (llvm-objdump lines) under the two rules above."""
    out, pair = [], []  # pair: the two instructions expected right after an s_getpc_b64 s[lo:hi]
    for line in lines:
        ins = line.split("//")[0].strip()  # (without the address and the encoding)
        if not ins:
            continue
        m = re.fullmatch(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
        if m:
            lo, hi = m.groups()
            pair = [f"s_add_u32 s{lo}, s{lo}, ", f"s_addc_u32 s{hi}, s{hi}, "]
        elif pair:  # only the pair that follows directly, on the getpc's own registers
            want = pair.pop(0)
            if ins.startswith(want):
                ins = want + "<pcrel>"
            else:
                pair = []
        out.append(ins)
    while out and out[-1] in ("s_nop 0", "..."):
        out.pop()
    return out


def code(co):
    """{symbol: (instruction count, hash)} of every function of a code object."""
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True,
                          check=True).stdout
    out, name, body = {}, None, []

    def close():
        if name is not None:
            ins = normalised(body)
            out[name] = (len(ins), hashlib.sha256("\n".join(ins).encode()).hexdigest()[:16])

    for line in text.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            close()
            name, body = m.group(1), []
        elif name is not None:
            body.append(line)
    close()
    return out


def kernels(lib, with_code=False):
    out = []
    with tempfile.TemporaryDirectory() as d:
        fb = os.path.join(d, "fb.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", lib, os.path.join(d, "x")],
                       check=True)
        data = open(fb, "rb").read()
        starts = [i for i in range(len(data)) if data.startswith(MAGIC, i)]
        for n, a in enumerate(starts):  # (one bundle per compiled unit)
            b = starts[n + 1] if n + 1 < len(starts) else len(data)
            part, co = os.path.join(d, f"b{n}.bin"), os.path.join(d, f"co{n}.o")
            open(part, "wb").write(data[a:b])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--input={part}", f"--output={co}", "--unbundle"], check=True)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True,
                                   check=True).stdout
            unit = parse_notes(notes)
            if with_code:
                fns = code(co)
                for k in unit:
                    k["instructions"], k["code_hash"] = fns[k["name"]]
            out += unit
    return out


def parse_notes(notes):
    out, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "agpr_count" and line.lstrip().startswith("-"):
            cur = {}
            out.append(cur)
        if cur is None:
            continue
        if k in FIELDS:
            cur.setdefault(k, v)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("lib", help="liblbk8s.so or a unit's object file")
    ap.add_argument("patterns", nargs="*", help="kernel name substrings")
    ap.add_argument("--code", action="store_true", help="instruction count and normalised code hash per kernel")
    ap.add_argument("--json", action="store_true", help="one JSON list in place of the text lines")
    args = ap.parse_args()
    lib, pats, with_code, as_json = args.lib, args.patterns, args.code, args.json
    rows =[k for k in kernels(lib, with_code) if not pats or any(p in k.get("name", "?") for p in pats)]
    if as_json:
        print(json.dumps(rows, indent=0))
        return
    for k in rows:
        n = k.get("name", "?")
        tail = f" n={k['instructions']} code={k['code_hash']}" if with_code else ""
        print(f"{n if with_code else n[:90]:90s} v={k.get('vgpr_count')} a={k.get('agpr_count')} s={k.get('sgpr_count')} "
              f"vspill={k.get('vgpr_spill_count')} sspill={k.get('sgpr_spill_count')} "
              f"scratch={k.get('private_segment_fixed_size')} lds={k.get('group_segment_fixed_size')}{tail}")


if __name__ == "__main__":
    main()
