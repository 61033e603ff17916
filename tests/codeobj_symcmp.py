"""Compare two AMDGPU code objects symbol by symbol: python tests/codeobj_symcmp.py <a.co> <b.co>
(code objects as `llvm-objdump --offloading <object file>` extracts them; LLVM_READELF names the llvm-readelf to use).

Every FUNC / OBJECT symbol must exist in both with the same kind, section, size and bytes.  When the compiler emitted the same kernels
in another order, two things have to change with a kernel's address and are accepted if they changed by exactly that much:
  * the kernel_code_entry_byte_offset of its .kd descriptor (bytes 16..23) = address of the body - address of the descriptor;
  * 32-bit pc-relative literals in its body (references to device globals): shifted by minus the displacement of the body.
Exit status 0: no other difference."""
import os
import re
import shutil
import struct
import subprocess
import sys

READELF = os.environ.get("LLVM_READELF") or shutil.which("llvm-readelf") or "/opt/rocm/llvm/bin/llvm-readelf"


def readelf(flag, path):
    return subprocess.run([READELF, flag, "--wide", path], capture_output=True, text=True, check=True).stdout.splitlines()


def load(path):
    """name -> (type, section name, size, bytes, address) of the FUNC / OBJECT symbols"""
    data = open(path, "rb").read()
    secs = {}
    for line in readelf("-S", path):
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S*)\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs[int(m.group(1))] = (m.group(2), m.group(3), int(m.group(4), 16), int(m.group(5), 16))
    syms = {}
    for line in readelf("-s", path):
        m = re.match(r"\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(.*)$", line)
        if not m or int(m.group(4)) not in secs:
            continue
        addr, size, name = int(m.group(1), 16), int(m.group(2)), m.group(5)
        sname, stype, saddr, soff = secs[int(m.group(4))]
        body = b"" if stype == "NOBITS" else data[soff + addr - saddr: soff + addr - saddr + size]
        syms[name] = (m.group(3), sname, size, body, addr)
    return syms


def moved_descriptor(name, a, b):
    """.kd descriptors equal but for the entry offset, which is body - descriptor in both"""
    body = name[:-3]
    if body not in a or body not in b:
        return False
    da, db = a[name][3], b[name][3]
    off_a, off_b = struct.unpack("<q", da[16:24])[0], struct.unpack("<q", db[16:24])[0]
    return da[:16] == db[:16] and da[24:] == db[24:] and off_a == a[body][4] - a[name][4] and off_b == b[body][4] - b[name][4]


def moved_body(sa, sb):
    """bodies equal but for dwords shifted by the body's displacement; returns how many, or -1"""
    disp = (sa[4] - sb[4]) & 0xffffffff
    n = 0
    for i in range(0, sa[2] - 3, 4):
        wa, wb = struct.unpack_from("<I", sa[3], i)[0], struct.unpack_from("<I", sb[3], i)[0]
        if wa != wb:
            if (wb - wa) & 0xffffffff != disp:
                return -1
            n += 1
    return n


def main(path_a, path_b):
    a, b = load(path_a), load(path_b)
    bad = [("only in first", n) for n in sorted(set(a) - set(b))] + [("only in second", n) for n in sorted(set(b) - set(a))]
    same = kd = rel = lits = 0
    for n in sorted(set(a) & set(b)):
        if a[n][:3] != b[n][:3]:
            bad.append(("kind / section / size", n))
        elif a[n][3] == b[n][3]:
            same += 1
        elif n.endswith(".kd") and moved_descriptor(n, a, b):
            kd += 1
        elif a[n][0] == "FUNC" and moved_body(a[n], b[n]) >= 0:
            rel += 1
            lits += moved_body(a[n], b[n])
        else:
            bad.append(("bytes", n))
    where = [n for n in a if n in b and a[n][4] != b[n][4]]
    print(f"{len(a)} / {len(b)} symbols; {same} byte-identical, {len(where)} at another address; {kd} descriptors equal but for the entry offset; "
          f"{rel} bodies equal but for {lits} pc-relative literals shifted by the body's displacement; {len(bad)} other differences")
    for kind, n in bad[:20]:
        print("  DIFF", kind, n[:150])
    for n in where[:8] if not kd and not rel else []:
        print(f"  moved {n}: {a[n][4]:#x} -> {b[n][4]:#x}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
