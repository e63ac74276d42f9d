#!/usr/bin/env python3
"""Digest of every gfx950 kernel in a HIP shared library: one line per kernel, sorted by name -

    <mangled name>  text:<sha256 of the kernel's .text bytes>  kd:<sha256 of its 64-byte kernel descriptor>

Two listings diffed answer "which kernels did this change touch?" without a GPU: equal digests are the same machine code with
the same registers, LDS, scratch and occupancy hints.  It hashes bytes and looks at no instruction.  The descriptor is hashed
with KERNEL_CODE_ENTRY_BYTE_OFFSET (its bytes 16 - 23: the distance from the descriptor to the code) zeroed - that field
moves with every kernel laid out in front of this one and says nothing about the kernel itself.

    python tools/kernel_digest.py diffsound_amd/csrc/libdiffsound_hip.so > after.txt
"""
import hashlib
import os
import shutil
import struct
import subprocess
import sys
import tempfile


def gfx950_code_objects(lib_path):
    """The gfx950 code objects inside a HIP shared library: the .hip_fatbin section is a sequence of clang offload
    bundles (one per translation unit: magic, entry count, then (offset, size, triple) records)."""
    data = open(lib_path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos, out = data.find(magic), []
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(magic))
        p = pos + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(magic, pos + len(magic))
    return out


def kernel_digests(blob, readelf):
    """{kernel name: (sha256 of its code, sha256 of its descriptor)} of one code object (an ELF in memory)."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(blob)
        f.flush()
        text = subprocess.run([readelf, "-S", "-s", "-W", f.name], capture_output=True, text=True, check=True).stdout
    sections, symbols = {}, {}  # index -> (address, file offset); name -> (value, size, type, section index)
    for line in text.splitlines():
        t = line.replace("[", " ").replace("]", " ").split()
        if line.lstrip().startswith("[") and len(t) >= 6 and t[0].isdigit() and t[1] != "NULL":
            sections[int(t[0])] = (int(t[3], 16), int(t[4], 16))
        elif len(t) >= 8 and t[0].endswith(":") and t[3] in ("FUNC", "OBJECT") and t[6].isdigit():
            symbols[line.split(None, 7)[7]] = (int(t[1], 16), int(t[2]), t[3], int(t[6]))

    def content(name):
        value, size, _, shndx = symbols[name]
        addr, offset = sections[shndx]
        return blob[value - addr + offset:value - addr + offset + size]

    def sha(b):
        return hashlib.sha256(b).hexdigest()

    out = {}
    for k, v in symbols.items():
        if v[2] == "FUNC" and k + ".kd" in symbols:
            kd = content(k + ".kd")
            assert len(kd) == 64, (k, len(kd))
            out[k] = (sha(content(k)), sha(kd[:16] + bytes(8) + kd[24:]))
    return out


def main(argv):
    args = [a for a in argv if not a.startswith("-")]
    if len(args) != 1:
        sys.exit(__doc__)
    readelf = shutil.which("llvm-readelf") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib/llvm/bin/llvm-readelf")
    found = {}
    for blob in gfx950_code_objects(args[0]):
        found.update(kernel_digests(blob, readelf))
    print("\n".join(f"{k}  text:{t}  kd:{d}" for k, (t, d) in sorted(found.items())))


if __name__ == "__main__":
    main(sys.argv[1:])
