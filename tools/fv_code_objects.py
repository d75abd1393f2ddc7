#!/usr/bin/env python3
"""SHA-256 of the device code (.rodata + .text) of every gfx950 code object in a built libldc_hip.so, one per translation
unit, in link order.

The library is one hipcc line over several units; each unit's device code travels as a clang offload bundle in the
``.hip_fatbin`` section.  Two builds whose lists agree entry for entry run the same device instructions in those units
(the repository's rule: the existing kernels "must not change by an instruction" when a unit is added beside them).
The kernel names of each code object are listed so that an entry can be told from the next.

Usage:  python tools/fv_code_objects.py LIB [OTHER_LIB]      (two libraries: the entries of the first that the second lacks)
"""
from __future__ import annotations

import hashlib
import re
import struct
import sys
from pathlib import Path

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def text_section(obj):
    """The bytes of the ``.rodata`` (kernel descriptors: registers, LDS, scratch) and ``.text`` (instructions) sections of an
    ELF64 code object, without the symbol and hash tables: every unit carries a ``__hip_cuid_`` symbol whose name is hashed
    from the compile line, so the tables of ALL units move when a source file is added to the hipcc line."""
    shoff, = struct.unpack_from("<Q", obj, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", obj, 0x3A)
    sec = [struct.unpack_from("<IIQQQQ", obj, shoff + k * shentsize) for k in range(shnum)]
    stroff = sec[shstrndx][4]
    found = {}
    for name, _, _, _, off, size in sec:
        end = obj.index(b"\0", stroff + name)
        found[obj[stroff + name: end]] = obj[off: off + size]
    if b".text" not in found:
        raise ValueError("no .text section")
    return found.get(b".rodata", b"") + found[b".text"]


def code_objects(path):
    """[(sha256 of .rodata + .text, bytes of the object, a few kernel names)] of the gfx950 entries, in file order."""
    blob = Path(path).read_bytes()
    out = []
    for m in re.finditer(re.escape(MAGIC), blob):
        base = m.start()
        pos = base + len(MAGIC)
        (count,) = struct.unpack_from("<Q", blob, pos)
        pos += 8
        if not 0 < count < 64:
            continue
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            pos += 24
            triple = blob[pos: pos + tlen].decode("ascii", "replace")
            pos += tlen
            if "gfx950" not in triple or size == 0:
                continue
            obj = blob[base + off: base + off + size]
            names = sorted(set(re.findall(rb"_Z[A-Za-z0-9_]*kernel[A-Za-z0-9_]*", obj)))
            if obj[:4] != b"\x7fELF":
                raise ValueError(f"{path}: a gfx950 entry that is not an ELF object (compressed bundle?)")
            out.append((hashlib.sha256(text_section(obj)).hexdigest(), size, [n.decode() for n in names[:3]]))
    return out


def main(argv):
    if not 1 <= len(argv) <= 2:
        raise SystemExit(__doc__)
    mine = code_objects(argv[0])
    for h, size, names in mine:
        print(h, size, " ".join(names))
    if len(argv) == 2:
        theirs = {h for h, _, _ in code_objects(argv[1])}
        missing = [h for h, _, _ in mine if h not in theirs]
        print(f"{len(mine)} code objects, {len(missing)} not in {argv[1]}")
        for h in missing:
            print("  only here:", h)
        return 1 if missing else 0
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
