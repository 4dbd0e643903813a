#!/usr/bin/env python3
"""Registers, LDS and scratch of every k_doc_completion instantiation, from the
kernel descriptors of the built library's gfx950 code object (walked as
ldagibbssampling_amd/codeobj.py walks it).  Exits 1 if one uses scratch.

  python tools/heldout_isa.py [path/to/liblda_mi355x.so]
"""
import os
import re
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ldagibbssampling_amd import capi, codeobj  # noqa: E402


def describe(kd: bytes) -> dict:
    """The fields of an amdhsa kernel descriptor (64 bytes) used here."""
    lds, scratch = struct.unpack_from("<II", kd, 0)
    rsrc3, rsrc1, rsrc2 = struct.unpack_from("<III", kd, 44)
    vgprs = ((rsrc1 & 0x3F) + 1) * 8            # unified VGPR + AGPR file, granule 8
    accum_offset = ((rsrc3 & 0x3F) + 1) * 4     # first AGPR: the architected VGPRs
    return {"vgprs_total": vgprs, "arch_vgprs": accum_offset, "lds_bytes": lds, "scratch_bytes": scratch,
            "scratch_enabled": bool(rsrc2 & 1)}


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else capi.LIB_PATH
    ks = codeobj.kernels(codeobj.device_code_object(lib))
    pre = codeobj.mangled_prefix("k_doc_completion")
    rows = []
    for name, (text, kd) in ks.items():
        m = re.match(re.escape(pre) + r"ILi(\d+)ELi(\d+)E", name)
        if m and kd:
            rows.append((int(m.group(1)), int(m.group(2)), len(text), describe(kd)))
    if not rows:
        sys.exit(f"{lib}: no k_doc_completion kernel")
    bad = False
    print("| C | T | arch VGPRs | VGPRs + AGPRs | LDS B | scratch B | text B |")
    print("|---|---|---|---|---|---|---|")
    for C, T, size, d in sorted(rows):
        print(f"| {C} | {T} | {d['arch_vgprs']} | {d['vgprs_total']} | {d['lds_bytes']} | {d['scratch_bytes']} | {size} |")
        bad |= d["scratch_bytes"] != 0 or d["scratch_enabled"]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
