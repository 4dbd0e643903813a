#!/usr/bin/env python3
"""Registers, LDS and scratch of the top-documents kernels
(k_topic_docs_count, k_topic_docs_slab, k_topic_docs_merge), from the kernel
descriptors of the built library's gfx950 code object (as tools/readout_isa.py
reads them).  The count kernel's LDS (16 Kp bytes) and the slab kernel's
(512 n bytes) are dynamic, so the descriptor shows only the static part.  Exits
1 if a kernel uses scratch.  Facts from the descriptors only: no disassembly is
searched.

With --against OTHER.so it also compares every kernel of OTHER's code object
with the same kernel here -- text and descriptor, byte for byte -- and exits 1
if one differs or is missing: the check that a library built from the parent
commit and this one share every earlier kernel unchanged.

  python tools/topic_docs_isa.py [path/to/liblda_mi355x.so] [--against parent/liblda_mi355x.so]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ldagibbssampling_amd import capi, codeobj  # noqa: E402
from heldout_isa import describe  # noqa: E402

KERNELS = ["k_topic_docs_count", "k_topic_docs_slab", "k_topic_docs_merge"]


def main():
    args = sys.argv[1:]
    against = None
    if "--against" in args:
        i = args.index("--against")
        against = args[i + 1]
        del args[i:i + 2]
    lib = args[0] if args else capi.LIB_PATH
    ks = codeobj.kernels(codeobj.device_code_object(lib))
    bad = False
    print("| kernel | arch VGPRs | VGPRs + AGPRs | static LDS B | scratch B | text B |")
    print("|---|---|---|---|---|---|")
    for k in KERNELS:
        pre = codeobj.mangled_prefix(k)
        found = [(name, v) for name, v in ks.items() if name.startswith(pre) and v[1]]
        if not found:
            sys.exit(f"{lib}: no {k} kernel")
        for name, (text, kd) in found:
            d = describe(kd)
            print(f"| {k} | {d['arch_vgprs']} | {d['vgprs_total']} | {d['lds_bytes']} | {d['scratch_bytes']} | {len(text)} |")
            bad |= d["scratch_bytes"] != 0 or d["scratch_enabled"]
    if against:
        old = codeobj.kernels(codeobj.device_code_object(against))
        differ = [name for name, v in old.items() if ks.get(name) != v]
        new = sorted(set(ks) - set(old))
        print(f"\n{len(old)} kernels in {against}: {len(old) - len(differ)} byte-identical here (text and "
              f"descriptor), {len(differ)} differ or are missing; {len(new)} new")
        for name in differ:
            print("  differs:", name)
        bad |= bool(differ)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
