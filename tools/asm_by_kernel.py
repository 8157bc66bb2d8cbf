"""Per-kernel comparison of two builds' device assembly.

    python tools/asm_by_kernel.py PARENT_DIR NEW_DIR unit [unit ...]

PARENT_DIR/<unit>.s and NEW_DIR/<unit>.s are the device assembly of one translation unit each,
compiled with the Makefile's CXXFLAGS and the unit's TUFLAGS plus `--cuda-device-only -S`
(no debug information, from the csrc directory so that paths agree).  A unit is hashed whole
(sha256, first 16 hex digits, the compile-unit id symbol masked); one that differs is listed per
function, label to .Lfunc_end.  The lists under profiles/r*/ come from this.
"""
import hashlib
import re
import sys


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def load(path):
    text = open(path).read()
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    return text.split("\n")


def functions(lines):
    out, name, start = {}, None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", l)
        if m and name is None and not l.startswith(".L"):
            name, start = m.group(1), i
        elif l.startswith(".Lfunc_end") and name is not None:
            out[name] = lines[start:i + 1]
            name = None
    return out


def short(name):
    # the mangled name up to the first function parameter: enough to tell the instantiations apart
    m = re.match(r"^(_ZN3ikg\d+\w+?E)v", name)
    return m.group(1) if m else name


def main():
    pdir, ndir, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    for u in units:
        a, b = load(f"{pdir}/{u}.s"), load(f"{ndir}/{u}.s")
        ha, hb = digest(a), digest(b)
        if ha == hb:
            print(f"{u} parent {ha} new {hb} identical ({len(a)} lines)")
            continue
        print(f"{u} parent {ha} new {hb} differs ({len(a)} / {len(b)} lines); per function:")
        fa, fb = functions(a), functions(b)
        for n in sorted(set(fa) | set(fb)):
            if n not in fa or n not in fb:
                print(f"  {short(n)} only in {'new' if n in fb else 'parent'}")
                continue
            da, db = digest(fa[n]), digest(fb[n])
            print(f"  {short(n)} parent {da} new {db} {'identical' if da == db else 'CHANGED'} "
                  f"({len(fa[n])} / {len(fb[n])} lines)")


if __name__ == "__main__":
    main()
