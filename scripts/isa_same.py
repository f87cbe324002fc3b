"""Are the rome:: functions of two sets of device assembly files (hipcc -S --cuda-device-only) the same, body for body?
    python scripts/isa_same.py old.s [more.s ...] -- new_a.s new_b.s [...]
The check of a change that only MOVES kernels between translation units.  A function is the text from its `_ZN4rome...:` label to its
`.Lfunc_end`; comments after `;` are dropped and the function number inside local labels (.LBB<fn>_<n>, .LJTI<fn>_<n>, .LCPI<fn>_<n>,
.Lfunc_*<fn>) is blanked, since it counts the functions of the unit.  Whole bodies are compared by hash.  Prints the number of functions
on each side, the names on one side only (or defined twice on a side) and the names whose bodies differ; exit status 1 if there are any."""
import hashlib
import re
import sys

LABEL = re.compile(r"\.L(BB|JTI|CPI|func_begin|func_end)\d+")


def functions(paths):
    out, twice = {}, set()
    for path in paths:
        name, h = None, None
        for line in open(path, errors="replace"):
            line = line.split(";", 1)[0].rstrip()
            if name is None:
                m = re.match(r"(_ZN4rome\w*):$", line)
                if m:
                    name, h = m.group(1), hashlib.sha256()
                continue
            if line.strip():
                h.update((LABEL.sub(r".L\1", line) + "\n").encode())
            if line.startswith(".Lfunc_end"):
                if name in out:
                    twice.add(name)
                out[name] = h.hexdigest()
                name = None
    return out, twice


def main(argv):
    if "--" not in argv or argv.index("--") in (0, len(argv) - 1):
        sys.exit(__doc__)
    cut = argv.index("--")
    (a, a2), (b, b2) = functions(argv[:cut]), functions(argv[cut + 1:])
    only = sorted(set(a) ^ set(b))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    for n in only:
        print("only %s: %s" % ("left" if n in a else "right", n))
    for n in sorted(a2 | b2):
        print("defined twice on the %s: %s" % ("left" if n in a2 else "right", n))
    for n in differ:
        print("differs: %s" % n)
    print("isa_same: %d functions left, %d right; %d on one side only, %d defined twice, %d differing bodies"
          % (len(a), len(b), len(only), len(a2 | b2), len(differ)))
    return 1 if only or differ or a2 or b2 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
