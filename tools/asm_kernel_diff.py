#!/usr/bin/env python3
"""Which kernels' instruction text differs between two outputs of `make -C cgraytracing_amd/csrc asm`.

  python tools/asm_kernel_diff.py parent.s this.s [--allow REGEX]

`make asm` writes to a fixed path, so copy the parent's output aside before building the second one.  The files are split at
the function symbols (`name:` lines that a `.type name,@function` announced); comments, directives, local labels and the
`__hip_cuid_<hash>` label (new in every build) are dropped, and what is left is compared as text, function by function.
Prints one line per function that differs -- lines before, lines after, lines changed -- and the functions only one file has.
--allow: exit status 1 if a function whose name does not match REGEX differs (e.g. the family a refactor may touch)."""
import difflib
import re
import sys


def functions(path):
    funcs, names, cur = {}, set(), None
    with open(path, errors="replace") as fh:
        for ln in fh:
            m = re.match(r"\s*\.type\s+([^,\s]+),@function", ln)
            if m:
                names.add(m.group(1))
                continue
            s = ln.split(";", 1)[0].split("//", 1)[0].strip()
            if not s:
                continue
            m = re.match(r"([^\s:]+):$", s)
            if m:
                if m.group(1) in names:
                    cur = funcs.setdefault(m.group(1), [])
                elif m.group(1).startswith("__hip_cuid_") or not m.group(1).startswith(".L"):
                    cur = None  # a data symbol: the function before it has ended
                continue
            if s.startswith(".") or cur is None:
                continue
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))  # (a label carries its function's number in the file)
    return funcs


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    allow = re.compile(sys.argv[sys.argv.index("--allow") + 1]) if "--allow" in sys.argv else None
    if "--allow" in sys.argv:
        args.remove(sys.argv[sys.argv.index("--allow") + 1])
    a, b = functions(args[0]), functions(args[1])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-7s %s" % ("removed" if name in a else "added", name))
        elif a[name] != b[name]:
            sm = difflib.SequenceMatcher(None, a[name], b[name])
            changed = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
            print("%6d -> %6d lines, %5d changed  %s" % (len(a[name]), len(b[name]), changed, name))
        else:
            continue
        bad += allow is not None and not allow.search(name)
    print("%d functions in %s, %d in %s" % (len(a), args[0], len(b), args[1]))
    if bad:
        raise SystemExit("%d function(s) outside --allow differ" % bad)


if __name__ == "__main__":
    main()
