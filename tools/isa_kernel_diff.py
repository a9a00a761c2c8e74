r"""Compare the kernels of two sets of gfx950 assembly listings, kernel by kernel.

Make a device-only listing of any translation unit of csrc/ with csrc/build.sh's flags plus -S --cuda-device-only, in the two
trees to compare:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -S --cuda-device-only -o /tmp/a_ba.s ba_solver.hip
(for sdf_refine.hip, tools/check_mfma_hazards.compile_isa is that command, the one tests/conftest.py uses)
then  python tools/isa_kernel_diff.py A1.s[,A2.s ...] B1.s[,B2.s ...]  [-v NAME] [--alias REGEX=REPL ...]
Each side is one listing or several joined by commas -- code that moved from one translation unit to another is then compared
where it is now.  A function that two listings of a side hold with the same body (an inline helper both units emit) is one
function; different bodies under one name are an error.  Every function body is cut out by its mangled symbol (label to .Lfunc_end, its .size or the next function) and paired by its
demangled name; assembler comments, the numbers of local labels, section directives and the function's own symbol are dropped
(source positions, counters over the function or the file, and where the code is placed: not code).  Prints the kernels that are
identical, differ, are missing, and are new; -v NAME shows the first lines of the difference of a kernel whose demangled name
contains NAME.  --alias pairs kernels under a renaming: re.sub(REGEX, REPL) on the demangled names (up to the argument list) of
the first listing, e.g. --alias 'k_twin_(\w+)<(.*)>$=k_\1<\2, true>'.  Exit status 1 if any kernel of the first listing differs
or is missing in the second."""
import difflib
import re
import subprocess
import sys


def bodies(path):
    out, cur, buf = {}, None, []
    for line in open(path).read().split("\n"):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            if cur:
                out[cur] = buf
            cur, buf = m.group(1), []
            continue
        if cur and (line.startswith(".Lfunc_end") or re.match(r"^\s*\.size\s+" + re.escape(cur) + ",", line)):
            out[cur] = buf
            cur = None
            continue
        if cur:
            s = re.sub(r";.*$", "", line).rstrip().replace(cur, "<self>")      # (its own symbol: the kernel descriptor names it)
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            s = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", s)      # (long branches: a counter over the whole file)
            if s and not re.match(r"\s*\.(text|section)\b", s):      # (where the code goes -- .text, or a template's own section --
                buf.append(s)                                       #  is not code)
    return out


def named(paths, alias=()):
    """bodies() of the comma-separated listings keyed by demangled name without the argument list, the aliases applied in the
    order given"""
    out = {}
    for path in paths.split(","):
        raw = bodies(path)
        dm = subprocess.run(["c++filt"], input="\n".join(raw), capture_output=True, text=True).stdout.split("\n")
        seen = set()
        for sym, name in zip(raw, dm):
            name = name.replace("void ", "", 1).split("(")[0]
            for pat, repl in alias:
                name = re.sub(pat, repl, name)
            assert name not in seen and out.get(name, raw[sym]) == raw[sym], "two functions named " + name
            seen.add(name)
            out[name] = raw[sym]
    return out


def main():
    alias = [sys.argv[i + 1].split("=", 1) for i, x in enumerate(sys.argv) if x == "--alias"]
    a, b = named(sys.argv[1], alias), named(sys.argv[2])
    same = [n for n in a if n in b and a[n] == b[n]]
    diff = [n for n in a if n in b and a[n] != b[n]]
    missing = [n for n in a if n not in b]
    new = [n for n in b if n not in a]
    for tag, lst in (("DIFFERENT", diff), ("MISSING", missing), ("NEW", new)):
        for n in sorted(lst):
            print("%-9s %s" % (tag, n))
    print("identical %d, different %d, missing %d, new %d" % (len(same), len(diff), len(missing), len(new)))
    if "-v" in sys.argv:
        key = sys.argv[sys.argv.index("-v") + 1]
        for n in diff:
            if key in n:
                print("\n".join(list(difflib.unified_diff(a[n], b[n], lineterm="", n=1))[:80]))
                break
    return 1 if diff or missing else 0


if __name__ == "__main__":
    sys.exit(main())
