"""Compare the kernels of two gfx950 assembly listings of csrc/sdf_refine.hip, kernel by kernel.

Make each listing with tools/check_mfma_hazards.compile_isa (the command tests/conftest.py uses), in the two trees to compare:
    python -c "import sys; sys.path.insert(0, 'tools'); import check_mfma_hazards as c; c.compile_isa('/tmp/a.s')"
then  python tools/isa_kernel_diff.py /tmp/a.s /tmp/b.s  [-v NAME]
Every function body is cut out by its mangled symbol (label to .Lfunc_end, its .size or the next function); assembler comments and the numbers of local basic
block labels are dropped (they carry source positions and a function-wide counter, not code).  Prints the kernels that are
identical, differ, are missing, and are new; -v NAME shows the first lines of the difference of a kernel whose demangled name
contains NAME.  Exit status 1 if any kernel of the first listing differs or is missing in the second."""
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
            s = re.sub(r";.*$", "", line).rstrip()
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            if s:
                buf.append(s)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, r))


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    dm = demangle(sorted(set(a) | set(b)))
    same = [n for n in a if n in b and a[n] == b[n]]
    diff = [n for n in a if n in b and a[n] != b[n]]
    missing = [n for n in a if n not in b]
    new = [n for n in b if n not in a]
    for tag, lst in (("DIFFERENT", diff), ("MISSING", missing), ("NEW", new)):
        for n in sorted(lst, key=lambda x: dm[x]):
            print("%-9s %s" % (tag, dm[n].split("(")[0]))
    print("identical %d, different %d, missing %d, new %d" % (len(same), len(diff), len(missing), len(new)))
    if "-v" in sys.argv:
        key = sys.argv[sys.argv.index("-v") + 1]
        for n in diff:
            if key in dm[n]:
                print("\n".join(list(difflib.unified_diff(a[n], b[n], lineterm="", n=1))[:80]))
                break
    return 1 if diff or missing else 0


if __name__ == "__main__":
    sys.exit(main())
