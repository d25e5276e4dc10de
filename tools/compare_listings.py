"""(CPU) Two device listings of rt_capi.hip compared function by function, instruction for instruction.
  hipcc $(make -s -C ray-tracing-practice_amd print-render-flags) --cuda-device-only -S -o parent.s csrc/rt_capi.hip     (in each tree)
  python3 tools/compare_listings.py parent.s tree.s [--as 'OLD DEMANGLED NAME=NEW DEMANGLED NAME' …] > profiles/rNN/listing_compare.txt
A function's text is its instructions and labels: comments, directives and the .L label numbering (which shifts with every function
emitted before it) are left out, so "same" means the same instructions with the same operands in the same order.  --as compares a
function of the old listing with one of another name in the new listing (a kernel that was renamed)."""
import argparse
import re
import subprocess
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^([A-Za-z_][A-Za-z0-9_$.]*):", line)
        if m and not line.startswith(".L"):
            if m.group(1).startswith(("amdhsa.", "__hip_cuid")):      # the metadata's YAML keys, the translation unit's id: no functions
                name = None
                continue
            name, body = m.group(1), []
            out[name] = body
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        if name is None:
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip():
            continue
        if s.startswith("\t.") or s.startswith("\t;"):
            continue
        body.append(s.strip())
    return out


def normalise(body, own_name):
    """Local labels renumbered in order of first appearance; the function's own mangled name (in s_getpc / relocation operands) blanked."""
    seen = {}

    def lab(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")
    return [re.sub(r"\.L[A-Za-z0-9_$]+", lab, ln).replace(own_name, "@self") for ln in body]


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--as", dest="renamed", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    old, new = functions(args.old), functions(args.new)
    dm_old, dm_new = demangle(list(old)), demangle(list(new))
    by_name_new = {dm_new[k]: k for k in new}
    renamed = dict(r.split("=", 1) for r in args.renamed)
    same, differ, gone = [], [], []
    matched_new = set()
    for k, body in old.items():
        d = dm_old[k]
        target = renamed.get(d, d)
        k2 = by_name_new.get(target)
        if k2 is None:
            gone.append(d)
            continue
        matched_new.add(k2)
        a, b = normalise(body, k), normalise(new[k2], k2)
        what = d if target == d else f"{d}  ->  {target}"
        (same if a == b else differ).append((what, len(a), len(b)))
    added = [dm_new[k] for k in new if k not in matched_new]
    print(f"# {args.old} against {args.new}: {len(old)} / {len(new)} functions")
    print(f"same instructions ({len(same)}):")
    for what, n, _ in same:
        print(f"  {n:6d}  {what}")
    print(f"different ({len(differ)}):")
    for what, n, m in differ:
        print(f"  {n:6d} -> {m:6d}  {what}")
    print(f"only in the old listing ({len(gone)}):")
    for d in gone:
        print(f"  {d}")
    print(f"only in the new listing ({len(added)}):")
    for d in added:
        print(f"  {d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
