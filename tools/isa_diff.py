"""Kernel-by-kernel text comparison of hipcc -S dumps: python tools/isa_diff.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...]
A kernel is the lines between its label and .end_amdhsa_kernel (instructions and .amdhsa_* descriptor lines), comment lines
dropped and the function number of basic-block labels (.LBB<n>_<m>) normalised.  Exit status 1 if a kernel is on one side only
or its text differs."""
import sys, re
sep = sys.argv.index("--")
def kernels(paths):
    out = {}
    for p in paths:
        s = "\n" + open(p).read()
        for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", s, re.M):
            i = s.index("\n" + name + ":"); j = s.index(".end_amdhsa_kernel", i)
            lines = [l.split(";")[0].rstrip() for l in s[i:j].split("\n")]
            out[name] = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines if l.strip()]
    return out
old, new = kernels(sys.argv[1:sep]), kernels(sys.argv[sep + 1:])
missing, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
different = sorted(k for k in set(old) & set(new) if old[k] != new[k])
for k in sorted(set(old) & set(new)):
    print("%-9s %6d lines  %s" % ("DIFFERENT" if k in different else "same", len(new[k]), k))
for k in missing: print("MISSING   %s" % k)
for k in added: print("ADDED     %s" % k)
for k in different:
    n = next((i for i, (a, b) in enumerate(zip(old[k], new[k])) if a != b), min(len(old[k]), len(new[k])))
    print("first difference in %s at line %d:\n  - %s\n  + %s" % (k, n, (old[k] + [""])[n], (new[k] + [""])[n]))
print("%d kernels, %d missing, %d added, %d different" % (len(set(old) | set(new)), len(missing), len(added), len(different)))
sys.exit(1 if missing or added or different else 0)
