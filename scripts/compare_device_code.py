"""Device code of two trees, kernel by kernel: has a change that moves kernels between source files left every one as it was?
    python scripts/compare_device_code.py <before dir> <after dir>
Each directory holds one assembly file per source, compiled with the library's flags plus --cuda-device-only -S
(<source stem>.s).  A file whose kernels are the same set in both trees is compared whole, the compilation-unit id masked
(as in profiles/host_layer_device_code.txt).  The kernels of any other file are looked up in the whole after-tree by their
mangled names and compared one by one: the .amdhsa_kernel descriptor, and the body from its .type line to its .Lfunc_end,
comments stripped and the numbers of file-local labels masked (they count functions and blocks of the FILE).  Prints one row
per kernel or file; the exit status is the number of rows that differ."""
import hashlib
import os
import re
import sys

MASKS = [(r"\.LBB\d+_", ".LBB#_"), (r"\.LJTI\d+_", ".LJTI#_"), (r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#"), (r"\.Ltmp\d+", ".Ltmp#"),
         (r"__hip_cuid_\w+", "__hip_cuid_#")]


def masked(text):
    text = re.sub(r"[ \t]*;.*", "", text)
    for pat, rep in MASKS:
        text = re.sub(pat, rep, text)
    return text


def kernels(text):
    """{mangled name: (descriptor, masked body)} of one assembly file."""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        name = m.group(1)
        body = re.search(r"^\s*\.type\s+%s,@function\n.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        out[name] = (m.group(0), masked(body.group(0)))
    return out


def main(before, after):
    read = lambda d: {f[:-2]: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith(".s")}
    a, b = read(before), read(after)
    ka, kb = {f: kernels(t) for f, t in a.items()}, {f: kernels(t) for f, t in b.items()}
    where = {k: f for f, ks in kb.items() for k in ks}  # (a template of a header may be in two files; those compare whole)
    rows = []
    for f in a:
        if f in b and set(ka[f]) == set(kb[f]):
            ta, tb = (re.sub(MASKS[-1][0], MASKS[-1][1], t) for t in (a[f], b[f]))
            rows.append((f, f, "(whole file, %d kernels)" % len(ka[f]), hashlib.sha256(ta.encode()).hexdigest()[:16],
                         "identical" if ta == tb else "DIFFERS"))
            continue
        for k, (desc, body) in ka[f].items():
            g = where.get(k)
            result = "MISSING" if g is None else "identical" if (desc, body) == kb[g][k] else \
                "DIFFERS (%s)" % ("descriptor" if desc != kb[g][k][0] else "body")
            rows.append((f, g or "-", k, hashlib.sha256(body.encode()).hexdigest()[:16], result))
    new = sorted(k for k in where if not any(k in ks for ks in ka.values()))
    rows += [("-", where[k], k, hashlib.sha256(kb[where[k]][k][1].encode()).hexdigest()[:16], "NEW") for k in new]
    wf, wg = (max(len(r[i]) for r in rows) + 4 for i in (0, 1))
    print("%-*s %-*s %-16s  %-18s %s" % (wf, "file before", wg, "file after", "body sha256", "result", "kernel"))
    for f, g, k, h, result in rows:
        print("%-*s %-*s %-16s  %-18s %s" % (wf, f + ".hip" if f != "-" else f, wg, g + ".hip" if g != "-" else g, h, result, k))
    bad = [r for r in rows if r[4] != "identical"]
    moved = [r for r in rows if not r[2].startswith("(whole")]
    print("\n%d kernels compared one by one (%d kept their file, %d moved), %d files compared whole; %d rows differ" % (
        len(moved), sum(r[0] == r[1] for r in moved), sum(r[0] != r[1] for r in moved), len(rows) - len(moved), len(bad)))
    return len(bad)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
