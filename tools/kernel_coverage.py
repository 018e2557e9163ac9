#!/usr/bin/env python3
"""Which kernel instantiations of libuwt_hip.so the GPU suite launches: the kernel names in the symbol tables of the library's gfx950
code objects against the per-kernel launch counts rocprofv3 wrote while each test file ran
(`rocprofv3 --kernel-trace --stats --mangled-kernels --output-format csv -d <dir>/<file> -- python -m pytest -m gpu tests/<file>`).
Names only: nothing is disassembled.  Matching is on mangled names; c++filt is for display.  A kernel with internal linkage that
several translation units carry has one name and is one row.

usage: python tools/kernel_coverage.py --runs <dir with one sub-directory of *kernel_stats.csv per test file>
                                       [TAG=<stats csv or directory> ...] [--lib uw-slam_amd/libuwt_hip.so]
                                       [--rules profiles/r29/coverage_rules.txt] [--asserts-nothing test_x.py ...]
                                       [-o profiles/r29/kernel_coverage.md] [--golden tests/golden/kernel_coverage.txt]

The rules file names what may stay unlaunched: one line per rule, `status<TAB>regular expression over the pretty name<TAB>reason`,
status `exempt` or `unreachable`; the first match holds.  A kernel is `exempt` when such a rule names it, `compared` when a file
outside --asserts-nothing launched it (files that compare calls of the library with each other only), `unreachable` by its rule, and
`uncovered` when none of that applies (tests/test_kernel_coverage_cpu.py accepts no such line in the golden file)."""
import argparse
import csv
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = "/opt/rocm/llvm/bin"
STATUSES = ("compared", "exempt", "unreachable")


def library_kernels(lib):
    """the mangled kernel names of every gfx950 code object inside `lib`: the symbols that have a kernel descriptor (`<name>.kd`)"""
    objdump = os.path.join(LLVM_BIN, "llvm-objdump")
    tmp = tempfile.mkdtemp(prefix="uwt_cov_")
    try:
        dst = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, dst)
        subprocess.run([objdump, "--offloading", dst], check=True, capture_output=True, cwd=tmp)
        names = set()
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" in f and "gfx950" in f:
                table = subprocess.run([objdump, "-t", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
                names.update(kernel_symbols(table))
        return names
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernel_symbols(symbol_table):
    """kernel names in the text of a symbol table (`llvm-objdump -t`): the last field of every line that ends in `.kd`"""
    return {line.split()[-1][:-3] for line in symbol_table.splitlines() if line.rstrip().endswith(".kd")}


def demangle(names):
    names = list(names)
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    lines = out.stdout.splitlines()
    return lines if out.returncode == 0 and len(lines) == len(names) else names


def pretty(demangled):
    """`void uwt::k<A<1>, (X)2>(uwt::Args<int>)` -> `k<A<1>, (X)2>`: the return type, the namespaces and the parameter list go; the
    template arguments stay, nested ones and parenthesised ones included"""
    s = re.sub(r"^void ", "", demangled).replace("(anonymous namespace)::", "").replace("uwt::", "")
    depth = 0
    for i, c in enumerate(s):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            return s[:i]
    return s


def template_of(pretty_name):
    return pretty_name.split("<", 1)[0]


def read_stats(path):
    """{mangled name: calls} of one *kernel_stats.csv"""
    calls = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = (row.get("Name") or "").strip()
            if name.endswith(".kd"):
                name = name[:-3]
            if name:
                calls[name] = calls.get(name, 0) + int(row.get("Calls") or 0)
    return calls


def stats_files(path):
    """`path` itself, or every *kernel_stats.csv below it (one per traced process)"""
    if os.path.isfile(path):
        return [path]
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs if f.endswith("kernel_stats.csv"))


def merge(kernels, runs):
    """kernels: mangled names of the library; runs: [(tag, [stats csv, ...])].
    -> ({name: {"calls": total, "files": {tag: calls}}} over the library's kernels, {name: calls} of launched kernels not in it)"""
    ledger = {k: {"calls": 0, "files": {}} for k in kernels}
    other = {}
    for tag, files in runs:
        for path in files:
            for name, n in read_stats(path).items():
                if n <= 0:
                    continue
                if name in ledger:
                    ledger[name]["calls"] += n
                    ledger[name]["files"][tag] = ledger[name]["files"].get(tag, 0) + n
                else:
                    other[name] = other.get(name, 0) + n
    return ledger, other


def read_rules(path):
    rules = []
    if path:
        for line in open(path):
            line = line.rstrip("\n")
            if not line.strip() or line.startswith("#"):
                continue
            status, pattern, reason = line.split("\t", 2)
            assert status in ("exempt", "unreachable"), line
            rules.append((status, re.compile(pattern), reason))
    return rules


def classify(ledger, names, rules, asserts_nothing):
    """{name: (status, reason)}: an exempt rule holds first; launched by a file that compares -> compared; else the first rule that
    matches; else uncovered"""
    out = {}
    for k, row in ledger.items():
        comparing = sorted(t for t in row["files"] if t not in asserts_nothing)
        hit = next(((s, r) for s, p, r in rules if p.search(names[k])), None)
        if hit and hit[0] == "exempt":   # no result to compare, whoever launches it
            out[k] = hit
        elif comparing:
            out[k] = ("compared", " ".join(comparing))
        elif hit:
            out[k] = hit
        elif row["files"]:
            out[k] = ("uncovered", "launched only by files that assert nothing about its result: " + " ".join(sorted(row["files"])))
        else:
            out[k] = ("uncovered", "never launched")
    return out


def report(ledger, other, names, status, title):
    order = sorted(ledger, key=lambda k: names[k])
    by_tpl = {}
    for k in order:
        t = by_tpl.setdefault(template_of(names[k]), [0, 0, 0])
        t[0] += 1
        t[1] += bool(ledger[k]["calls"])
        t[2] += status[k][0] == "compared"
    n_l = sum(1 for k in order if ledger[k]["calls"])
    L = ["# " + title, "",
         "%d distinct kernels in the library, %d launched, %d never launched; %d compared, %d exempt, %d unreachable, %d uncovered."
         % (len(order), n_l, len(order) - n_l, *(sum(1 for k in order if status[k][0] == s) for s in STATUSES + ("uncovered",))), "",
         "## By template", "", "| template | instantiations | launched | compared | never launched |", "|---|---|---|---|---|"]
    for t in sorted(by_tpl):
        n, l, c = by_tpl[t]
        L.append("| `%s` | %d | %d | %d | %d |" % (t, n, l, c, n - l))
    L += ["", "## Never launched, by template", ""]
    for t in sorted(by_tpl):
        rows = [k for k in order if template_of(names[k]) == t and not ledger[k]["calls"]]
        if rows:
            L += ["### `%s` (%d of %d)" % (t, len(rows), by_tpl[t][0]), ""]
            L += ["- `%s` — %s: %s" % (names[k], *status[k]) for k in rows]
            L.append("")
    weak = [k for k in order if ledger[k]["calls"] and status[k][0] != "compared"]
    L += ["## Launched, but only by files that assert nothing about the result", ""]
    L += ["- `%s` — %s: %s" % (names[k], *status[k]) for k in weak] or ["none"]
    L += ["", "## Ledger", "", "| kernel | launches | status | launched by |", "|---|---|---|---|"]
    for k in order:
        files = ", ".join("%s (%d)" % (t, n) for t, n in sorted(ledger[k]["files"].items()))
        L.append("| `%s` | %d | %s | %s |" % (names[k], ledger[k]["calls"], status[k][0], files))
    L += ["", "%d launches of %d kernels that are not the library's (the array library's own) are not listed." % (sum(other.values()), len(other))]
    return "\n".join(L) + "\n"


def golden_text(ledger, status):
    """the machine-readable form: `mangled name<TAB>status<TAB>reason`, sorted by name"""
    return "".join("%s\t%s\t%s\n" % (k, status[k][0], status[k][1]) for k in sorted(ledger))


def read_golden(path):
    """{mangled name: (status, reason)}"""
    out = {}
    for line in open(path):
        if line.strip():
            name, st, reason = line.rstrip("\n").split("\t", 2)
            out[name] = (st, reason)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "uw-slam_amd", "libuwt_hip.so"))
    ap.add_argument("--kernel-list", help="read the library's mangled kernel names from this file (one per line) instead of --lib")
    ap.add_argument("--runs", action="append", default=[], help="a directory with one sub-directory of stats files per test file")
    ap.add_argument("tagged", nargs="*", help="TAG=<stats csv or directory>")
    ap.add_argument("--rules")
    ap.add_argument("--asserts-nothing", nargs="*", default=[])
    ap.add_argument("--title", default="Kernel instantiations launched by the GPU suite")
    ap.add_argument("-o", "--output")
    ap.add_argument("--golden")
    a = ap.parse_args(argv)
    kernels = set(open(a.kernel_list).read().split()) if a.kernel_list else library_kernels(a.lib)
    runs = []
    for d in a.runs:
        for sub in sorted(os.listdir(d)):
            if os.path.isdir(os.path.join(d, sub)):
                runs.append((sub if sub.endswith(".py") else sub + ".py", stats_files(os.path.join(d, sub))))
    for spec in a.tagged:
        tag, path = spec.split("=", 1)
        runs.append((tag, stats_files(path)))
    ledger, other = merge(kernels, runs)
    order = sorted(ledger)
    names = dict(zip(order, (pretty(n) for n in demangle(order))))
    status = classify(ledger, names, read_rules(a.rules), set(a.asserts_nothing))
    empty = [t for t, fs in runs if not fs]
    text = report(ledger, other, names, status, a.title)
    if empty:
        text += "\nNo stats file: " + ", ".join(empty) + "\n"
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    if a.golden:
        with open(a.golden, "w") as f:
            f.write(golden_text(ledger, status))
    return 0


if __name__ == "__main__":
    sys.exit(main())
