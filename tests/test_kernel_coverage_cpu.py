"""tools/kernel_coverage.py on the CPU: its parsing and merging on a fabricated kernel list and statistics tables, and the committed
ledger (tests/golden/kernel_coverage.txt) against the kernel names of the built library — an instantiation added or renamed fails the
second test until the suite's launches are measured again (profiles/r29/README.md) and the ledger says where it is tested."""
import importlib.util
import os

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# three kernels of a library: one launched under two test files, one never launched, one whose name demangles with nested
# template arguments (and a parameter list that has template arguments of its own)
K_TWICE = "_ZN3uwt7k_halveIhLi4EEEvPKT_PS1_i"
K_NEVER = "_ZN3uwt8k_finishENS_8IterArgsE"
K_NESTED = "_ZN3uwt13k_pyramid_allINS_4WrapINS_4PairIhLi2EEEEEEEvNS_11PyramidArgsIT_EE"
K_FOREIGN = "_ZN2at6native18elementwise_kernelILi128EEEvi"
HEADER = '"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
SYMBOLS = """
SYMBOL TABLE:
0000000000001a00 l     F .text	0000000000000040 _ZN3uwt6helperEv
0000000000002000 g     F .text	0000000000000400 %s
0000000000008f00 g     O .rodata	0000000000000040 %s.kd
0000000000008f40 g     O .rodata	0000000000000040 %s.kd
0000000000008f80 g     O .rodata	0000000000000040 %s.kd
""" % (K_TWICE, K_TWICE, K_NEVER, K_NESTED)


def row(name, calls):
    return '"%s",%d,%d,%.1f,1.5,10,20,0.5\n' % (name, calls, 100 * calls, 100.0)


def test_parse_and_merge(tmp_path):
    """kernel names off a symbol table; launch counts summed over the processes of one file and over files; a kernel outside the
    library kept apart; the statuses; the report's unlaunched section and the golden text"""
    T = tool()
    assert T.kernel_symbols(SYMBOLS) == {K_TWICE, K_NEVER, K_NESTED}
    a = tmp_path / "runs" / "test_a"
    b = tmp_path / "runs" / "test_b" / "host"
    a.mkdir(parents=True)
    b.mkdir(parents=True)
    (a / "11_kernel_stats.csv").write_text(HEADER + row(K_TWICE, 3) + row(K_FOREIGN, 7))
    (a / "12_kernel_stats.csv").write_text(HEADER + row(K_TWICE + ".kd", 2))          # a child process of the same file
    (b / "13_kernel_stats.csv").write_text(HEADER + row(K_TWICE, 4) + row(K_NESTED, 1))
    (b / "13_kernel_trace.csv").write_text("not a statistics table\n")
    runs = [("test_a.py", T.stats_files(str(a))), ("test_b.py", T.stats_files(str(tmp_path / "runs" / "test_b")))]
    assert [len(f) for _, f in runs] == [2, 1]
    ledger, other = T.merge({K_TWICE, K_NEVER, K_NESTED}, runs)
    assert ledger[K_TWICE] == {"calls": 9, "files": {"test_a.py": 5, "test_b.py": 4}}
    assert ledger[K_NEVER] == {"calls": 0, "files": {}}
    assert ledger[K_NESTED] == {"calls": 1, "files": {"test_b.py": 1}}
    assert other == {K_FOREIGN: 7}

    order = sorted(ledger)
    names = dict(zip(order, (T.pretty(n) for n in T.demangle(order))))
    assert names[K_TWICE] == "k_halve<unsigned char, 4>"
    assert names[K_NEVER] == "k_finish"
    assert names[K_NESTED] == "k_pyramid_all<Wrap<Pair<unsigned char, 2> > >" or names[K_NESTED] == "k_pyramid_all<Wrap<Pair<unsigned char, 2>>>"
    assert T.template_of(names[K_NESTED]) == "k_pyramid_all"
    assert T.pretty("void (anonymous namespace)::k_spread_rows<unsigned short>(unsigned short const*, int)") == "k_spread_rows<unsigned short>"
    assert T.pretty("void uwt::k<(uwt::Mode)2, uwt::A<1> >(uwt::Args<int>)") == "k<(Mode)2, A<1> >"

    rules = tmp_path / "rules.txt"
    rules.write_text("# status, pattern, reason\nunreachable\t^k_finish$\tnothing launches it (made up)\n")
    status = T.classify(ledger, names, T.read_rules(str(rules)), {"test_b.py"})
    assert status[K_TWICE] == ("compared", "test_a.py")
    assert status[K_NEVER] == ("unreachable", "nothing launches it (made up)")
    assert status[K_NESTED][0] == "uncovered"            # launched, but only by a file that asserts nothing
    assert T.classify(ledger, names, [], set())[K_NEVER] == ("uncovered", "never launched")

    text = T.report(ledger, other, names, status, "t")
    never = text.split("## Never launched, by template")[1].split("## Launched, but only")[0]
    assert "### `k_finish` (1 of 1)" in never and "k_halve" not in never and "k_pyramid_all" not in never
    assert "| `k_halve<unsigned char, 4>` | 9 | compared | test_a.py (5), test_b.py (4) |" in text
    golden = tmp_path / "golden.txt"
    golden.write_text(T.golden_text(ledger, status))
    assert T.read_golden(str(golden)) == status

    # the command line over the same files
    out = tmp_path / "report.md"
    kl = tmp_path / "kernels.txt"
    kl.write_text("\n".join(order) + "\n")
    assert T.main(["--kernel-list", str(kl), "--runs", str(tmp_path / "runs"), "--rules", str(rules), "--asserts-nothing", "test_b.py",
                   "-o", str(out), "--golden", str(golden)]) == 0
    assert T.read_golden(str(golden)) == status and "3 distinct kernels in the library, 2 launched, 1 never launched" in out.read_text()


def test_ledger_names_every_kernel_of_the_library():
    """the kernel names of the built library are the names of tests/golden/kernel_coverage.txt, and every line says compared, exempt or
    unreachable, with a reason"""
    T = tool()
    lib = os.path.join(ROOT, "uw-slam_amd", "libuwt_hip.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build)"
    built = T.library_kernels(lib)
    golden = T.read_golden(os.path.join(ROOT, "tests", "golden", "kernel_coverage.txt"))
    missing, stale = sorted(built - set(golden)), sorted(set(golden) - built)
    if missing or stale:
        print("in the library, not in the ledger (measure again: profiles/r29/README.md):")
        print("\n".join("  " + T.pretty(n) for n in T.demangle(missing)))
        print("in the ledger, not in the library:")
        print("\n".join("  " + T.pretty(n) for n in T.demangle(stale)))
    assert not missing and not stale, (len(missing), len(stale))
    bad = {k: v for k, v in golden.items() if v[0] not in T.STATUSES or not v[1].strip()}
    assert not bad, bad
