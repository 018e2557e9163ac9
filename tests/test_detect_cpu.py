"""The pure host parts of the detector driver (uwt_detect.h: chunk_frames, provided_rows; uwt_ctx.h: Carve, which lays out a chunk's
scratch): a small host-only program over the headers prints them for given inputs.  A chunk never exceeds the budget unless it is
one frame, is never shorter than it could be, and never exceeds a launch's grid; the rows of a describe launch are the largest
count of the chunk's frames; arrays carved from one allocation do not overlap and start on their alignment."""
import os
import subprocess

import pytest

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uw-slam_amd", "csrc")

MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "uwt_ctx.h"
#include "uwt_detect.h"
int main(int argc, char** argv) {
  std::printf("%zu %d\n", uwt::kChunkBytes, uwt::kMaxChunk);
  for (int i = 1; i + 1 < argc; i += 2) std::printf("%d\n", uwt::chunk_frames((size_t)std::atoll(argv[i]), std::atoi(argv[i + 1])));
  const std::vector<int32_t> n_in = {3, 0, 7, 2, 9};
  std::printf("%d %d %d\n", uwt::provided_rows(n_in.data(), 5), uwt::provided_rows(n_in.data() + 1, 3), uwt::provided_rows(n_in.data(), 0));
  uwt::Carve cv(16);
  const size_t a = cv.take<int>(3), b = cv.take<uint8_t>(17), c = cv.take<double>(0), d = cv.take<unsigned long long>(2);
  std::printf("%zu %zu %zu %zu %zu %zu\n", a, b, c, d, cv.tight(), cv.total());
  uwt::Carve g(16, 100);   // the same with guards (uwt_debug_guards): a gap of 100 bytes, rounded up to the alignment, behind every array
  const size_t ga = g.take<int>(3), gb = g.take<uint8_t>(17);
  g.align = 64;
  const size_t gc = g.take<double>(2);
  std::printf("%zu %zu %zu %zu %zu", ga, gb, gc, g.tight(), g.total());
  for (const uwt::GuardGap& q : g.gaps) std::printf(" %lld %zu %d", q.at, q.bytes, q.array);
  std::printf("\n");
  return 0;
}
'''


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("detect")
    src, exe = d / "main.hip", d / "detect_rules"
    src.write_text(MAIN)
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", CSRC,
                    "-Wno-unused-function", "-o", str(exe), str(src)], check=True, capture_output=True)

    def run(cases):
        out = subprocess.run([str(exe)] + [str(v) for c in cases for v in c], check=True, capture_output=True, text=True).stdout.split("\n")
        budget, grid = (int(v) for v in out[0].split())
        n = len(cases)
        run.guarded = [int(v) for v in out[3 + n].split()]
        return budget, grid, [int(v) for v in out[1:1 + n]], [int(v) for v in out[1 + n].split()], [int(v) for v in out[2 + n].split()]
    return run


def test_frames_per_chunk_rule(ask):
    mib = 1 << 20
    pers = [1, 4096, 10 * mib + 123, 128 * mib, 128 * mib + 16, 256 * mib - 1, 256 * mib, 256 * mib + 1, 3 << 30]
    cases = [(per, n) for per in pers for n in (1, 2, 24, 33, 4096, 4097, 100000)]
    budget, grid, frames, _, _ = ask(cases)
    assert (budget, grid) == (256 * mib, 4096)
    for (per, n), c in zip(cases, frames):
        assert 1 <= c <= min(n, grid), (per, n, c)
        assert c == 1 or c * per <= budget, (per, n, c)                       # within the budget, unless it is one frame
        assert c == n or c == grid or (c + 1) * per > budget, (per, n, c)     # and as long as it can be
    assert frames[cases.index((10 * mib + 123, 33))] == 25                      # a call of 33 such frames runs as 25 + 8
    assert frames[cases.index((256 * mib, 24))] == 1 and frames[cases.index((128 * mib, 24))] == 2


def test_rows_rule_and_carving(ask):
    _, _, _, rows, carve = ask([])
    assert rows == [9, 7, 0]
    a, b, c, d, tight, total = carve
    assert (a, b, c, d) == (0, 16, 48, 48)     # each array on the next multiple of 16 behind the one before; an empty one takes none
    assert tight == 64 and total == 64


def test_carving_with_guards(ask):
    """a gap behind every array, from the array's last byte to the next array (the pad in front of it included), each at least the
    guard rounded up to the alignment in force; the arrays keep their alignment; the last gap ends the block"""
    ask([])
    a, b, c, tight, total, *gaps = ask.guarded
    assert (a, b, c) == (0, 128, 320) and tight == total == 512
    assert gaps == [12, 116, 0, 145, 175, 1, 336, 176, 2]   # (offset, bytes, the array in front) x 3
