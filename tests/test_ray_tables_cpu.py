"""The host side of k_residual's ray tables (uwt_kernels.h: ray_table_rows_max, ray_tables_fit — what launch_residual asks before it
takes a typed form): a small host-only program over the header prints both for given (pitch, groups per block).  The bound must cover
every row a block's walk can reach, the supported levels must fit — so the typed forms ARE what runs there — and a pitch beyond the
table space must not."""
import os
import subprocess

import numpy as np
import pytest

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uw-slam_amd", "csrc")

MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include "uwt_kernels.h"
int main(int argc, char** argv) {
  std::printf("%d %d\n", uwt::kRayTabFloats, uwt::kBlock);
  for (int i = 1; i + 1 < argc; i += 2) {
    const int pitch = std::atoi(argv[i]), gpb = std::atoi(argv[i + 1]);
    std::printf("%d %d\n", uwt::ray_table_rows_max(pitch, gpb), uwt::ray_tables_fit(pitch, gpb) ? 1 : 0);
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("ray_tables")
    src, exe = d / "main.hip", d / "ray_tables"
    src.write_text(MAIN)
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", CSRC,
                    "-Wno-unused-function", "-o", str(exe), str(src)], check=True, capture_output=True)

    def run(cases):
        out = subprocess.run([str(exe)] + [str(v) for c in cases for v in c], check=True, capture_output=True, text=True).stdout.split()
        vals = [int(v) for v in out]
        return vals[0], vals[1], [(vals[2 + 2 * i], bool(vals[3 + 2 * i])) for i in range(len(cases))]
    return run


def test_supported_levels_take_the_typed_forms_and_an_oversized_pitch_does_not(ask):
    cap, block, res = ask([(1280, 16 * 256), (1280, 1280 * 960 // 4), (640, 640 * 480 // 4), (8, 256), (4, 256), (1284, 256),
                           (8668, 256), (8670, 256), (8672, 256), (9000, 256), (20000, 4096)])
    assert (cap, block) == (8672, 256)   # the reduction image's floats; groups of four per step
    rows = [r for r, _ in res]
    fit = [f for _, f in res]
    # 1280-wide level 0 at the batch slicing (16 groups per thread), the same level and 640 x 480 as ONE slice (a batch of thousands
    # of pairs), the 8 x 6 level (12 groups for 256 lanes: 128 rows of walk), a pitch of one group, an odd-sized 1281-wide level
    assert fit[:6] == [True] * 6
    assert rows[0] == 15 and rows[1] == 962 and rows[2] == 482 and rows[3] == 130 and rows[4] == 258
    # at the edge of the table space: 8668 + 3 rows fit 8672 floats, 8670 + 3 do not; beyond: the plain forms
    assert fit[6:] == [True, False, False, False, False]


def test_the_row_bound_covers_every_walk(ask):
    """Rows from the one a slice begins in to the one its last step's last lane reads (inactive lanes included: every lane takes all
    the steps), counted directly, against the bound — slices that begin anywhere in a row, pitches around and above one step."""
    rng = np.random.default_rng(11)
    cases = [(int(p), int(s) * 256) for p in (4, 8, 76, 152, 640, 1020, 1024, 1028, 1280, 4000) for s in (1, 2, 3, 16, 19)]
    _, block, res = ask(cases)
    for (pitch, gpb), (rows, _) in zip(cases, res):
        for g_begin in [0, gpb, 7 * gpb] + [int(v) * gpb for v in rng.integers(1, 40, 4)]:
            first = (g_begin * 4) // pitch
            last = ((g_begin + gpb) * 4 - 1) // pitch   # the last pixel of group g_begin + steps * 256 - 1
            assert last - first + 1 <= rows - 1, (pitch, gpb, g_begin)   # (the bound's last row is the magic division's slack)
        assert rows <= (gpb * 4) // pitch + 3
