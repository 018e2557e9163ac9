"""The guard-band harness (tests/guard_bands.py) on its numpy backend: what it must report, it reports — no GPU."""
import ctypes as C

import numpy as np
import pytest

import guard_bands as GB

ARITH_INDEPENDENT = True   # no arithmetic here


def specs():
    rows = np.arange(3 * 5 * 12, dtype=np.uint8)   # 3 pairs x cap 5 x 12-byte records, pair 2 holding 3 rows
    return [GB.Buf("matches", data=rows, align=4, stride=5 * 12, dead=[(2 * 60 + 36, 3 * 60)]),
            GB.Buf("counts", data=np.array([5, 5, 3], np.int32), align=4, stride=12),
            GB.Buf("good", nbytes=3 * 5 * 12, align=4, stride=5 * 12),
            GB.Buf("info", nbytes=3 * 88, align=8, stride=3 * 88),
            GB.Buf("plane", nbytes=3 * 168 * 99, align=4, stride=168 * 99),
            GB.Buf("points", nbytes=37 * 16, align=16, stride=37 * 16)]


def poke(arena, name, offset, value=0x11):
    """one byte written through the ADDRESS the call under test would get, `offset` bytes from the buffer's first byte"""
    C.c_ubyte.from_address(arena.ptr(name) + offset).value = value


def test_an_untouched_arena_passes_and_buffers_sit_at_their_alignment_exactly():
    seen = {}

    def call(arena):
        for s in arena.specs:
            p = arena.ptr(s.name)
            assert p % s.align == 0 and p % (2 * s.align) != 0 and p % 256 != 0
            seen[s.name] = p
        # the guards: at least 4096 bytes, and a full stride of the buffer they protect
        for name, side, a, b, _ in arena.guards:
            s = next(x for x in arena.specs if x.name == name)
            assert b - a >= 4096 and b - a >= s.stride
        assert [g[3] - g[2] for g in arena.guards if g[0] == "plane"] == [168 * 99] * 2
        spans = sorted((a, b) for _, _, a, b, _ in arena.guards) + sorted((arena.at[s.name], arena.at[s.name] + s.nbytes) for s in arena.specs)
        spans.sort()
        assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))   # nothing overlaps

    outs = GB.run_twice(GB.NumpyBackend(), specs(), call)
    assert len(seen) == 6
    assert sorted(outs) == ["good", "info", "plane", "points"] and all(set(v) == {GB.OUT_FILL} for v in outs.values())


def test_inputs_arrive_with_their_dead_rows_and_guards_under_the_fill():
    for fill in GB.FILLS:
        arena = GB.Arena(GB.NumpyBackend(), specs(), fill)
        got = arena.check()
        m = np.frombuffer(got["matches"], np.uint8)
        assert np.array_equal(m[:156], np.arange(156, dtype=np.uint8)) and (m[156:] == fill).all()
        assert np.frombuffer(got["counts"], np.int32).tolist() == [5, 5, 3]
        at = arena.at["matches"]
        assert (arena.mem[at - 4096:at] == fill).all() and (arena.mem[at + 180:at + 180 + 4096] == fill).all()
        at = arena.at["good"]
        assert (arena.mem[at - 4096:at] == GB.GUARD_FILL).all() and (arena.mem[at + 180:at + 180 + 4096] == GB.GUARD_FILL).all()


@pytest.mark.parametrize("fill", GB.FILLS)
def test_one_byte_before_and_one_after_are_reported_by_name_side_and_offset(fill):
    def call(arena):
        poke(arena, "good", -1)            # the byte before the first record
        poke(arena, "good", 3 * 5 * 12)    # one past the last pair's cap
        poke(arena, "points", 37 * 16 + 15)   # the last byte of a 16-byte record one past cap
        poke(arena, "points", 37 * 16)

    with pytest.raises(GB.GuardDamage) as e:
        GB.run_once(GB.NumpyBackend(), specs(), call, fill)
    assert e.value.records == [("good", "before", -1, -1, 1), ("good", "after", 0, 0, 1), ("points", "after", 0, 15, 2)]
    assert "guard after of 'points' damaged: 2 byte(s), offsets 0..15" in str(e.value)


def test_a_byte_at_the_far_end_of_a_guard_is_reported():
    def call(arena):
        poke(arena, "plane", 3 * 168 * 99 + 168 * 99 - 1)   # a whole plane past the last pair's: the guard's last byte
        poke(arena, "plane", -168 * 99)                      # and the first byte of the guard before
        poke(arena, "info", -4096)

    with pytest.raises(GB.GuardDamage) as e:
        GB.run_once(GB.NumpyBackend(), specs(), call, 0x5A)
    assert e.value.records == [("info", "before", -4096, -4096, 1), ("plane", "before", -168 * 99, -168 * 99, 1),
                               ("plane", "after", 168 * 99 - 1, 168 * 99 - 1, 1)]


def test_a_guard_byte_rewritten_with_its_own_value_is_no_damage_but_any_other_value_is():
    # (the fills differ between input and output guards, so a stray copy of one buffer's fill into another's guard shows)
    def call(arena):
        poke(arena, "good", -2, GB.GUARD_FILL)
        poke(arena, "matches", -2, arena.fill)

    GB.run_once(GB.NumpyBackend(), specs(), call, 0x5A)
    with pytest.raises(GB.GuardDamage) as e:
        GB.run_once(GB.NumpyBackend(), specs(), lambda a: poke(a, "matches", 180, GB.OUT_FILL), 0x5A)
    assert e.value.records == [("matches", "after", 0, 0, 1)]


def test_an_output_that_follows_the_fill_fails_read_independence():
    def reads_a_dead_row(arena):   # a "kernel" that copies row 3 of pair 2, which has 3 rows
        src = (C.c_ubyte * 12).from_address(arena.ptr("matches") + 2 * 60 + 36)
        C.memmove(arena.ptr("good"), src, 12)

    def reads_past_the_counts(arena):
        C.memmove(arena.ptr("info"), arena.ptr("counts") + 12, 4)

    for call in (reads_a_dead_row, reads_past_the_counts):
        with pytest.raises(AssertionError, match="depends on the bytes around"):
            GB.run_twice(GB.NumpyBackend(), specs(), call)
    GB.run_twice(GB.NumpyBackend(), specs(), lambda a: C.memmove(a.ptr("good"), a.ptr("matches"), 12))   # a live row: fine
