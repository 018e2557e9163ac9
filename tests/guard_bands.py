"""Guard bands around caller memory: a harness for the entry points that read and write through caller DEVICE pointers.

Every GPU test of this suite compares bytes INSIDE the buffers it hands over.  This module looks outside them: one uint8 arena per call
under test, every input and output cut out of it with a guard band before and after, each buffer placed at exactly the alignment
include/uwt.h states for its pointer and never better (its address is `align` modulo 256, so it is no multiple of 2 * align).

    specs = [Buf("traj", data=traj, align=4, stride=28), Buf("points", nbytes=cap * 16, align=16, stride=cap * 16), ...]
    outs = run_twice(TorchBackend(torch), specs, lambda a: (ctx.some_call_async(a.ptr("traj"), a.ptr("points")), ctx.sync()))

  - a guard is max(4096, stride) bytes: `stride` is the full extent one record index too far can reach — cap x record size of a per-pair
    table, pitch x img_h of a plane;
  - an input (`data` given) is copied in; its `dead` byte ranges (the rows past a pair's count) and the guards on both of its sides take
    the run's fill, 0x00 or 0x5A;
  - an output (`nbytes` given) is filled with OUT_FILL, its guards with GUARD_FILL, the same in both runs;
  - after the call (which waits for the device itself) EVERY guard byte is compared with what it was filled with.  Damage raises
    GuardDamage, whose `records` name the buffer, the side, and the first and last damaged offsets: on side "before" the offset counts
    back from the buffer's first byte (-1: the byte just before it), on side "after" it counts from its end (0: the first byte past it);
  - run_twice runs the call under both fills and requires every output byte — inside a count and past it — to be the same: nothing the
    call computes or leaves may depend on bytes outside what it was given.

The arena is assembled on the host and copied to the backend in one piece, and read back in one piece: NumpyBackend keeps it in host
memory (the self-test of tests/test_guard_bands_cpu.py), TorchBackend in one torch.uint8 tensor on the device."""
import numpy as np

GUARD_MIN = 4096
FILLS = (0x00, 0x5A)
OUT_FILL = 0xA5
GUARD_FILL = 0xC3


class Buf:
    """One buffer of a call.  name; data: the input's bytes (any contiguous array) or None for an output of `nbytes`; align: the
    alignment the header states for the pointer (a power of two below 256); stride: the extent a guard has to cover at least; dead:
    (start, stop) byte ranges of an input that the call must not depend on."""

    def __init__(self, name, data=None, nbytes=None, align=4, stride=0, dead=()):
        assert (data is None) != (nbytes is None), name
        assert 1 <= align < 256 and align & (align - 1) == 0, (name, align)
        self.name, self.align, self.stride = name, int(align), int(stride)
        self.data = None if data is None else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        self.nbytes = int(self.data.size if data is not None else nbytes)
        self.dead = [(int(a), int(b)) for a, b in dead]
        assert all(0 <= a <= b <= self.nbytes for a, b in self.dead), (name, self.dead)
        self.guard = max(GUARD_MIN, self.stride)


class GuardDamage(AssertionError):
    """records: [(buffer name, "before" | "after", first offset, last offset, damaged bytes)]"""

    def __init__(self, records):
        self.records = records
        super().__init__("; ".join("guard %s of %r damaged: %d byte(s), offsets %d..%d" % (side, name, n, first, last)
                                   for name, side, first, last, n in records))


class NumpyBackend:
    def alloc(self, nbytes):
        mem = np.zeros(nbytes, np.uint8)
        return mem, mem.ctypes.data

    def upload(self, mem, image):
        mem[:] = image

    def download(self, mem):
        return mem.copy()


class TorchBackend:
    """device memory of torch's allocator; upload and download wait for the device, so the call's own stream sees the fills"""

    def __init__(self, torch):
        self.torch = torch

    def alloc(self, nbytes):
        mem = self.torch.empty(nbytes, dtype=self.torch.uint8, device="cuda")
        return mem, mem.data_ptr()

    def upload(self, mem, image):
        mem.copy_(self.torch.from_numpy(image))
        self.torch.cuda.synchronize()

    def download(self, mem):
        self.torch.cuda.synchronize()
        return mem.cpu().numpy()


def _place(addr, align):
    """the first address >= addr that is `align` modulo 256: aligned to `align` exactly"""
    return addr + ((align - addr) % 256)


class Arena:
    def __init__(self, backend, specs, fill):
        assert len({s.name for s in specs}) == len(specs)
        self.backend, self.specs, self.fill = backend, list(specs), fill
        self.mem, self.base = backend.alloc(sum(s.nbytes + 2 * s.guard + 256 for s in specs) + 256)
        self.at = {}      # name -> offset of the buffer in the arena
        self.guards = []  # (name, side, start, stop, fill value)
        end = 0
        for s in self.specs:
            off = _place(self.base + end + s.guard, s.align) - self.base
            self.at[s.name] = off
            gfill = fill if s.data is not None else GUARD_FILL
            self.guards.append((s.name, "before", off - s.guard, off, gfill))
            self.guards.append((s.name, "after", off + s.nbytes, off + s.nbytes + s.guard, gfill))
            end = off + s.nbytes + s.guard
        image = np.full(end, GUARD_FILL, np.uint8)
        for _, _, a, b, v in self.guards:
            image[a:b] = v
        for s in self.specs:
            body = image[self.at[s.name]:self.at[s.name] + s.nbytes]
            if s.data is None:
                body[:] = OUT_FILL
            else:
                body[:] = s.data
                for a, b in s.dead:
                    body[a:b] = fill
        self.image = image
        backend.upload(self.mem, self._padded(image))
        for s in self.specs:   # every placement legal by the contract, none better than it
            p = self.ptr(s.name)
            assert p % s.align == 0 and p % (2 * s.align) != 0 and p % 256 != 0, (s.name, hex(p))

    def _padded(self, image):
        full = np.full(self.mem.shape[0], GUARD_FILL, np.uint8)
        full[:image.size] = image
        return full

    def ptr(self, name, byte_offset=0):
        """the address of a buffer (plus a byte offset into it: a row of an earlier result as the next call's input)"""
        return self.base + self.at[name] + int(byte_offset)

    def check(self):
        """Reads the arena back; GuardDamage if a guard byte changed, else {name: bytes of the buffer} for every buffer."""
        got = self.backend.download(self.mem)
        records = []
        for (name, side, a, b, v) in self.guards:
            bad = np.flatnonzero(got[a:b] != v)
            if bad.size:
                origin = b if side == "before" else a
                records.append((name, side, int(a + bad[0] - origin), int(a + bad[-1] - origin), int(bad.size)))
        if records:
            raise GuardDamage(records)
        return {s.name: got[self.at[s.name]:self.at[s.name] + s.nbytes].tobytes() for s in self.specs}


def run_once(backend, specs, call, fill):
    """One arena under `fill`, call(arena) (which enqueues and waits), the guard check.  Returns {name: bytes} of every buffer."""
    arena = Arena(backend, specs, fill)
    call(arena)
    return arena.check()


def run_twice(backend, specs, call):
    """The call under both fills: guards intact both times, and every OUTPUT byte the same.  Returns the outputs' bytes."""
    a, b = (run_once(backend, specs, call, fill) for fill in FILLS)
    for s in specs:
        if s.data is None:
            assert a[s.name] == b[s.name], "output %r depends on the bytes around the call's inputs (first difference at byte %d)" % (
                s.name, next(i for i, (x, y) in enumerate(zip(a[s.name], b[s.name])) if x != y))
    return {s.name: a[s.name] for s in specs if s.data is None}
