"""What SURF and ORB share on the device (uwt_select.h, uwt_detect.h), where no other test reaches: the selection routine over more
than one LDS tile of 1024 candidates, with and without the capacity cut, and calls that run as more than one chunk, delivered to
host and to device memory.  Bit for bit with the numpy restatements (tests/surf_ref.py, tests/orb_ref.py) and with the single-frame
calls — no tolerance anywhere.  The first test runs without a device: it checks that the inputs are worth testing on."""
import importlib
import os

import numpy as np
import pytest

import orb_cases as KO
import orb_ref as O
import surf_cases as K
import surf_ref as S

ARITH_INDEPENDENT = True   # neither detector has an arithmetic set
TILE = 1024                # candidates of an LDS tile: the selection kernels' block
CHUNK_BYTES = 256 << 20    # the scratch a chunk of frames may take (uwt_detect.h)
INTR = {(400, 304): (330.0, 330.0, 199.5, 151.5), (640, 480): (525.0, 525.0, 319.5, 239.5)}
SURF_TILES = dict(hessian_threshold=0.0)
ORB_TILES = dict(fast_threshold=5, edge_threshold=16, n_features=3000)
ORB_QUOTA = [652, 543, 452, 377, 314, 262, 218, 182]
DETECTORS = ["surf", "orb"]


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def make_ctx(capi, w, h, max_frames=2):
    return capi.Context(capi.default_params(w, h, *INTR[(w, h)], max_frames=max_frames, max_pairs=1, n_levels=1, first_level=0, last_level=0))


_ref = {}


def tiles_frame():
    return K.texture(400, 304, 21)


def surf_ref_of(cap):
    if ("surf", cap) not in _ref:
        p = S.default_params()
        p.update(SURF_TILES)
        _ref[("surf", cap)] = S.detect_describe(tiles_frame(), p, cap)
    return _ref[("surf", cap)]


def orb_ref_of(cap):
    if ("orb", cap) not in _ref:
        p = O.default_params()
        p.update(ORB_TILES)
        _ref[("orb", cap)] = O.detect_describe(tiles_frame(), p, cap)
    return _ref[("orb", cap)]


def surf_raw_bytes(w, h, n_octaves=4, n_octave_layers=2):
    """a lower bound of a frame's SURF scratch: the raw candidates alone, surf_raw_bound records of 32 + 8 + 1 bytes"""
    n = sum(n_octave_layers * (((w >> o) + 1) // 2) * (((h >> o) + 1) // 2) for o in range(n_octaves))
    return max(n, 64) * 41


def orb_raw_bytes(w, h, n_levels=8, edge=31):
    """the same for ORB: every layer's orb_raw_bound candidates, a key and a Harris measure of 8 bytes each"""
    n = 0
    for l in range(n_levels):
        lw, lh = O.layer_size(w, h, l)
        bw, bh = lw - 2 * edge, lh - 2 * edge
        n += ((bw + 1) // 2) * ((bh + 1) // 2) if bw >= 1 and bh >= 1 else 0
    return n * 16


def chunked_length(raw_bytes):
    """entries of a slot list that cannot run as one chunk"""
    return CHUNK_BYTES // raw_bytes + 1


def test_inputs_are_worth_testing():
    """on the CPU: the selection cases span the tiles they are chosen for, and the chunked lists exceed the chunk budget"""
    full = surf_ref_of(4096)[0]
    assert len(full) == 1093 and TILE < len(full) <= 2 * TILE                    # two tiles; cap = 600 cuts across them
    p = O.default_params()
    p.update(ORB_TILES)
    assert O.level_quota(p["n_features"], p["n_levels"]) == ORB_QUOTA and sum(ORB_QUOTA) == 3000
    assert len(O.layer_candidates(tiles_frame(), p)[2]) == 2091                   # three tiles in k_orb_rank
    kept = orb_ref_of(4096)[0]
    assert np.bincount(kept["octave"], minlength=8).tolist() == ORB_QUOTA         # every layer fills its quota: three tiles in k_orb_select
    assert len(orb_ref_of(2000)[0]) == 2000
    n_surf, n_orb = chunked_length(surf_raw_bytes(640, 480)), chunked_length(orb_raw_bytes(640, 480))
    assert n_surf * surf_raw_bytes(640, 480) > CHUNK_BYTES and n_orb * orb_raw_bytes(640, 480) > CHUNK_BYTES
    assert n_surf <= 34 and n_orb <= 110                                         # (the lists stay short)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uw-slam_amd", "csrc")
    assert "kChunkBytes = 256u << 20" in open(os.path.join(csrc, "uwt_detect.h")).read()   # the budget the lengths are worked out for


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [4096, 600])
def test_gpu_surf_selection_over_two_tiles(capi, cap):
    ctx = make_ctx(capi, 400, 304)
    ctx.upload_frames(0, tiles_frame()[None])
    kp, desc = ctx.surf_detect_describe_batch([0], params=capi.default_surf_params(**SURF_TILES), cap=cap)[0]
    wk, wd = surf_ref_of(cap)
    assert len(wk) == min(cap, 1093)
    assert K.same_keypoints(kp, wk) is None, K.same_keypoints(kp, wk)
    assert K.same_descriptors(desc, wd) is None, K.same_descriptors(desc, wd)
    if cap == 600:   # exactly the 600 strongest, in contract order: the order of the full list
        full = surf_ref_of(4096)[0]
        strongest = np.sort(np.lexsort((np.arange(len(full)), -full["response"].astype(np.float64)))[:cap])
        assert K.same_keypoints(kp, full[strongest]) is None
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [4096, 2000])
def test_gpu_orb_selection_over_three_tiles(capi, cap):
    ctx = make_ctx(capi, 400, 304)
    ctx.upload_frames(0, tiles_frame()[None])
    kp, desc = ctx.orb_detect_describe_batch([0], params=capi.default_orb_params(**ORB_TILES), cap=cap)[0]
    wk, wd = orb_ref_of(cap)
    assert len(wk) == min(cap, 3000)
    assert K.same_keypoints(kp, wk) is None, K.same_keypoints(kp, wk)
    assert KO.same_descriptors(desc, wd) is None, KO.same_descriptors(desc, wd)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("det", DETECTORS)
def test_gpu_chunk_boundary_both_deliveries(capi, det):
    """A slot list over two resident frames, long enough that the call must run as more than one chunk: every entry equals the
    single-frame result of its slot, from the synchronous call (rows past a frame's count stay as they were, on both sides of the
    boundary) and from the asynchronous call into device memory."""
    import torch
    w, h, cap = 640, 480, 4096
    row, dtype, raw = (64, np.float32, surf_raw_bytes(w, h)) if det == "surf" else (32, np.uint8, orb_raw_bytes(w, h))
    n = chunked_length(raw)
    assert n * raw > CHUNK_BYTES
    ctx = make_ctx(capi, w, h)
    ctx.upload_frames(0, np.stack([K.texture(w, h, 11), K.texture(w, h, 12)]))
    sync_call = getattr(ctx, det + "_detect_describe_batch")
    async_call = getattr(ctx, det + "_detect_describe_batch_async")
    alone = [sync_call([s], cap=cap)[0] for s in (0, 1)]
    assert all(0 < len(k) < cap for k, _ in alone) and alone[0][0].tobytes() != alone[1][0].tobytes()
    slots = [(f * 7 // 3) % 2 for f in range(n)]   # 0 0 0 1 1 1 0 0 0 1 ...: both slots on both sides of any boundary
    assert 0 in slots[:8] and 1 in slots[:8] and 0 in slots[-8:] and 1 in slots[-8:]
    kp = np.zeros((n, cap), capi.KEYPOINT)
    kp.view(np.uint8)[:] = 0xA5
    desc = np.full((n, cap, row), 9, dtype)
    cnt = np.full(n, -1, np.int32)
    got = sync_call(slots, cap=cap, out=(kp, desc, cnt))
    for f, s in enumerate(slots):
        m = len(alone[s][0])
        assert cnt[f] == m, (f, s)
        assert got[f][0].tobytes() == alone[s][0].tobytes() and got[f][1].tobytes() == alone[s][1].tobytes(), (f, s)
    for f, s in enumerate(slots):
        m = len(alone[s][0])
        assert (kp[f, m:].view(np.uint8) == 0xA5).all() and (desc[f, m:] == 9).all(), (f, s)
    d_kp = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((n, cap, row), dtype=torch.float32 if det == "surf" else torch.uint8, device="cuda")
    d_cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
    async_call(slots, d_kp.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap=cap)
    ctx.sync()
    a_cnt = d_cnt.cpu().numpy()
    a_kp = d_kp.cpu().numpy().view(capi.KEYPOINT).reshape(n, cap)
    a_desc = d_desc.cpu().numpy()
    assert a_cnt.tolist() == cnt.tolist()
    for f, s in enumerate(slots):
        m = len(alone[s][0])
        assert a_kp[f, :m].tobytes() == alone[s][0].tobytes() and a_desc[f, :m].tobytes() == alone[s][1].tobytes(), (f, s)
    ctx.close()
