"""nv_depth_merge on the MI355X: dst = maximum of dst and every source on the BIT PATTERNS, against np.maximum on uint32.
Ragged sizes (scalar tail), unaligned pointers (scalar path), 1 / 2 / 8 / more-than-one-launch sources, special values by the documented
rule (NaN and negative patterns order by their bits), memory around the targets untouched, and the argument checks."""
import numpy as np
import pytest

SIZES = [(1, 1), (3, 1), (5, 7), (17, 9), (333, 207), (1023, 3), (1920, 1080), (16384, 1), (1, 16384)]
SPECIALS = np.array([0x00000000, 0x3f800000, 0x00000001, 0x007fffff, 0x00800000, 0x3f7fffff, 0x7f800000, 0x7fc00000, 0x7fffffff,
                     0x80000000, 0x80000001, 0xbf800000, 0xff800000, 0xffc00000, 0xffffffff, 0xabababab], np.uint32)
#                    0, 1.0, denormals, the smallest normal, just under 1, +inf, NaNs, -0.0, negative denormal, -1.0, -inf, negative NaNs, the poison


@pytest.fixture(scope="module")
def ctx():
    from niagara_amd import pipeline as P
    c = P.Context()
    yield c
    c.close()


def _bits(rng, n, specials):
    a = rng.uniform(0.0, 1.0, n).astype(np.float32).view(np.uint32)
    if specials:
        pick = rng.random(n) < 0.3
        a[pick] = rng.choice(SPECIALS, int(pick.sum()))
    return a


def _merge(ctx, dst, srcs, w, h, offset=0):
    """runs nv_depth_merge on copies placed `offset` floats into guard-banded device buffers; returns (dst after, guards intact)"""
    import torch
    dev, n, guard = ctx.device, w * h, 64
    def put(a):
        t = torch.from_numpy(np.full(n + 2 * guard + offset, 0xABABABAB, np.uint32).view(np.int32)).to(dev)
        t[guard + offset:guard + offset + n] = torch.from_numpy(a.view(np.int32)).to(dev)
        return t
    td, ts = put(dst), [put(s) for s in srcs]
    view = lambda t: t[guard + offset:guard + offset + n].view(torch.float32)
    ctx.depth_merge(view(td), [view(t) for t in ts], w, h)
    ctx.status()
    out = td.cpu().numpy().view(np.uint32)
    intact = (out[:guard + offset] == 0xABABABAB).all() and (out[guard + offset + n:] == 0xABABABAB).all()
    for t, s in zip(ts, srcs):  # the sources are only read
        intact = intact and t.cpu().numpy().view(np.uint32)[guard + offset:guard + offset + n].tobytes() == s.tobytes()
    return out[guard + offset:guard + offset + n], intact


@pytest.mark.gpu
@pytest.mark.parametrize("sources", [1, 2, 8])
@pytest.mark.parametrize("size", SIZES)
def test_merge_equals_the_maximum_of_the_bit_patterns(ctx, size, sources):
    w, h = size
    rng = np.random.default_rng(w * 31 + h * 7 + sources)
    for specials in (False, True):
        dst = _bits(rng, w * h, specials)
        srcs = [_bits(rng, w * h, specials) for _ in range(sources)]
        want = dst.copy()
        for s in srcs:
            want = np.maximum(want, s)
        got, intact = _merge(ctx, dst, srcs, w, h)
        assert intact and got.tobytes() == want.tobytes()
        if not specials:  # for depth values the bits' maximum IS the floats' maximum
            fl = dst.view(np.float32).copy()
            for s in srcs:
                fl = np.maximum(fl, s.view(np.float32))
            assert got.view(np.float32).tobytes() == fl.tobytes()


@pytest.mark.gpu
def test_every_special_pattern_against_every_other(ctx):
    a, b = np.meshgrid(SPECIALS, SPECIALS)
    a, b = a.reshape(-1).copy(), b.reshape(-1).copy()
    got, intact = _merge(ctx, a, [b], len(a), 1)
    assert intact and got.tobytes() == np.maximum(a, b).tobytes()
    # the documented order: any pattern with the sign bit set is above every positive float, a NaN above the infinity of its sign
    one = np.array([0x3f800000], np.uint32)
    for above in (0x80000000, 0xbf800000, 0x7fc00000):
        got, _ = _merge(ctx, one, [np.array([above], np.uint32)], 1, 1)
        assert got[0] == above


@pytest.mark.gpu
@pytest.mark.parametrize("sources", [9, 17])
def test_more_sources_than_one_launch_folds(ctx, sources):
    rng = np.random.default_rng(sources)
    w, h = 333, 207
    dst = _bits(rng, w * h, True)
    srcs = [_bits(rng, w * h, True) for _ in range(sources)]
    got, intact = _merge(ctx, dst, srcs, w, h)
    assert intact and got.tobytes() == np.maximum.reduce([dst] + srcs).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_pointers_off_the_16_byte_grid_take_the_scalar_path(ctx, offset):
    rng = np.random.default_rng(offset)
    for w, h in ((1, 1), (37, 5), (640, 3)):
        dst = _bits(rng, w * h, True)
        srcs = [_bits(rng, w * h, True) for _ in range(3)]
        got, intact = _merge(ctx, dst, srcs, w, h, offset=offset)
        assert intact and got.tobytes() == np.maximum.reduce([dst] + srcs).tobytes()


@pytest.mark.gpu
def test_repeated_sources_and_a_cleared_destination(ctx):
    """the composite as LocalShards uses it: the first shard's target accumulates the others'; a source may appear twice"""
    rng = np.random.default_rng(5)
    s0, s1 = _bits(rng, 320 * 192, False), _bits(rng, 320 * 192, False)
    got, intact = _merge(ctx, np.zeros(320 * 192, np.uint32), [s0, s1, s0], 320, 192)
    assert intact and got.tobytes() == np.maximum(s0, s1).tobytes()


@pytest.mark.gpu
def test_merge_is_captured_into_a_graph(ctx):
    """it only enqueues: the pointer list is consumed during the call"""
    import torch
    dev = ctx.device
    rng = np.random.default_rng(6)
    a, b, c = (_bits(rng, 333 * 7, False) for _ in range(3))
    ta, tb, tc = (torch.from_numpy(x.view(np.float32).copy()).to(dev) for x in (a, b, c))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            ctx.depth_merge(ta, [tb, tc], 333, 7)
        torch.cuda.synchronize()
        assert ta.cpu().numpy().view(np.uint32).tobytes() == a.tobytes()  # nothing ran during capture
        g.replay()
        torch.cuda.synchronize()
        assert ta.cpu().numpy().view(np.uint32).tobytes() == np.maximum.reduce([a, b, c]).tobytes()
    ctx.status()


@pytest.mark.gpu
def test_argument_checks(ctx):
    import ctypes as C
    import torch
    from niagara_amd._lib import NvError, lib
    d = torch.zeros(64, dtype=torch.float32, device=ctx.device)
    s = torch.ones(64, dtype=torch.float32, device=ctx.device)
    for bad in (lambda: ctx.depth_merge(None, [s], 8, 8), lambda: ctx.depth_merge(d, [], 8, 8), lambda: ctx.depth_merge(d, [s, None], 8, 8),
                lambda: ctx.depth_merge(d, [s], 0, 8), lambda: ctx.depth_merge(d, [s], 8, 0), lambda: ctx.depth_merge(d, [s], 16385, 1),
                lambda: ctx.depth_merge(d, [s], 1, 16385), lambda: ctx.depth_merge(d, [s, d], 8, 8),
                lambda: ctx.depth_merge(d.view(torch.uint8)[1:5].view(torch.uint8), [s], 1, 1)):
        with pytest.raises(NvError):
            bad()
    ptrs = (C.c_void_p * 1)(s.data_ptr())
    assert lib.nv_depth_merge(None, None, C.c_void_p(d.data_ptr()), ptrs, 1, 8, 8) == -1
    assert lib.nv_depth_merge(ctx.h, None, C.c_void_p(d.data_ptr()), None, 1, 8, 8) == -1
    ctx.status()
    assert d.cpu().numpy().tobytes() == np.zeros(64, np.float32).tobytes()  # a refused call enqueues nothing
    ctx.depth_merge(d, [s], 8, 8)
    ctx.status()
    assert (d.cpu().numpy() == 1.0).all()
