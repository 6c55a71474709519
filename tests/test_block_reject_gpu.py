"""The filter form's block test (clustercull.hip BLOCK, filtermath.h block_outside): bit-identical to the oracle where 64-meshlet block
spheres straddle the frustum's planes, for unaligned and short commands, commands in the mirror's last blocks, blocks holding NaN / inf /
65504 bounds, a re-uploaded mirror, two contexts sharing a scene — and the block table itself, read back and checked in exact arithmetic."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import oracle
from niagara_amd import host, synth
from niagara_amd import layouts as L
from niagara_amd import lib
from niagara_amd import pipeline as P

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = P.Context()
    c.set_option(P.NV_OPT_CULL_FORM, 1)  # the filter form, whatever the statistic says
    yield c
    c.close()


def cull_data(n_draws, cam=(0, 0, 0), camq=(0, 0, 0, 1), znear=0.5, draw_distance=300.0):
    return host.build_cull_data(cam_pos=cam, cam_quat=camq, draw_count=n_draws, cullingEnabled=1, clusterBackfaceEnabled=1, draw_distance=draw_distance,
                                znear=znear)


def run_both(c, cd, draws, meshlets, commands, n, upload=True):
    """oracle and GPU for one early pass without visibility bits; returns (count, ids) of each"""
    count4 = synth.count4_for(n)
    cap = int(count4[1]) * 64 * 64 + 256
    cib_o, cc4_o = np.zeros(cap, np.uint32), np.zeros(4, np.uint32)
    oracle.clustercull(cd, 0, commands, count4, draws, meshlets, None, None, cib_o, cc4_o)
    dev = c.device
    db, mlb, dcb = P.to_device(draws, dev), P.to_device(meshlets, dev), P.to_device(commands, dev)
    if upload:
        c.upload_meshlets(mlb, len(meshlets))
    dccb = torch.from_numpy(count4.view(np.int32).copy()).to(dev)
    cib = torch.zeros(cap, dtype=torch.int32, device=dev)
    ccb = torch.zeros(4, dtype=torch.int32, device=dev)
    for _ in range(2):  # the second launch has the first one's statistic and plan
        ccb.zero_()
        c.clustercull(cd, 0, dcb, dccb, db, mlb, None, None, cib, ccb)
    c.status()
    got_n = int(ccb[0].item())
    got = cib.cpu().numpy().view(np.uint32)[:got_n]
    return (int(cc4_o[0]), cib_o[:int(cc4_o[0])]), (got_n, got), (db, mlb)


def assert_same(ref, got, what):
    assert got[0] == ref[0], (what, got[0], ref[0])
    assert got[1].tobytes() == ref[1].tobytes(), what


def block_table(c):
    n = C_u32()
    lib.nv_debug_block_table(c.h, None, 0, n)
    out = np.zeros((n.value, 4), np.uint32)
    assert lib.nv_debug_block_table(c.h, out.ctypes.data, n.value, n) == 0
    return out


def C_u32():
    import ctypes
    return ctypes.c_uint32()


def half(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def check_table_exact(table, meshlets):
    """every meshlet sphere of a block inside its record: ||v_i - C|| <= D and |r_i| <= rho, in exact rationals (squared); non-finite or
    empty blocks carry D = rho = inf"""
    cnt = len(meshlets)
    assert len(table) == (cnt + 63) // 64 + 1
    cen, rad = meshlets["center"], meshlets["radius"]
    for b, rec in enumerate(table):
        lo, hi = b * 64, min(cnt, b * 64 + 64)
        dbits, rbits = int(rec[3]) & 0xffff, int(rec[3]) >> 16
        h = np.concatenate([cen[lo:hi].ravel(), rad[lo:hi]])
        if hi <= lo or ((h & 0x7c00) == 0x7c00).any():
            assert dbits == 0x7c00 and rbits == 0x7c00, b
            continue
        C = [Fraction(float(x)) for x in rec[:3].view(np.float32)]
        D = Fraction(float(half(dbits)))
        for j in range(3):
            v = half(cen[lo:hi, j])
            assert v.min() <= float(C[j]) <= v.max(), b  # the centre lies inside the block's box
        assert float(half(rbits)) >= np.abs(half(rad[lo:hi])).max(), b
        v = cen[lo:hi].astype(np.uint16).view(np.float16).astype(np.float64)
        # fp64 screen, then exact for the meshlets within 2^-30 of the bound
        d2 = ((v - np.array([float(x) for x in C])) ** 2).sum(axis=1)
        assert (d2 <= float(D) ** 2 * (1 + 2.0 ** -30)).all(), b
        for i in np.nonzero(d2 >= float(D) ** 2 * (1 - 2.0 ** -30))[0]:
            assert sum((Fraction(float(v[i, j])) - C[j]) ** 2 for j in range(3)) <= D * D, (b, i)


def test_bench_scene_and_table(ctx):
    """config 3A's geometry at 1/8 scale: nearly every command finished by its block, the rest by pass A / B — identical IDs; the table exact"""
    draws, meshlets, commands, n = synth.cluster_scene(2000, 10, seed=2, scene_radius=300.0)
    cd = cull_data(len(draws))
    ref, got, _ = run_both(ctx, cd, draws, meshlets, commands, n)
    assert ref[0] > 0
    assert_same(ref, got, "3A")
    check_table_exact(block_table(ctx), meshlets)


def test_straddling_planes(ctx):
    """draws placed so that the blocks' spheres straddle each plane (side, near, far) from a few ulps inside to past the margin: blocks made of
    tight meshlet clusters and scaled so that the block bound is close to the meshlets' own"""
    rng = np.random.default_rng(17)
    n_draws, cpd = 1500, 2
    draws, meshlets, commands, n = synth.cluster_scene(n_draws, cpd, seed=5, scene_radius=60.0)
    cen = meshlets["center"].view(np.float16).reshape(-1, 3).astype(np.float64)
    blk = np.repeat(rng.uniform(-1, 1, (len(meshlets) // 64, 3)), 64, axis=0)
    meshlets["center"] = (blk + 0.02 * cen).astype(np.float16).view(np.uint16).reshape(meshlets["center"].shape)
    cd = cull_data(n_draws, znear=1.0, draw_distance=80.0)
    fr, zn, zf = cd["frustum"][0].astype(np.float64), float(cd["znear"][0]), float(cd["zfar"][0])
    # put each draw's position on one of the planes in view space, then nudge it by a random amount from 1e-6 to 3
    pos = np.zeros((n_draws, 3))
    z = rng.uniform(zn + 2, zf - 2, n_draws)
    side = rng.integers(0, 4, n_draws)
    pos[:, 2] = np.where(side == 2, zn, np.where(side == 3, zf, z))
    sgn = rng.choice([-1.0, 1.0], n_draws)
    pos[:, 0] = np.where(side == 0, sgn * z * fr[1] / fr[0], rng.uniform(-0.2, 0.2, n_draws) * z * fr[1] / fr[0])  # (|x| = z f1 / f0 on the side plane)
    pos[:, 1] = np.where(side == 1, sgn * z * fr[3] / fr[2], rng.uniform(-0.2, 0.2, n_draws) * z * fr[3] / fr[2])
    pos += rng.normal(0, 1, (n_draws, 3)) * 10.0 ** rng.uniform(-6, 0.5, (n_draws, 1))
    Vm = cd["view"][0].astype(np.float64).reshape(4, 4).T  # column-major: view space = Vm (world, 1)
    draws["position"] = (np.linalg.inv(Vm) @ np.c_[pos, np.ones(n_draws)].T).T[:, :3].astype(f32)
    draws["scale"] = f32(1.0)
    draws["orientation"] = np.array([0, 0, 0, 1], f32)
    ref, got, _ = run_both(ctx, cd, draws, meshlets, commands, n)
    assert ref[0] > 0
    assert_same(ref, got, "straddle")


def test_unaligned_short_and_last_blocks(ctx):
    """unaligned taskOffset (two blocks), taskCount < 64 and 0, and commands in the mirror's last (partial) block"""
    rng = np.random.default_rng(23)
    draws, meshlets, commands, n = synth.cluster_scene(900, 7, seed=4, scene_radius=120.0)
    meshlets = meshlets[:len(meshlets) - 37]  # a partial last block
    total = len(meshlets)
    tc = rng.integers(0, 65, n).astype(np.uint32)
    off = rng.integers(0, total - 64, n).astype(np.uint32)
    off[::5] = total - tc[::5]  # ranges that end at the mirror's last meshlet
    commands["taskCount"][:n] = tc
    commands["taskOffset"][:n] = off
    cd = cull_data(len(draws))
    ref, got, _ = run_both(ctx, cd, draws, meshlets, commands, n)
    assert_same(ref, got, "unaligned")
    check_table_exact(block_table(ctx), meshlets)


def test_special_values_in_blocks(ctx):
    """blocks holding NaN / inf centres or radii, 65504 and subnormal values: such blocks never finish a command, the others still do"""
    rng = np.random.default_rng(29)
    draws, meshlets, commands, n = synth.cluster_scene(600, 10, seed=6, scene_radius=300.0)
    cen, rad = meshlets["center"], meshlets["radius"]  # (views into the records: the writes below land in them)
    nb = len(meshlets) // 64
    for k, bits in enumerate((0x7e00, 0x7c00, 0xfc00, 0x7bff, 0xfbff, 0x0001, 0x03ff)):
        for b in rng.integers(0, nb, 12):
            i = int(b) * 64 + int(rng.integers(0, 64))
            if k % 2:
                rad[i] = bits
            else:
                cen[i, int(rng.integers(0, 3))] = bits
    ref, got, _ = run_both(ctx, cull_data(len(draws)), draws, meshlets, commands, n)
    assert_same(ref, got, "special")
    check_table_exact(block_table(ctx), meshlets)


def test_reupload_and_shared_scene(ctx):
    """a mirror re-uploaded with different meshlets (same size: the table is rebuilt in place, never stale) and a second context sharing the
    scene"""
    draws, meshlets, commands, n = synth.cluster_scene(1000, 10, seed=2, scene_radius=300.0)
    cd = cull_data(len(draws))
    ref, got, (db, mlb) = run_both(ctx, cd, draws, meshlets, commands, n)
    assert_same(ref, got, "first upload")
    # different meshlets in the same buffer: every centre moved towards the camera's view axis, so that blocks finished before are visible now
    m2 = meshlets.copy()
    m2["center"] = (m2["center"].view(np.float16) * np.float16(0.01)).view(np.uint16)
    m2["radius"] = (m2["radius"].view(np.float16) * np.float16(4.0)).view(np.uint16)
    ref2, got2, _ = run_both(ctx, cd, draws, m2, commands, n)
    assert ref2[1].tobytes() != ref[1].tobytes()
    assert_same(ref2, got2, "re-upload")
    check_table_exact(block_table(ctx), m2)
    other = P.Context()
    try:
        other.set_option(P.NV_OPT_CULL_FORM, 1)
        other.share_scene(ctx)
        count4 = synth.count4_for(n)
        dev = ctx.device
        db2, mlb2, dcb = P.to_device(draws, dev), P.to_device(m2, dev), P.to_device(commands, dev)
        ctx.upload_meshlets(mlb2, len(m2))  # registered through the sharing scene: `other` culls over the same mirror and table
        dccb = torch.from_numpy(count4.view(np.int32).copy()).to(dev)
        cib = torch.zeros(int(count4[1]) * 64 * 64 + 256, dtype=torch.int32, device=dev)
        ccb = torch.zeros(4, dtype=torch.int32, device=dev)
        other.clustercull(cd, 0, dcb, dccb, db2, mlb2, None, None, cib, ccb)
        other.status()
        k = int(ccb[0].item())
        assert k == ref2[0] and cib.cpu().numpy().view(np.uint32)[:k].tobytes() == ref2[1].tobytes()
    finally:
        other.close()
