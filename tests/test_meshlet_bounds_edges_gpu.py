"""SURVEY.md §8(f) N2 at its edges, on the device: nv_meshlet_bounds against orc_meshlet_bounds on the named cases of
tests/bounds_cases.py (tests/test_meshlet_bounds_edges_cpu.py holds the oracle to a second restatement on the same cases) —
one buffer, one launch, records and floats byte for byte; partial workgroups with poisoned records behind the count; count 0."""
import numpy as np
import pytest

import oracle
from niagara_amd import layouts as L

import bounds_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    meshlets, data, vertices, names = C.build()
    want = meshlets.copy()
    f = oracle.meshlet_bounds(vertices, data, want, want_float=True)
    return meshlets, data, vertices, names, want, f


@pytest.fixture(scope="module")
def device(cases):
    import torch
    from niagara_amd import pipeline as P
    ctx = P.Context()
    vb = P.to_device(np.ascontiguousarray(cases[2]), ctx.device)
    dd = torch.from_numpy(cases[1].view(np.int32).copy()).to(ctx.device)
    yield ctx, vb, dd
    ctx.close()


def _differences(names, got, want, gf=None, wf=None, index=None):
    g, w = got.view(np.uint8).reshape(-1, 24), want.view(np.uint8).reshape(-1, 24)
    lines = []
    for k in range(len(g)):
        name = names[k if index is None else index[k]]
        if g[k].tobytes() != w[k].tobytes():
            lines.append("%s (meshlet %d)\n  device %s\n  oracle %s" % (name, k, g[k].tobytes().hex(" ", 4), w[k].tobytes().hex(" ", 4)))
        if gf is not None and gf[k].tobytes() != wf[k].tobytes():
            lines.append("%s (meshlet %d) floats\n  device %s\n  oracle %s" % (name, k, gf[k].tobytes().hex(" ", 4), wf[k].tobytes().hex(" ", 4)))
    if lines:
        print("\n".join(lines[:40]))
    return len(lines)


def test_all_groups_in_one_launch_equal_the_oracle(cases, device):
    import torch
    from niagara_amd import pipeline as P
    meshlets, data, vertices, names, want, wf = cases
    ctx, vb, dd = device
    n = len(meshlets)
    mlb = P.to_device(meshlets.copy(), ctx.device)
    f = torch.full((n, 8), float("nan"), dtype=torch.float32, device=ctx.device)
    ctx.meshlet_bounds(vb, dd, mlb, n, f)
    ctx.status()
    got, gf = P.from_device(mlb, L.MESHLET).copy(), f.cpu().numpy()
    assert _differences(names, got, want, gf, wf) == 0
    # without the float output, from a zero pre-fill, then a second time in place
    zeroed = meshlets.copy()
    zeroed.view(np.uint8).reshape(-1, 24)[:, :12] = 0
    mlb2 = P.to_device(zeroed, ctx.device)
    ctx.meshlet_bounds(vb, dd, mlb2, n)
    ctx.status()
    assert _differences(names, P.from_device(mlb2, L.MESHLET).copy(), want) == 0
    ctx.meshlet_bounds(vb, dd, mlb2, n)
    ctx.status()
    assert _differences(names, P.from_device(mlb2, L.MESHLET).copy(), want) == 0


def _interleaved(first):
    """growth and tie meshlets in turn, beginning with group `first`; of the ties the hand-made orders (a first occurrence in a
    higher lane or a later slice) come before the planar grids"""
    names, groups = C.build()[3], C.groups()
    ties = sorted(groups["ties"], key=lambda k: ("first at" not in names[k], k))
    pair = (list(groups["growth"]), ties) if first == "growth" else (ties, list(groups["growth"]))
    return [x for two in zip(*pair) for x in two]


@pytest.mark.parametrize("first", ["growth", "ties"])
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 9])
def test_partial_workgroups_leave_everything_behind_the_count_alone(cases, device, count, first):
    """prefixes of the growth and tie groups, taken in turn and beginning with either: the last workgroup has idle waves; one
    poisoned record and eight poisoned floats sit behind the count"""
    import torch
    from niagara_amd import pipeline as P
    meshlets, data, vertices, names, want, wf = cases
    ctx, vb, dd = device
    index = _interleaved(first)[:count]
    assert len(index) == count and names[index[0]].startswith(first)
    held = {names[k].split("/")[0] for k in index}
    assert held == ({"growth", "ties"} if count >= 2 else {first})
    if first == "ties" or count >= 2:
        assert any("first at" in names[k] for k in index)  # a tie whose first occurrence is not in the lowest lane's first slice
    poison = np.zeros(1, L.MESHLET)
    poison.view(np.uint8)[:] = 0xC3  # as an input it would be 64 vertices at a far offset: it must not be read either
    buf = np.concatenate([meshlets[index], poison])
    mlb = P.to_device(buf.copy(), ctx.device)
    f = torch.full((count + 1, 8), -123.5, dtype=torch.float32, device=ctx.device)
    ctx.meshlet_bounds(vb, dd, mlb, count, f)
    ctx.status()
    got, gf = P.from_device(mlb, L.MESHLET).copy(), f.cpu().numpy()
    assert _differences(names, got[:count], want[index], gf[:count], wf[index], index) == 0
    assert got[count:].tobytes() == poison.tobytes() and (gf[count] == -123.5).all()
    assert (got.view(np.uint8).reshape(-1, 24)[:, 12:] == buf.view(np.uint8).reshape(-1, 24)[:, 12:]).all()


def test_a_count_of_zero_launches_nothing(cases, device):
    import torch
    from niagara_amd import lib
    from niagara_amd import pipeline as P
    meshlets = cases[0]
    ctx, vb, dd = device
    mlb = P.to_device(meshlets[:2].copy(), ctx.device)
    f = torch.full((2, 8), -123.5, dtype=torch.float32, device=ctx.device)
    assert lib.nv_meshlet_bounds(ctx.h, P._stream(), P._ptr(vb), P._ptr(dd), P._ptr(mlb), 0, P._ptr(f)) == 0
    ctx.status()
    assert P.from_device(mlb, L.MESHLET).tobytes() == meshlets[:2].tobytes() and (f.cpu().numpy() == -123.5).all()
