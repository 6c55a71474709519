"""The BC7 decode on every partition and header field, on the CPU: tests/golden/textures/bc7_fields.npz holds blocks that
walk every (mode, partition) pair of the partitioned modes, every rotation and index selection of modes 4 and 5, every p-bit pair of mode 6
and the extremes of the index and endpoint fields, with the bytes niagara's decoder writes for them.  What the file must contain is asserted
from its blocks alone; then every block goes bit for bit through each host decode path of texmath.h and through tests/texture_ref.c, and the
generator's recipe is rerun where a niagara checkout is present.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_textures_gpu as TG
import texture_ref as TR
from niagara_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
TEXTURES = os.path.join(HERE, "golden", "textures")
REFERENCE = "/root/reference"  # the tree oracle.build() translates from; absent on most machines
PARTITIONED = {0: 4, 1: 6, 2: 6, 3: 6, 7: 6}  # mode: partition bits
# mode: (subsets, partition, rotation, selection, colour, alpha, p-bits, index, index2 bits): the BPTC block layout, fields in this order from bit mode + 1
LAYOUT = {0: (3, 4, 0, 0, 4, 0, 6, 3, 0), 1: (2, 6, 0, 0, 6, 0, 2, 3, 0), 2: (3, 6, 0, 0, 5, 0, 0, 2, 0), 3: (2, 6, 0, 0, 7, 0, 4, 2, 0),
          4: (1, 0, 2, 1, 5, 6, 0, 2, 3), 5: (1, 0, 2, 0, 7, 8, 0, 2, 2), 6: (1, 0, 0, 0, 7, 7, 2, 4, 0), 7: (2, 6, 0, 0, 5, 5, 4, 2, 0)}


def header(block):
    """the header fields of one BC7 block, parsed here from its bits: dict(mode, partition, rotation, selection, pbits, index, index_bits) — index is
    the whole primary index field as one integer of index_bits bits; mode -1: reserved"""
    v = int.from_bytes(bytes(bytearray(block)), "little")
    if v & 255 == 0:
        return dict(mode=-1)
    mode = (v & -v).bit_length() - 1
    ns, pb, rb, sb, cb, ab, pbits, ib, ib2 = LAYOUT[mode]
    out, at = dict(mode=mode), mode + 1
    for name, n in (("partition", pb), ("rotation", rb), ("selection", sb), ("endpoints", 6 * ns * cb + 2 * ns * ab), ("pbits", pbits), ("index", 16 * ib - ns)):
        out[name] = v >> at & ((1 << n) - 1)
        at += n
    out["index_bits"] = 16 * ib - ns
    assert at + (16 * ib2 - 1 if ib2 else 0) == 128
    return out


@pytest.fixture(scope="module")
def fields():
    f = np.load(os.path.join(TEXTURES, "bc7_fields.npz"))
    return f["bc7"], f["bc7_rgba"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return TR.load(tmp_path_factory.mktemp("texture_ref_bc7_fields"))


# ---- the input condition

def test_the_fixture_walks_every_partition_and_field(fields):
    blocks, want = fields
    assert blocks.shape == (672, 16) and want.shape == (672, 64) and blocks.dtype == want.dtype == np.uint8
    assert os.path.getsize(os.path.join(TEXTURES, "bc7_fields.npz")) < 96 * 1024
    heads = [header(b) for b in blocks]
    assert all(h["mode"] >= 0 for h in heads)
    pairs = {(h["mode"], h["partition"]) for h in heads if h["mode"] in PARTITIONED}
    assert pairs == {(m, p) for m, bits in PARTITIONED.items() for p in range(1 << bits)} and len(pairs) == 272
    assert {(h["rotation"], h["selection"]) for h in heads if h["mode"] == 4} == {(r, s) for r in range(4) for s in range(2)}
    assert {h["rotation"] for h in heads if h["mode"] == 5} == {0, 1, 2, 3}
    assert {h["pbits"] for h in heads if h["mode"] == 6} == {0, 1, 2, 3}
    for mode in range(8):
        index = [(h["index"], h["index_bits"]) for h in heads if h["mode"] == mode]
        assert any(i == 0 for i, n in index), mode
        assert any(i == (1 << n) - 1 for i, n in index), mode


# ---- every block through every host path

def _words(block):
    lo, hi = np.ascontiguousarray(block, np.uint8).view("<u8")
    return int(lo), int(hi)


def test_the_strip_decode_equals_the_reference_decoders_bytes(fields):
    blocks, want = fields
    n = len(blocks)
    descs, texels = host.texture_decode_host([TG._dds(7, 4 * n, 4, 1, blocks)])
    assert descs[1].tolist() == (0, 4 * n, 4, 1)
    got = np.ascontiguousarray(texels.reshape(4, n, 4).transpose(1, 0, 2)).reshape(n, 16).view(np.uint8).reshape(n, 64)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "blocks %s differ; first: %s" % (bad[:8], header(blocks[bad[0]]))


def test_the_block_fetch_equals_the_reference_decoders_bytes_at_every_texel(fields):
    blocks, want = fields
    n = len(blocks)
    bdescs, buf = host.texture_blocks_host([TG._dds(7, 4 * n, 4, 1, blocks)])
    got = np.array([[host.texture_block_fetch_host(bdescs[1], buf, 0, x, y) for x in range(4 * n)] for y in range(4)], np.uint32)
    got = np.ascontiguousarray(got.reshape(4, n, 4).transpose(1, 0, 2)).reshape(n, 16)
    bad = np.nonzero((got != want.view(np.uint32).reshape(n, 16)).any(axis=1))[0]
    assert len(bad) == 0, "blocks %s differ; first: %s" % (bad[:8], header(blocks[bad[0]]))


def test_the_alpha_decode_and_the_header_split_equal_the_reference_decoders_bytes(fields):
    blocks, want = fields
    for i, (block, rgba) in enumerate(zip(blocks, want.reshape(-1, 16, 4))):
        alpha, split = host.texture_block_decode_host(7, *_words(block))
        assert alpha.tolist() == rgba[:, 3].tolist(), (i, header(block))
        assert split.tobytes() == rgba.view(np.uint32).tobytes(), (i, header(block))


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_the_restatement_equals_the_reference_decoders_bytes_in_both_builds(real, fields, ref):
    blocks, want = fields
    out = np.zeros((len(blocks), 16), np.uint32)
    for i in range(len(blocks)):
        ref.libs[real].tr_decode_block(C.c_uint32(7), TR._p(np.ascontiguousarray(blocks[i])), TR._p(out[i]))
    got = out.view(np.uint8).reshape(len(blocks), 64)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "blocks %s differ; first: %s" % (bad[:8], header(blocks[bad[0]]))


# ---- the stand-alone program under the host sanitizers, over these blocks

def test_the_standalone_program_runs_clean_over_the_fixture_blocks(fields, tmp_path):
    """tools/texture_block_check.cpp (host code only, its own main, AddressSanitizer and UBSan linked statically: test_texture_blocks_cpu.py's build)
    fills its textures from the file it is given; its 256 x 64 BC7 chain alone takes more blocks than the fixture has, so every block is decoded
    through the fetch, the alpha-only decode and the header split there — the all-zero and all-one fields are where a shift could leave its range"""
    root = os.path.dirname(HERE)
    exe = tmp_path / "texture_block_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tools", "texture_block_check.cpp"),
                           os.path.join(root, "niagara_amd", "csrc", "texload.cpp"), "-o", str(exe)])
    raw = tmp_path / "bc7_fields.bin"
    raw.write_bytes(fields[0].tobytes())
    out = subprocess.run([str(exe), str(raw)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(out.stdout.decode())
    assert out.returncode == 0 and b"texture_block_check: ok" in out.stdout


# ---- the recipe

@pytest.mark.skipif(not os.path.exists(os.path.join(REFERENCE, "extern", "bcdec.h")), reason="no reference tree (oracle/_ref is built from it where it exists)")
def test_the_generator_reproduces_both_committed_fixtures(tmp_path):
    out = tmp_path / "out"
    subprocess.check_call([sys.executable, os.path.join(HERE, "golden", "generate_bc.py"), "--reference", REFERENCE, "--scratch", str(tmp_path / "scratch"),
                           "--out", str(out)], stdout=subprocess.DEVNULL)
    for name in ("bc_blocks.npz", "bc7_fields.npz"):
        a, b = np.load(os.path.join(TEXTURES, name)), np.load(str(out / name))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
