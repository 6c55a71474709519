"""Block-resident texture sets on the CPU: the block layout, the per-texel fetch against the decoded chain and the bytes of
niagara's decoder (tests/golden/textures/bc_blocks.npz), the alpha-only decode and the BC7 header / per-texel split against the plain decode,
the block sampler against the decoded sampler bit for bit, the descriptor check, the ABI, and tools/texture_block_check.cpp under the host
sanitizers.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_textures_gpu as TG
from niagara_amd import host
from niagara_amd import layouts as L
from niagara_amd._lib import DdsInfo, NvError, lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMATS = [("bc1", 1), ("bc2", 2), ("bc3", 3), ("bc7", 7)]
EINVAL, ETEXFORMAT = -1, -7


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "textures", "bc_blocks.npz"))


def _words(block):
    b = np.zeros(16, np.uint8)
    b[:len(block)] = block
    lo, hi = b.view("<u8")
    return int(lo), int(hi)


def _units(payload_bytes):
    return (payload_bytes + 15) // 16


# ---- addressing

@pytest.mark.parametrize("name,fmt", FORMATS)
def test_fetch_equals_the_decoded_chain_at_every_texel(name, fmt, golden):
    """a 20 x 12 texture with its five levels (partial blocks, the 2 x 1 and 1 x 1 tail) and a 4n x 4 strip of all the fixture's blocks:
    nv_texture_block_fetch_host at every (level, x, y) is the word nv_texture_decode_host put there; the strip is the fixture's *_rgba"""
    blocks, want = golden[name], golden[name + "_rgba"]
    n = len(blocks)
    rng = np.random.default_rng(fmt)
    files = [TG._dds(fmt, 20, 12, 5, blocks[rng.integers(0, n, 25)]), TG._dds(fmt, 4 * n, 4, 1, blocks)]
    descs, texels = host.texture_decode_host(files)
    bdescs, buf = host.texture_blocks_host(files)
    assert len(buf) % 16 == 0 and [int(d["levelsFormat"]) for d in bdescs] == [0, 5 | fmt << 8, 1 | fmt << 8]
    for i in (1, 2):
        w0, h0, levels = (int(descs[i][k]) for k in ("width", "height", "levels"))
        at = int(descs[i]["offset"])
        for level in range(levels):
            w, h = max(1, w0 >> level), max(1, h0 >> level)
            got = np.array([[host.texture_block_fetch_host(bdescs[i], buf, level, x, y) for x in range(w)] for y in range(h)], np.uint32)
            assert got.tobytes() == texels[at:at + w * h].tobytes(), (name, i, level)
            at += w * h
            if i == 2:
                strip = np.ascontiguousarray(got.reshape(4, n, 4).transpose(1, 0, 2)).reshape(n, 16).view(np.uint8).reshape(n, 64)
                assert strip.tobytes() == want.tobytes()
            for bad in ((level, w, 0), (level, 0, h)):
                with pytest.raises(NvError):
                    host.texture_block_fetch_host(bdescs[i], buf, *bad)
        with pytest.raises(NvError):
            host.texture_block_fetch_host(bdescs[i], buf, levels, 0, 0)


# ---- the alpha-only decode and the BC7 split

@pytest.mark.parametrize("name,fmt", FORMATS)
def test_alpha_decode_and_bc7_split_equal_the_plain_decode_on_every_fixture_block(name, fmt, golden):
    blocks, want = golden[name], golden[name + "_rgba"].reshape(-1, 16, 4)
    if fmt == 7:
        assert int((blocks[:, 0] == 0).sum()) == 32  # the reserved-mode blocks are in
    rotated = 0
    for block, rgba in zip(blocks, want):
        lo, hi = _words(block)
        alpha, split = host.texture_block_decode_host(fmt, lo, hi)
        assert alpha.tolist() == rgba[:, 3].tolist()                 # == tx_decode_texel(...) >> 24: the fixture pins that decode
        assert split.tobytes() == rgba.view(np.uint32).tobytes()
        if fmt == 7 and block[0] & 0x30 and not block[0] & 0x0F:     # modes 4 and 5 carry the rotation
            mode = 4 if block[0] & 0x10 else 5
            rotated += ((lo >> (mode + 1)) & 3) != 0
    assert fmt != 7 or rotated >= 32, "no rotated BC7 block in the fixture"
    with pytest.raises(NvError):
        host.texture_block_decode_host(4, 0, 0)


# ---- the sampler

def _samples(descs):
    """one list for the five textures from a fixed seed: (texture id, uv, duvdx, duvdy, tag)"""
    rng = np.random.default_rng(2024)
    out = []
    for tid in range(1, len(descs)):
        W, H, levels = (int(descs[tid][k]) for k in ("width", "height", "levels"))
        for _ in range(400):  # anywhere over several periods, derivatives over every level
            uv = rng.uniform(-2.5, 2.5, 2)
            s = 2.0 ** rng.uniform(-16, 1)
            out.append((tid, uv, rng.uniform(-1, 1, 2) * s, rng.uniform(-1, 1, 2) * s, "random"))
        z = (0.0, 0.0)
        if W >= 8:
            out.append((tid, ((4.0) / W, (1.5) / H if H > 1 else 0.5), z, z, "edge-x"))     # u * W - 0.5 = 3.5: texels 3 | 4, a block edge
        if H >= 8:
            out.append((tid, ((1.5) / W, (4.0) / H), z, z, "edge-y"))
        if W > 1:
            out.append((tid, (0.25 / W, 0.5), z, z, "wrap-x"))                              # u * W - 0.5 = -0.25: i0 = W - 1, i1 = 0
        if H > 1:
            out.append((tid, (0.5, 0.25 / H), z, z, "wrap-y"))
        if levels >= 3:
            out.append((tid, (0.3, 0.7), (2.8 / W, 0.0), (0.0, 2.8 / H), "fraction"))       # lambda = log2(2.8) = 1.49: levels 1 and 2
        out.append((tid, (0.3, 0.7), (1e3, 0.0), (0.0, 1e3), "top"))                        # lambda far past the last level
        for bad in (np.nan, np.inf, -np.inf):
            out.append((tid, (bad, 0.25), z, z, "nonfinite-uv"))
            out.append((tid, (0.25, bad), (0.01, 0.0), z, "nonfinite-uv"))
            out.append((tid, (0.4, 0.6), (bad, 0.0), (0.0, 0.01), "nonfinite-derivative"))
            out.append((tid, (0.4, 0.6), (0.0, 0.01), (0.0, bad), "nonfinite-derivative"))
    return out


def _axis(x, size):
    """texmath.h's tx_axis in fp32: (i0, i1)"""
    x = np.float32(x)
    s = x - np.floor(x)
    u = np.float32(np.float32(s * np.float32(size)) - np.float32(0.5))
    i = int(np.floor(u))
    return (i + size if i < 0 else i), (i + 1 - size if i + 1 >= size else i + 1)


def test_block_sampler_equals_the_decoded_sampler_bit_for_bit():
    files = TG._texture_files(np.random.default_rng(23))
    descs, texels = host.texture_decode_host(files)
    bdescs, buf = host.texture_blocks_host(files)
    samples = _samples(descs)
    # the list contains what it must: asserted from the sampler's own index rule
    seen = set()
    for tid, uv, dx, dy, tag in samples:
        W, H, levels = (int(descs[tid][k]) for k in ("width", "height", "levels"))
        if tag in ("edge-x", "wrap-x"):
            i0, i1 = _axis(uv[0], W)
            assert (i0 >> 2 != i1 >> 2 and i1 == i0 + 1) if tag == "edge-x" else (i0 == W - 1 and i1 == 0)
        if tag in ("edge-y", "wrap-y"):
            i0, i1 = _axis(uv[1], H)
            assert (i0 >> 2 != i1 >> 2 and i1 == i0 + 1) if tag == "edge-y" else (i0 == H - 1 and i1 == 0)
        if tag in ("fraction", "top"):
            rho = max(np.hypot(dx[0] * W, dx[1] * H), np.hypot(dy[0] * W, dy[1] * H))
            lam = np.log2(rho)
            assert (lam % 1 > 0.1 and int(lam) + 1 < levels) if tag == "fraction" else lam > levels
        seen.add(tag)
    assert seen == {"random", "edge-x", "edge-y", "wrap-x", "wrap-y", "fraction", "top", "nonfinite-uv", "nonfinite-derivative"}
    differ = 0
    with np.errstate(all="ignore"):
        for tid, uv, dx, dy, tag in samples:
            a = host.texture_block_sample_host(bdescs, buf, tid, uv, dx, dy)
            b = host.texture_sample_host(descs, texels, tid, uv, dx, dy)
            nan = np.isnan(a) & np.isnan(b)  # a NaN for a NaN (§4.13: sign and payload are no result)
            differ += int(((a.view(np.uint32) != b.view(np.uint32)) & ~nan).any())
    assert differ == 0, "%d of %d samples differ" % (differ, len(samples))


# ---- layout and the descriptor check

def _infos(specs):
    infos = (DdsInfo * len(specs))()
    for i, (fmt, w, h, levels) in enumerate(specs):
        infos[i].format, infos[i].width, infos[i].height, infos[i].levels = fmt, w, h, levels
    return infos


def _layout(specs):
    descs = np.zeros(len(specs) + 1, L.TEXTUREBLOCKDESC)
    units = C.c_uint64(0)
    rc = lib.nv_texture_block_layout(_infos(specs), len(specs), descs.ctypes.data, C.byref(units))
    return rc, descs, int(units.value)


def test_layout_places_each_payload_rounded_up_to_16_bytes():
    files = TG._texture_files(np.random.default_rng(23)) + [TG._dds(1, 4, 4, 1, np.zeros(8, np.uint8)), TG._dds(1, 20, 12, 5, np.zeros(25 * 8, np.uint8))]
    bdescs, units, infos = host.texture_block_layout(files)
    payloads = [int(infos[i].payloadBytes) for i in range(len(files))]
    assert any(p % 16 for p in payloads)  # the BC1 textures of 1 and 25 blocks do not fill their last unit
    assert bdescs[0].tolist() == (0, 0, 0, 0)
    at = 0
    for i, p in enumerate(payloads):
        assert int(bdescs[i + 1]["offset"]) == at
        assert int(bdescs[i + 1]["levelsFormat"]) == infos[i].levels | infos[i].format << 8
        assert (int(bdescs[i + 1]["width"]), int(bdescs[i + 1]["height"])) == (infos[i].width, infos[i].height)
        at += _units(p)
    assert units == at == sum(_units(p) for p in payloads)
    # the resident bytes against the decoded set: 8 x for BC1, 4 x for the rest, up to the partial blocks
    words = host.texture_set_layout(files)[1]
    assert units * 16 < words * 4 / 2
    _, buf = host.texture_blocks_host(files)
    for i, f in enumerate(files):
        payload = np.frombuffer(f, np.uint8)[infos[i].payloadOffset:]
        o = int(bdescs[i + 1]["offset"]) * 16
        assert buf[o:o + len(payload)].tobytes() == payload.tobytes()


def test_layout_refuses_what_the_set_layout_refuses():
    table = [((1, 8, 8, 1), 0), ((4, 8, 8, 1), ETEXFORMAT), ((5, 8, 8, 1), ETEXFORMAT), ((6, 8, 8, 1), ETEXFORMAT), ((0, 8, 8, 1), EINVAL), ((8, 8, 8, 1), EINVAL),
             ((1, 0, 8, 1), EINVAL), ((1, 8, 0, 1), EINVAL), ((1, 8, 8, 0), EINVAL), ((1, 16385, 8, 1), EINVAL), ((1, 8, 16385, 1), EINVAL), ((1, 8, 8, 16), EINVAL),
             ((7, 16384, 16384, 15), 0)]
    for spec, want in table:
        rc, _, _ = _layout([spec])
        words = C.c_uint64(0)
        decoded = np.zeros(2, L.TEXTUREDESC)
        rc_decoded = lib.nv_texture_set_layout(_infos([spec]), 1, decoded.ctypes.data, C.byref(words))
        assert rc == want and rc == rc_decoded, (spec, rc, rc_decoded)
    units = C.c_uint64(0)
    assert lib.nv_texture_block_layout(None, 1, np.zeros(2, L.TEXTUREBLOCKDESC).ctypes.data, C.byref(units)) == EINVAL
    assert lib.nv_texture_block_layout(_infos([(1, 8, 8, 1)]), 1, None, C.byref(units)) == EINVAL
    assert lib.nv_texture_block_layout(_infos([(1, 8, 8, 1)]), 1, np.zeros(2, L.TEXTUREBLOCKDESC).ctypes.data, None) == EINVAL
    # a set of 64 GiB is past the 32-bit unit offset: a 16384^2 BC7 chain is 2^24 units x 4 / 3, so 200 of them pass 2^32 units
    rc, _, _ = _layout([(7, 16384, 16384, 15)] * 200)
    assert rc == EINVAL
    rc, descs, units = _layout([(7, 16384, 16384, 15)] * 60)
    assert rc == 0 and units * 16 > 1 << 34 and int(descs[60]["offset"]) * 16 > 1 << 34  # past what a 32-bit word offset of RGBA8 can hold at all


def test_descriptor_check_refuses_a_chain_past_the_buffer_a_foreign_format_and_too_many_levels():
    files = TG._texture_files(np.random.default_rng(23))
    bdescs, buf = host.texture_blocks_host(files)
    last = len(bdescs) - 1
    units = len(buf) // 16
    fetch = lambda d, u=units: host.texture_block_fetch_host(d, buf, 0, 0, 0, units16=u)
    fetch(bdescs[last])
    with pytest.raises(NvError):
        fetch(bdescs[last], units - 1)          # the chain ends one unit past units16
    d = bdescs[last].copy()
    d["offset"] += 1
    with pytest.raises(NvError):
        fetch(d)
    d["offset"] = 0xFFFFFFFF                     # computed in 64 bits: nothing wraps
    with pytest.raises(NvError):
        fetch(d)
    for fmt in (0, 4, 5, 6, 8, 255):
        d = bdescs[1].copy()
        d["levelsFormat"] = 1 | fmt << 8
        with pytest.raises(NvError):
            fetch(d)
    for lf in (16 | 7 << 8, 0 | 7 << 8, 7 | 7 << 8 | 1 << 16, 7 | 7 << 8 | 1 << 31):
        d = bdescs[1].copy()
        d["levelsFormat"] = lf
        with pytest.raises(NvError):
            fetch(d)
    for k, v in (("width", 0), ("height", 0), ("width", 16385), ("height", 16385)):
        d = bdescs[1].copy()
        d[k] = v
        with pytest.raises(NvError):
            fetch(d)
    out = np.zeros(4, np.float32)
    uv = np.zeros(2, np.float32)
    args = lambda tid, u=units: (bdescs.ctypes.data, len(bdescs), buf.ctypes.data, u, tid, uv.ctypes.data, uv.ctypes.data, uv.ctypes.data, out.ctypes.data)
    assert lib.nv_texture_block_sample_host(*args(last)) == 0
    assert [lib.nv_texture_block_sample_host(*args(t)) for t in (0, len(bdescs), 0xFFFFFFFF)] == [EINVAL] * 3
    assert lib.nv_texture_block_sample_host(*args(last, units - 1)) == EINVAL


# ---- ABI

def test_block_descriptor_layout_is_the_headers(tmp_path):
    assert L.TEXTUREBLOCKDESC.itemsize == 16
    assert [L.TEXTUREBLOCKDESC.fields[k][1] for k in ("offset", "width", "height", "levelsFormat")] == [0, 4, 8, 12]
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "niagara_vis.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(NvTextureBlockDesc), '
                   'offsetof(NvTextureBlockDesc, offset), offsetof(NvTextureBlockDesc, width), offsetof(NvTextureBlockDesc, height), '
                   'offsetof(NvTextureBlockDesc, levelsFormat)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"16", b"0", b"4", b"8", b"12"]


# ---- the stand-alone program under the host sanitizers

def test_the_standalone_program_runs_clean_under_the_host_sanitizers(tmp_path, golden):
    """tools/texture_block_check.cpp with texload.cpp, host code only, its own main: AddressSanitizer and UBSan linked statically into the program
    itself.  Once over its own pseudo-random blocks (every BC7 mode forced) and once over the fixture's blocks"""
    exe = tmp_path / "texture_block_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "texture_block_check.cpp"),
                           os.path.join(ROOT, "niagara_amd", "csrc", "texload.cpp"), "-o", str(exe)])
    raw = tmp_path / "fixture_blocks.bin"
    raw.write_bytes(b"".join(golden[n].tobytes() for n in ("bc7", "bc3", "bc2")))
    for argv in ([str(exe)], [str(exe), str(raw)]):
        out = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        print(out.stdout.decode())
        assert out.returncode == 0 and b"texture_block_check: ok" in out.stdout
