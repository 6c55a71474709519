"""Generator of tests/golden/textures/bc_blocks.npz and bc7_fields.npz: BC1 / BC2 / BC3 / BC7 blocks and the 64 RGBA8 bytes niagara's CPU decoder
(the one behind decodeImageRGBA, src/textures.cpp:295) produces for each.  The fixtures are the DEFINITION of the decode; they
are regenerated only by hand (tests/test_bc7_fields_cpu.py reruns the recipe into a temporary directory where a checkout is present and holds
the committed arrays to it):

    python tests/golden/generate_bc.py --reference <niagara checkout> [--scratch <dir>] [--out <dir>]

A throw-away C program is written into the scratch directory; it includes the checkout's decoder header by path and is compiled with the host
compiler (a plain build, no sanitizer).  Nothing of the checkout is copied into this tree; the tests read the .npz only.

Contents (uint8 arrays): bc7 (64 blocks per mode 0-7 with the mode bits forced and the rest random, then 32 reserved blocks: mode byte 0),
bc1 (256: c0 > c1, c0 <= c1 with every index, equal endpoints), bc2 (128), bc3 (256: a0 > a1, a0 <= a1, equal endpoints); <name>_rgba holds the
decoder's output, 64 bytes per block, row-major texels.

bc7_fields.npz (uint8 arrays bc7, bc7_rgba; 672 blocks from a generator of their own, so bc_blocks.npz's stream is untouched) walks the BC7 header
fields and tables the 64 random blocks per mode above leave holes in:
  pairs     modes 0, 1, 2, 3, 7 x every partition (16 + 4 x 64 = 272 pairs) x 2 random blocks: every row of the subset and anchor tables
  fields    mode 4: every rotation x both index selections, 4 blocks each; mode 5: every rotation, 4 each; mode 6: every pair of p-bits, 4 each
  extremes  8 per mode (a random partition where the mode has one):
            0, 1  every payload bit 0; every payload bit 1
            2, 3  every index field 0; every index field 1 — random endpoints: each texel IS an endpoint (unpack, p-bit, bit replication)
            4, 5  even endpoints (and their p-bits) all 0 against odd ones all 1, and the reverse — random indices: weights over the full range
            6, 7  modes 4, 5: primary indices all 0 with secondary all 1, and the reverse (mode 4: index selection 0, then 1);
                  the other modes: the endpoints of 4 and 5 under the index ramp t mod 2^bits, so every weight of the mode occurs
"""
import argparse
import os
import subprocess
import tempfile

import numpy as np

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#define BCDEC_IMPLEMENTATION
#include "%s"
int main(int argc, char** argv)
{
    int format = atoi(argv[1]), size = format == 1 ? 8 : 16;
    unsigned char block[16], rgba[64];
    while (fread(block, 1, size, stdin) == (size_t)size)
    {
        switch (format)
        {
        case 1: bcdec_bc1(block, rgba, 16); break;
        case 2: bcdec_bc2(block, rgba, 16); break;
        case 3: bcdec_bc3(block, rgba, 16); break;
        default: bcdec_bc7(block, rgba, 16); break;
        }
        fwrite(rgba, 1, 64, stdout);
    }
    return 0;
}
"""


def blocks(rng):
    out = {}
    # BC7: the mode is the position of the lowest set bit of byte 0
    b7 = rng.integers(0, 256, (8 * 64 + 32, 16), dtype=np.uint8)
    for mode in range(8):
        rows = slice(mode * 64, mode * 64 + 64)
        b7[rows, 0] = (b7[rows, 0] & ~np.uint8((2 << mode) - 1)) | np.uint8(1 << mode)
    b7[8 * 64:, 0] = 0
    out["bc7"] = b7

    def colour(n):
        c = rng.integers(0, 256, (n, 8), dtype=np.uint8)
        w = c[:, :4].copy().view("<u2")  # (n, 2): c0, c1
        k = n // 8
        lo, hi = np.minimum(w[:, 0], w[:, 1]), np.maximum(w[:, 0], w[:, 1])
        w[: 3 * k, 0], w[: 3 * k, 1] = hi[: 3 * k], lo[: 3 * k]                     # c0 >= c1 (mostly >)
        w[3 * k : 6 * k, 0], w[3 * k : 6 * k, 1] = lo[3 * k : 6 * k], hi[3 * k : 6 * k]  # c0 <= c1: three colours and transparent
        w[6 * k :, 1] = w[6 * k :, 0]                                                # equal endpoints
        c[:, :4] = w.view(np.uint8)
        c[3 * k, 4:] = (0x1B, 0xE4, 0xFF, 0x00)                                       # every index in both orders
        return c

    out["bc1"] = colour(256)
    out["bc2"] = np.concatenate([rng.integers(0, 256, (128, 8), dtype=np.uint8), colour(128)], axis=1)
    a = rng.integers(0, 256, (256, 8), dtype=np.uint8)
    lo, hi = np.minimum(a[:, 0], a[:, 1]), np.maximum(a[:, 0], a[:, 1])
    a[:96, 0], a[:96, 1] = hi[:96], lo[:96]            # a0 >= a1: six interpolants
    a[96:192, 0], a[96:192, 1] = lo[96:192], hi[96:192]  # a0 <= a1: four interpolants, 0 and 255
    a[192:, 1] = a[192:, 0]                            # equal endpoints
    a[96, 2:] = (0x88, 0xC6, 0xFA, 0x88, 0xC6, 0xFA)   # the indices 0..7 twice over
    out["bc3"] = np.concatenate([a, colour(256)], axis=1)
    return out


# BC7 block layout, restated from the format's definition (Khronos Data Format Specification, BPTC): per mode the subsets, the bits of the
# partition, rotation, index selection, of a colour and an alpha endpoint channel, the p-bits (per endpoint / shared per subset) and the bits
# of a primary and a secondary index.  Fields follow one another from bit mode + 1 in this order; every mode sums to 128.
BC7_MODES = {  # mode: (subsets, partition, rotation, selection, colour, alpha, p-bits, index, index2)
    0: (3, 4, 0, 0, 4, 0, 6, 3, 0), 1: (2, 6, 0, 0, 6, 0, 2, 3, 0), 2: (3, 6, 0, 0, 5, 0, 0, 2, 0), 3: (2, 6, 0, 0, 7, 0, 4, 2, 0),
    4: (1, 0, 2, 1, 5, 6, 0, 2, 3), 5: (1, 0, 2, 0, 7, 8, 0, 2, 2), 6: (1, 0, 0, 0, 7, 7, 2, 4, 0), 7: (2, 6, 0, 0, 5, 5, 4, 2, 0),
}


def bc7_fields(mode):
    """name -> (first bit, bits) of the fields of a BC7 block of `mode`"""
    ns, pb, rb, sb, cb, ab, pbits, ib, ib2 = BC7_MODES[mode]
    out, at = {}, mode + 1
    for name, n in (("partition", pb), ("rotation", rb), ("selection", sb), ("colour", 6 * ns * cb), ("alpha", 2 * ns * ab), ("pbits", pbits),
                    ("index", 16 * ib - ns), ("index2", 16 * ib2 - 1 if ib2 else 0)):
        out[name] = (at, n)
        at += n
    assert at == 128, (mode, at)
    return out


def _put(v, field, value):
    at, n = field
    mask = ((1 << n) - 1) << at
    return (v & ~mask) | ((value << at) & mask)


def _endpoints(v, mode, even, odd):
    """every even endpoint's channels (and p-bit) all `even` (0 / 1), every odd endpoint's all `odd`; a shared p-bit is left as it is"""
    ns, pb, rb, sb, cb, ab, pbits, ib, ib2 = BC7_MODES[mode]
    f = bc7_fields(mode)
    for name, bits, channels in (("colour", cb, 3), ("alpha", ab, 1 if ab else 0)):
        for c in range(channels):
            for e in range(2 * ns):
                v = _put(v, (f[name][0] + (c * 2 * ns + e) * bits, bits), -1 if (odd if e & 1 else even) else 0)
    if pbits == 2 * ns:
        for e in range(2 * ns):
            v = _put(v, (f["pbits"][0] + e, 1), odd if e & 1 else even)
    return v


def _ramp(v, mode, anchors):
    """primary index of texel t := t mod 2^bits (an anchor texel keeps the bits it has)"""
    ib = BC7_MODES[mode][7]
    at = bc7_fields(mode)["index"][0]
    for t in range(16):
        n = ib - 1 if t in anchors else ib
        v = _put(v, (at, n), t % (1 << ib))
        at += n
    return v


def bc7_field_blocks(rng, anchors_of):
    """the blocks of bc7_fields.npz, (n, 16) uint8; anchors_of(mode, partition) -> the anchor texels (only the ramp of extremes 6 and 7 needs to
    know where the narrower indices sit)"""
    def block(mode, **fields):
        v = int.from_bytes(rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), "little")
        v = (v & ~((2 << mode) - 1)) | 1 << mode
        f = bc7_fields(mode)
        for name, value in fields.items():
            if f[name][1]:
                v = _put(v, f[name], value)
        return v

    out = []
    for mode in (0, 1, 2, 3, 7):  # pairs
        for partition in range(1 << BC7_MODES[mode][1]):
            out += [block(mode, partition=partition) for _ in range(2)]
    for rotation in range(4):  # fields
        for selection in range(2):
            out += [block(4, rotation=rotation, selection=selection) for _ in range(4)]
    for rotation in range(4):
        out += [block(5, rotation=rotation) for _ in range(4)]
    for pbits in range(4):
        out += [block(6, pbits=pbits) for _ in range(4)]
    for mode in range(8):  # extremes
        f = bc7_fields(mode)
        payload = (mode + 1, 127 - mode)
        out.append(_put(block(mode), payload, 0))
        out.append(_put(block(mode), payload, -1))
        out.append(block(mode, index=0, index2=0))
        out.append(block(mode, index=-1, index2=-1))
        out.append(_endpoints(block(mode), mode, 0, 1))
        out.append(_endpoints(block(mode), mode, 1, 0))
        if f["index2"][1]:
            out.append(block(mode, index=0, index2=-1, selection=0))
            out.append(block(mode, index=-1, index2=0, selection=1))
        else:
            for even, odd in ((0, 1), (1, 0)):
                v = _endpoints(block(mode), mode, even, odd)
                partition = v >> f["partition"][0] & ((1 << f["partition"][1]) - 1)
                out.append(_ramp(v, mode, anchors_of(mode, partition)))
    return np.frombuffer(b"".join(v.to_bytes(16, "little") for v in out), np.uint8).reshape(-1, 16).copy()


# the anchor texels of the BPTC partitions (Khronos Data Format Specification, tables of anchor indices): second subset of two, second and
# third subset of three.  Used only to place the index ramp of the extremes; the decoders under test have tables of their own.
ANCHOR2 = [15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
           15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15]
ANCHOR3A = [3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
            8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3]
ANCHOR3B = [15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
            15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8]


def bc7_anchors(mode, partition):
    ns = BC7_MODES[mode][0]
    return {0} | ({ANCHOR2[partition]} if ns == 2 else {ANCHOR3A[partition], ANCHOR3B[partition]} if ns == 3 else set())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a niagara checkout (extern/bcdec.h is included by path)")
    ap.add_argument("--scratch", default=None)
    ap.add_argument("--out", default=None, help="the directory both .npz files are written to (default: textures/ beside this file)")
    args = ap.parse_args()
    header = os.path.join(os.path.abspath(args.reference), "extern", "bcdec.h")
    assert os.path.exists(header), header
    scratch = args.scratch or tempfile.mkdtemp()
    os.makedirs(scratch, exist_ok=True)
    src, exe = os.path.join(scratch, "bc_golden.c"), os.path.join(scratch, "bc_golden")
    with open(src, "w") as f:
        f.write(PROGRAM % header)
    subprocess.check_call(["gcc", "-O1", "-w", src, "-o", exe])
    data = blocks(np.random.default_rng(0xBC7))
    out = {}
    for name, fmt in (("bc1", 1), ("bc2", 2), ("bc3", 3), ("bc7", 7)):
        res = subprocess.run([exe, str(fmt)], input=data[name].tobytes(), stdout=subprocess.PIPE, check=True).stdout
        out[name] = data[name]
        out[name + "_rgba"] = np.frombuffer(res, np.uint8).reshape(len(data[name]), 64)
    fields = bc7_field_blocks(np.random.default_rng(0xBC7F), bc7_anchors)  # a generator of its own: the stream above is bc_blocks.npz's
    res = subprocess.run([exe, "7"], input=fields.tobytes(), stdout=subprocess.PIPE, check=True).stdout
    second = dict(bc7=fields, bc7_rgba=np.frombuffer(res, np.uint8).reshape(len(fields), 64))
    where = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "textures")  # (a directory of its own: tests/test_golden.py reads every .npz beside this file as a cull scene)
    os.makedirs(where, exist_ok=True)
    for name, arrays in (("bc_blocks.npz", out), ("bc7_fields.npz", second)):
        path = os.path.join(where, name)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
