"""Generator of tests/golden/textures/bc_blocks.npz: BC1 / BC2 / BC3 / BC7 blocks and the 64 RGBA8 bytes niagara's CPU decoder (the one behind
decodeImageRGBA, src/textures.cpp:295) produces for each.  The fixture is the DEFINITION of the decode; it is regenerated
only by hand:

    python tests/golden/generate_bc.py --reference <niagara checkout> [--scratch <dir>]

A throw-away C program is written into the scratch directory; it includes the checkout's decoder header by path and is compiled with the host
compiler (a plain build, no sanitizer).  Nothing of the checkout is copied into this tree; the tests read the .npz only.

Contents (uint8 arrays): bc7 (64 blocks per mode 0-7 with the mode bits forced and the rest random, then 32 reserved blocks: mode byte 0),
bc1 (256: c0 > c1, c0 <= c1 with every index, equal endpoints), bc2 (128), bc3 (256: a0 > a1, a0 <= a1, equal endpoints); <name>_rgba holds the
decoder's output, 64 bytes per block, row-major texels.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a niagara checkout (extern/bcdec.h is included by path)")
    ap.add_argument("--scratch", default=None)
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
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "textures", "bc_blocks.npz")  # (a directory of its own: tests/test_golden.py reads every .npz beside this file as a cull scene)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
