"""Rebuilds the shadow trace's TLAS on the device with whatever library NV_LIBRARY_PATH names and compares every result with the host twin;
prints "tlas_runner: ok".  tests/test_tlas_build_gpu.py runs it with the experiments build, whose library-owned blocks start as 0xAB bytes
between canary zones (context.hip scratch_alloc): a large build, a small one behind it, an empty one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import shadow_ref as SH  # noqa: E402
import tlas_ref as TR  # noqa: E402
from niagara_amd import _lib, host  # noqa: E402
from niagara_amd import pipeline as P  # noqa: E402


def main():
    scene = TR.with_empty_mesh(SH.fuzz_scene(20, 11, 8.0))
    blob = host.rt_scene_build(scene["meshes"], scene["indices"], scene["vertices"], scene["draws"])
    check = getattr(_lib.lib, "nv_debug_check_scratch", None)
    c = P.Context()
    try:
        c.rt_scene_upload(blob)
        c.rt_scene_reserve_dynamic(3 * 2048 + 5)
        for n in (3 * 2048 + 5, 2049, 3, 0, 1, 600):
            draws = TR.mixed_draws(n, 900 + n, 2, 40.0, empty_mesh=2)
            dev = P.to_device(draws if n else np.zeros(1, draws.dtype), c.device)
            c.rt_tlas_build(dev, n)
            c.status()
            got, want = c.rt_scene_download(), host.rt_tlas_build_host(blob, draws)
            if got.tobytes() != want.tobytes():
                print("tlas_runner: n = %d differs from the host twin" % n)
                return 1
            if check is not None and check() != 0:
                print("tlas_runner: n = %d wrote outside a library-owned block" % n)
                return 1
    finally:
        c.close()
    print("tlas_runner: ok (%s)" % ("canaries checked" if check is not None else "no canaries in this library"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
