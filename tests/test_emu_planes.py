"""The byte-plane kernels (csrc/planes.hip) on the CPU under tools/hipemu, built with AddressSanitizer (tests/emu/planes_emu.cpp has the
cases: split and join, elements of 1, 2, 4 and 8 bytes, all 256 pairs of source and destination alignment at element counts around 0, 16
and the tile, launches of 1, 63, 64, 65 and 1,000 entries with empty entries first, in the middle and last and the widths mixed, guard
bytes around every destination, every source ending with its allocation, a scalar loop as the reference).

A tile of 64 bytes makes tile boundaries cheap to cross, but holds at most four 16-element units and none of 8-byte elements; a tile of
256 bytes has units and a tail for every width; the kernel's own tile (every 37th alignment pair) is the only one at which a lane takes
several units per pass."""
import os
import subprocess

import pytest

from test_emu_kernels import build

ASAN = ["-fsanitize=address", "-g", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("tile,step,cases", [(64, 1, 19088), (256, 1, 19088), (None, 37, 2386)])
def test_plane_kernels_emulated(tmp_path, tile, step, cases):
    exe = build("planes_emu", tmp_path, extra=(["-DKNZ_EMU_PLANES_TILE=%du" % tile] if tile else []) + ASAN)
    for order in ("0", "2"):                    # (workgroup dispatch order is not defined)
        env = dict(os.environ, HIPEMU_ORDER=order, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
        r = subprocess.run([exe, str(step)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and "OK %d cases" % cases in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
