"""The batched copy kernel (csrc/copy_many.hip) on the CPU under tools/hipemu with a tile of 64 bytes, built with AddressSanitizer
(tests/emu/copy_many_emu.cpp has the cases: all 256 pairs of source and destination alignment at lengths around 0, 16 and the tile size,
launches of 1, 63, 64, 65 and 1,000 copies with empty copies first, in the middle and last, guard bytes around every destination, every
source ending with its allocation)."""
import os
import subprocess

from test_emu_kernels import build

TILE = 64
ASAN = ["-fsanitize=address", "-g", "-fno-omit-frame-pointer"]


def test_copy_many_kernel_emulated(tmp_path):
    exe = build("copy_many_emu", tmp_path, extra=["-DKNZ_EMU_COPY_TILE=%du" % TILE] + ASAN)
    for order in ("0", "2"):                    # (workgroup dispatch order is not defined)
        env = dict(os.environ, HIPEMU_ORDER=order, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and "OK 3579 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
