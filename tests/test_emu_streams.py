"""The many-stream framing kernels (csrc/streams.hip) on the CPU under tools/hipemu: the segmented framing scan and the two-pass
multi-stream walk against today's single-stream kernels run one stream at a time (tests/emu/streams_emu.cpp has the cases: 1, 63, 64, 65,
257 and 1,000 streams of 0-5 blocks, empty streams in front, in the middle and at the end, totals beyond 2^32 bits, damaged prefixes)."""
import os
import subprocess

from test_emu_kernels import build


def test_stream_framing_kernels_emulated(tmp_path):
    exe = build("streams_emu", tmp_path)
    for order in ("0", "2"):                    # (workgroup dispatch order is not defined)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, HIPEMU_ORDER=order))
        assert r.returncode == 0 and "OK 83 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
