"""TEST TOOLING: writes tests/golden/png_encode.json, the SHA-256 of the PNG files that the two encode kernels write ON THE CPU
EMULATOR for the seeded inputs of tests/test_emu_png_encode.py: golden_inputs().  tests/test_gpu_png_encode.py requires the same
digests from api.png_encode_batch on the GPU, which is where emulator bytes and GPU bytes meet.  The file holds recorded results only.

    python tools/make_png_encode_golden.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stage_launch as SL  # noqa: E402
import test_emu_png_encode as E  # noqa: E402

if __name__ == "__main__":
    SL.KERNELS.update(E.KERNELS)
    rec = {name: hashlib.sha256(E.kernels_file(im, filt, level, pal, trns)).hexdigest() for name, im, filt, level, pal, trns in E.golden_inputs()}
    with open(E.golden_path(), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", E.golden_path(), len(rec), "digests")
