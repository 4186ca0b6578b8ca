"""TEST TOOLING: writes tests/golden/png_encode_lz.json, the SHA-256 of the level-3 PNG files that the filter kernel and the lz kernel
write ON THE CPU EMULATOR for the seeded inputs of tests/test_emu_png_encode_lz.py: golden_inputs().
tests/test_gpu_png_encode_lz.py requires the same digests from api.png_encode_batch_lz on the GPU, which is where emulator bytes and
GPU bytes meet.  The file holds recorded results only.

    python tools/make_png_encode_lz_golden.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stage_launch as SL  # noqa: E402
import test_emu_png_encode_lz as Q  # noqa: E402

if __name__ == "__main__":
    SL.KERNELS.update(Q.KERNELS)
    rec = {name: hashlib.sha256(Q.kernels_file(im, filt, pal, trns)).hexdigest() for name, im, filt, pal, trns in Q.golden_inputs()}
    with open(Q.golden_path(), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", Q.golden_path(), len(rec), "digests")
