"""The GPU cases of the elastic deformation battery (tests/test_emu_png_elastic.py) under the ids they have always had.  What they run and
assert is tests/test_gpu_png_stage_kernels.py's: its MODULES, EXCLUDED, NO_LAUNCH, FULL_GRID and ALSO_WARP tables and its run_case."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_png_stage_kernels as GK  # noqa: E402
from test_gpu_png_stage_kernels import on_the_gpu, test_every_battery_case_runs_or_is_excluded  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key,kw", GK._cases(["test_emu_png_elastic"]))
def test_battery(key, kw, on_the_gpu):
    GK.run_case(key, kw, on_the_gpu)
