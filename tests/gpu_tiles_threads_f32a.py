"""Launched by tests/test_gpu_fp32_arith_variant.py: tests/gpu_tiles_threads.py with its "f32" runs taken by libpomgpu_f32a.so (the
fp32-arithmetic variant) instead of libpomgpu_f32.so.  Same arguments; the tiles are compared with the single tile of the same build."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from extpom_amd import lib as _lib

_lib.LIBPATH_F32 = _lib.LIBPATH_F32A
runpy.run_path(os.path.join(ROOT, "tests", "gpu_tiles_threads.py"), run_name="__main__")
