"""Launched by tests/test_gpu_water.py: the tile check of tests/water_checks.py on the device, in a process of its own like
tests/gpu_forcing_tiles.py -- 2x2 tiles as four contexts on GPU 0, one host thread and one stream each, the asynchronous event-ordered
mover between them, which needs torch (imported FIRST, so that the library and torch share one HIP runtime).

    python tests/gpu_water_tiles.py
"""
import os
import pathlib
import sys
import tempfile

import torch  # noqa: F401  (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import water_checks as chk

if __name__ == "__main__":
    with tempfile.TemporaryDirectory(prefix="water_tiles_") as d:
        chk.tiles_equal_single_tile(None, pathlib.Path(d))
    print("WATER-TILES-OK")
