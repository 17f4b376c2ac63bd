"""Launched by tests/test_gpu_tides.py: the tile check of tests/tide_checks.py on the device, in a process of its own like
tests/gpu_tracer_tiles.py -- 2 x 2 tiles as contexts on GPU 0, one host thread and one stream each, the asynchronous event-ordered mover
between them, which needs torch (imported FIRST, so that the library and torch share one HIP runtime).

    python tests/gpu_tide_tiles.py
"""
import os
import sys

import torch  # noqa: F401  (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tide_checks as chk

if __name__ == "__main__":
    chk.tiles(None, 2, 2)
    print("TIDE TILES OK")
