"""Launched by tests/test_gpu_mean_output.py: the tile check of tests/mean_output_checks.py on the device, in a process of its own like
tests/gpu_lateral_sides_tiles.py -- 2x2 tiles as four contexts on GPU 0, one host thread and one stream each, the asynchronous
event-ordered mover between them, which needs torch (imported FIRST, so that the library and torch share one HIP runtime).

    python tests/gpu_mean_output_tiles.py
"""
import os
import sys

import torch  # noqa: F401  (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mean_output_checks as chk

if __name__ == "__main__":
    chk.tiles(None)
    print("MEAN-OUTPUT-TILES-OK")
