"""Launched by tests/test_gpu_tracer_files.py: the tile check of tests/tracer_files_checks.py on the device, in a process of its own like
tests/gpu_tracer_tiles.py -- nx x ny tiles as contexts on GPU 0, one host thread and one stream each, the asynchronous event-ordered
mover between them, which needs torch (imported FIRST, so that the library and torch share one HIP runtime).

    python tests/gpu_tracer_files_tiles.py NX NY
"""
import os
import pathlib
import sys
import tempfile

import torch  # noqa: F401  (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracer_files_checks as chk

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        chk.tiles(None, int(sys.argv[1]), int(sys.argv[2]), pathlib.Path(tmp))
    print("TRACER FILES TILES OK")
