"""Launched by tests/test_gpu_ztosig_line.py: the file-based tile check of tests/ztosig_line_files_checks.py on the device, in a process of its
own like tests/gpu_ztosig_tiles.py -- 2x2 tiles as four contexts on GPU 0, one host thread and one stream each, the asynchronous
event-ordered mover between them, which needs torch (imported FIRST, so that the library and torch share one HIP runtime).

    python tests/gpu_ztosig_line_tiles.py
"""
import os
import pathlib
import sys
import tempfile

import torch  # noqa: F401  (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ztosig_line_files_checks as fchk

if __name__ == "__main__":
    with tempfile.TemporaryDirectory(prefix="ztosig_line_tiles_") as d:
        fchk.tiles(None, pathlib.Path(d))
    print("ZTOSIG-LINE-FILE-TILES-OK")
