"""The stored reference results under tests/golden/ by file stem (the session fixtures of conftest.py hold the three oldest)."""
import json
import os


def golden_file(stem):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", stem + ".json")) as f:
        return json.load(f)
