"""tests/golden/water_reader_schema.json -- the file-name format, the variable name and the dimension order read_water_pnetcdf asks for,
extracted from the reference's source by tests/golden/make_water_schema.py -- against the name and the file tests/water_expect.py writes
(that the library looks `w` up by that name and in that order is the refusals check of tests/water_checks.py), and (where the reference
tree is present) against a fresh extraction."""
import importlib.util
import json
import os

import numpy as np
import pytest
from scipy.io import netcdf_file

import water_expect as wx

HERE = os.path.dirname(os.path.abspath(__file__))


def _schema():
    with open(os.path.join(HERE, "golden", "water_reader_schema.json")) as f:
        return json.load(f)


def _generator():
    spec = importlib.util.spec_from_file_location("make_water_schema", os.path.join(HERE, "golden", "make_water_schema.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_files_of_the_tests_carry_the_readers_name_and_order(tmp_path):
    s = _schema()
    f = s["name_format"]
    assert f["number_width"] == f["number_min_digits"] == 4   # i4.4: 0000 .. 9999, **** beyond
    for n in (0, 7, 9999):
        assert wx.name("P", n) == "P" + f["infix"] + str(n).zfill(f["number_min_digits"]) + f["suffix"]
    assert [v["name"] for v in s["vars"]] == ["w"] and s["vars"][0]["dims"] == ["y", "x"]
    field = np.arange(6.).reshape(2, 3)                       # (jm, im) = (2, 3)
    with netcdf_file(wx.write_water(str(tmp_path / "P"), 0, field), "r", mmap=False) as nc:
        v = nc.variables[s["vars"][0]["name"]]
        assert v.shape == (2, 3) and np.array_equal(v[:], field)


def test_the_committed_schema_is_what_the_reference_source_says():
    gen = _generator()
    if not os.path.exists(gen.SRC):
        pytest.skip("the reference tree is not present")
    assert gen.generate() == _schema()
