"""tests/golden/forcing_reader_schema.json -- the variable names and dimension orders the reference's forcing readers ask for, extracted
from its source by tests/golden/make_forcing_schema.py -- against the names tests/forcing_expect.py writes (that the library looks every one of them up by name is the refusals check of
tests/forcing_files_checks.py: a file without it is refused with its name), and
(where the reference tree is present) against a fresh extraction."""
import importlib.util
import json
import os

import pytest

import forcing_expect as fx

HERE = os.path.dirname(os.path.abspath(__file__))


def _schema():
    with open(os.path.join(HERE, "golden", "forcing_reader_schema.json")) as f:
        return json.load(f)


def _generator():
    spec = importlib.util.spec_from_file_location("make_forcing_schema", os.path.join(HERE, "golden", "make_forcing_schema.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_files_of_the_tests_carry_the_readers_names():
    r = _schema()["readers"]
    by_suffix = {}
    for reader in r.values():
        by_suffix.setdefault(reader["suffix"], []).extend(reader["vars"])
    assert set(by_suffix) == {".sfrc.nc", ".lbry.nc", ".clim.nc"}
    assert [v["name"] for v in by_suffix[".sfrc.nc"]] == list(fx.SFRC)
    assert [v["name"] for v in by_suffix[".lbry.nc"]] == list(fx.LBRY)
    assert [v["name"] for v in by_suffix[".clim.nc"]] == list(fx.CLIM)
    for v in by_suffix[".sfrc.nc"]:
        assert v["dims"] == ["record", "y", "x"] and v["record_index"] is None
    for v in by_suffix[".lbry.nc"]:
        side = "y" if v["name"].endswith(".east") else "x"
        assert v["dims"] == (["record", side] if v["name"].startswith("zeta.") else ["record", "z", side])
    for v in by_suffix[".clim.nc"]:
        assert v["dims"] == ["record", "z", "y", "x"] and v["record_index"] == [9, 12, 1]


def test_the_committed_schema_is_what_the_reference_source_says():
    gen = _generator()
    if not os.path.exists(gen.SRC):
        pytest.skip("the reference tree is not present")
    assert gen.generate() == _schema()
