"""tests/golden/cold_start_reader_schema.json -- the variable names and dimension roles the reference's three cold-start readers ask for
-- against the names tests/cold_start_expect.py writes (that the library looks every one of them up by name is the refusals check of
tests/cold_start_checks.py: a file without it is refused with its name), and, where the reference tree is present, against the names
in the readers' own nfmpi_inq_varid calls."""
import json
import os
import re

import pytest

import cold_start_expect as E

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "/root/reference/pom/io_pnetcdf.F"


def _schema():
    with open(os.path.join(HERE, "golden", "cold_start_reader_schema.json")) as f:
        return json.load(f)["readers"]


def test_the_files_of_the_tests_carry_the_readers_names():
    r = _schema()
    assert {v["suffix"] for v in r.values()} == {".grid.nc", ".init.nc", ".clim.nc"}
    grid = r["read_grid_pnetcdf"]["vars"]
    assert [v["name"] for v in grid] == ["z", "zz"] + list(E.GRID_PLANES)
    assert {v["name"]: v["into"] for v in grid[2:]} == E.GRID_PLANES and all(v["dims"] == ["y", "x"] for v in grid[2:])
    init = r["read_initial_ts_pnetcdf"]
    assert init["unlimited_dimension"] and [v["name"] for v in init["vars"]] == ["Level", "T", "S"]
    assert all(v["dims"] == ["record", "level", "y", "x"] and v["record_index"] == 1 for v in init["vars"][1:])
    clim = r["read_clim_ts_pnetcdf"]["vars"]
    assert [v["name"] for v in clim] == ["Tclim", "Sclim"] and all(v["dims"] == ["record", "z", "y", "x"] and v["record_index"] == 10 for v in clim)


def test_the_committed_schema_is_what_the_reference_source_says():
    if not os.path.exists(SRC):
        pytest.skip("the reference tree is not present")
    text = open(SRC, errors="replace").read()
    for sub, reader in _schema().items():
        body = re.search(r"^ {6}subroutine %s\b.*?^ {6}end *$" % sub, text, re.S | re.M | re.I).group(0)
        active = "\n".join(l for l in body.splitlines() if l[:1] not in "!cC*")
        assert re.findall(r"nfmpi_inq_varid\(ncid,'([^']+)'", active) == [v["name"] for v in reader["vars"]], sub
        if reader.get("unlimited_dimension"):
            assert "nfmpi_inq_unlimdim" in active
