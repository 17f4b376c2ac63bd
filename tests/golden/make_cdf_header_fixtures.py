"""Regenerate tests/golden/cdf_header_*.nc: three small NetCDF classic files whose headers tools/check_cdf_header.cpp damages
(tests/test_host_logic.py::test_header_parser_survives_damaged_headers_under_sanitizers).  Between them: CDF-1 and CDF-2, global and
variable attributes of several types, fixed and record variables, NC_BYTE / NC_INT / NC_FLOAT / NC_DOUBLE, a scalar.

    python tests/golden/make_cdf_header_fixtures.py
"""
import os

import numpy as np
from scipy.io import netcdf_file

HERE = os.path.dirname(os.path.abspath(__file__))
IM, JM, KB, KS = 5, 4, 3, 4


def grid(path):
    with netcdf_file(path, "w", version=2) as nc:
        nc.title = "header fixture: a grid file"
        nc.createDimension("z", KB)
        nc.createDimension("y", JM)
        nc.createDimension("x", IM)
        for n in ("z", "zz"):
            nc.createVariable(n, "d", ("z",))[:] = -np.linspace(0.0, 1.0, KB)
        for k, n in enumerate(("dx", "dy", "lat_rho", "h")):
            v = nc.createVariable(n, "f" if k % 2 else "d", ("y", "x"))
            v.units = "metre"
            v[:] = 100.0 + k + np.arange(JM * IM).reshape(JM, IM)
        v = nc.createVariable("fsm", "b", ("y", "x"))
        v.valid_range = np.array([0, 1], dtype=np.int8)
        v[:] = 1
        nc.createVariable("count", "i", ())[...] = 7


def clim(path):
    with netcdf_file(path, "w", version=1) as nc:
        nc.createDimension("month", None)
        nc.createDimension("z", KS)
        nc.createDimension("y", JM)
        nc.createDimension("x", IM)
        nc.createVariable("z", "f", ("z",))[:] = [5.0, 50.0, 500.0, 5000.0]
        for n in ("Tclim", "Sclim"):
            v = nc.createVariable(n, "f", ("month", "z", "y", "x"))
            v.long_name = "a monthly climatology"
            v[:] = np.arange(12 * KS * JM * IM, dtype=np.float32).reshape(12, KS, JM, IM)


def restart(path):
    with netcdf_file(path, "w", version=2) as nc:
        nc.description = "restart file"
        nc.createDimension("time", 1)
        nc.createDimension("z", KB)
        nc.createDimension("y", JM)
        nc.createDimension("x", IM)
        nc.createVariable("iint", "d", ())[...] = 3.0
        nc.createVariable("time", "d", ("time",))[:] = 0.25
        nc.createVariable("el", "d", ("y", "x"))[:] = 0.5
        nc.createVariable("u", "d", ("z", "y", "x"))[:] = 0.125


if __name__ == "__main__":
    for name, make in (("grid", grid), ("clim", clim), ("restart", restart)):
        make(os.path.join(HERE, f"cdf_header_{name}.nc"))
