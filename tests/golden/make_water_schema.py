"""Generates tests/golden/water_reader_schema.json: what the reference's read_water_pnetcdf (pom/io_pnetcdf.F:3227-3272) asks of its input
-- the file-name format, the variable name and the dimension order of the hyperslab it reads -- taken out of the reference's own source
by interpreting the ACTIVE (uncommented) statements, with the statement reader of tests/golden/make_forcing_schema.py:

    write(<file>,'(a,''in/'',a,''.water.'',i4.4,''.nc'')') ...   the file name: one file per record number
    status=nfmpi_inq_varid(ncid,'<name>',<x>_varid)               name -> id
    start(k)=<i_global(1)|j_global(1)>      edge(k)=<im|jm>
    status=nfmpi_get_vara_double_all(ncid,<x>_varid,start,edge,...)

The fixture is data (names and numbers), not source text.  Dimensions are recorded in the FILE's (C / CDL) order, i.e. start / edge
reversed: "x" = the tile's columns from i_global(1), "y" = its rows from j_global(1); there is no record dimension.  name_format: the
edit descriptors between the path and ".nc" -- the literal ".water." and the width and minimum digits of the record number's I edit
descriptor.  Run where the reference is present:

    python tests/golden/make_water_schema.py
"""
import importlib.util
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_forcing_schema", os.path.join(HERE, "make_forcing_schema.py"))
mfs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfs)
SRC = mfs.SRC
READER = "read_water_pnetcdf"


def generate():
    with open(SRC) as f:
        lines = f.readlines()
    fmt, names, variables, start, edge = None, {}, [], {}, {}
    for st in mfs.statements(mfs.routine(lines, READER)):
        m = re.search(r"'\(a,''in/'',a,''(\.[a-z]+\.)'',i(\d+)\.(\d+),''(\.nc)''\)'", st)
        if m and st.lower().startswith("write("):
            fmt = {"directory": "in/", "infix": m.group(1), "number_width": int(m.group(2)), "number_min_digits": int(m.group(3)), "suffix": m.group(4)}
            continue
        part = mfs_one(st, names, start, edge)
        if part is not None:
            variables.append(part)
    return {"source": "pom/io_pnetcdf.F: " + READER + " (active statements interpreted by tests/golden/make_water_schema.py)",
            "reader": READER, "name_format": fmt, "vars": variables}


def mfs_one(st, names, start, edge):
    """make_forcing_schema.interpret_one for a reader whose hyperslab has no record dimension"""
    flat = st.replace(" ", "")
    m = re.match(r"status=nfmpi_get_vara_double_all\(ncid,(\w+),start,edge", flat)
    if not m:
        mfs.interpret_one(st, names, start, edge)             # names, start, edge: filled in place
        return None
    dims = [mfs.axis(start[k], edge[k])[0] for k in range(max(start), 0, -1)]
    return {"name": names[m.group(1)], "dims": dims}


def main():
    if not os.path.exists(SRC):
        sys.exit(f"{SRC} not found: run where the reference is present")
    out = generate()
    with open(os.path.join(HERE, "water_reader_schema.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out["name_format"], out["vars"])


if __name__ == "__main__":
    main()
