"""Generates tests/golden/forcing_reader_schema.json: what the reference's forcing readers ask of their input files -- per reader the
file suffix, the variable names in the order they are looked up and, per variable, the dimension order of the hyperslab it reads --
taken out of the reference's own source (pom/io_pnetcdf.F: read_wind_pnetcdf, read_heat_pnetcdf, read_surface_pnetcdf,
read_boundary_conditions_pnetcdf, read_restore_ts_interior_pnetcdf) by interpreting the ACTIVE (uncommented) statements

    write(<file>,'(a,''in/'',a,''<suffix>'')') ...          the file name
    status=nfmpi_inq_varid(ncid,'<name>',<x>_varid)          name -> id
    start(k)=<i_global(1)|j_global(1)|1|n|mod(n+a,b)+c>      edge(k)=<im|jm|k|1>
    status=nfmpi_get_vara_double_all(ncid,<x>_varid,start,edge,...)   the read, under the start / edge in force

The fixture is data (names and numbers), not source text.  Dimensions are recorded in the FILE's (C / CDL) order, i.e. start / edge
reversed: "x" = the tile's columns from i_global(1), "y" = its rows from j_global(1), "z" = all levels from 1, "record" = one record;
record_index = [a, b, c]: the record read is mod(n+a, b)+c, null: n itself.  Run where the reference is present:

    python tests/golden/make_forcing_schema.py
"""
import json
import os
import re
import sys

REF = os.environ.get("POM_REFERENCE", "/root/reference")
SRC = os.path.join(REF, "pom", "io_pnetcdf.F")
READERS = ("read_wind_pnetcdf", "read_heat_pnetcdf", "read_surface_pnetcdf", "read_boundary_conditions_pnetcdf", "read_restore_ts_interior_pnetcdf")


def statements(lines):
    """fixed form: join continuation lines, drop comments and cpp lines"""
    out = []
    for ln in lines:
        ln = ln.rstrip("\n")
        if not ln.strip() or ln[0] in "!cC*#" or ln.lstrip().startswith("!"):
            continue
        if len(ln) > 5 and ln[5] not in " 0" and ln[:5].strip() == "":
            out[-1] += ln[6:].strip()
        else:
            out.append(ln.strip())
    return out


def routine(all_lines, name):
    start = next(n for n, ln in enumerate(all_lines) if re.match(rf"\s+subroutine {name}\b", ln))
    end = next(n for n in range(start + 1, len(all_lines)) if re.match(r"\s+end\s*$", all_lines[n]))
    return all_lines[start:end]


def axis(start, edge):
    s = start.replace(" ", "")
    if s == "i_global(1)" and edge == "im":
        return "x", None
    if s == "j_global(1)" and edge == "jm":
        return "y", None
    if s == "1" and edge == "k":
        return "z", None
    if s == "n" and edge == "1":
        return "record", None
    m = re.fullmatch(r"mod\(n\+(\d+),(\d+)\)\+(\d+)", s)
    if m and edge == "1":
        return "record", [int(v) for v in m.groups()]
    raise ValueError(f"start = {start!r}, edge = {edge!r}: not a hyperslab this generator knows")


def generate():
    with open(SRC) as f:
        lines = f.readlines()
    readers = {}
    for name in READERS:
        suffix, names, variables, start, edge = None, {}, [], {}, {}
        for st in statements(routine(lines, name)):
            if re.fullmatch(r"start\(1\)\s*=.*", st):           # start(1..r) is set as a block before the reads that use it: a block of
                start, edge = {}, {}                            # lower rank after one of higher rank must not see its stale entries
            part = interpret_one(st, names, start, edge)
            if isinstance(part, str):
                suffix = part
            elif part is not None:
                variables.append(part)
        readers[name] = {"suffix": suffix, "vars": variables}
    return {"source": "pom/io_pnetcdf.F: " + ", ".join(READERS) + " (active statements interpreted by tests/golden/make_forcing_schema.py)",
            "readers": readers}


def interpret_one(st, names, start, edge):
    """one statement; returns the suffix (str), a variable read (dict) or None"""
    m = re.search(r"''in/'',a,''(\.[a-z]+\.nc)''", st)
    if m and st.lower().startswith("write("):
        return m.group(1)
    flat = st.replace(" ", "")
    m = re.fullmatch(r"status=nfmpi_inq_varid\(ncid,'([^']+)',(\w+)\)", flat)
    if m:
        names[m.group(2)] = m.group(1)
        return None
    m = re.fullmatch(r"(start|edge)\((\d)\)=(.*)", flat)
    if m:
        (start if m.group(1) == "start" else edge)[int(m.group(2))] = m.group(3)
        return None
    m = re.match(r"status=nfmpi_get_vara_double_all\(ncid,(\w+),start,edge", flat)
    if m:
        dims, rec = [], None
        for k in range(max(start), 0, -1):
            name, how = axis(start[k], edge[k])
            dims.append(name)
            if name == "record":
                rec = how
        if dims[0] != "record":
            raise ValueError(f"{names[m.group(1)]}: the slowest dimension read is not the record")
        return {"name": names[m.group(1)], "dims": dims, "record_index": rec}
    return None


def main():
    if not os.path.exists(SRC):
        sys.exit(f"{SRC} not found: run where the reference is present")
    out = generate()
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "forcing_reader_schema.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k, v in out["readers"].items():
        print(k, v["suffix"], [(x["name"], x["dims"]) for x in v["vars"]])


if __name__ == "__main__":
    main()
