"""Regenerate tests/golden/ztosig_line.json: for every shape of tests/ztosig_line_expect.SHAPES, each of the four edges, T-like and S-like,
the digests of the generated inputs and the digest of what the REFERENCE's compiled ztosig_ (oracle/_ref, built by oracle/build_ref.sh)
makes of them when it is called as the commented blocks of bounds_forcing.f:636-716 call it (tests/test_ztosig_line_vs_reference.block).
Needs the reference build; the tests that read the file do not.

    python tests/golden/make_golden_ztosig_line.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ztosig_line_expect as ZL                              # noqa: E402
from test_ztosig_line_vs_reference import block             # noqa: E402


def main():
    out = {}
    for im, jm, ks, kb in ZL.SHAPES:
        for edge, name in enumerate(ZL.EDGES):
            for salt in (False, True):
                zs, line, zz, h = ZL.make_inputs(im, jm, ks, kb, edge, salt=salt)
                out[f"{im}x{jm}x{ks}x{kb}{name}{'S' if salt else 'T'}"] = {
                    "inputs": {n: ZL.digest(a) for n, a in (("zs", zs), ("line", line), ("zz", zz), ("h", h))},
                    "reference": ZL.digest(block(zs, line, zz, h, edge)),
                }
    with open(os.path.join(HERE, "ztosig_line.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(out)} entries")


if __name__ == "__main__":
    main()
