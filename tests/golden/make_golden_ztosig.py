"""Regenerate tests/golden/ztosig.json: for every shape of tests/ztosig_expect.SHAPES, T-like and S-like, the digests of the generated
inputs and the digest of what the REFERENCE's compiled ztosig_ (oracle/_ref, built by oracle/build_ref.sh) makes of them.  The inputs'
digests stand beside the output's, so a generator that has drifted shows as such and not as a wrong result.  Needs the reference build;
the tests that read the file do not.

    python tests/golden/make_golden_ztosig.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ztosig_expect as Z                                    # noqa: E402
from test_ztosig_vs_reference import reference_ztosig       # noqa: E402


def main():
    out = {}
    for im, jm, ks, kb in Z.SHAPES:
        for salt in (False, True):
            zs, src, zz, h = Z.make_inputs(im, jm, ks, kb, salt=salt)
            out[f"{im}x{jm}x{ks}x{kb}{'S' if salt else 'T'}"] = {
                "inputs": {n: Z.digest(a) for n, a in (("zs", zs), ("src", src), ("zz", zz), ("h", h))},
                "reference": Z.digest(reference_ztosig(zs, src, zz, h)),
            }
    with open(os.path.join(HERE, "ztosig.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(out)} entries")


if __name__ == "__main__":
    main()
