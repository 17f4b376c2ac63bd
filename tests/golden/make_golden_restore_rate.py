"""Regenerate tests/golden/restore_rate.json: for every shape of tests/restore_rate_expect.SHAPES the digests of the generated rate inputs --
the sponge of record 0 on its z levels, the grid it is mapped for -- and the digest of what the REFERENCE's compiled ztosig_ (oracle/_ref,
built by oracle/build_ref.sh) makes of them; the last shape twice, the second time with the steep sponge whose mapped field goes below
zero.  The inputs' digests stand beside the output's, so a generator that has drifted shows as such and not as a wrong result.  Needs the
reference build; the tests that read the file do not.

    python tests/golden/make_golden_restore_rate.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import restore_rate_expect as R                              # noqa: E402
from test_ztosig_vs_reference import reference_ztosig       # noqa: E402


def entries():
    for shape in R.SHAPES:
        yield shape, False
    yield R.SHAPES[-1], True


def main():
    out = {}
    for (im, jm, ks, kb), steep in entries():
        zs, rate, zz, h = R.make_rate(im, jm, ks, kb, steep=steep)
        out["x".join(str(n) for n in (im, jm, ks, kb)) + ("steep" if steep else "")] = {
            "inputs": {n: R.digest(a) for n, a in (("zs", zs), ("rate", rate), ("zz", zz), ("h", h))},
            "reference": R.digest(reference_ztosig(zs, rate, zz, h)),
        }
    with open(os.path.join(HERE, "restore_rate.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(out)} entries")


if __name__ == "__main__":
    main()
